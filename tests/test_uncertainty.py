"""Value uncertainty on the host (agz_search_set_value_moments / _set_lcb / _set_puct_variance): the
arithmetic of include/agz_uncertainty.h against its numpy restatement, the moment rule on a tree driven one call at a
time against a dict mirror, the LCB pick and the variance factor on hand-made rows, whole games on the simulator with
moments only (nothing changes) and with both rules (counters against a Python tally of the rows), the argument checks,
and a stand-alone sanitizer build.  The simulator is hs.Sim: agz_search.h itself, lane-serial.  CPU only."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import alphago_jl_amd as ag
import gpu_options
import hs
import puct_twin as pt
import uncertainty_twin as ut
from test_explore import run_sanitizer_part

f32, f64 = np.float32, np.float64
bits32, bits64 = hs.bits32, hs.bits64
NAN = float("nan")
G_SEARCH = 3


# ---------------------------------------------------------------- the header

def stat_rows():
    """(N, W, S) entries: unvisited ones, S just below W^2 / cnt (the clamp), negative means, large counts, random ones"""
    rows = [(0, 0.0, 0.0), (0, 0.6, 0.36), (0, -0.9, 0.81), (3, 2.0, float(f32(1.0) - f32(1e-6))), (3, 2.0, 1.0),
            (3, -2.0, float(np.nextafter(f32(1.0), f32(0)))), (7, 4.0, 2.0), (10, 2.2, 5.5), (8, 2.7, 0.95),
            (799, -310.5, 402.25), (1, 2.0, 2.0), (5, 0.0, 6.0), (2, 1e-3, 1e-9)]
    rng = np.random.RandomState(7)
    for _ in range(40):
        n = int(rng.randint(0, 60))
        v = rng.uniform(-1, 1, n + 1).astype(f32)
        rows.append((n, float(v.sum(dtype=f32)), float((v * v).sum(dtype=f32))))
    return rows


FACTOR_SETTINGS = [(0.85, 0.4, 2.0), (0.5, 0.01, 0.0), (0.999, 2.0, 1000.0), (0.0, 0.4, 2.0)]


def header_lcb(n, w, s, tp, z):
    out = np.zeros(3, f64)
    hs.lib().hs_value_lcb(n, w, s, tp, z, hs.pd(out))
    return out


def test_header_equals_the_restatement_bit_for_bit():
    """mean, sd, lcb and the factor of include/agz_uncertainty.h, as g++ compiles it into the simulator's library and as
    hipcc compiles the host side of libagz.so (agz_value_lcb, agz_puct_variance_factor), against the numpy restatement
    written from include/agz.h, with the square root taken from the library (hs_sqrt) and from its own restatement
    (puct_twin.agz_sqrt)"""
    L = hs.lib()
    clamped = 0
    for n, w, s in stat_rows():
        for tp in (1, -1):
            for z in (0.0, 1.96, 5.0, 100.0):
                got = header_lcb(n, w, s, tp, z)
                for sqrt in (ut.lib_sqrt, pt.agz_sqrt):
                    m, sd, l = ut.child_lcb([n], [w], [s], tp, z, sqrt)
                    want = np.array([m[0], sd[0], l[0]])
                    assert (bits64(got) == bits64(want)).all(), (n, w, s, tp, z, got, want)
                assert ag.value_lcb(n, w, s, tp, z) == tuple(got)
                if z == 0.0:
                    assert got[2] == got[0] * tp
        cnt, mean, var, _ = ut.child_stats([n], [w], [s])
        clamped += bool(f64(f32(s)) / cnt[0] - mean[0] * mean[0] < 0 and var[0] == 0)
        for k, prior, pw in FACTOR_SETTINGS:
            got = L.hs_variance_factor(n, w, s, k, prior, pw)
            for sqrt in (ut.lib_sqrt, pt.agz_sqrt):
                assert bits64(got) == bits64(ut.variance_factor(n, w, s, k, prior, pw, sqrt)), (n, w, s, k, prior, pw)
            assert ag.puct_variance_factor(n, w, s, k, prior, pw) == got
            if k == 0.0:
                assert got == 1.0
    assert clamped >= 2, "rows whose variance is negative before the clamp"


def test_header_against_math_sqrt():
    """The same comparison with math.sqrt (correctly rounded) in the restatement.  agz_sqrt is a Newton iteration that is
    deterministic, not correctly rounded; the margin is what agz_sqrt itself shows against math.sqrt on the very inputs
    of these rows, carried through the operations behind it: sd differs by exactly that; lcb by z times it plus one
    rounding each of the product z * se and of the subtraction; the factor by k / prior times it plus the four roundings
    of the divide, the subtract, the multiply and the add.  Measured on these rows: agz_sqrt differs from math.sqrt on 37
    of the 196 distinct inputs, by 1 ulp at the most."""
    worst, seen, differ = 0.0, set(), 0

    def gap(x):
        nonlocal worst, differ
        x = float(x)
        d = abs(ut.lib_sqrt(x) - math.sqrt(x))
        if x not in seen:
            seen.add(x)
            differ += d > 0
            if x > 0:
                worst = max(worst, d / math.ulp(math.sqrt(x)))
        return d

    for n, w, s in stat_rows():
        cnt, mean, var, _ = ut.child_stats([n], [w], [s])
        for tp in (1, -1):
            for z in (0.0, 1.96, 100.0):
                got = header_lcb(n, w, s, tp, z)
                m, sd, l = ut.child_lcb([n], [w], [s], tp, z, math.sqrt)
                assert bits64(got[0]) == bits64(m[0])
                assert abs(got[1] - sd[0]) <= gap(var[0])
                se = math.sqrt(var[0] / cnt[0])
                assert abs(got[2] - l[0]) <= z * gap(var[0] / cnt[0]) + math.ulp(z * se) + math.ulp(max(abs(got[2]), abs(l[0])))
        for k, prior, pw in FACTOR_SETTINGS:
            got = hs.lib().hs_variance_factor(n, w, s, k, prior, pw)
            want = ut.variance_factor(n, w, s, k, prior, pw, math.sqrt)
            c, mn = f64(f32(1) + f32(n)), f64(f32(w)) / f64(f32(1) + f32(n))
            v = ((((mn * mn) + (f64(prior) * f64(prior))) * f64(pw)) + ((f64(f32(s)) / c) * c)) / (f64(pw) + c) - (mn * mn)
            v = float(v) if v > 0 else 0.0
            assert abs(got - want) <= (k / prior) * gap(v) + 4 * math.ulp(max(abs(got), abs(want), math.sqrt(v) / prior, 1.0))
    print(f"agz_sqrt against math.sqrt: {differ} of {len(seen)} inputs differ, worst {worst} ulp")


# ---------------------------------------------------------------- the moments, one call at a time

def single_tree(N=5, seed=3, game_id=11, two_player=0, to_play=1, **kw):
    sim = hs.Sim(board_size=N, games=1, num_readouts=64, parallel_readouts=8, seed=seed, max_nodes_per_game=256,
                 two_player_mode=two_player, **kw)
    assert sim.set_value_moments(True) == ut.OK
    root = sim.tree_init(0, np.zeros(N * N, np.int8), to_play=to_play)
    sim.L.hs_game_set(sim.h, 0, 0, float(game_id))
    return sim, root


def leaf_feats(sim, leaf, g=0):
    """something for PeakedNet to hash: the leaf's stones by side to move"""
    m, feats = sim.meta(g, leaf), np.zeros((1, 17 * sim.P), f32)
    feats[0, : sim.P] = sim.board(g, leaf) == m.to_play
    feats[0, sim.P: 2 * sim.P] = sim.board(g, leaf) == -m.to_play
    return feats


def test_moments_follow_rule_1_call_by_call():
    """select, virtual loss add and revert, incorporate, a duplicate incorporate, play and re-root, one call at a time
    on the simulator; after every call every live node's S row, every node's own S and the root's S are the dict
    mirror's (uncertainty_twin.MomentMirror: rule 1 in float32, in the engine's order), bit for bit"""
    sim, root = single_tree()
    net = hs.PeakedNet(5)
    mir = ut.MomentMirror(sim)
    mir.init(root)
    mir.check("init")
    ops = dups = plays = 0
    for move in range(3):
        for it in range(26):
            top = sim.game(0).root
            leaves = []
            for _ in range(2 if it % 3 == 1 else 1):        # (two descents before either is incorporated)
                st, leaf = sim.op(hs.TOP_SELECT, node=top)
                assert st == 0
                leaves.append(leaf)
                mir.check(("select", move, it))
            for leaf in leaves:
                m = sim.meta(0, leaf)
                if m.flags & 2:
                    continue                                # a finished leaf: nothing to expand
                assert sim.op(hs.TOP_VLOSS_ADD, node=leaf, up_to=top)[0] == 0
                mir.virtual_loss(leaf, top, +1)
                mir.check(("vloss", move, it))
                pi, v = net(leaf_feats(sim, leaf))
                assert sim.op(hs.TOP_VLOSS_REVERT, node=leaf, up_to=top)[0] == 0
                mir.virtual_loss(leaf, top, -1)
                mir.check(("revert", move, it))
                fresh = not (m.flags & 1)
                assert sim.op(hs.TOP_INCORPORATE, node=leaf, up_to=top, probs=pi[0], value=float(v[0]))[0] == 0
                if fresh:
                    mir.incorporate(leaf, top, v[0])
                else:
                    dups += 1                               # the same leaf again: its visits are reverted, W and S stay
                mir.check(("incorporate", move, it))
                ops += 1
        r = sim.game(0).root
        a = int(np.argmax(sim.row(0, r, 0)))
        child = int(sim.children(0, r)[a])
        assert child >= 0 and sim.row_S(0, r)[a] != 0
        assert sim.op(hs.TOP_PLAY, a=a) == (0, 1)
        mir.reroot(a, child)
        live = set(mir.live())
        mir.rows = {k: v for k, v in mir.rows.items() if k in live}
        n = mir.check(("play", move))
        assert n > 3 and f32(sim.S_(0, child)) == mir.root_S != 0
        plays += 1
    assert ops > 60 and dups > 0 and plays == 3
    sim.close()


# ---------------------------------------------------------------- the LCB pick on hand-made rows

def set_rows(sim, node, N=None, W=None, S=None, P=None, g=0):
    for k, row in ((0, N), (1, W), (2, P)):
        if row is not None:
            sim.row(g, node, k)[:] = np.asarray(row, f32)
    if S is not None:
        sim.row_S(g, node)[:] = np.asarray(S, f32)


def hand_rows(A, entries):
    """rows of A actions, zero but for entries {a: (N, W, S)}"""
    N, W, S = np.zeros(A, f32), np.zeros(A, f32), np.zeros(A, f32)
    for a, (n, w, s) in entries.items():
        N[a], W[a], S[a] = n, w, s
    return N, W, S


@pytest.mark.parametrize("to_play", [1, -1])
def test_lcb_pick_on_hand_made_rows(to_play):
    sim, root = single_tree(two_player=1, to_play=to_play)     # two_player_mode: the arg-max branch at every ply
    off, off_root = single_tree(two_player=1, to_play=to_play)
    A, t = sim.A, float(to_play)
    z, lcb = 2.0, (2.0, 5, 0.5)
    assert sim.set_lcb(*lcb) == ut.OK

    def pick(rows, setting=lcb, key=5):
        assert sim.set_lcb(*setting) == ut.OK               # (restarts the counters)
        set_rows(sim, root, *rows)
        sim.L.hs_game_set(sim.h, 0, 0, float(key))
        st, a = sim.op(hs.TOP_PICK)
        assert st == 0
        return a, sim.uncertainty_counts()[:2]

    # a. the 8-visit child with a tight value beats the 10-visit child with a noisy one
    rows = hand_rows(A, {3: (10, t * 4.4, 9.0), 7: (8, t * 3.6, 1.5), 12: (6, t * 0.7, 3.0), 20: (1, t * 1.9, 1.9)})
    _, _, l = ut.child_lcb(*rows, to_play, z)
    assert rows[0].argmax() == 3 and l[7] > l[3] > l[12] and l[20] > l[7], "the premise: a better bound on fewer visits"
    assert ut.lcb_pick(*rows, to_play, lcb) == 7            # (20 is below min_visits and below the ratio)
    assert pick(rows) == (7, (1, 1))
    m, sd, got = sim.child_lcb(root, z)
    assert (bits64(got) == bits64(l)).all() and (bits64(m) == bits64(ut.child_stats(*rows)[1])).all()
    # b. below min_visits at the top: the arg-max branch as it is, tie draw included
    rows = hand_rows(A, {3: (4, t * 0.4, 3.0), 9: (4, t * 3.9, 3.9), 15: (4, t * 2.0, 2.0), 21: (2, t * 1.9, 1.9)})
    assert rows[0].max() < lcb[1] and ut.lcb_pick(*rows, to_play, lcb) is None
    picks = set()
    for key in range(24):
        a, counts = pick(rows, key=key)
        set_rows(off, off_root, *rows)
        off.L.hs_game_set(off.h, 0, 0, float(key))
        assert off.op(hs.TOP_PICK) == (0, a) and counts == (0, 0), key
        picks.add(a)
    assert picks == {3, 9, 15}, "the tie draw picks each of the tied children"
    # c. the ratio gate: a child with enough visits for min_visits, too few for the ratio, and the best bound
    rows = hand_rows(A, {2: (20, t * 6.0, 8.0), 11: (6, t * 6.5, 6.1), 17: (12, t * 5.0, 4.0)})
    _, _, l = ut.child_lcb(*rows, to_play, z)
    assert l[11] > l[17] > l[2] and rows[0][11] >= lcb[1] and rows[0][11] < lcb[2] * rows[0].max()
    assert pick(rows) == (17, (1, 1)) and ut.lcb_pick(*rows, to_play, lcb) == 17
    assert pick(rows, (z, 5, 0.25)) == (11, (1, 1)) and pick(rows, (z, 5, 0.0)) == (11, (1, 1))
    assert pick(rows, (z, 5, 1.0)) == (2, (1, 0)), "only the most visited child is eligible"
    assert pick(rows, (z, 13, 0.0)) == (2, (1, 0)) and pick(rows, (z, 12, 0.0)) == (17, (1, 1))
    # d. the tie order: equal bounds go to the larger N, then to the lower action; no draw is made
    rows = hand_rows(A, {4: (3, t * 2.0, 1.0), 6: (7, t * 4.0, 2.0), 19: (7, t * 4.0, 2.0), 23: (1, t * 1.0, 0.5)})
    _, _, l = ut.child_lcb(*rows, to_play, z)
    assert l[4] == l[6] == l[19] == l[23] == 0.5, "the premise: four equal bounds (no variance at all)"
    for key in range(8):
        assert pick(rows, (z, 1, 0.0), key=key) == (6, (1, 0))
    rows[0][19] = 6
    rows[1][19], rows[2][19] = t * 3.5, 1.75
    assert ut.child_lcb(*rows, to_play, z)[2][19] == 0.5 and pick(rows, (z, 1, 0.0)) == (6, (1, 0))
    rows = hand_rows(A, {4: (3, t * 2.0, 1.0), 6: (7, t * 4.0, 2.0), 2: (9, t * 1.0, 6.0)})
    assert pick(rows, (z, 1, 0.0)) == (6, (1, 1)), "... and a tie below the most visited child counts as off it"
    # z = 0 is off: the arg-max of the visits
    assert pick(rows, (0.0, 1, 0.0)) == (2, (0, 0))
    sim.close()
    off.close()


# ---------------------------------------------------------------- the variance factor on hand-made statistics

PV = (0.85, 0.4, 2.0)
C_PUCT = 0.96


@pytest.mark.parametrize("setting", [pt.OFF, (1, 0.2, 0.05, 19652.0)], ids=["plain", "fpu_cbase"])
def test_variance_factor_in_the_scores(setting):
    """agz_tree_node_scores (TOP_SCORES) of the root and of a node one level down under hand-made own (n, W_s, S_s)
    equals the restatement: pt.puct_scores with the scale multiplied by the factor"""
    sim, root = single_tree(c_puct=C_PUCT)
    sim.set_puct(*setting)
    assert sim.set_puct_variance(*PV) == ut.OK
    rng = np.random.RandomState(2)
    A = sim.A
    st, child = sim.op(hs.TOP_ADD_CHILD, node=root, a=7)
    assert st == 0 and child > 0
    seen = set()
    for n, w, s in [(0, 0.0, 0.0), (12, 3.5, 6.0), (12, -3.5, 1.1), (40, 30.0, 22.5), (5, 0.5, 5.9), (200, -20.0, 180.0)]:
        N = np.floor(rng.rand(A) * 4).astype(f32)
        W = (rng.uniform(-1, 1, A) * (1 + N)).astype(f32)
        P = rng.dirichlet(np.ones(A)).astype(f32)
        # the root: its own statistics are the slot's
        set_rows(sim, root, N, W, np.abs(W), P)
        sim.L.hs_game_set(sim.h, 0, 2, float(n))
        sim.L.hs_root_set(sim.h, 0, w, s)
        assert (f32(sim.N_(0, root)), f32(sim.W_(0, root)), f32(sim.S_(0, root))) == (f32(n), f32(w), f32(s))
        want = ut.scores(N, W, P, n, w, s, 1, True, C_PUCT, setting, PV)
        assert (bits64(sim.scores(root)) == bits64(want)).all(), ("root", n, w, s)
        plain = pt.puct_scores(N, W, P, n, w, 1, True, C_PUCT, setting)
        factor = ut.variance_factor(n, w, s, *PV)
        seen.add(factor > 1.0)
        assert (plain != want).any() or factor == 1.0
        # one level down: the node's own statistics are its entries of the root's rows
        sim.row(0, root, 0)[7], sim.row(0, root, 1)[7], sim.row_S(0, root)[7] = n, w, s
        set_rows(sim, child, N, W, np.abs(W), P)
        want = ut.scores(N, W, P, n, w, s, -1, False, C_PUCT, setting, PV)
        assert (bits64(sim.scores(child)) == bits64(want)).all(), ("child", n, w, s)
    assert seen == {True, False}, "factors above and below 1"
    assert sim.set_puct_variance(0.0, 0.4, 2.0) == ut.OK            # off: the scores of the PUCT options alone
    assert (bits64(sim.scores(child)) == bits64(pt.puct_scores(N, W, P, n, w, -1, False, C_PUCT, setting))).all()
    sim.close()


def test_variance_factor_in_the_pruned_target(monkeypatch):
    """agz_tree_pruned_pi (pruned_pi, which finds the node's own W and S from its row index) under the variance factor:
    the row of the root and of a node one level down, on the second slot of the simulator, equals selfplay_twin's
    pruned_pi with its scale multiplied by the restated factor of the node's own (n, W, S)"""
    import selfplay_twin as tw
    sim = hs.Sim(board_size=5, games=2, num_readouts=64, seed=3, max_nodes_per_game=64, c_puct=C_PUCT)
    assert sim.set_value_moments(True) == ut.OK and sim.set_puct_variance(*PV) == ut.OK
    g = 1
    root = sim.tree_init(g, np.zeros(25, np.int8))
    st, child = sim.op(hs.TOP_ADD_CHILD, g=g, node=root, a=7)
    assert st == 0 and child > 0
    plain, factor = tw.action_scores, [1.0]

    def scored(N, W, P, tp, rootN, c_puct):
        _, qs, scale = plain(N, W, P, tp, rootN, c_puct)
        scale = scale * f64(factor[0])
        denom = f32(1) + np.asarray(N, f32)
        return qs.astype(f64) + (scale * np.asarray(P, f32).astype(f64)) / denom.astype(f64), qs, scale

    monkeypatch.setattr(tw, "action_scores", scored)
    rng = np.random.RandomState(4)
    A, k, changed = sim.A, 2.0, 0
    for n, w, s in [(30, 3.5, 16.0), (30, -3.5, 1.1), (64, 30.0, 22.5)]:
        N = np.floor(rng.rand(A) * 6).astype(f32)
        N[3] = 12
        W = (rng.uniform(-1, 1, A) * (1 + N)).astype(f32)
        P = rng.dirichlet(np.ones(A)).astype(f32)
        factor[0] = ut.variance_factor(n, w, s, *PV)
        assert factor[0] != 1.0
        set_rows(sim, root, N, W, np.abs(W), P, g=g)
        sim.L.hs_game_set(sim.h, g, 2, float(n))
        sim.L.hs_root_set(sim.h, g, w, s)
        got, ch = sim.pruned_pi(g, root, k)
        want, wch = tw.pruned_pi(N, W, P, 1, n, C_PUCT, k, True)
        assert (bits32(got) == bits32(want)).all() and ch == wch, ("root", n, w, s)
        factor[0] = 1.0
        changed += not (bits32(got) == bits32(tw.pruned_pi(N, W, P, 1, n, C_PUCT, k, True)[0])).all()
        factor[0] = ut.variance_factor(n, w, s, *PV)
        sim.row(g, root, 0)[7], sim.row(g, root, 1)[7], sim.row_S(g, root)[7] = n, w, s
        set_rows(sim, child, N, W, np.abs(W), P, g=g)
        got, ch = sim.pruned_pi(g, child, k)
        want, wch = tw.pruned_pi(N, W, P, -1, n, C_PUCT, k, True)
        assert (bits32(got) == bits32(want)).all() and ch == wch, ("child", n, w, s)
    assert changed > 0, "the factor changed a pruned row"
    sim.close()


def test_factor_counters_on_a_tree_searched_descent_by_descent():
    """out[2] and out[3] against a Python tally: after every select_leaf the levels of its path that were scored (every
    expanded node of it but one left by the pass-first rule) are counted with the factor of the node's own (n, W, S) as
    the descent saw them -- n after the descent's own visit, W and S untouched by it"""
    sim, root = single_tree()
    assert sim.set_puct_variance(*PV) == ut.OK
    net = hs.PeakedNet(5)
    levels = raised = 0
    for it in range(80):
        st, leaf = sim.op(hs.TOP_SELECT, node=root)
        assert st == 0
        chain = ut.MomentMirror(sim).chain(leaf)[::-1]
        for x, nxt in zip(chain, chain[1:]):
            m, nm = sim.meta(0, x), sim.meta(0, nxt)
            ps = sim.A - 1
            if m.last_move == ps and nm.fmove == ps and sim.row(0, x, 0)[ps] == 1:
                continue                                    # the pass-first rule: nothing was scored
            levels += 1
            raised += ut.variance_factor(sim.N_(0, x), sim.W_(0, x), sim.S_(0, x), *PV) > 1.0
        m = sim.meta(0, leaf)
        if m.flags & 2:
            continue
        pi, v = net(leaf_feats(sim, leaf))
        assert sim.op(hs.TOP_INCORPORATE, node=leaf, up_to=root, probs=pi[0], value=float(v[0]))[0] == 0
    print("levels", levels, "raised", raised)
    assert sim.uncertainty_counts() == (0, 0, levels, raised) and 0 < raised < levels
    sim.close()


# ---------------------------------------------------------------- games

GAMES, SLOTS, R, SEED = 6, 3, 24, 4
LCB, PVG = (5.0, 3, 0.15), (0.85, 0.4, 2.0)


def tally_pick(sim, g, lcb, tally):
    """what the move phase of slot g is about to do under the LCB rule, from the simulator's rows"""
    G = sim.game(g)
    m = sim.meta(g, G.root)
    qp = f32(f32(G.rootW) / (f32(1) + f32(G.rootN))) * f32(m.to_play)
    if float(qp) < G.resign_threshold:
        return None
    if m.n < sim.tau:
        return None                                         # the soft pick
    N, W, S = sim.row(g, G.root, 0), sim.row(g, G.root, 1), sim.row_S(g, G.root)
    a = ut.lcb_pick(N, W, S, m.to_play, lcb)
    if a is None:
        return None
    tally[0] += 1
    tally[1] += bool(N[a] != N.max())
    return a


def play_games(lcb=None, pv=None, moments=None, tally=None):
    sim = hs.Sim(board_size=5, games=SLOTS, num_readouts=R, seed=SEED, record_capacity_games=GAMES + 8)
    gpu_options.configure(sim, dict(lcb=lcb, pv=pv, moments=moments))
    net = hs.PeakedNet(5)
    sim.start(GAMES)
    expect, thresholds = {}, {}
    for _ in range(40000):
        for g in range(SLOTS):
            G = sim.game(g)
            if G.phase == G_SEARCH:
                thresholds[int(G.game_id)] = G.resign_threshold      # (the game's resign coin: -1 where it fell on "never")
        if tally is not None:
            for g in range(SLOTS):
                G = sim.game(g)
                if G.phase == G_SEARCH and not G.rootN < G.target:
                    a = tally_pick(sim, g, lcb, tally)
                    if a is not None:
                        expect[(int(G.game_id), int(G.nqs))] = a
        sim.step(net)
        if sim.L.hs_records_count(sim.h) >= GAMES:
            break
    recs, cnt, counts = sim.records(), sim.all_counters(), sim.uncertainty_counts()
    sim.close()
    assert len(recs) == GAMES and cnt["CT_POOL_EXHAUSTED"] == 0
    for (gid, k), a in expect.items():
        r = [x for x in recs if x["game_id"] == gid][0]
        assert r["moves"][k] == a, (gid, k)
    return recs, cnt, counts, thresholds


def same_records(a, b):
    return len(a) == len(b) and all(
        x["game_id"] == y["game_id"] and x["num_moves"] == y["num_moves"] and (x["moves"] == y["moves"]).all() and
        x["result"] == y["result"] and x["was_resign"] == y["was_resign"] and (bits32(x["pis"]) == bits32(y["pis"])).all() and
        (bits32(x["qs"]) == bits32(y["qs"])).all() and f32(x["final_score"]) == f32(y["final_score"]) for x, y in zip(a, b))


def test_moments_alone_change_nothing_and_the_rules_change_the_games():
    off = play_games()
    mom = play_games(moments=True)
    assert same_records(off[0], mom[0]) and off[1] == mom[1], "records and every counter of the enum"
    assert off[2] == mom[2] == (0, 0, 0, 0)
    tally = [0, 0]
    on = play_games(LCB, PVG, tally=tally)
    print("counters", on[2], "tally", tally)
    assert not same_records(off[0], on[0]), "the rules changed no game"
    assert on[2][:2] == tuple(tally)
    # all four counters: the same games again call by call on a single tree, every select phase and every pick predicted
    # from the rows before the simulator runs it -- the same moves, the same counters, and the Python tallies equal them
    sim = hs.Sim(board_size=5, games=1, num_readouts=R, parallel_readouts=8, seed=SEED, max_nodes_per_game=2048)
    gpu_options.configure(sim, dict(lcb=LCB, pv=PVG))
    tally = [0] * 7
    for r in on[0]:
        moves = game_call_by_call(sim, hs.PeakedNet(5), int(r["game_id"]), R, 8, LCB, PVG, SEED, tally,
                                  resign_threshold=on[3][int(r["game_id"])], c_puct=0.96)
        assert moves == [int(a) for a in r["moves"]], r["game_id"]
    counts = sim.uncertainty_counts()
    sim.close()
    print("call by call: counters", counts, "tally", tally)
    assert on[2] == counts == tuple(tally[:4]), "all four counters equal the tallies of a Python loop over the rows"
    assert tally[4] > 100 and tally[5] >= 1, "descents with visits in flight, finished leaves backed up inside a phase"
    assert on[2][1] >= 1 and on[2][3] >= 1, "the condition on this set: a move off the most visited child, a raised scale"
    assert on[2][2] > on[2][3]
    # each rule alone: the other's counters stay at zero
    only_lcb = play_games(LCB, None)[2]
    only_pv = play_games(None, PVG)[2]
    assert only_lcb[0] > 0 and only_lcb[2:] == (0, 0) and only_pv[:2] == (0, 0) and only_pv[2] > 0


def game_call_by_call(sim, net, game_id, R, par, lcb, pv, seed, tally, resign_threshold=None, c_puct=None):
    """One self-play game on slot 0 of `sim` through the single-tree calls, as selfplay.jl plays it: the root expanded
    alone, then per move noise, select phases of up to `par` leaves with their virtual losses in flight and finished
    leaves backed up in between, incorporate, the resign check, pick, play and re-root.  Every select phase is predicted
    from the rows first (uncertainty_twin.predict_phase) and held to the prediction; tally = [LCB picks, those off the
    most visited child, levels scored under a factor, those with factor > 1, descents made with visits in flight,
    finished leaves backed up, phases].  -> the moves"""
    root = sim.tree_init(0, np.zeros(sim.P, np.int8))
    sim.L.hs_game_set(sim.h, 0, 0, float(game_id))
    if resign_threshold is not None:                        # the game's own, as its resign coin set it
        sim.L.hs_game_set(sim.h, 0, 3, float(resign_threshold))
    c_puct = C_PUCT if c_puct is None else c_puct
    st, leaf = sim.op(hs.TOP_SELECT, node=root)
    assert st == 0 and leaf == root
    feats = np.zeros((1, 17 * sim.P), f32)                  # the features of the empty board, Black to play
    feats[0, 16 * sim.P:] = 1.0
    pi, v = net(feats)
    assert sim.op(hs.TOP_INCORPORATE, node=root, up_to=root, probs=pi[0], value=float(v[0]))[0] == 0
    moves = []
    while True:
        root = sim.game(0).root
        assert sim.op(hs.TOP_NOISE, node=root)[0] == 0
        target = sim.game(0).rootN + R
        while sim.game(0).rootN < target:
            want, counts, sh = ut.predict_phase(sim, par, c_puct, seed, pv)
            st, n = sim.op(hs.TOP_SEARCH_SELECT, par=par)
            assert st == 0 and n == len(want)
            ut.assert_phase(sim, want, sh)
            for k, key in ((2, "levels"), (3, "raised"), (4, "in_flight"), (5, "terminal")):
                tally[k] += counts[key]
            tally[6] += 1
            if n:
                feats = np.zeros((n, 17 * sim.P), f32)
                sim.L.hs_tree_leaf_features(sim.h, 0, hs.pf(feats))
                pi, v = net(feats)
                sim.L.hs_set_batch_outputs(sim.h, hs.pf(pi), hs.pf(v), n)
            assert sim.op(hs.TOP_SEARCH_POST)[0] == 0
        if sim.op(hs.TOP_RESIGN)[1]:
            break
        want = tally_pick(sim, 0, lcb, tally)
        st, a = sim.op(hs.TOP_PICK)
        assert st == 0 and (want is None or a == want)
        assert sim.op(hs.TOP_PLAY, a=a) == (0, 1)
        moves.append(a)
        m = sim.meta(0, sim.game(0).root)
        if (m.flags & 2) or m.n >= sim.mgl:
            break
    return moves


# ---------------------------------------------------------------- refusals

REFUSED = {
    "hs_set_value_moments": ((2,), (-1,), (0,)),                       # (0: a rule is on)
    "hs_set_lcb": ((NAN, 1, 0.0), (-1e-9, 1, 0.0), (100.001, 1, 0.0), (1.0, 0, 0.0), (1.0, -3, 0.0), (1.0, 1, -1e-9),
                   (1.0, 1, 1.000001), (1.0, 1, NAN)),
    "hs_set_puct_variance": ((NAN, 0.4, 2.0), (-1e-9, 0.4, 2.0), (1.0, 0.4, 2.0), (0.5, 0.00999, 2.0), (0.5, 2.001, 2.0),
                             (0.5, NAN, 2.0), (0.5, 0.4, -1e-9), (0.5, 0.4, 1000.001), (0.5, 0.4, NAN)),
}
TAKEN = (("hs_set_lcb", (100.0, 1, 1.0)), ("hs_set_lcb", (0.5, 2000000, 0.0)), ("hs_set_puct_variance", (0.999999, 0.01, 0.0)),
         ("hs_set_puct_variance", (0.1, 2.0, 1000.0)))


def test_refusals_keep_the_setting():
    """the argument checks the engine and the simulator share (agz_state.h): every refusal leaves the setting in force.
    (Games in flight and a pending select phase are states of the engine alone: tests/test_gpu_uncertainty.py.)"""
    sim = hs.Sim(board_size=5, games=2, num_readouts=8, max_nodes_per_game=16, arena_mode=1)    # an arena takes all three
    # either rule while moments are off
    assert sim.set_lcb(1.0, 1, 0.0) == ut.BAD_ARGUMENT and sim.set_puct_variance(0.5, 0.4, 2.0) == ut.BAD_ARGUMENT
    assert sim.set_lcb(0.0, 1, 0.0) == ut.OK and sim.set_puct_variance(0.0, 0.4, 2.0) == ut.OK      # off is taken
    assert sim.uncertainty_setting() == (0, 0.0, 0, 0.0, 0.0, 0.0, 0.0)
    assert sim.set_value_moments(True) == ut.OK
    assert sim.set_lcb(2.5, 4, 0.25) == ut.OK and sim.set_puct_variance(0.7, 0.5, 3.0) == ut.OK
    kept = (1, 2.5, 4, 0.25, 0.7, 0.5, 3.0)
    for fn, cases in REFUSED.items():
        for args in cases:
            assert getattr(sim.L, fn)(sim.h, *args) == ut.BAD_ARGUMENT, (fn, args)
            assert sim.uncertainty_setting() == kept, (fn, args)
    for fn, args in TAKEN:                                  # the bounds themselves are in range
        assert getattr(sim.L, fn)(sim.h, *args) == ut.OK, (fn, args)
    # moments go off once both rules are off, and come back on the arrays made the first time
    assert sim.set_lcb(0.0, 1, 0.0) == ut.OK and sim.set_value_moments(False) == ut.BAD_ARGUMENT
    assert sim.set_puct_variance(0.0, 0.4, 2.0) == ut.OK and sim.set_value_moments(False) == ut.OK
    assert sim.uncertainty_setting()[0] == 0 and sim.set_value_moments(True) == ut.OK
    sim.close()
    # the host-only calls of the library refuse a null output
    L = ag.load()
    d = C.c_double()
    assert L.agz_value_lcb(1.0, 0.5, 0.5, 1, 1.0, None, C.byref(d), C.byref(d)) == ag._lib.BAD_ARGUMENT
    assert L.agz_puct_variance_factor(1.0, 0.5, 0.5, 0.5, 0.4, 2.0, None) == ag._lib.BAD_ARGUMENT
    assert L.agz_search_set_value_moments(None, 1) == ag._lib.BAD_ARGUMENT


# ---------------------------------------------------------------- the rate tool

def test_recorded_windows_give_the_recorded_summary():
    """tools/uncertainty_rate.py without a device: the windows recorded in profiles/uncertainty_rate.json give, through
    measure(), the summary and the measured block recorded beside them (keys and rounding, not the device)"""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import uncertainty_rate as ur
    rec = json.load(open(os.path.join(root, "profiles", "uncertainty_rate.json")))
    assert set(rec["windows"]) == set(ur.MODES) and len({len(w) for w in rec["windows"].values()}) == 1
    res, measured = ur.measure(rec["windows"])
    assert res == rec["summary"] and measured == rec["measured"]
    assert all(w["counts_per_step"] == [0.0] * 4 for m in ("off", "moments") for w in rec["windows"][m])
    assert all(w["counts_per_step"][0] > 0 and w["counts_per_step"][2] > 0 for w in rec["windows"]["on"])
    ab = json.load(open(os.path.join(root, "profiles", "uncertainty_bench_ab.json")))
    assert ab["dump_outputs_byte_equal_to_parent"] is True and ab["within_parent_spread"] is True
    assert abs(ab["this_minus_parent_median"]) <= ab["parent"]["spread"]


# ---------------------------------------------------------------- sanitizers

def test_sanitizer_build_plays_a_game():
    """the `uncertainty` part of the stand-alone sanitizer program (tests/hostsim/hostsim_sanitize.cpp, built once per
    process by test_explore.run_sanitizer_part): 5x5 games with all three options on, the rows of every root read once per
    step.  A check of memory and undefined behaviour, not of results."""
    run_sanitizer_part("uncertainty")

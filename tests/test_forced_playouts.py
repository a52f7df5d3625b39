"""Forced playouts and policy target pruning (agz_selfplay_set_forced_playouts) on the host simulator.
tests/selfplay_twin.py restates the descent and the pruned target; with k = 0 the restated descent is held to the
oracle's own before anything rests on it.  Then: the worked example of the rules on a single tree, whole games against the twin bit
for bit, the off path against the cap simulator byte for byte, and the properties of the pruned rows.  CPU only."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import alphago_jl_amd as ag
import hs
import orc
import selfplay_twin as tw
from test_hostsim_selfplay import OracleNet, bits_equal, oracle_game
from test_playout_cap import run_cap_sim

L = orc.lib()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_RESIGN = dict(resign_threshold=-2.0, resign_disable_fraction=0.0)


# ---------------------------------------------------------------- 1. the restated descent is the oracle's

@pytest.mark.parametrize("N,R,games,r,p", [(5, 16, 3, 4, 0.4), (5, 16, 2, 4, 1.0), (9, 16, 1, 4, 0.3)])
def test_twin_at_k_0_is_the_cap_twin(N, R, games, r, p):
    """forced = (0, .) plays the whole game on the restated descent under no rule; without the option every descent is
    or_select_leaf.  p < 1: the cap on; p = 1: every search full, which is the cap off (the twin's r = 0 form as well),
    and there the game from the empty board is or_selfplay_ex's, the C loop's, too"""
    net = OracleNet(N, 1, seed=0)
    starts = tw.random_starts(N, (4, 7, 1), seed=0)
    for gid in range(games):
        st = starts[gid % 3] if gid % 2 else None
        want = tw.twin_selfplay(N, net.cb, R, 3, gid, st, -0.1, 0.0, cap=(r, p))
        forms = [(r, p)] + ([(0, 1.0)] if p == 1.0 else [])
        for rr, pp in forms:
            got = tw.twin_selfplay(N, net.cb, R, 3, gid, st, -0.1, 0.0, cap=(rr, pp), forced=(0.0, True))
            assert got["num_moves"] == want["num_moves"] and (got["moves"] == want["moves"]).all()
            assert got["result"] == want["result"] and got["was_resign"] == want["was_resign"]
            assert got["evals"] == want["evals"] and (got["full"] == want["full"]).all()
            assert (got["searched_full"] == want["searched_full"]).all()
            assert bits_equal(got["pis"], want["pis"]) and bits_equal(got["qs"], want["qs"])
            assert bits_equal(got["raw_pis"], want["pis"])
            assert got["forced_sel"] == 0 and not got["pruned_rows"].any()
            if pp == 1.0 and st is None:
                o = oracle_game(N, net, R, 3, gid, -0.1, 0.0)
                assert got["full"].all() and got["searched_full"].all()
                assert got["num_moves"] == o["num_moves"] and (got["moves"] == o["moves"][: got["num_moves"]]).all()
                assert got["result"] == o["result"] and got["evals"] == o["evals"]
                assert got["was_resign"] == (o["result_string"] in (b"B+R", b"W+R"))
                assert bits_equal(got["pis"], o["pis"]) and bits_equal(got["qs"], o["qs"])
                assert bits_equal(got["raw_pis"], o["pis"])
    net.close()


# ---------------------------------------------------------------- 2. the worked example on a single tree

EX_N = [60, 20, 12, 1, 6]
EX_P = [0.50, 0.20, 0.10, 0.05, 0.15]
EX_W = [30.5, 0, 6.25, 0, 3.5]
EX_TABLE = [60, 13.707, 8.882, 0, 6]          # N' as the rules' table prints it


def example_tree(k, rows=(EX_N, EX_W, EX_P), at=(0, 1, 2, 3, 4), rootN=99.0, n=None, last_move=-1, N=5, prune=True):
    """a single tree on the simulator whose expanded root has the given child rows at actions `at` (zero elsewhere),
    c_puct = 1, N(root) = rootN, position.n = n (default: past tau, no squash); the engine's setting is (k, prune)"""
    sim = hs.Sim(board_size=N, games=1, num_readouts=8, seed=1, c_puct=1.0)
    sim.set_forced_playouts(k, prune)
    root = sim.tree_init(0, np.zeros(N * N, np.int8), n=sim.tau + 1 if n is None else n, last_move=last_move)
    st, leaf = sim.op(hs.TOP_SELECT, node=root)
    assert st == 0 and leaf == root
    st, _ = sim.op(hs.TOP_INCORPORATE, node=root, up_to=root, probs=np.full(sim.A, 1.0 / sim.A, np.float32), value=0.0)
    assert st == 0
    for field, vals in enumerate(rows):
        row = sim.row(0, root, field)
        row[:] = 0
        row[list(at)] = np.asarray(vals, np.float32)
    sim.L.hs_node_set_N(sim.h, 0, root, rootN)
    return sim, root


def rows_of(sim, root):
    return [sim.row(0, root, f).copy() for f in range(3)]


def descend(sim, root):
    """one agz_tree_select_leaf from the root -> the action picked at the root level"""
    st, leaf = sim.op(hs.TOP_SELECT, node=root)
    assert st == 0
    a = np.flatnonzero(sim.children(0, root) == leaf)
    assert len(a) == 1
    return int(a[0])


def table_visits():
    """N' of the worked example from the rules, in plain float64"""
    T, scale, k = 99.0, 10.0, 2.0
    s_star = EX_W[0] / (1 + EX_N[0]) + scale * EX_P[0] / (1 + EX_N[0])
    out = [float(EX_N[0])]
    for n, p, w in list(zip(EX_N, EX_P, EX_W))[1:]:
        gap = s_star - w / (1 + n)
        n_min = n if gap <= 0 else scale * p / gap - 1
        m = min(n, max(n - math.sqrt(k * p * T), n_min, 0.0))
        out.append(0.0 if (m < n and m <= 1) else m)
    return out, s_star


def test_example_forced_pick_and_k_0_pick():
    # N(root) = 98: the descent's own increment makes it 99, scale = 10 -- the example's numbers
    sim, root = example_tree(2.0, rootN=98.0)
    assert sim.forced_counts() == (0, 0)
    assert descend(sim, root) == 3                      # 1 < 2 * 0.05 * 99: a3 is under-forced, alone
    assert sim.N_(0, root) == 99.0
    assert sim.forced_counts() == (1, 0)
    # the rule reads the rows as they are now: a3 has N = 1 still (the leaf's own N is in this row: 2 after the visit)
    assert sim.row(0, root, 0)[3] == 2.0
    sim.close()
    sim, root = example_tree(0.0, rootN=98.0)
    score, _, scale = tw.action_scores(EX_N, EX_W, EX_P, 1, 99.0, 1.0)
    assert scale == 10.0 and abs(score[0] - 0.58197) < 5e-6
    best = int(np.argmax(score))
    assert best == 4                                    # the example: a4's score is above S*
    assert descend(sim, root) == best
    assert sim.forced_counts() == (0, 0)
    sim.close()
    # the twin's descent rule on the same rows
    uf = tw.under_forced(2.0, EX_N, EX_P, 99.0)
    assert list(uf) == [False, False, False, True, False]


def test_example_descent_from_a_child_does_not_force():
    """agz_tree_select_leaf from a node that is not the root is a depth-0 level of another kind: never forced"""
    sim, root = example_tree(2.0, rootN=98.0)
    a = descend(sim, root)
    assert a == 3
    child = int(sim.children(0, root)[3])
    st, _ = sim.op(hs.TOP_INCORPORATE, node=child, up_to=root, probs=np.full(sim.A, 1.0 / sim.A, np.float32), value=0.0)
    assert st == 0
    for field, vals in enumerate((EX_N, EX_W, EX_P)):
        row = sim.row(0, child, field)
        row[:] = 0
        row[:5] = np.asarray(vals, np.float32)
    before = sim.forced_counts()
    st, leaf = sim.op(hs.TOP_SELECT, node=child)
    assert st == 0
    pick = int(np.flatnonzero(sim.children(0, child) == leaf)[0])
    assert pick != 3 and sim.forced_counts() == before
    sim.close()


def test_example_pass_hack_keeps_its_precedence():
    P = 25
    sim, root = example_tree(2.0, rootN=98.0, last_move=P)
    assert sim.row(0, root, 0)[P] == 0.0
    assert descend(sim, root) == P                      # mcts.jl:119-126 first, although a3 is under-forced
    assert sim.forced_counts() == (0, 0)
    assert descend(sim, root) == 3                      # the pass has a visit now: the forced rule decides
    assert sim.forced_counts() == (1, 0)
    sim.close()


def test_example_pruned_row():
    sim, root = example_tree(0.0)                       # agz_tree_pruned_pi does not look at the setting
    got, changed = sim.pruned_pi(0, root, 2.0)
    want, wch = tw.pruned_pi(*rows_of(sim, root), 1, 99.0, 1.0, 2.0, False)
    assert changed and wch and bits_equal(got, want)
    visits, s_star = table_visits()
    assert abs(s_star - 0.58197) < 5e-6
    for v, t in zip(visits, EX_TABLE):
        assert abs(v - t) < 6e-4, (v, t)                # the table prints 3-4 digits
    row = np.array(visits) / sum(visits)
    assert np.abs(got[:5].astype(np.float64) - row).max() < 1e-6
    assert (got[5:] == 0).all() and got[3] == 0.0
    assert abs(float(got.astype(np.float64).sum()) - 1.0) < 1e-6
    # k = 0: nothing to take out -- children_as_pi's row, bit for bit
    plain, ch0 = sim.pruned_pi(0, root, 0.0)
    cn = sim.row(0, root, 0)
    assert not ch0 and bits_equal(plain, cn / np.float32(cn.sum()))
    sim.close()


def test_example_pruned_row_squashed():
    sim, root = example_tree(0.0, n=0)                  # position.n = 0 <= tau: the squash
    assert sim.meta(0, root).n <= sim.tau
    got, changed = sim.pruned_pi(0, root, 2.0)
    want, _ = tw.pruned_pi(*rows_of(sim, root), 1, 99.0, 1.0, 2.0, True)
    assert changed and bits_equal(got, want)
    visits, _ = table_visits()
    sq = np.array([v ** 0.98 for v in visits])
    assert np.abs(got[:5].astype(np.float64) - sq / sq.sum()).max() < 1e-6
    plain, ch0 = sim.pruned_pi(0, root, 0.0)
    cn = sim.row(0, root, 0).astype(np.float64)
    # children_as_pi with the squash, from the oracle's own pow
    pw = np.array([tw.L.or_det_pow(float(x), 0.98) for x in cn])
    s = 0.0
    for x in pw:
        s += x
    assert not ch0 and bits_equal(plain, (pw / s).astype(np.float32))
    sim.close()


def test_example_tied_most_visited_child():
    """a0 and a1 tie on visits: c* is a0, the lowest index, so a1 is pruned against a0's score"""
    Nv, Wv, Pv = [30, 30, 12, 1, 6], [15.5, 3.0, 6.25, 0, 3.5], [0.40, 0.30, 0.10, 0.05, 0.15]
    for at in ((0, 1, 2, 3, 4), (3, 7, 2, 9, 25)):      # ... and away from action 0, the pass among the children
        sim, root = example_tree(0.0, rows=(Nv, Wv, Pv), at=at, rootN=79.0)
        got, changed = sim.pruned_pi(0, root, 2.0)
        Nr, Wr, Pr = rows_of(sim, root)
        want, _ = tw.pruned_pi(Nr, Wr, Pr, 1, 79.0, 1.0, 2.0, False)
        assert changed and bits_equal(got, want)
        vis = tw.pruned_visits(Nr, Wr, Pr, 1, 79.0, 1.0, 2.0)
        cs = min(a for a in at if Nr[a] == 30)
        other = max(a for a in at if Nr[a] == 30)
        assert vis[cs] == 30.0 and vis[other] < 30.0
        assert got[cs] > Nr[cs] / Nr.sum()
        sim.close()


# ---------------------------------------------------------------- 3. whole games against the twin

def run_forced_sim(N, net, R, cap, k, prune, seed, games, slots, starts=None, reset=False, max_steps=400000, **cfg):
    sim = hs.Sim(board_size=N, games=slots, num_readouts=R, seed=seed, game_id_base=0, game_id_stride=1,
                 record_capacity_games=games + 8, **cfg)
    if starts:
        sim.set_starts(starts)
    if cap:
        sim.set_playout_cap(*cap)
    if k is not None:
        sim.set_forced_playouts(k, prune)
    if reset:
        sim.set_forced_playouts(0.0, False)
    sim.start(games)
    steps = 0
    while sim.counters()["finished"] < games and steps < max_steps:
        sim.step(net.on_feats)
        steps += 1
    out = sim.records(), sim.counters(), sim.all_counters()
    sim.close()
    return out


# N, R, k, seed, games, slots: seeds chosen so that the twin alone meets the condition asserted below
GAME_SETS = [
    (5, 16, 2.0, 3, 4, 3),
    (5, 16, 16.0, 3, 4, 2),
    (9, 32, 2.0, 5, 2, 2),
    (9, 32, 16.0, 5, 2, 2),
]
CAP = (8, 0.5)
THR = -0.1
_games = {}


def game_set(i):
    """(records of the simulator, twins, all counters) of GAME_SETS[i], computed once"""
    if i not in _games:
        N, R, k, seed, games, slots = GAME_SETS[i]
        net = OracleNet(N, 1, seed=0)
        starts = tw.random_starts(N, (4, 7, 1), seed=0)
        recs, cnt, allc = run_forced_sim(N, net, R, CAP, k, True, seed, games, slots, starts=starts,
                                         resign_threshold=THR, resign_disable_fraction=0.0)
        twins = [tw.twin_selfplay(N, net.cb, R, seed, int(r["game_id"]), starts[int(r["game_id"]) % len(starts)], THR, 0.0,
                                  cap=CAP, forced=(k, True)) for r in recs]
        net.close()
        _games[i] = (recs, twins, cnt, allc)
    return _games[i]


@pytest.mark.parametrize("i", range(len(GAME_SETS)))
def test_sim_games_equal_the_twin(i):
    N, R, k, seed, games, slots = GAME_SETS[i]
    recs, twins, cnt, allc = game_set(i)
    assert len(recs) == games and cnt["pool_exhausted"] == 0
    for o in twins:       # the condition of the set, on the twin alone
        assert o["forced_sel"] >= 1, "a game of the set has no forced selection"
        assert o["pruned_rows"].any(), "a game of the set has no row that pruning changed"
    for rec, o in zip(recs, twins):
        gid = int(rec["game_id"])
        assert rec["num_moves"] == o["num_moves"] and (rec["moves"] == o["moves"]).all(), gid
        assert rec["result"] == o["result"] and rec["was_resign"] == o["was_resign"], gid
        assert np.float32(rec["final_score"]) == np.float32(o["final_score"]), gid
        assert bits_equal(rec["qs"], o["qs"]), gid
        full = o["full"]
        got = np.ascontiguousarray(rec["pis"], np.float32).reshape(-1, N * N + 1)
        assert (got[~full].view(np.uint32) == 0).all(), (gid, "a fast row is not all zero")
        assert bits_equal(got[full], o["pis"][full]), gid
        assert rec["short_searches"] == 0
    assert cnt["evals"] == sum(o["evals"] for o in twins)
    assert cnt["positions"] == sum(o["num_moves"] for o in twins)
    assert allc["CT_FORCED_SEL"] == sum(o["forced_sel"] for o in twins)
    assert allc["CT_PRUNED_ROWS"] == sum(int(o["pruned_rows"].sum()) for o in twins)
    assert allc["CT_CAP_FULL"] == sum(int(o["full"].sum()) for o in twins)
    assert allc["CT_CAP_FAST"] == sum(int((~o["full"]).sum()) for o in twins)
    assert {o["was_resign"] for o in twins} == {0, 1} or N == 9


def test_forcing_without_pruning_records_the_raw_rows():
    """prune = 0: the descent is forced, the target is children_as_pi of the raw visits"""
    N, R, k, seed, games, slots = GAME_SETS[0]
    net = OracleNet(N, 1, seed=0)
    starts = tw.random_starts(N, (4, 7, 1), seed=0)
    recs, cnt, allc = run_forced_sim(N, net, R, CAP, k, False, seed, 2, 2, starts=starts, resign_threshold=THR,
                                     resign_disable_fraction=0.0)
    for rec in recs:
        gid = int(rec["game_id"])
        o = tw.twin_selfplay(N, net.cb, R, seed, gid, starts[gid % 3], THR, 0.0, cap=CAP, forced=(k, False))
        assert (rec["moves"] == o["moves"]).all() and bits_equal(rec["pis"], o["raw_pis"]) and bits_equal(rec["qs"], o["qs"])
        assert o["forced_sel"] >= 1 and not o["pruned_rows"].any()
    assert allc["CT_PRUNED_ROWS"] == 0 and allc["CT_FORCED_SEL"] >= 2
    net.close()


# ---------------------------------------------------------------- 4. off is the cap simulator, byte for byte

@pytest.mark.parametrize("cap", [None, CAP])
def test_off_and_reset_are_the_cap_simulator(cap):
    N, R, seed, games, slots = 5, 16, 3, 4, 3
    net = OracleNet(N, 1, seed=0)
    starts = tw.random_starts(N, (4, 7, 1), seed=0)
    kw = dict(resign_threshold=THR, resign_disable_fraction=0.0)
    r, p = cap if cap else (0, 1.0)
    want, wct, wcaps = run_cap_sim(N, net, R, r, p, seed, games, slots, starts=starts, **kw)
    ran = [run_forced_sim(N, net, R, cap, None, False, seed, games, slots, starts=starts, **kw),
           run_forced_sim(N, net, R, cap, 0.0, False, seed, games, slots, starts=starts, **kw),
           run_forced_sim(N, net, R, cap, 2.0, True, seed, games, slots, starts=starts, reset=True, **kw)]
    for got, gct, allc in ran:
        assert len(got) == len(want) == games
        for x, y in zip(got, want):
            assert sorted(x) == sorted(y)
            for key in x:
                a, b = np.asarray(x[key]), np.asarray(y[key])
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
        assert gct == wct
        assert (allc["CT_CAP_FULL"], allc["CT_CAP_FAST"]) == wcaps
        assert allc["CT_FORCED_SEL"] == 0 and allc["CT_PRUNED_ROWS"] == 0
        assert allc == ran[0][2]
    net.close()


# ---------------------------------------------------------------- 5. the pruned rows

@pytest.mark.parametrize("i", range(len(GAME_SETS)))
def test_row_properties(i):
    recs, twins, _, _ = game_set(i)
    nchanged = 0
    for rec, o in zip(recs, twins):
        full = o["full"]
        got = np.ascontiguousarray(rec["pis"], np.float32).reshape(len(full), -1)[full]
        raw = o["raw_pis"][full]
        assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() < 1e-6
        assert (got[raw == 0] == 0).all(), "mass where the search never went"
        cs = raw.argmax(axis=1)                      # the most visited child, lowest index: children_as_pi is monotone
        rows = np.arange(len(got))
        assert (got[rows, cs] >= raw[rows, cs]).all(), "c* lost mass"
        ch = o["pruned_rows"][full]
        assert ((got != raw).any(axis=1) <= ch).all()
        assert (got[ch, cs[ch]] > raw[ch, cs[ch]]).all(), "a changed row gives c* nothing"
        nchanged += int(ch.sum())
    assert nchanged >= len(recs)


# ---------------------------------------------------------------- the ABI

NEW_CALLS = ("agz_selfplay_set_forced_playouts", "agz_selfplay_forced_counts", "agz_tree_pruned_pi")


def test_header_declares_the_new_calls_and_keeps_the_abi():
    hdr = open(os.path.join(ROOT, "include", "agz.h")).read()
    assert re.search(r"#define AGZ_VERSION 103\b", hdr)
    for name in NEW_CALLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert C.sizeof(ag._lib.Config) == 112 and C.sizeof(ag._lib.GameHeader) == 32 and C.sizeof(hs.GameState) == 112
    lib = ag.load()
    assert lib.agz_version() == 103
    for name in NEW_CALLS:
        assert name in lib._agz_signatures and hasattr(lib, name)
    for who in ("selfplay", "train"):
        sig = inspect.signature(getattr(ag, who)).parameters
        assert "forced_playouts" in sig and sig["prune_targets"].default is True, who
    for m in ("set_forced_playouts", "forced_counts", "tree_pruned_pi"):
        assert hasattr(ag.Engine, m), m
    from alphago_jl_amd.api import NodeView
    assert hasattr(NodeView, "pruned_pi")
    jl = open(os.path.join(ROOT, "alphago.jl_amd", "julia", "AlphaGoMI.jl")).read()
    for name in NEW_CALLS:
        assert ":%s" % name in jl, name
    names = hs.counter_names()
    assert names[-2:] == ["CT_FORCED_SEL", "CT_PRUNED_ROWS"] and names.index("CT_PEAK_NODES") == len(hs.CT) - 1

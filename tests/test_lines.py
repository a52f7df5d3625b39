"""Analysis lines (top-K candidates with principal variations), CPU side: the agz_line layout (C / ctypes / Julia), the
entry points exported, bound and called, the argument checks of analyze() / review(), and the wave templates
(node_lines, agz_search.h) on the host simulator against the numpy twin of lines_twin.py -- exactly: moves, lengths and
the bits of every float."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

import alphago_jl_amd as ag
import hs
import lines_twin
from test_abi import _c_layout, _julia_ccalls, _julia_struct_layout, declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "alphago.jl_amd", "julia", "AlphaGoMI.jl")
NEW = ("agz_analyze_set_lines", "agz_analyze_lines", "agz_tree_lines")


# ---------------------------------------------------------------- 1. layout and entry points

def test_line_layout_agrees_between_c_ctypes_and_julia():
    ct = ag._lib.Line
    size, offs = _c_layout("agz_line", len(ct._fields_))
    assert C.sizeof(ct) == size == 24
    assert [f[0] for f in ct._fields_] == ["move", "pv_len", "N", "W", "prior", "end_W"]
    assert [getattr(ct, f[0]).offset for f in ct._fields_] == offs
    jsize, joffs, _ = _julia_struct_layout(open(JL).read(), "AgzLine")
    assert (jsize, joffs) == (size, offs)


def test_lines_entry_points_are_exported_bound_and_called():
    L = ag.load()
    declared = declared_functions()
    jl_calls = {c[0] for c in _julia_ccalls(open(JL).read())}
    for name in NEW:
        assert name in declared and hasattr(L, name) and name in L._agz_signatures, name
        assert name in jl_calls, name
    assert L.agz_version() == 103


# ---------------------------------------------------------------- 2. argument checks

@pytest.mark.parametrize("kw", [dict(lines=-1), dict(lines=17), dict(lines=4, pv_depth=0), dict(lines=4, pv_depth=65),
                                dict(lines=4, pv_min_visits=0), dict(lines=1.5), dict(lines=True)])
def test_analyze_and_review_check_the_lines_arguments(kw):
    env = ag.GoEnv(5)
    with pytest.raises(ValueError):
        ag.analyze(env, object(), [ag.Position(env)], **kw)
    with pytest.raises(ValueError):
        ag.review(env, object(), [[(0, 0)]], **kw)


def test_lines_off_is_the_plain_call():
    env = ag.GoEnv(5)
    assert ag.analyze(env, object(), [], lines=0) == [] and ag.review(env, object(), [], lines=0) == []
    with pytest.raises(TypeError):                      # valid lines arguments: the next check is the old one
        ag.analyze(env, object(), [ag.Position(env)], lines=4, pv_depth=16, pv_min_visits=2)
    assert ag.AnalysisLines._fields == ag.Analysis._fields + ("lines",)
    assert ag.Line._fields == ("move", "N", "W", "Q", "prior", "pv", "pv_N", "end_Q")
    assert len(ag.Analysis._fields) == 11               # callers unpack Analysis by position


# ---------------------------------------------------------------- 3. the wave templates on the host simulator

def twin(sim, node, K, D, mv, g=0):
    """lines_twin.walk over the rows of the simulator's tree"""
    return lines_twin.walk(lambda n, f: sim.row(g, n, f).copy(), lambda n: sim.children(g, n).copy(), node, K, D, mv)


def crc_net(A):
    """the network of the searched-tree cases: a function of the feature row alone"""
    def net(feats):
        pi, v = np.zeros((len(feats), A), np.float32), np.zeros(len(feats), np.float32)
        for i, row in enumerate(feats):
            rs = np.random.RandomState(zlib.crc32(np.ascontiguousarray(row, np.float32).tobytes()))
            x = 2.0 * rs.randn(A)
            e = np.exp(x - x.max())
            pi[i] = (e / e.sum()).astype(np.float32)
            v[i] = np.float32(np.tanh(0.3 * rs.randn()))
        return pi, v
    return net


def search(sim, net, visits):
    n0 = sim.game(0).rootN
    while sim.game(0).rootN < n0 + visits:
        st, ns = sim.op(hs.TOP_SEARCH_SELECT, par=8)
        assert st == 0
        if ns:
            feats = np.zeros((ns, 17 * sim.P), np.float32)
            sim.L.hs_tree_leaf_features(sim.h, 0, hs.pf(feats))
            pi, v = net(feats)
            sim.L.hs_set_batch_outputs(sim.h, hs.pf(pi), hs.pf(v), ns)
        st, _ = sim.op(hs.TOP_SEARCH_POST)
        assert st == 0


def test_node_lines_on_searched_trees_equal_the_twin():
    """9x9 from the empty board, 200 readouts, seeds 0..5, three plies each on re-rooted (kept) trees; lines at the root
    and at the first line's first child, K = 4, D in (16, 4), min_visits in (1, 2).  The conditions at the end keep the
    comparison from passing on trivial trees; they were checked with the twin alone on these inputs."""
    K = 4
    roots = first_pv = ties = 0
    full_d4, full_d16, longest = 0, 0, 0
    for seed in range(6):
        sim = hs.Sim(board_size=9, num_readouts=200, two_player_mode=1, seed=seed, games=1)
        net = crc_net(sim.A)
        sim.tree_init(0, np.zeros(sim.P, np.int8))
        sim.L.hs_game_set(sim.h, 0, 0, float(seed))
        for ply in range(3):
            search(sim, net, 200)
            root = sim.game(0).root
            t16 = None
            for D in (16, 4):
                for mv in (1, 2):
                    got, want = sim.lines(root, K, D, mv), twin(sim, root, K, D, mv)
                    assert lines_twin.same(got, want) is None, (seed, ply, D, mv, lines_twin.same(got, want))
                    child = int(sim.children(0, root)[want["move"][0]])
                    assert child >= 0
                    g2, w2 = sim.lines(child, K, D, mv), twin(sim, child, K, D, mv)
                    assert lines_twin.same(g2, w2) is None, (seed, ply, D, mv, "child", lines_twin.same(g2, w2))
                    if mv == 1 and D == 16:
                        t16 = want
                        full_d16 += int((want["pv_len"] == D).sum() + (w2["pv_len"] == D).sum())
                        longest = max(longest, int(want["pv_len"].max()))
                    if mv == 1 and D == 4:
                        full_d4 += int((want["pv_len"] == D).sum())
            roots += 1
            assert (t16["move"] >= 0).all(), (seed, ply)                 # every searched root gave 4 lines
            assert t16["pv_len"][0] >= 4, (seed, ply, t16["pv_len"])     # every first PV has at least 4 moves
            first_pv += int(t16["pv_len"][0])
            top5 = np.sort(sim.row(0, root, 0))[::-1][:5]
            ties += int(len(np.unique(top5)) < 5)                        # the second sort key decides something
            st, a = sim.op(hs.TOP_PICK)
            assert st == 0
            st, ok = sim.op(hs.TOP_PLAY, a=a)
            assert st == 0 and ok == 1
        sim.close()
    print(f"roots {roots}, mean first PV {first_pv / roots:.2f}, longest PV {longest}, ties {ties}, "
          f"PVs at the limit: D=4 {full_d4}, D=16 {full_d16}")
    assert roots == 18
    assert 2 * ties >= roots
    assert full_d4 >= 1 and full_d16 == 0


def hand_tree():
    """a 5x5 root with real child nodes under actions 3, 7, 11 and 20, and a grandchild under (7, 2); every row zero"""
    sim = hs.Sim(board_size=5, num_readouts=8, two_player_mode=1, seed=0, games=1)
    root = sim.tree_init(0, np.zeros(sim.P, np.int8))
    kids = {}
    for a in (3, 7, 11, 20):
        st, c = sim.op(hs.TOP_ADD_CHILD, node=root, a=a)
        assert st == 0 and c >= 0
        kids[a] = c
    st, gc = sim.op(hs.TOP_ADD_CHILD, node=kids[7], a=2)
    assert st == 0 and gc >= 0
    for n in [root, gc] + list(kids.values()):
        for f in (0, 1, 2):
            sim.row(0, n, f)[:] = 0
    return sim, root, kids, gc


def both(sim, node, K, D, mv):
    got, want = sim.lines(node, K, D, mv), twin(sim, node, K, D, mv)
    assert lines_twin.same(got, want) is None, lines_twin.same(got, want)
    return got


def test_node_lines_on_hand_written_rows():
    sim, root, kids, gc = hand_tree()
    N, W, Pr = (sim.row(0, root, f) for f in (0, 1, 2))
    # equal child_N with different priors: the larger prior first, whatever the action
    N[[3, 7, 11]] = (5, 5, 2)
    Pr[[3, 7, 11]] = (0.125, 0.5, 0.25)
    W[[3, 7, 11]] = (1.5, -2.25, 0.75)
    r = both(sim, root, 4, 8, 1)
    assert list(r["move"]) == [7, 3, 11, -1] and list(r["pv_len"]) == [1, 1, 1, 0]      # fewer than K visited children
    assert r["end_W"][0] == np.float32(-2.25) and r["pv"][3, 0] == -1 and r["N"][3] == 0
    # equal child_N and equal priors: the lower action first
    Pr[[3, 7]] = 0.5
    assert list(both(sim, root, 4, 8, 1)["move"]) == [3, 7, 11, -1]
    assert list(both(sim, root, 2, 8, 1)["move"]) == [3, 7]
    assert list(both(sim, root, 1, 1, 1)["move"]) == [3]
    # a PV level whose maximum is shared by several actions: findmax takes the lowest, the prior plays no part
    cn, cw, cp = (sim.row(0, kids[7], f) for f in (0, 1, 2))
    cn[[2, 9, 14]] = (3, 3, 1)
    cp[[2, 9, 14]] = (0.1, 0.9, 0.0)
    cw[[2, 9]] = (0.5, -0.5)
    gn, gw = sim.row(0, gc, 0), sim.row(0, gc, 1)
    gn[24] = 1
    gw[24] = 0.25
    r = both(sim, root, 4, 8, 1)
    assert list(r["pv"][1, :4]) == [7, 2, 24, -1] and r["pv_len"][1] == 3
    assert list(r["pv_N"][1, :3]) == [5, 3, 1] and r["end_W"][1] == np.float32(0.25)
    # min_visits 2 (mvp_gg) stops in front of the single visit, the depth limit in front of everything beyond it
    r = both(sim, root, 4, 8, 2)
    assert r["pv_len"][1] == 2 and r["end_W"][1] == np.float32(0.5)
    assert both(sim, root, 4, 2, 1)["pv_len"][1] == 2 and both(sim, root, 4, 1, 1)["pv_len"][1] == 1
    # a child with visits but no node: the line is the candidate alone
    N[15] = 9
    Pr[15] = 0.01
    assert int(sim.children(0, root)[15]) < 0
    r = both(sim, root, 4, 8, 1)
    assert list(r["move"]) == [15, 3, 7, 11] and r["pv_len"][0] == 1 and r["end_W"][0] == W[15]
    # ... and the same below the root: (7, 9) has visits and no node once it is the only maximum
    cn[9] = 4
    r = both(sim, root, 4, 8, 1)
    assert list(r["pv"][2, :3]) == [7, 9, -1] and r["end_W"][2] == np.float32(-0.5)
    # lines of an inner node, of a leaf, and all 16
    assert list(both(sim, kids[7], 3, 8, 1)["move"]) == [9, 2, 14]
    assert (both(sim, gc, 4, 8, 3)["move"] == [24, -1, -1, -1]).all()
    assert (both(sim, kids[3], 4, 8, 1)["move"] == -1).all()
    N[:] = np.arange(sim.A, dtype=np.float32) % 5
    Pr[:] = (np.arange(sim.A, dtype=np.float32) * 7 % 11) / 16
    r = both(sim, root, 16, 3, 1)
    assert (r["move"] >= 0).all() and len(set(r["move"])) == 16
    sim.close()


@pytest.mark.parametrize("N", [5, 13, 19])
def test_node_lines_on_every_row_width(N):
    """R = ceil(A / 64) entries per lane slot is a template parameter: 1 (5x5), 3 (13x13) and 6 (19x19) besides the 2 of
    9x9, on random rows over real child nodes"""
    sim = hs.Sim(board_size=N, num_readouts=8, two_player_mode=1, seed=0, games=1, max_nodes_per_game=64)
    root = sim.tree_init(0, np.zeros(sim.P, np.int8))
    rng = np.random.RandomState(N)
    nodes = [root]
    for depth in range(3):
        for parent in list(nodes[-4:] if depth else nodes):
            for a in rng.choice(sim.P, 4, replace=False):
                st, c = sim.op(hs.TOP_ADD_CHILD, node=parent, a=int(a))
                if st == 0 and c >= 0 and c not in nodes:
                    nodes.append(c)
    for n in nodes:
        sim.row(0, n, 0)[:] = rng.randint(0, 4, sim.A)              # many ties, on purpose
        sim.row(0, n, 1)[:] = rng.randn(sim.A)
        sim.row(0, n, 2)[:] = rng.randint(0, 3, sim.A) / 4
    for n in nodes[:6]:
        for K, D, mv in ((4, 16, 1), (16, 4, 2), (5, 2, 3)):
            both(sim, n, K, D, mv)
    sim.close()

"""Value uncertainty on the device (agz_search_set_value_moments / _set_lcb / _set_puct_variance),
engine against the host simulator (hs.Sim: agz_search.h lane-serial, on the engine's own forward), floats
bit for bit: self-play games with their counters and the S rows of the live roots; one single tree per register-row width
of the descent with every node's rows and agz_tree_child_lcb, and hand-made rows with entries at the lane boundaries;
analyze and review against the single-tree player; an arena; every refusal keeps the setting.  Tower 1 everywhere."""
import ctypes as C

import numpy as np
import pytest

import alphago_jl_amd as ag
import gpu_options as go
import hs
import uncertainty_twin as ut
from gpu_options import RECORD, api_game, api_positions, peaked_engine, play, same_game, sharpen
from test_hostsim_selfplay import bits_equal

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
bits64 = hs.bits64
BAD_ARGUMENT, OK = ag._lib.BAD_ARGUMENT, ag._lib.OK
F_N, F_W, F_P, F_S = ag._lib.F_CHILD_N, ag._lib.F_CHILD_W, ag._lib.F_CHILD_PRIOR, ag._lib.F_CHILD_S
C_PUCT = 0.96
LCB, PV = (5.0, 3, 0.15), (0.85, 0.4, 2.0)
G_SEARCH = 3


# ---------------------------------------------------------------- a. self-play

GAMES, R, SEED = 4, 16, 3
CFG = dict(board_size=5, games=GAMES, num_readouts=R, seed=SEED, record_capacity_games=GAMES + 8, c_puct=C_PUCT)
FIELDS = RECORD + ("resign_disabled", "final_score")


def lockstep_games(lcb, pv, moments):
    """the engine and the simulator step by step through GAMES games -> (engine records, simulator records, engine
    counters, simulator counters, the live roots whose S rows were compared)"""
    eng = peaked_engine(5, 1, **{k: v for k, v in CFG.items() if k != "board_size"})
    fwd = peaked_engine(5, 1, games=1, num_readouts=8, max_nodes_per_game=16)
    sim = hs.Sim(**CFG)
    go.configure(eng, dict(lcb=lcb, pv=pv, moments=moments))
    go.configure(sim, dict(lcb=lcb, pv=pv, moments=moments))
    eng.start(GAMES)
    sim.start(GAMES)
    compared = 0
    for step in range(20000):
        eng.step(1)
        sim.step(fwd.forward_features)
        if step % 3 == 0:
            # (which slot claims which game is the device's to decide: the games are matched by their ids)
            slot_of = {int(eng.debug_live_record(e)[0]): e for e in range(GAMES)}
            for g in range(GAMES):
                G = sim.game(g)
                if G.phase != G_SEARCH:
                    continue
                e = slot_of[int(G.game_id)]
                assert eng.debug_live_record(e)[1] == G.nqs and eng.tree_root(e) == G.root, (step, g)
                assert bits_equal(eng.node_floats(e, G.root, F_S), sim.row_S(g, G.root)), (step, g)
                assert bits_equal(f32(eng.node_S(e, G.root)), f32(sim.S_(g, G.root))), (step, g)
                compared += 1
        if sim.L.hs_records_count(sim.h) >= GAMES:
            break
    assert eng.records_count() == GAMES
    out = (sorted(eng.records(), key=lambda r: r["game_id"]), sim.records(), eng.uncertainty_counts(),
           sim.uncertainty_counts(), compared)
    for x in (eng, fwd):
        x.close()
    sim.close()
    return out


def test_selfplay_equals_the_simulator_and_moments_alone_change_nothing():
    off = peaked_engine(5, 1, **{k: v for k, v in CFG.items() if k != "board_size"})
    plain, _ = play(off, GAMES)
    assert off.uncertainty_counts() == (0, 0, 0, 0)
    with pytest.raises(ag.AgzError):                        # no S rows with the moments off
        off.node_floats(0, off.tree_root(0), F_S)
    off.close()
    recs, want, counts, wcounts, compared = lockstep_games(None, None, True)
    assert counts == wcounts == (0, 0, 0, 0) and compared > 20
    for r, o, p in zip(recs, want, plain):
        assert same_game(r, o, FIELDS), r["game_id"]
        assert same_game(r, p, FIELDS), ("moments only against everything off", r["game_id"])
    recs, want, counts, wcounts, compared = lockstep_games(LCB, PV, None)
    print("both rules: counters", counts, "simulator", wcounts, "roots compared", compared)
    for r, o in zip(recs, want):
        assert same_game(r, o, FIELDS), r["game_id"]
    assert counts == wcounts and counts[0] > 0 and counts[2] > counts[3] > 0 and compared > 20
    assert any(r["num_moves"] != p["num_moves"] or (r["moves"] != p["moves"]).any() for r, p in zip(recs, plain)), \
        "the rules changed no move"


# ---------------------------------------------------------------- b. single trees, one per descent width

def assert_same_tree(eng, sim, node, z, count):
    for k, f in enumerate((F_N, F_W, F_P)):
        assert bits_equal(eng.node_floats(0, node, f), sim.row(0, node, k)), (node, k)
    assert bits_equal(eng.node_floats(0, node, F_S), sim.row_S(0, node)), (node, "S")
    assert bits_equal(f32(eng.node_S(0, node)), f32(sim.S_(0, node))), (node, "own S")
    for got, want in zip(eng.tree_child_lcb(0, node, z), sim.child_lcb(node, z)):
        assert (bits64(got) == bits64(want)).all(), (node, "lcb")
    ec, sc = eng.node_children(0, node), sim.children(0, node)
    assert (ec == sc).all(), node
    count[0] += 1
    for c in ec:
        if c >= 0:
            assert_same_tree(eng, sim, int(c), z, count)


@pytest.mark.parametrize("N", [5, 9, 13, 19])            # register-row widths R = 1, 2, 3, 6
def test_single_tree_equals_the_simulator(N):
    cfg = dict(board_size=N, games=1, num_readouts=64, parallel_readouts=8, seed=5, max_nodes_per_game=128, c_puct=C_PUCT,
               two_player_mode=1)
    eng = ag.Engine(tower_height=1, **cfg)
    eng.init_synthetic(0)
    fwd = ag.Engine(board_size=N, tower_height=1, games=1, num_readouts=8, max_nodes_per_game=16)
    fwd.init_synthetic(0)
    sim = hs.Sim(**cfg)
    go.configure(eng, dict(lcb=LCB, pv=PV))
    go.configure(sim, dict(lcb=LCB, pv=PV))
    root = eng.tree_init(0, np.zeros(N * N, np.int8))
    eng.set_draw(0, 11, 0)
    assert sim.tree_init(0, np.zeros(N * N, np.int8)) == root
    sim.L.hs_game_set(sim.h, 0, 0, 11.0)
    for _ in range(3):
        n = eng.tree_search(0, 8)
        st, ns = sim.op(hs.TOP_SEARCH_SELECT, par=8)
        assert st == 0 and ns == n
        if ns:
            feats = np.zeros((ns, 17 * sim.P), f32)
            sim.L.hs_tree_leaf_features(sim.h, 0, hs.pf(feats))
            pi, v = fwd.forward_features(feats)
            sim.L.hs_set_batch_outputs(sim.h, hs.pf(np.ascontiguousarray(pi, f32)), hs.pf(np.ascontiguousarray(v, f32)), ns)
        assert sim.op(hs.TOP_SEARCH_POST)[0] == 0
    count = [0]
    assert_same_tree(eng, sim, root, LCB[0], count)
    counts = sim.uncertainty_counts()
    print(f"N {N}: {count[0]} nodes, counters {counts}")
    assert count[0] > 8 and counts[2] > 0 and eng.uncertainty_counts() == counts
    assert (bits64(eng.node_scores(0, root)) == bits64(sim.scores(root))).all()
    st, a = eng.pick_move(0)
    assert (st, a) == sim.op(hs.TOP_PICK) and st == 0
    # hand-made rows with entries on both sides of a lane boundary and at the row's end
    A = sim.A
    spots = sorted({a for a in (63, 64, A - 1, 0, 7) if a < A})
    Nr, Wr, Sr = np.zeros(A, f32), np.zeros(A, f32), np.zeros(A, f32)
    rng = np.random.RandomState(N)
    for k, a in enumerate(spots):
        Nr[a] = 4 + 2 * k
        vals = rng.uniform(-1, 1, int(Nr[a]) + 1).astype(f32)
        Wr[a], Sr[a] = vals.sum(dtype=f32), (vals * vals).sum(dtype=f32)
    Nr[A - 1] = 5
    Wr[A - 1], Sr[A - 1] = f32(0.9) * (1 + Nr[A - 1]), f32(0.81) * (1 + Nr[A - 1]) + f32(1e-3)     # the best bound, not the most visits
    for row, f, k in ((Nr, F_N, 0), (Wr, F_W, 1)):
        eng.node_set_floats(0, root, f, row)
        sim.row(0, root, k)[:] = row
    eng.node_set_floats(0, root, F_S, Sr)
    sim.row_S(0, root)[:] = Sr
    want = ut.child_lcb(Nr, Wr, Sr, 1, LCB[0])
    for got, sgot, w in zip(eng.tree_child_lcb(0, root, LCB[0]), sim.child_lcb(root, LCB[0]), want):
        assert (bits64(got) == bits64(sgot)).all() and (bits64(got) == bits64(w)).all()
    st, a = eng.pick_move(0)
    assert st == 0 and a == ut.lcb_pick(Nr, Wr, Sr, 1, LCB) == A - 1 and sim.op(hs.TOP_PICK) == (0, a)
    assert Nr[a] != Nr.max()
    assert (bits64(eng.node_scores(0, root)) == bits64(sim.scores(root))).all()
    assert eng.uncertainty_counts() == sim.uncertainty_counts()
    for x in (eng, fwd):
        x.close()
    sim.close()


# ---------------------------------------------------------------- c. analysis and review

def test_analyze_equals_the_player_under_the_rules():
    env = ag.GoEnv(5)
    nn = ag.NeuralNet(env, tower_height=1, seed=1)
    sharpen(nn.engine, 5)
    positions = api_positions(env, 3, 6, 10)
    kw = dict(num_readouts=48, seed=4, two_player_mode=True, lcb=LCB, puct_variance=PV)
    res = ag.analyze(env, nn, positions, game_id_base=100, slots=2, **kw)
    plain = ag.analyze(env, nn, positions, num_readouts=48, seed=4, two_player_mode=True, game_id_base=100, slots=2)
    assert not hasattr(plain[0], "child_S")
    differs = off_max = 0
    for k, pos in enumerate(positions):
        p = ag.MCTSPlayer(env, nn, game_id=100 + k, **kw)
        p.initialize_game(pos)
        mv = p.suggest_move()
        root = p.root
        a = res[k]
        assert a.status == OK and ag.to_flat(a.move, env) == ag.to_flat(mv, env), k
        assert bits_equal(a.N, f32(root.N)) and bits_equal(a.W, f32(root.W)), k
        for got, want in ((a.child_N, root.child_N), (a.child_W, root.child_W), (a.prior, root.child_prior),
                          (a.child_S, root.child_S)):
            assert bits_equal(got, want), k
        assert bits_equal(f32(a.root_S), f32(p.engine.node_S(0, root.id))), k
        tp = p.engine.node_info(0, root.id).pos.to_play
        mean, sd, l = ut.child_lcb(a.child_N, a.child_W, a.child_S, tp, LCB[0])
        assert (bits64(root.child_lcb(LCB[0])) == bits64(l)).all() and (bits64(root.child_stdev) == bits64(sd)).all()
        assert ag.to_flat(a.move, env) == ut.lcb_pick(a.child_N, a.child_W, a.child_S, tp, LCB), k
        off_max += a.child_N[ag.to_flat(a.move, env)] != a.child_N.max()
        differs += not bits_equal(a.child_N, plain[k].child_N)
        p.engine.close()
    print("analysis: moves off the most visited child", off_max, "rows that differ from the plain search", differs)
    assert differs > 0, "the variance factor changed no search"


def test_review_equals_the_player_under_the_rules():
    env = ag.GoEnv(5)
    nn = ag.NeuralNet(env, tower_height=1, seed=1)
    sharpen(nn.engine, 5)
    games = [api_game(env, 10 + j, 6) for j in range(2)]
    kw = dict(num_readouts=16, seed=4, lcb=LCB, puct_variance=PV)
    res = ag.review(env, nn, games, game_id_base=100, slots=2, **kw)
    for j, g in enumerate(games):
        p = ag.MCTSPlayer(env, nn, game_id=100 + j, two_player_mode=True, **kw)
        p.initialize_game(None)
        for k, m in enumerate(g):
            mv = p.suggest_move()
            root = p.root
            a = res[j][k]
            assert a.status == OK and a.move == mv, (j, k)
            assert bits_equal(a.N, f32(root.N)) and bits_equal(a.W, f32(root.W)), (j, k)
            for got, want in ((a.child_N, root.child_N), (a.child_W, root.child_W), (a.prior, root.child_prior),
                              (a.child_S, root.child_S)):
                assert bits_equal(got, want), (j, k)
            assert bits_equal(f32(a.root_S), f32(p.engine.node_S(0, root.id))), (j, k)
            assert p.play_move(m)
        p.engine.close()


# ---------------------------------------------------------------- d. the arena

def test_evaluate_equals_the_simulator_arena_under_lcb():
    env = ag.GoEnv(5)
    a, b = ag.NeuralNet(env, tower_height=1, seed=0), ag.NeuralNet(env, tower_height=1, seed=5)
    games = 2
    ok, st = ag.evaluate(env, a, b, num_games=games, ro=16, seed=2, return_stats=True, lcb=LCB, c_puct=C_PUCT)
    sim = hs.Sim(board_size=5, games=2 * games, num_readouts=16, seed=2, arena_mode=1, record_capacity_games=games + 8,
                 c_puct=C_PUCT)
    go.configure(sim, dict(lcb=LCB))
    sim.start(games)
    for _ in range(20000):
        sim.step(a.engine.forward_features, b.engine.forward_features)
        if sim.L.hs_records_count(sim.h) >= games:
            break
    want = sim.records()
    got = sorted(st.records, key=lambda r: r["game_id"])
    counts = sim.uncertainty_counts()
    print("arena: counters", counts)
    assert len(want) == len(got) == games and counts[0] > 0 and counts[2:] == (0, 0)
    for r, o in zip(got, want):
        assert r["game_id"] // 2 == o["game_id"] // 2 and r["num_moves"] == o["num_moves"], r["game_id"]
        assert (r["moves"] == o["moves"]).all() and bits_equal(r["qs"], o["qs"]) and r["result"] == o["result"]
    sim.close()


# ---------------------------------------------------------------- e. refusals

def test_refusals_keep_the_setting():
    eng = ag.Engine(board_size=5, tower_height=1, games=2, num_readouts=8, c_puct=C_PUCT, seed=1, two_player_mode=1)
    eng.init_synthetic(0)
    L, h = eng.L, eng.h
    nan = float("nan")
    # either rule while the moments are off; the S read-outs too
    assert L.agz_search_set_lcb(h, 1.0, 1, 0.0) == BAD_ARGUMENT and L.agz_search_set_puct_variance(h, 0.5, 0.4, 2.0) == BAD_ARGUMENT
    root = eng.tree_init(0, np.zeros(25, np.int8))
    d = np.zeros(26, f64)
    assert L.agz_tree_child_lcb(h, 0, root, 1.0, hs.pd(d), hs.pd(d), hs.pd(d)) == BAD_ARGUMENT
    assert L.agz_tree_node_S(h, 0, root, C.byref(C.c_float())) == BAD_ARGUMENT
    env = ag.GoEnv(5)
    positions = api_positions(env, 3, 2, 6)
    boards, hist, infos = np.zeros((2, 25), np.int8), np.zeros((2, 7, 25), np.int8), (ag._lib.PositionInfo * 2)()
    for k, p in enumerate(positions):
        boards[k], infos[k], hh = ag.position_arrays(p)
        hist[k, :len(hh)] = hh
    eng.analyze_start(boards, infos, hist, 0)
    while eng.analyze_progress() < 2:
        eng.step(4)
    cs, rs = np.zeros((2, 26), f32), np.zeros(2, f32)
    assert L.agz_analyze_child_S(h, hs.pf(cs), hs.pf(rs)) == BAD_ARGUMENT, "a run begun with the moments off"
    eng.set_value_moments(True)
    assert L.agz_analyze_child_S(h, hs.pf(cs), hs.pf(rs)) == BAD_ARGUMENT, "... stays without S rows"
    kept_lcb, kept_pv = (2.5, 4, 0.25), (0.7, 0.5, 3.0)
    eng.set_lcb(kept_lcb)
    eng.set_puct_variance(kept_pv)
    root = eng.tree_init(0, np.zeros(25, np.int8))
    eng.tree_search(0, 8)
    eng.tree_search(0, 8)

    def in_force(what):
        r = eng.tree_root(0)
        rows = [eng.node_floats(0, r, f) for f in (F_N, F_W, F_P, F_S)]
        info = eng.node_info(0, r)
        want = ut.scores(rows[0], rows[1], rows[2], f32(info.N), f32(info.W), f32(eng.node_S(0, r)), info.pos.to_play, True,
                         C_PUCT, (0, 0.0, 0.0, 0.0), kept_pv)
        assert (bits64(eng.node_scores(0, r)) == bits64(want)).all(), what
        pick = ut.lcb_pick(rows[0], rows[1], rows[3], info.pos.to_play, kept_lcb)
        if pick is not None:
            assert eng.pick_move(0) == (0, pick), what

    def refused(fn, *args):
        assert getattr(L, fn)(h, *args) == BAD_ARGUMENT, (fn, args)
        in_force((fn, args))

    in_force("before")
    for args in ((2,), (-1,), (0,)):                        # (0: a rule is on)
        refused("agz_search_set_value_moments", *args)
    for args in ((nan, 1, 0.0), (-1e-9, 1, 0.0), (100.001, 1, 0.0), (1.0, 0, 0.0), (1.0, 1, -1e-9), (1.0, 1, 1.000001),
                 (1.0, 1, nan)):
        refused("agz_search_set_lcb", *args)
    for args in ((nan, 0.4, 2.0), (-1e-9, 0.4, 2.0), (1.0, 0.4, 2.0), (0.5, 0.00999, 2.0), (0.5, 2.001, 2.0),
                 (0.5, 0.4, -1e-9), (0.5, 0.4, 1000.001), (0.5, 0.4, nan)):
        refused("agz_search_set_puct_variance", *args)
    with pytest.raises(ag.AgzError):
        eng._ck(L.agz_search_uncertainty_counts(h, None))
    # between select and incorporate
    assert eng.tree_search_select(0, 4) > 0
    refused("agz_search_set_lcb", 1.0, 1, 0.0)
    refused("agz_search_set_puct_variance", 0.0, 0.4, 2.0)
    refused("agz_search_set_value_moments", 1)
    eng.tree_search_incorporate(0)
    # games in flight
    eng.start(2)
    eng.step(3)
    assert eng.stats()["live_games"] > 0
    assert L.agz_search_set_lcb(h, 0.0, 1, 0.0) == BAD_ARGUMENT and L.agz_search_set_puct_variance(h, 0.0, 0.4, 2.0) == BAD_ARGUMENT
    assert L.agz_search_set_value_moments(h, 1) == BAD_ARGUMENT
    for _ in range(20000):
        eng.step(8)
        if eng.records_count() >= 2:
            break
    c = eng.uncertainty_counts()
    assert c[0] > 0 and c[2] > 0
    eng.set_lcb(None)                                       # between games they are taken, and the counters restart
    assert eng.uncertainty_counts() == (0, 0, 0, 0)
    eng.set_puct_variance(None)
    eng.set_value_moments(False)
    eng.close()
    arena = ag.Engine(board_size=5, tower_height=1, games=2, num_readouts=8, arena_mode=1)
    arena.set_value_moments(True)                           # an arena engine takes all three
    arena.set_lcb(LCB)
    arena.set_puct_variance(PV)
    arena.close()

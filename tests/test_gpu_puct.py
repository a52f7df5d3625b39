"""PUCT rule options on the device (agz_search_set_puct): the scores of searched trees against the
numpy restatement and whole trees against the host simulator at the four register-row widths of the descent and at the
two boards (15x15, 17x17: 4 and 5 row elements per lane) that the widest one runs, rounded up;
self-play games with every other search option, root exploration and the move temperature among them, against the
simulator, counters included; analyze, review and evaluate
under the rule against their single-tree / per-game forms; off is the engine that never made the call; every refusal
keeps the setting in force.  The simulator runs on the engine's own forward.  Tower 1 everywhere."""
import functools

import numpy as np
import pytest

import alphago_jl_amd as ag
import explore_twin as ex
import hs
import puct_twin as pt
import selfplay_twin as tw
from gpu_options import RECORD, api_game, api_positions, configure, peaked_engine, play, same_game, sharpen
from test_hostsim_selfplay import bits_equal

pytestmark = pytest.mark.gpu
f32 = np.float32
C_PUCT = 0.96
BOTH = (1, 0.2, 0.05, 19652.0)
FPU, CB = (0.2, 0.05), 19652.0
BAD_ARGUMENT = ag._lib.BAD_ARGUMENT
F_N, F_W, F_P = ag._lib.F_CHILD_N, ag._lib.F_CHILD_W, ag._lib.F_CHILD_PRIOR
BOARDS = [5, 9, 13, 15, 17, 19]  # register-row widths R = 1, 2, 3, 6; 15 and 17 (4 and 5 per lane) are run by R = 6


def forward_engine(N, peaked=False):
    if peaked:
        return peaked_engine(N, 1, games=1, num_readouts=8, max_nodes_per_game=16)
    e = ag.Engine(board_size=N, tower_height=1, games=1, num_readouts=8, max_nodes_per_game=16)
    e.init_synthetic(0)
    return e


def assert_scores(eng, g, node, setting, what):
    info = eng.node_info(g, node)
    rows = [eng.node_floats(g, node, f) for f in (F_N, F_W, F_P)]
    is_root = node == eng.tree_root(g)
    want = pt.puct_scores(*rows, f32(info.N), f32(info.W), info.pos.to_play, is_root, C_PUCT, setting)
    got = eng.node_scores(g, node)
    assert (pt.bits64(got) == pt.bits64(want)).all(), what
    return got, rows


# ---------------------------------------------------------------- a. scores

@pytest.mark.parametrize("N", BOARDS)
def test_scores_of_a_searched_tree(N):
    eng = ag.Engine(board_size=N, tower_height=1, games=1, num_readouts=16, max_nodes_per_game=128, c_puct=C_PUCT, seed=2)
    eng.init_synthetic(0)
    eng.set_puct(FPU, CB)
    root = eng.tree_init(0, np.zeros(N * N, np.int8))
    eng.set_draw(0, 9, 0)
    while eng.node_info(0, root).N < 16:
        eng.tree_search(0, 8)
    kids, todo = [], [root]                       # the expanded nodes below the root, breadth first
    while todo and len(kids) < 2:
        x = todo.pop(0)
        for c in eng.node_children(0, x):
            if c >= 0 and eng.node_info(0, int(c)).is_expanded:
                kids.append(int(c))
                todo.append(int(c))
    assert len(kids) >= 2
    for name, setting in (("both", BOTH), ("fpu", (1, 0.2, 0.05, 0.0)), ("growth", (0, 0.0, 0.0, 1.0)), ("off", pt.OFF)):
        eng.set_puct(FPU if setting[0] else None, setting[3])
        got, rows = assert_scores(eng, 0, root, setting, (N, name, "root"))
        assert (rows[0] > 0).any() and (rows[0] == 0).any()
        for k in kids[:2]:
            assert_scores(eng, 0, k, setting, (N, name, k))
        if name == "off":
            ref, _, _ = tw.action_scores(*rows, 1, f32(eng.node_info(0, root).N), C_PUCT)
            assert (pt.bits64(got) == pt.bits64(ref)).all()
    eng.close()


# ---------------------------------------------------------------- b. trees

def assert_same_tree(eng, sim, enode, snode, count):
    for k, f in enumerate((F_N, F_W, F_P)):
        assert bits_equal(eng.node_floats(0, enode, f), sim.row(0, snode, k)), (enode, k)
    ec, sc = eng.node_children(0, enode), sim.children(0, snode)
    assert (ec == sc).all(), enode
    count[0] += 1
    for c in ec:
        if c >= 0:
            assert_same_tree(eng, sim, int(c), int(c), count)


def tree_case(N, readouts, external):
    cfg = dict(board_size=N, games=1, num_readouts=readouts, parallel_readouts=8, seed=5, max_nodes_per_game=256, c_puct=C_PUCT)
    fwd = forward_engine(N)
    if external:
        eng = ag.Engine(tower_height=0, external_network=1, **cfg)
    else:
        eng = ag.Engine(tower_height=1, **cfg)
        eng.init_synthetic(0)
    sim = hs.Sim(**cfg)
    eng.set_puct(FPU, CB)
    sim.set_puct(*BOTH)
    root = eng.tree_init(0, np.zeros(N * N, np.int8))
    eng.set_draw(0, 11, 0)
    sroot = sim.tree_init(0, np.zeros(N * N, np.int8))
    sim.L.hs_game_set(sim.h, 0, 0, 11.0)
    assert root == sroot
    while sim.game(0).rootN < readouts:
        n = eng.tree_search(0, 8, network=fwd.forward_features if external else None)
        st, ns = sim.op(hs.TOP_SEARCH_SELECT, par=8)
        assert st == 0 and ns == n
        if ns:
            feats = np.zeros((ns, 17 * sim.P), f32)
            sim.L.hs_tree_leaf_features(sim.h, 0, hs.pf(feats))
            pi, v = fwd.forward_features(feats)
            sim.L.hs_set_batch_outputs(sim.h, hs.pf(np.ascontiguousarray(pi, f32)), hs.pf(np.ascontiguousarray(v, f32)), ns)
        assert sim.op(hs.TOP_SEARCH_POST)[0] == 0
    info = eng.node_info(0, root)
    assert f32(info.N) == f32(sim.N_(0, sroot)) and bits_equal(f32(info.W), f32(sim.W_(0, sroot)))
    count = [0]
    assert_same_tree(eng, sim, root, sroot, count)
    levels, unvisited = sim.puct_counts()
    print(f"N {N}: {count[0]} nodes, {levels} levels scored, {unvisited} picked an unvisited child")
    assert count[0] > readouts // 2 and unvisited > 0
    assert eng.puct_counts() == (levels, unvisited)
    for e in (eng, fwd):
        e.close()
    sim.close()


@pytest.mark.parametrize("N,readouts", [(5, 64), (9, 64), (13, 24), (15, 24), (17, 24), (19, 24)])
def test_trees_equal_the_simulator(N, readouts):
    tree_case(N, readouts, external=False)


def test_external_network_tree_equals_the_simulator():
    tree_case(5, 64, external=True)


# ---------------------------------------------------------------- c / e. whole games

GAMES, R, SEED = 4, 16, 3
CFG = dict(board_size=5, games=GAMES, num_readouts=R, seed=SEED, record_capacity_games=GAMES + 8, c_puct=C_PUCT)
EXPLORATION = ex.setting(pt=(1.25, 1.1, 5.0), noise=(10.83, True), mt=(0.75, 0.15, 5.0))
OPTIONS = {"alone": {}, "playout_cap": dict(cap=(4, 0.5)), "forced_playouts": dict(forced=(2.0, True)), "gumbel": dict(gumbel=4),
           "symmetry": dict(symmetry=True), "exploration": dict(explore=EXPLORATION)}
FIELDS = RECORD + ("resign_disabled", "final_score")


def device_games(opt, puct, clear=False):
    """-> (records, the two PUCT counters, the four exploration counters)"""
    eng = peaked_engine(5, 1, **{k: v for k, v in CFG.items() if k != "board_size"})
    configure(eng, opt)
    if puct:
        eng.set_puct(FPU, CB)
    if clear:
        eng.set_puct(None, 0.0)
    recs, st = play(eng, GAMES)
    counts = eng.puct_counts(), eng.explore_counts()
    eng.close()
    return (recs,) + counts


@functools.lru_cache(maxsize=None)
def unset_games():
    return device_games({}, False)


def sim_games(opt):
    fwd = forward_engine(5, peaked=True)
    sim = hs.Sim(**CFG)
    configure(sim, opt)
    sim.set_puct(*BOTH)
    sim.start(GAMES)
    for _ in range(20000):
        if "symmetry" in opt:
            sim.step_sym(fwd.forward_features)
        else:
            sim.step(fwd.forward_features)
        if sim.L.hs_records_count(sim.h) >= GAMES:
            break
    recs, counts = sim.records(), (sim.puct_counts(), sim.explore_counts())
    sim.close()
    fwd.close()
    assert len(recs) == GAMES
    return (recs,) + counts


@pytest.mark.parametrize("option", list(OPTIONS))
def test_games_equal_the_simulator(option):
    opt = OPTIONS[option]
    recs, counts, xcounts = device_games(opt, True)
    want, wcounts, wxcounts = sim_games(opt)
    for r, o in zip(recs, want):
        print(f"{option} game {r['game_id']}: {r['num_moves']} moves, result {r['result']}; simulator {o['num_moves']} / {o['result']}")
        assert same_game(r, o, FIELDS), (option, r["game_id"])
    print(f"{option}: counters {counts} {xcounts}, simulator {wcounts} {wxcounts}")
    assert counts == wcounts and counts[0] > 0 and counts[1] > 0
    assert xcounts == wxcounts and (option != "exploration" or xcounts[2] > 0)
    if option == "alone":
        unset, c0, _ = unset_games()
        assert c0 == (0, 0)
        assert any(r["num_moves"] != u["num_moves"] or (r["moves"] != u["moves"]).any() for r, u in zip(recs, unset)), \
            "the rule changed no move"


def test_set_then_clear_is_the_engine_that_never_set():
    unset, _, _ = unset_games()
    recs, counts, _ = device_games({}, True, clear=True)
    assert counts == (0, 0)
    for r, u in zip(recs, unset):
        assert same_game(r, u, FIELDS), r["game_id"]


# ---------------------------------------------------------------- d. modes

def test_analyze_equals_the_player_under_the_rule():
    env = ag.GoEnv(5)
    nn = ag.NeuralNet(env, tower_height=1, seed=1)
    sharpen(nn.engine, 5)                      # a peaked policy: the searches go deep enough for the rule to matter
    positions = api_positions(env, 3, 3, 10)
    res = ag.analyze(env, nn, positions, num_readouts=48, seed=4, game_id_base=100, slots=2, fpu=FPU, c_base=CB)
    plain = ag.analyze(env, nn, positions, num_readouts=48, seed=4, game_id_base=100, slots=2)
    differs = False
    for k, pos in enumerate(positions):
        p = ag.MCTSPlayer(env, nn, num_readouts=48, seed=4, game_id=100 + k, fpu=FPU, c_base=CB)
        p.initialize_game(pos)
        mv = p.suggest_move()
        root = p.root
        a = res[k]
        assert a.status == ag._lib.OK and ag.to_flat(a.move, env) == ag.to_flat(mv, env), k
        assert bits_equal(a.N, f32(root.N)) and bits_equal(a.W, f32(root.W)), k
        for got, want in ((a.child_N, root.child_N), (a.child_W, root.child_W), (a.prior, root.child_prior)):
            assert bits_equal(got, want), k
        want = pt.puct_scores(root.child_N, root.child_W, root.child_prior, f32(root.N), f32(root.W),
                              p.engine.node_info(0, root.id).pos.to_play, True, p.engine.cfg.c_puct, BOTH)
        assert (pt.bits64(root.child_action_score) == pt.bits64(want)).all()      # NodeView follows the setting
        differs = differs or not bits_equal(a.child_N, plain[k].child_N)
        p.engine.close()
    assert differs, "the rule changed no analysis"


def test_review_equals_the_player_under_the_rule():
    env = ag.GoEnv(5)
    nn = ag.NeuralNet(env, tower_height=1, seed=1)
    sharpen(nn.engine, 5)
    games = [api_game(env, 10 + j, 6) for j in range(2)]
    res = ag.review(env, nn, games, num_readouts=16, seed=4, game_id_base=100, slots=2, fpu=FPU, c_base=CB)
    for j, g in enumerate(games):
        p = ag.MCTSPlayer(env, nn, num_readouts=16, seed=4, game_id=100 + j, two_player_mode=True, fpu=FPU, c_base=CB)
        p.initialize_game(None)
        for k, m in enumerate(g):
            mv = p.suggest_move()
            root = p.root
            a = res[j][k]
            assert a.status == ag._lib.OK and a.move == mv, (j, k)
            assert bits_equal(a.N, f32(root.N)) and bits_equal(a.W, f32(root.W)), (j, k)
            for got, want in ((a.child_N, root.child_N), (a.child_W, root.child_W), (a.prior, root.child_prior)):
                assert bits_equal(got, want), (j, k)
            assert p.play_move(m)
        p.engine.close()


def test_evaluate_equals_the_simulator_arena_under_the_rule():
    env = ag.GoEnv(5)
    a, b = ag.NeuralNet(env, tower_height=1, seed=0), ag.NeuralNet(env, tower_height=1, seed=5)
    games = 3
    ok, st = ag.evaluate(env, a, b, num_games=games, ro=16, seed=2, return_stats=True, fpu=FPU, c_base=CB, c_puct=C_PUCT)
    sim = hs.Sim(board_size=5, games=2 * games, num_readouts=16, seed=2, arena_mode=1, record_capacity_games=games + 8,
                 c_puct=C_PUCT)
    sim.set_puct(*BOTH)
    sim.start(games)
    for _ in range(20000):
        sim.step(a.engine.forward_features, b.engine.forward_features)
        if sim.L.hs_records_count(sim.h) >= games:
            break
    want = sim.records()
    got = sorted(st.records, key=lambda r: r["game_id"])
    assert len(want) == len(got) == games and sim.puct_counts()[1] > 0
    for r, o in zip(got, want):
        assert r["game_id"] // 2 == o["game_id"] // 2 and r["num_moves"] == o["num_moves"], r["game_id"]
        assert (r["moves"] == o["moves"]).all() and bits_equal(r["qs"], o["qs"]) and r["result"] == o["result"]
    sim.close()


# ---------------------------------------------------------------- f. refusals

def test_refusals_keep_the_setting():
    kept = (1, 0.3, 0.1, 100.0)
    eng = ag.Engine(board_size=5, tower_height=1, games=2, num_readouts=8, c_puct=C_PUCT, seed=1)
    eng.init_synthetic(0)
    eng.set_puct((0.3, 0.1), 100.0)
    root = eng.tree_init(0, np.zeros(25, np.int8))
    eng.tree_search(0, 8)
    eng.tree_search(0, 8)

    def refused(*args):
        assert eng.L.agz_search_set_puct(eng.h, *args) == BAD_ARGUMENT, args
        assert_scores(eng, 0, eng.tree_root(0), kept, args)

    nan = float("nan")
    for args in ((1, nan, 0.0, 0.0), (1, 0.0, nan, 0.0), (1, 0.0, 0.0, nan), (0, nan, 0.0, 0.0),
                 (1, -1e-9, 0.0, 0.0), (1, 4.000001, 0.0, 0.0), (1, 0.0, -1e-9, 0.0), (1, 0.0, 4.000001, 0.0),
                 (1, 0.0, 0.0, 0.999999), (1, 0.0, 0.0, -1.0), (1, 0.0, 0.0, 1.0000001e9), (2, 0.0, 0.0, 0.0),
                 (-1, 0.0, 0.0, 0.0)):
        refused(*args)
    for args in ((1, 0.0, 4.0, 1.0), (1, 4.0, 0.0, 1.0e9), kept):           # the bounds themselves are in range
        assert eng.L.agz_search_set_puct(eng.h, *args) == ag._lib.OK, args
    with pytest.raises(ag.AgzError):
        eng._ck(eng.L.agz_search_puct_counts(eng.h, None))
    # between select and incorporate
    assert eng.tree_search_select(0, 4) > 0
    refused(1, 0.0, 0.0, 0.0)
    refused(0, 0.0, 0.0, 0.0)
    eng.tree_search_incorporate(0)
    eng.set_puct((0.3, 0.1), 100.0)
    # games in flight
    eng.start(2)
    eng.step(3)
    assert eng.stats()["live_games"] > 0
    assert eng.L.agz_search_set_puct(eng.h, 0, 0.0, 0.0, 0.0) == BAD_ARGUMENT
    assert_scores(eng, 0, eng.tree_root(0), kept, "in flight")
    for _ in range(20000):
        eng.step(8)
        if eng.records_count() >= 2:
            break
    assert eng.puct_counts()[0] > 0
    eng.set_puct(None, 0.0)                                                   # between games it is taken
    assert eng.puct_counts() == (0, 0)
    eng.close()
    arena = ag.Engine(board_size=5, tower_height=1, games=2, num_readouts=8, arena_mode=1)
    arena.set_puct(0.2, CB)                                                   # an arena engine takes it
    arena.close()

"""Batched analysis (agz_analyze_*, alphago_jl_amd.analyze): suggest_move over many positions in one device run.

Position i must give bit for bit what MCTSPlayer(seed, game id base + i) + initialize_game(pos_i) + suggest_move() gives:
checked against the oracle's player (or_player_*) and against the single-tree path (MCTSPlayer)."""
import ctypes as C

import numpy as np
import pytest

import alphago_jl_amd as ag
import orc
from gpu_common import GpuNetForOracle
from test_hostsim_selfplay import OracleNet, bits_equal

pytestmark = pytest.mark.gpu
L = orc.lib()
OK, BAD_ARGUMENT, POOL_EXHAUSTED = ag._lib.OK, ag._lib.BAD_ARGUMENT, ag._lib.POOL_EXHAUSTED


# ---------------------------------------------------------------- oracle positions

def random_game(N, seed, nmoves):
    """oracle positions along a random game (no passes): captures and ko fights come up on their own"""
    rng = np.random.RandomState(seed)
    pos = orc.make_pos(N)
    out = [pos.copy()]
    legal = np.zeros(N * N + 1, np.int8)
    for _ in range(nmoves):
        L.or_all_legal_moves(C.byref(pos), legal.ctypes.data_as(C.POINTER(C.c_int8)))
        cand = np.flatnonzero(legal[:N * N])
        if len(cand) == 0:
            break
        _, pos = orc.play(pos, int(rng.choice(cand)))
        out.append(pos.copy())
    return out


def case_positions(N):
    """the cases the contract names: empty board, short history, captures with a live ko, only pass legal, a finished
    position, n on both sides of tau_threshold"""
    P = N * N
    tau = (P // 12) // 2 * 2
    out = [orc.make_pos(N)]                                        # empty board, n = 0 < tau: soft pick
    g = random_game(N, 1, 3)
    out.append(g[min(3, len(g) - 1)])                              # history_len 3 < 7
    ko = None
    for s in range(200):                                           # captures and a live ko
        for p in random_game(N, 100 + s, 3 * P):
            if p.ko >= 0 and (p.caps[0] + p.caps[1]) > 0 and p.n > tau:
                ko = p
                break
        if ko is not None:
            break
    assert ko is not None
    out.append(ko)
    mid = random_game(N, 7, P // 2)
    out.append(mid[-1])                                            # mid-game, n > tau: arg-max pick
    b = np.ones(P, np.int8)                                        # one Black group with two eyes: White may only pass
    b[0] = b[P - 1] = 0
    out.append(orc.make_pos(N, board=b, n=tau + 3, to_play=orc.WHITE))
    fin = random_game(N, 11, P // 3)[-1]                           # two passes: a finished position
    _, fin = orc.play(fin, P)
    _, fin = orc.play(fin, P)
    assert fin.done
    out.append(fin)
    return out


def opos_arrays(positions):
    """oracle positions -> agz_analyze_start's (boards, info, history)"""
    N = positions[0].N
    P, B = N * N, len(positions)
    boards = np.zeros((B, P), np.int8)
    hist = np.zeros((B, 7, P), np.int8)
    infos = (ag._lib.PositionInfo * B)()
    for k, p in enumerate(positions):
        boards[k] = p.board_np()
        cur = boards[k].astype(np.int16)
        for d in range(p.ndeltas):
            cur = cur - np.frombuffer(p.deltas[d], np.int8, count=P)
            hist[k, d] = cur
        f = infos[k]
        f.n, f.to_play, f.ko = p.n, p.to_play, p.ko
        f.caps_black, f.caps_white = p.caps[0], p.caps[1]
        f.last_move = p.recent_move[p.recent_len - 1] if p.recent_len > 0 else -1
        f.prev_move = p.recent_move[p.recent_len - 2] if p.recent_len > 1 else -1
        f.history_len = p.ndeltas
        f.komi = p.komi
    return boards, infos, hist


def oracle_suggest(N, net_cb, R, seed, game, pos, two_player=0):
    """MCTSPlayer + initialize_game! + suggest_move on the oracle: move, status, root N / W and its rows"""
    A = N * N + 1
    op = L.or_player_new(N, net_cb, None, R, two_player, -0.9, seed, game)
    L.or_player_initialize_game(op, C.byref(pos))
    n0 = L.or_node_N(L.or_player_root(op))
    while L.or_node_N(L.or_player_root(op)) < n0 + R:
        L.or_player_tree_search(op, 8)
    a = C.c_int(-1)
    st = L.or_player_pick_move(op, C.byref(a))
    root = L.or_player_root(op)
    out = dict(move=a.value if st == orc.OK else -1, status=st, N=np.float32(L.or_node_N(root)),
               W=np.float32(L.or_node_W(root)),
               child_N=orc.node_arr(L.or_node_child_N(root), A).copy(),
               child_W=orc.node_arr(L.or_node_child_W(root), A).copy(),
               prior=orc.node_arr(L.or_node_child_prior(root), A).copy())
    L.or_player_free(op)
    return out


def run_analysis(eng, boards, infos, hist, base=0, network=None, max_steps=100000):
    eng.analyze_start(boards, infos, hist, base)
    B = boards.shape[0]
    for _ in range(max_steps):
        if eng.analyze_progress() >= B:
            break
        if network is None:
            eng.step(8)
        else:
            eng.step_external(network)
    return eng.analyze_results()


def assert_row_equal(r, k, o, what):
    assert int(r["move"][k]) == o["move"], (what, k, int(r["move"][k]), o["move"])
    assert int(r["status"][k]) == o["status"], (what, k)
    assert bits_equal(r["N"][k], o["N"]) and bits_equal(r["W"][k], o["W"]), (what, k, r["N"][k], o["N"])
    for f in ("child_N", "child_W", "prior"):
        assert bits_equal(r[f][k], o[f]), (what, k, f)


# ---------------------------------------------------------------- 1. against the oracle, external network

@pytest.mark.parametrize("N,R,slots", [(5, 16, 3), (9, 32, 4)])
def test_external_network_matches_oracle(N, R, slots):
    net = OracleNet(N, 1, seed=0)
    positions = case_positions(N)
    seed, base = 5, 40
    eng = ag.Engine(board_size=N, tower_height=0, games=slots, num_readouts=R, seed=seed, external_network=1)
    r = run_analysis(eng, *opos_arrays(positions), base=base, network=net.on_feats)
    assert slots < len(positions)
    for k, pos in enumerate(positions):
        o = oracle_suggest(N, net.cb, R, seed, base + k, pos)
        assert o["status"] == orc.OK
        assert_row_equal(r, k, o, "oracle")
        assert r["status"][k] == OK and r["N"][k] >= R
        assert r["Q"][k] == np.float32(r["W"][k] / (np.float32(1) + r["N"][k]))
    # the records ring is not written by analysis, and the per-position statuses are all OK
    assert eng.records_count() == 0
    eng.close()
    net.close()


def test_two_player_mode_matches_oracle():
    N, R = 5, 16
    net = OracleNet(N, 1, seed=3)
    positions = case_positions(N)[:4]
    eng = ag.Engine(board_size=N, tower_height=0, games=2, num_readouts=R, seed=9, external_network=1, two_player_mode=1)
    r = run_analysis(eng, *opos_arrays(positions), base=0, network=net.on_feats)
    for k, pos in enumerate(positions):
        assert_row_equal(r, k, oracle_suggest(N, net.cb, R, 9, k, pos, two_player=1), "two_player")
    eng.close()
    net.close()


# ---------------------------------------------------------------- 2. engine's own network vs MCTSPlayer

def api_positions(env, seed, count, max_moves):
    """Positions of the public API along random games (board_deltas, recent, ko, caps as play_move makes them)"""
    rng = np.random.RandomState(seed)
    out = [ag.Position(env)]
    while len(out) < count:
        pos = ag.Position(env)
        for _ in range(rng.randint(1, max_moves)):
            legal = np.flatnonzero(pos.all_legal_moves()[:-1])
            if len(legal) == 0:
                break
            pos = pos.play_move(ag.from_flat(int(rng.choice(legal)), env))
        out.append(pos)
    return out


def mcts_player_result(env, nn, pos, R, seed, game_id, symmetry=None, two_player_mode=False):
    p = ag.MCTSPlayer(env, nn, num_readouts=R, seed=seed, game_id=game_id, symmetry=symmetry,
                      two_player_mode=two_player_mode)
    p.initialize_game(pos)
    mv = p.suggest_move()
    root = p.root
    out = dict(move=ag.to_flat(mv, env), status=OK, N=np.float32(root.N), W=np.float32(root.W),
               child_N=root.child_N, child_W=root.child_W, prior=root.child_prior)
    p.engine.close()
    return out


def check_against_player(env, nn, positions, res, R, seed, base, **kw):
    for k, pos in enumerate(positions):
        o = mcts_player_result(env, nn, pos, R, seed, base + k, **kw)
        a = res[k]
        assert a.status == OK and a.game_id == base + k
        assert ag.to_flat(a.move, env) == o["move"], (k, a.move, o["move"])
        assert bits_equal(a.N, o["N"]) and bits_equal(a.W, o["W"]), k
        for f, g in (("child_N", a.child_N), ("child_W", a.child_W), ("prior", a.prior)):
            assert bits_equal(g, o[f]), (k, f)
        assert bits_equal(a.child_Q, a.child_W / (np.float32(1) + a.child_N))


@pytest.mark.parametrize("N,tower,R,count,slots", [(9, 2, 32, 7, 3), (19, 1, 16, 3, 2)])
def test_internal_network_matches_mcts_player(N, tower, R, count, slots):
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=tower, seed=1)
    positions = api_positions(env, 3, count, 3 * N)
    res = ag.analyze(env, nn, positions, num_readouts=R, seed=4, game_id_base=100, slots=slots)
    check_against_player(env, nn, positions, res, R, 4, 100)


def test_configs1_shape_matches_oracle():
    """BASELINE configs[1]: 9x9, tower 10, R = 400, 64 positions; the oracle's search runs on the HIP network"""
    N, R, B = 9, 400, 64
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=10, seed=0)
    positions = []
    for s in range(B):
        g = random_game(N, 1000 + s, 40)
        positions.append(g[min(len(g) - 1, (s * 7) % 40)])
    eng = ag.Engine(board_size=N, tower_height=10, games=32, num_readouts=R, seed=6, max_nodes_per_game=2 * R + 256)
    nn.engine.copy_weights_to(eng)
    r = run_analysis(eng, *opos_arrays(positions), base=0)
    fwd = GpuNetForOracle(nn.engine)
    for k, pos in enumerate(positions):
        assert_row_equal(r, k, oracle_suggest(N, fwd.cb, R, 6, k, pos), "configs[1]")
    eng.close()


# ---------------------------------------------------------------- 3. independence of scheduling

def test_results_do_not_depend_on_slots_or_splitting():
    N, R = 5, 16
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=2)
    positions = api_positions(env, 8, 10, 12)
    B = len(positions)
    runs = [ag.analyze(env, nn, positions, num_readouts=R, seed=1, game_id_base=50, slots=s) for s in (1, 3, 64)]
    half = B // 2
    split = (ag.analyze(env, nn, positions[:half], num_readouts=R, seed=1, game_id_base=50)
             + ag.analyze(env, nn, positions[half:], num_readouts=R, seed=1, game_id_base=50 + half))
    for other in runs[1:] + [split]:
        for a, b in zip(runs[0], other):
            assert a.move == b.move and a.status == b.status and a.game_id == b.game_id
            for f in ("N", "W", "Q", "child_N", "child_W", "prior"):
                assert bits_equal(getattr(a, f), getattr(b, f)), f


# ---------------------------------------------------------------- 4. symmetry

@pytest.mark.parametrize("symmetry", ["random", 3])
def test_symmetry_matches_mcts_player(symmetry):
    N, R = 5, 16
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=5)
    positions = api_positions(env, 9, 5, 10)
    res = ag.analyze(env, nn, positions, num_readouts=R, seed=2, game_id_base=7, slots=2, symmetry=symmetry)
    check_against_player(env, nn, positions, res, R, 2, 7, symmetry=symmetry)


# ---------------------------------------------------------------- 5. invalid positions

def test_invalid_boards_fail_alone():
    N, R = 5, 16
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=6)
    good = api_positions(env, 10, 3, 8)
    dead = np.zeros((N, N), np.int8)
    dead[0, 0], dead[0, 1], dead[1, 0] = 1, -1, -1                # a Black stone without a liberty
    two = np.zeros((N, N), np.int8)
    two[2, 2] = 2                                                 # not a stone value
    ko = np.zeros((N, N), np.int8)
    ko[1, 1] = 1                                                  # the ko point is occupied
    bad = [ag.Position(env, board=dead, n=3), ag.Position(env, board=two, n=1),
           ag.Position(env, board=ko, n=1, ko=(1, 1), to_play=ag.WHITE)]
    positions = [good[0], bad[0], good[1], bad[1], bad[2], good[2]]
    res = ag.analyze(env, nn, positions, num_readouts=R, seed=3, game_id_base=0, slots=2)
    for k in (1, 3, 4):
        assert res[k].status == BAD_ARGUMENT and res[k].move is None and res[k].N == 0, k
    for k in (0, 2, 5):
        o = mcts_player_result(env, nn, positions[k], R, 3, k)
        assert res[k].status == OK and ag.to_flat(res[k].move, env) == o["move"]
        assert bits_equal(res[k].child_N, o["child_N"]) and bits_equal(res[k].prior, o["prior"])


def test_bad_scalar_field_fails_the_call():
    N = 5
    eng = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=8)
    eng.init_synthetic(0)
    boards, infos, hist = opos_arrays([orc.make_pos(N)] * 4)
    for field, value in (("to_play", 0), ("history_len", 8), ("n", -1), ("last_move", N * N + 1), ("ko", N * N)):
        bad = (ag._lib.PositionInfo * 4)(*infos)
        setattr(bad[2], field, value)
        with pytest.raises(ag.AgzError) as ex:
            eng.analyze_start(boards, bad, hist)
        assert ex.value.status == BAD_ARGUMENT and "position 2" in str(ex.value), field
    with pytest.raises(ag.AgzError) as ex:
        eng.analyze_results()
    assert ex.value.status == BAD_ARGUMENT
    env = ag.GoEnv(N)
    with pytest.raises(ag.AgzError):
        ag.analyze(env, ag.NeuralNet(env, tower_height=1), [ag.Position(env, to_play=0)], num_readouts=8)
    eng.close()
    arena = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=8, arena_mode=1)
    with pytest.raises(ag.AgzError) as ex:
        arena.analyze_start(boards, infos, hist)
    assert ex.value.status == BAD_ARGUMENT
    arena.close()


def test_results_not_ready_until_done():
    N = 5
    eng = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=32)
    eng.init_synthetic(0)
    eng.analyze_start(*opos_arrays([orc.make_pos(N)] * 3))
    eng.step(1)
    assert eng.analyze_progress() < 3
    with pytest.raises(ag.AgzError) as ex:
        eng.analyze_results()
    assert ex.value.status == ag._lib.NOT_READY
    while eng.analyze_progress() < 3:
        eng.step(4)
    assert (eng.analyze_results()["status"] == OK).all()
    eng.close()


# ---------------------------------------------------------------- 6. pool

def test_small_pool_moves_early():
    N, R = 5, 64
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=7)
    positions = api_positions(env, 12, 4, 6)
    res = ag.analyze(env, nn, positions, num_readouts=R, seed=1, slots=2, max_nodes_per_game=24)
    short = [a for a in res if a.status == POOL_EXHAUSTED]
    assert short
    for a in short:
        assert a.N < R and a.move is not None and a.nodes_used == 24


def test_stall_policy_and_abandon():
    N, R = 5, 64
    eng = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=R, max_nodes_per_game=24, pool_policy=1)
    eng.init_synthetic(0)
    eng.analyze_start(*opos_arrays([orc.make_pos(N)] * 3))
    abandoned = 0
    for _ in range(2000):
        if eng.analyze_progress() >= 3:
            break
        eng.step(1)
        st, _, _ = eng.slot_status()
        for g in np.flatnonzero(st == POOL_EXHAUSTED):
            eng.slot_abandon(int(g))
            abandoned += 1
    r = eng.analyze_results()
    assert abandoned == 3 and (r["status"] == POOL_EXHAUSTED).all() and (r["move"] == -1).all()
    assert eng.stats()["abandoned_games"] == 0
    eng.close()


# ---------------------------------------------------------------- 7. self-play is not changed

def test_selfplay_after_analysis_is_unchanged():
    N, games = 5, 4
    kw = dict(board_size=N, tower_height=1, games=3, num_readouts=16, seed=2, record_capacity_games=games + 8)

    def play(eng):
        eng.start(games)
        for _ in range(20000):
            eng.step(8)
            if eng.stats()["games_finished"] >= games:
                break
        return sorted(eng.records(), key=lambda r: int(r["game_id"]))

    eng = ag.Engine(**kw)
    eng.init_synthetic(0)
    first = play(eng)
    st0 = eng.stats()
    run_analysis(eng, *opos_arrays(case_positions(N)))
    st1 = eng.stats()
    assert eng.records_count() == games
    for f in ("positions", "games_started", "games_finished", "resigned_games", "abandoned_games"):
        assert st1[f] == st0[f], f
    second = play(eng)
    fresh = ag.Engine(**kw)
    fresh.init_synthetic(0)
    ref = play(fresh)
    for recs in (first, second):
        assert len(recs) == len(ref)
        for a, b in zip(recs, ref):
            assert a["game_id"] == b["game_id"] and a["num_moves"] == b["num_moves"]
            assert (a["moves"] == b["moves"]).all() and bits_equal(a["pis"], b["pis"]) and bits_equal(a["qs"], b["qs"])
    eng.close()
    fresh.close()

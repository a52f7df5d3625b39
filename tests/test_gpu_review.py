"""Batched game review (agz_review_start, alphago_jl_amd.review): play() over recorded games on reused trees.

Row k of game j must give bit for bit what MCTSPlayer(seed, game id base + j) + initialize_game(start_j), then k times
suggest_move() / play_move(m_i), then suggest_move() gives: checked against the oracle's player (or_player_*) and against
the single-tree path (MCTSPlayer), with the recorded move -- not the suggested one -- re-rooting the tree."""
import ctypes as C

import numpy as np
import pytest

import alphago_jl_amd as ag
import orc
from test_hostsim_selfplay import OracleNet, bits_equal

pytestmark = pytest.mark.gpu
L = orc.lib()
OK, BAD_ARGUMENT, POOL_EXHAUSTED = ag._lib.OK, ag._lib.BAD_ARGUMENT, ag._lib.POOL_EXHAUSTED


# ---------------------------------------------------------------- games

def oracle_selfplay_moves(N, net, R, seed, game, max_moves):
    """the moves of one oracle self-play game (or_selfplay), flat actions"""
    p = L.or_selfplay(N, net.cb, None, R, seed, game, max_moves)
    pos = L.or_node_pos(L.or_player_root(p)).contents
    moves = [int(pos.recent_move[k]) for k in range(pos.recent_len)]
    L.or_player_free(p)
    return moves


def random_moves(N, seed, nmoves, pass_prob=0.15):
    """a random legal game of oracle positions with passes (never two in a row, so the game goes on)"""
    rng = np.random.RandomState(seed)
    P = N * N
    pos = orc.make_pos(N)
    out = []
    for _ in range(nmoves):
        cand = np.flatnonzero(orc.legal_moves(pos)[:P])
        if len(cand) == 0 or (rng.rand() < pass_prob and (not out or out[-1] != P)):
            a = P
        else:
            a = int(rng.choice(cand))
        rc, pos = orc.play(pos, a)
        assert rc == orc.OK
        out.append(a)
    return out


def oracle_review(N, net_cb, R, seed, game, moves, two_player):
    """the play() loop on the oracle: suggest_move's row, then play_move!(m_k)"""
    A = N * N + 1
    op = L.or_player_new(N, net_cb, None, R, two_player, -0.9, seed, game)
    L.or_player_initialize_game(op, None)
    rows = []
    for m in moves:
        n0 = L.or_node_N(L.or_player_root(op))
        while L.or_node_N(L.or_player_root(op)) < n0 + R:
            L.or_player_tree_search(op, 8)
        a = C.c_int(-1)
        st = L.or_player_pick_move(op, C.byref(a))
        root = L.or_player_root(op)
        rows.append(dict(move=a.value if st == orc.OK else -1, status=st, N=np.float32(L.or_node_N(root)),
                         W=np.float32(L.or_node_W(root)),
                         child_N=orc.node_arr(L.or_node_child_N(root), A).copy(),
                         child_W=orc.node_arr(L.or_node_child_W(root), A).copy(),
                         prior=orc.node_arr(L.or_node_child_prior(root), A).copy()))
        assert L.or_player_play_move(op, m) == 1
    L.or_player_free(op)
    return rows


def offsets(games):
    return np.concatenate([[0], np.cumsum([len(g) for g in games])]).astype(np.int64)


def run_review(eng, games, base=0, network=None, starts=None, max_steps=200000):
    moves = np.array([m for g in games for m in g], np.int16)
    off = offsets(games)
    eng.review_start(moves, off, *(starts or (None, None, None)), game_id_base=base)
    for _ in range(max_steps):
        if eng.review_progress() >= off[-1]:
            break
        if network is None:
            eng.step(8)
        else:
            eng.step_external(network)
    return eng.review_results(), off


def assert_row_equal(r, i, o, what):
    assert int(r["move"][i]) == o["move"], (what, i, int(r["move"][i]), o["move"])
    assert int(r["status"][i]) == o["status"], (what, i)
    assert bits_equal(r["N"][i], o["N"]) and bits_equal(r["W"][i], o["W"]), (what, i, r["N"][i], o["N"])
    for f in ("child_N", "child_W", "prior"):
        assert bits_equal(r[f][i], o[f]), (what, i, f)


def assert_tree_reuse(N_rows, child_N_rows, moves, R):
    """row k's N >= row k-1's child_N[m_{k-1}] + R; returns whether some row kept visits beyond the new R"""
    kept = False
    for k in range(1, len(moves)):
        inherited = child_N_rows[k - 1][moves[k - 1]]
        assert N_rows[k] >= inherited + R, (k, N_rows[k], inherited)
        kept |= inherited > 0 and N_rows[k] > R
    return kept


# ---------------------------------------------------------------- 1. against the oracle, external network

@pytest.mark.parametrize("N,R,slots,two_player", [(5, 16, 1, 1), (5, 40, 3, 0), (9, 16, 8, 1), (9, 40, 3, 1)])
def test_external_network_matches_oracle(N, R, slots, two_player):
    net = OracleNet(N, 1, seed=0)
    P = N * N
    sp_len = 2 * P if N == 5 else 24
    games = [oracle_selfplay_moves(N, net, 8, 3, 70 + s, sp_len) for s in range(2)]
    games += [random_moves(N, 200 + s, P // 2 + 3 * s) for s in range(3)]
    games.append([])                                              # a game without moves has no rows
    assert any(P in g for g in games)
    seed, base = 5, 40
    eng = ag.Engine(board_size=N, tower_height=0, games=slots, num_readouts=R, seed=seed, external_network=1,
                    two_player_mode=two_player)
    r, off = run_review(eng, games, base=base, network=net.on_feats)
    assert len(r["move"]) == off[-1]
    kept = False
    for j, g in enumerate(games):
        rows = oracle_review(N, net.cb, R, seed, base + j, g, two_player)
        for k, o in enumerate(rows):
            assert o["status"] in (orc.OK, orc.ASSERT_SOFTPICK)          # the soft pick's assertion is a row too
            assert_row_equal(r, off[j] + k, o, f"oracle game {j} ply {k}")
            assert r["Q"][off[j] + k] == np.float32(r["W"][off[j] + k] / (np.float32(1) + r["N"][off[j] + k]))
        s = slice(off[j], off[j + 1])
        kept |= assert_tree_reuse(r["N"][s], r["child_N"][s], g, R)
    assert kept, "no ply inherited visits from the previous search"
    assert eng.records_count() == 0
    eng.close()
    net.close()


# ---------------------------------------------------------------- 2. engine's own network vs MCTSPlayer

def api_game(env, seed, nmoves, start=None):
    """a random legal move list (board coordinates, passes included) from `start`"""
    rng = np.random.RandomState(seed)
    pos = ag.Position(env) if start is None else start
    out = []
    for _ in range(nmoves):
        legal = np.flatnonzero(pos.all_legal_moves()[:-1])
        c = None if len(legal) == 0 or rng.rand() < 0.1 else ag.from_flat(int(rng.choice(legal)), env)
        if c is None and out and out[-1] is None:
            c = ag.from_flat(int(rng.choice(legal)), env)
        pos = pos.play_move(c)
        out.append(c)
    return out


def player_review(env, nn, moves, R, seed, game_id, start=None, symmetry=None, two_player_mode=True):
    p = ag.MCTSPlayer(env, nn, num_readouts=R, seed=seed, game_id=game_id, symmetry=symmetry,
                      two_player_mode=two_player_mode)
    p.initialize_game(start)
    rows = []
    for m in moves:
        mv = p.suggest_move()
        root = p.root
        rows.append(dict(move=mv, N=np.float32(root.N), W=np.float32(root.W), child_N=root.child_N,
                         child_W=root.child_W, prior=root.child_prior))
        assert p.play_move(m)
    p.engine.close()
    return rows


def check_against_player(env, nn, games, res, R, seed, base, starts=None, **kw):
    for j, g in enumerate(games):
        rows = player_review(env, nn, g, R, seed, base + j, None if starts is None else starts[j], **kw)
        assert len(res[j]) == len(g)
        for k, (a, o) in enumerate(zip(res[j], rows)):
            assert a.status == OK and a.game_id == base + j
            assert a.move == o["move"], (j, k, a.move, o["move"])
            assert bits_equal(a.N, o["N"]) and bits_equal(a.W, o["W"]), (j, k)
            for f, v in (("child_N", a.child_N), ("child_W", a.child_W), ("prior", a.prior)):
                assert bits_equal(v, o[f]), (j, k, f)
            assert bits_equal(a.child_Q, a.child_W / (np.float32(1) + a.child_N))


@pytest.mark.parametrize("N,tower,R,nmoves,slots,symmetry", [(9, 2, 32, 14, 2, None), (9, 2, 16, 10, 3, "random"),
                                                              (19, 1, 16, 6, 2, None)])
def test_internal_network_matches_mcts_player(N, tower, R, nmoves, slots, symmetry):
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=tower, seed=1)
    mid = ag.Position(env, komi=5.5)                              # a mid-game start: history, captures state, komi
    for c in api_game(env, 77, 9):
        mid = mid.play_move(c)
    starts = [None, mid, ag.Position(env, komi=6.5)]
    games = [api_game(env, 10 + j, nmoves, None if s is None else s) for j, s in enumerate(starts)]
    res = ag.review(env, nn, games, num_readouts=R, starts=starts, seed=4, game_id_base=100, slots=slots,
                    symmetry=symmetry)
    check_against_player(env, nn, games, res, R, 4, 100, starts=starts, symmetry=symmetry)
    for j, g in enumerate(games):
        flat = [ag.to_flat(c, env) for c in g]
        assert_tree_reuse([a.N for a in res[j]], [a.child_N for a in res[j]], flat, R)


def test_soft_pick_and_default_start_match_mcts_player():
    N, R = 9, 16
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=3)
    games = [api_game(env, 30 + j, 12) for j in range(3)]
    res = ag.review(env, nn, games, num_readouts=R, two_player_mode=False, seed=8, game_id_base=3, slots=2)
    check_against_player(env, nn, games, res, R, 8, 3, two_player_mode=False)


# ---------------------------------------------------------------- 3. independence of scheduling; input forms

def test_results_do_not_depend_on_slots_or_splitting():
    N, R = 5, 16
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=2)
    games = [api_game(env, 50 + j, 4 + 2 * j) for j in range(9)]
    G = len(games)
    runs = [ag.review(env, nn, games, num_readouts=R, seed=1, game_id_base=50, slots=s) for s in (1, 7, 64)]
    half = G // 2
    split = (ag.review(env, nn, games[:half], num_readouts=R, seed=1, game_id_base=50)
             + ag.review(env, nn, games[half:], num_readouts=R, seed=1, game_id_base=50 + half))
    flat = [[ag.to_flat(c, env) for c in g] for g in games]       # the same games as flat actions
    runs.append(ag.review(env, nn, flat, num_readouts=R, seed=1, game_id_base=50, slots=3))
    for other in runs[1:] + [split]:
        assert len(other) == G
        for ga, gb in zip(runs[0], other):
            assert len(ga) == len(gb)
            for a, b in zip(ga, gb):
                assert a.move == b.move and a.status == b.status and a.game_id == b.game_id
                for f in ("N", "W", "Q", "child_N", "child_W", "prior"):
                    assert bits_equal(getattr(a, f), getattr(b, f)), f


def test_selfplay_players_and_records_review_alike():
    N, R = 5, 16
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=4)
    players = ag.selfplay(env, nn, 16, games=3, seed=2, game_id_base=0)
    a = ag.review(env, nn, players, num_readouts=R, seed=1)
    b = ag.review(env, nn, [p.moves for p in players], num_readouts=R, seed=1)
    assert [len(g) for g in a] == [len(p.moves) for p in players]
    for ga, gb in zip(a, b):
        for x, y in zip(ga, gb):
            assert x.status == OK and x.move == y.move and bits_equal(x.child_N, y.child_N)


# ---------------------------------------------------------------- 4. invalid records

def ko_game(env, seed_from=0):
    """a random legal game that ends with a live ko, and the ko point (its immediate recapture is illegal)"""
    for s in range(seed_from, seed_from + 400):
        rng = np.random.RandomState(s)
        pos, moves = ag.Position(env), []
        for _ in range(4 * env.N * env.N):
            legal = np.flatnonzero(pos.all_legal_moves()[:-1])
            if len(legal) == 0:
                break
            c = ag.from_flat(int(rng.choice(legal)), env)
            pos = pos.play_move(c)
            moves.append(c)
            if pos.ko is not None:
                return moves, pos.ko
    raise AssertionError("no ko found")


def test_invalid_records_fail_alone():
    N, R = 5, 16
    env = ag.GoEnv(N)
    P = N * N
    nn = ag.NeuralNet(env, tower_height=1, seed=6)
    ko_moves, ko_pt = ko_game(env)
    clean = [[12, 7, 11], [1, 20, 5], ko_moves, [12, P, P], [6, 18, 8, 16]]
    bad = [[12, 7, 11, 12, 13],                                   # occupied point
           [1, 20, 5, 0, 3],                                      # suicide: White in Black's corner
           ko_moves + [ko_pt, None],                              # ko recapture
           [12, P, P, 7],                                         # a move after two passes
           [6, 18, 8, 16]]                                        # a clean game beside them
    assert not ag.Position(env).play_move(ag.from_flat(1, env)).play_move(ag.from_flat(20, env)) \
        .play_move(ag.from_flat(5, env)).is_move_legal(ag.from_flat(0, env))
    res = ag.review(env, nn, bad, num_readouts=R, seed=3, game_id_base=0, slots=2)
    ref = ag.review(env, nn, clean, num_readouts=R, seed=3, game_id_base=0, slots=3)
    for j, (rb, rc) in enumerate(zip(res, ref)):
        n_ok = len(clean[j])
        assert len(rb) == len(bad[j])
        for k in range(n_ok):
            assert rb[k].status == OK and rb[k].move == rc[k].move, (j, k)
            for f in ("N", "W", "child_N", "child_W", "prior"):
                assert bits_equal(getattr(rb[k], f), getattr(rc[k], f)), (j, k, f)
        for k in range(n_ok, len(bad[j])):
            assert rb[k].status == BAD_ARGUMENT and rb[k].move is None and rb[k].N == 0, (j, k)


def test_host_range_errors_fail_the_call():
    N = 5
    P = N * N
    eng = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=8)
    eng.init_synthetic(0)
    cases = [(np.array([1, 2, P + 1], np.int16), [0, 2, 3], "game 1"),
             (np.array([1, -1, 3], np.int16), [0, 2, 3], "game 0"),
             (np.array([1, 2, 3], np.int16), [0, 2, 1, 3], "game 1")]
    for moves, off, what in cases:
        with pytest.raises(ag.AgzError) as ex:
            eng.review_start(moves, off)
        assert ex.value.status == BAD_ARGUMENT and what in str(ex.value), (off, str(ex.value))
    boards = np.zeros((2, P), np.int8)
    infos = (ag._lib.PositionInfo * 2)()
    for f in infos:
        f.to_play, f.ko, f.last_move, f.prev_move, f.komi = 1, -1, -1, -1, 7.5
    infos[1].to_play = 0
    with pytest.raises(ag.AgzError) as ex:
        eng.review_start(np.array([1, 2, 3], np.int16), [0, 2, 3], boards, infos)
    assert ex.value.status == BAD_ARGUMENT and "game 1" in str(ex.value)
    env = ag.GoEnv(N)
    with pytest.raises(ag.AgzError):
        ag.review(env, ag.NeuralNet(env, tower_height=1), [[1, 2]], starts=[ag.Position(env, to_play=0)],
                  num_readouts=8)
    eng.close()
    arena = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=8, arena_mode=1)
    with pytest.raises(ag.AgzError) as ex:
        arena.review_start(np.array([1], np.int16), [0, 1])
    assert ex.value.status == BAD_ARGUMENT
    arena.close()


# ---------------------------------------------------------------- 5. pool

def test_small_pool_moves_early_and_the_game_goes_on():
    N, R = 5, 64
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=7)
    games = [api_game(env, 60 + j, 8) for j in range(3)]
    res = ag.review(env, nn, games, num_readouts=R, seed=1, slots=2, max_nodes_per_game=24)
    rows = [a for g in res for a in g]
    assert len(rows) == sum(len(g) for g in games)
    short = [a for a in rows if a.status == POOL_EXHAUSTED]
    assert short
    for a in short:                                      # a valid short row (move None is a pass)
        assert 0 < a.N and a.nodes_used == 24 and a.child_N.sum() > 0
    assert all(a.status in (OK, POOL_EXHAUSTED) for a in rows)


def test_stall_policy_and_abandon_give_up_the_game():
    N, R = 5, 64
    eng = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=R, max_nodes_per_game=24, pool_policy=1)
    eng.init_synthetic(0)
    games = [[12, 7, 11], [6, 18], [2, 3, 4, 8]]
    moves = np.array([m for g in games for m in g], np.int16)
    off = offsets(games)
    eng.review_start(moves, off)
    abandoned = 0
    for _ in range(3000):
        if eng.review_progress() >= off[-1]:
            break
        eng.step(1)
        st, _, _ = eng.slot_status()
        for g in np.flatnonzero(st == POOL_EXHAUSTED):
            eng.slot_abandon(int(g))
            abandoned += 1
    r = eng.review_results()
    assert 1 <= abandoned <= len(games)
    assert (r["status"] == POOL_EXHAUSTED).any()
    for j in range(len(games)):
        s = r["status"][off[j]:off[j + 1]]
        first = np.flatnonzero(s == POOL_EXHAUSTED)
        if len(first):                                   # given up: every later row too, move -1 from there on
            k = first[0]
            assert (s[k:] == POOL_EXHAUSTED).all() and (r["move"][off[j] + k:off[j + 1]] == -1).all()
    assert eng.stats()["abandoned_games"] == 0
    eng.close()


# ---------------------------------------------------------------- 6. self-play and analysis are not changed

def test_selfplay_and_analysis_after_review_are_unchanged():
    N, games = 5, 4
    kw = dict(board_size=N, tower_height=1, games=3, num_readouts=16, seed=2, record_capacity_games=games + 8)

    def play(eng):
        eng.start(games)
        for _ in range(20000):
            eng.step(8)
            if eng.stats()["games_finished"] >= games:
                break
        return sorted(eng.records(), key=lambda r: int(r["game_id"]))

    def analyze(eng):
        boards = np.zeros((3, N * N), np.int8)
        infos = (ag._lib.PositionInfo * 3)()
        for k, f in enumerate(infos):
            f.to_play, f.ko, f.last_move, f.prev_move, f.komi = 1, -1, -1, -1, 7.5
            boards[k, k] = -1
        eng.analyze_start(boards, infos, None, 9)
        while eng.analyze_progress() < 3:
            eng.step(8)
        return eng.analyze_results()

    eng = ag.Engine(**kw)
    eng.init_synthetic(0)
    first = play(eng)
    st0 = eng.stats()
    r, _ = run_review(eng, [[12, 7, 11, 25], [6, 18]])
    assert (r["status"] == OK).all()
    st1 = eng.stats()
    assert eng.records_count() == games
    for f in ("positions", "games_started", "games_finished", "resigned_games", "abandoned_games"):
        assert st1[f] == st0[f], f
    second = play(eng)
    run_review(eng, [[12, 7, 11, 25], [6, 18]])
    an = analyze(eng)
    fresh = ag.Engine(**kw)
    fresh.init_synthetic(0)
    ref = play(fresh)
    ref_an = analyze(fresh)
    for recs in (first, second):
        assert len(recs) == len(ref)
        for a, b in zip(recs, ref):
            assert a["game_id"] == b["game_id"] and a["num_moves"] == b["num_moves"]
            assert (a["moves"] == b["moves"]).all() and bits_equal(a["pis"], b["pis"]) and bits_equal(a["qs"], b["qs"])
    for f in ("move", "status", "N", "W", "child_N", "prior"):
        assert bits_equal(an[f], ref_an[f]), f
    eng.close()
    fresh.close()

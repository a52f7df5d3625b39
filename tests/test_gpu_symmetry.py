"""Board symmetries on the GPU (DESIGN.md "Board symmetries"):
(1) agz_net_forward_features_sym == host transform -> agz_net_forward_features -> host un-permute, bit for bit, all eight
    s in one batch; symmetry="average" is invariant under the group (a network with a peaked policy);
(2) symmetry mode 0 through the new kernels == mode off, whole games bit for bit;
(3) whole self-play games (also with the mode switched on mid-game) and arena games with the symmetry on == the
    oracle's tree search whose network callable predicts s from the draw key, transforms, runs the plain GPU forward
    and un-permutes; MCTSPlayer searches == the same tree driven with those host-transformed evaluations;
(4) agz_replay_batch_sym == the host transform of agz_replay_batch; an augmented device batch trains;
(5) the draw is uniform over the evaluated leaves, the priors each leaf received on the device come from one of its
    game's drawn symmetries, and two engines with one seed play identical games."""
import ctypes as C

import numpy as np
import pytest

import alphago_jl_amd as ag
from alphago_jl_amd import symmetry as sy
from gpu_options import SymNetForOracle, peaked_engine, rand_feats, sharpen
from test_hostsim_arena import oracle_eval_game
from test_hostsim_selfplay import bits_equal, oracle_game

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,tower", [(9, 2), (19, 1)])
def test_forward_features_sym_is_the_host_transform(N, tower):
    e = peaked_engine(N, tower, games=1, num_readouts=8, max_nodes_per_game=16)
    x = rand_feats(N, 16, seed=N)
    sym = np.tile(np.arange(8, dtype=np.int32), 2)
    pi, v = e.forward_features_sym(x, sym)
    tx = np.stack([sy.apply_features(x[b], int(sym[b]), N) for b in range(len(x))])
    ppi, pv = e.forward_features(tx)
    want = np.stack([sy.apply_policy(ppi[b], sy.inverse(int(sym[b])), N) for b in range(len(x))])
    assert bits_equal(pi, want) and bits_equal(v, pv)
    assert ppi.max() > 0.4
    # a quarter turn really moves the policy: T_5 and T_6 of one row differ from each other and from T_0
    assert not (ppi[5] == ppi[0]).all() and not (ppi[5] == ppi[6]).all()
    e.close()


@pytest.mark.parametrize("N,tower", [(9, 2), (19, 1)])
def test_average_is_invariant(N, tower):
    nn = ag.NeuralNet(ag.GoEnv(N), tower_height=tower)
    sharpen(nn.engine, N)
    x = rand_feats(N, 3, seed=1)
    pi, v = nn.forward_features(x, symmetry="average")
    assert pi.shape == (3, N * N + 1) and v.shape == (3,)
    for s in range(1, 8):
        ps, vs = nn.forward_features(sy.apply_features(x, s, N), symmetry="average")
        assert np.abs(sy.apply_policy(ps, sy.inverse(s), N) - pi).max() <= 1e-6
        assert np.abs(vs - v).max() <= 1e-6
    # the plain network is not invariant: the average is not the identity evaluation
    p0, _ = nn.forward_features(x)
    assert p0.max() > 0.4 and np.abs(p0 - pi).max() > 1e-4
    nn.engine.close()


def run(eng, games, max_steps=100000):
    eng.start(games)
    steps = 0
    while steps < max_steps:
        eng.step(8)
        steps += 8
        if eng.stats()["games_finished"] >= games:
            break
    return eng.records(), eng.stats()


def same_records(a, b):
    assert len(a) == len(b)
    for r, o in zip(sorted(a, key=lambda r: r["game_id"]), sorted(b, key=lambda r: r["game_id"])):
        assert r["game_id"] == o["game_id"] and r["num_moves"] == o["num_moves"]
        assert (r["moves"] == o["moves"]).all() and r["result"] == o["result"]
        assert bits_equal(r["pis"], o["pis"]) and bits_equal(r["qs"], o["qs"])


def test_mode_zero_equals_off():
    N, tower, readouts, games = 9, 1, 24, 3
    out = []
    for mode in (None, 0):
        eng = peaked_engine(N, tower, games=games, num_readouts=readouts, seed=2, record_capacity_games=games + 8)
        if mode is not None:
            eng.set_symmetry(mode)
        out.append(run(eng, games))
        eng.close()
    same_records(out[0][0], out[1][0])
    assert out[0][1]["evals"] == out[1][1]["evals"] and out[0][1]["positions"] == out[1][1]["positions"]


@pytest.mark.parametrize("N,tower,readouts,games,mode", [
    (9, 1, 24, 2, sy.RANDOM),
    (9, 2, 16, 2, 5),            # a quarter turn: T_5 is not its own inverse
    (19, 1, 8, 1, sy.RANDOM),
])
def test_selfplay_with_symmetry_matches_oracle(N, tower, readouts, games, mode):
    seed = 4
    eng = peaked_engine(N, tower, games=games, num_readouts=readouts, seed=seed, record_capacity_games=games + 8)
    eng.set_symmetry(mode)
    recs, st = run(eng, games)
    assert len(recs) == games and st["pool_exhausted"] == 0
    fwd = peaked_engine(N, tower, games=1, num_readouts=8, max_nodes_per_game=16)
    evals, seen = 0, set()
    for r in recs:
        net = SymNetForOracle(fwd, seed, int(r["game_id"]), mode)
        o = oracle_game(N, net, readouts, seed, int(r["game_id"]))
        assert r["num_moves"] == o["num_moves"], r["game_id"]
        assert (r["moves"] == o["moves"][: r["num_moves"]]).all()
        assert r["result"] == o["result"]
        assert bits_equal(r["qs"], o["qs"]) and bits_equal(r["pis"], o["pis"])
        evals += o["evals"]
        seen |= set(net.syms)
    assert st["evals"] == evals
    assert seen == (set(range(8)) if mode == sy.RANDOM else {mode})
    fwd.close()
    eng.close()


@pytest.mark.parametrize("mode", [sy.RANDOM, 6])
def test_tree_search_with_symmetry_matches_host_transform(mode):
    """one MCTSPlayer search (agz_tree_search_*, engine network) under the symmetry == the same tree driven with
    the caller-supplied pi of the mirror network"""
    N, tower, seed, gid = 9, 1, 7, 11
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=tower)
    sharpen(nn.engine, N)
    a = ag.MCTSPlayer(env, nn, num_readouts=64, seed=seed, game_id=gid, symmetry="random" if mode == sy.RANDOM else mode)
    b = ag.MCTSPlayer(env, nn, num_readouts=64, seed=seed, game_id=gid)
    a.initialize_game()
    b.initialize_game()
    mirror = SymNetForOracle(nn.engine, seed, gid, mode)
    for _ in range(6):
        a.tree_search(8)
        e = b.engine
        n = e.tree_search_select(0, 8)
        if n == 0:
            e.tree_search_incorporate(0)
            continue
        lp = e.tree_leaf_positions(0, n)
        feats = nn.engine.features(lp["boards"], lp["deltas"], lp["ndeltas"], lp["to_play"])
        sym = []
        for _ in range(n):
            sym.append(mode if mode != sy.RANDOM else sy.draw_symmetry(seed, gid, mirror.e))
            mirror.e += 1
        gpi, gv = nn.engine.forward_features(np.stack([sy.apply_features(feats[k], sym[k], N) for k in range(n)]))
        gpi = np.stack([sy.apply_policy(gpi[k], sy.inverse(sym[k]), N) for k in range(n)])
        e.tree_search_incorporate(0, gpi, gv)
    ra, rb = a.engine.tree_root(0), b.engine.tree_root(0)
    for f in (0, 1, 2):
        assert bits_equal(a.engine.node_floats(0, ra, f), b.engine.node_floats(0, rb, f)), f
    ia, ib = a.engine.node_info(0, ra), b.engine.node_info(0, rb)
    assert ia.N == ib.N and ia.W == ib.W and ia.N > 30
    for p in (a, b):
        p.engine.close()
    nn.engine.close()


def test_arena_with_symmetry_matches_oracle():
    N, tower, readouts, games, seed = 9, 1, 16, 2, 3
    eng = ag.Engine(board_size=N, tower_height=tower, games=4, num_readouts=readouts, seed=seed, arena_mode=1,
                    record_capacity_games=games + 8)
    eng.init_synthetic(0)
    eng.net_select(1)
    eng.init_synthetic(5)
    eng.net_select(0)
    eng.set_symmetry("random")
    recs, st = run(eng, games)
    assert len(recs) == games and st["pool_exhausted"] == 0
    fb = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=8, max_nodes_per_game=16)
    fw = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=8, max_nodes_per_game=16)
    fb.init_synthetic(0)
    fw.init_synthetic(5)
    evals = 0
    for r in recs:
        g = int(r["game_id"]) // 2
        black = SymNetForOracle(fb, seed, 2 * g, sy.RANDOM)
        white = SymNetForOracle(fw, seed, 2 * g + 1, sy.RANDOM)
        o = oracle_eval_game(N, black, white, readouts, seed, g, -0.9)
        assert r["num_moves"] == o["num_moves"] and (r["moves"] == o["moves"]).all()
        assert bits_equal(r["qs"], o["qs"]) and r["result"] == o["result"]
        evals += sum(o["evals"])
    assert evals == st["evals"]
    for e in (eng, fb, fw):
        e.close()


def test_replay_batch_sym_and_augmented_training():
    N, tower, games = 9, 1, 2
    eng = peaked_engine(N, tower, games=games, num_readouts=16, seed=5, record_capacity_games=games + 8)
    recs, _ = run(eng, games)
    eng.replay_ingest(eng.records_packed())
    assert eng.replay_count() == games
    rng = np.random.RandomState(0)
    B = 24
    game = rng.randint(0, games, B).astype(np.int64)
    hdr = [int(eng.replay_record(k)["num_moves"]) for k in range(games)]
    ply = np.array([rng.randint(0, hdr[g]) for g in game], np.int32)
    sym = np.concatenate([np.arange(8), rng.randint(0, 8, B - 8)]).astype(np.int32)
    f0, p0, z0 = eng.replay_batch(game, ply)
    f1, p1, z1 = eng.replay_batch_sym(game, ply, sym)
    for b in range(B):
        s = int(sym[b])
        assert (f1[b] == sy.apply_features(f0[b], s, N)).all(), b
        assert (p1[b] == sy.apply_policy(p0[b], s, N)).all(), b
        if s == 0:
            assert bits_equal(f1[b], f0[b]) and bits_equal(p1[b], p0[b])
    assert bits_equal(z1, z0)
    # device outputs straight into agz_train_step
    import torch
    dev = torch.device("cuda", 0)
    df = torch.empty((B, 17 * N * N), dtype=torch.float32, device=dev)
    dp = torch.empty((B, N * N + 1), dtype=torch.float32, device=dev)
    dz = torch.empty(B, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    L = eng.L
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert L.agz_replay_batch_sym(eng.h, game.ctypes.data_as(C.POINTER(C.c_int64)), ply.ctypes.data_as(C.POINTER(C.c_int32)),
                                  sym.ctypes.data_as(C.POINTER(C.c_int32)), B, vp(df), vp(dp), vp(dz), 1) == 0
    losses = np.zeros(4, np.float32)
    assert L.agz_train_step(eng.h, vp(df), vp(dp), vp(dz), B, 1, C.c_float(0.02), C.c_float(0.9),
                            losses.ctypes.data_as(C.POINTER(C.c_float))) == 0
    eng.sync()
    assert np.isfinite(losses).all() and losses[0] > 0
    assert (df.cpu().numpy() == f1).all() and (dp.cpu().numpy() == p1).all()
    eng.close()


def test_bad_modes_are_refused():
    e = ag.Engine(board_size=5, tower_height=1, games=2, num_readouts=8)
    for bad in (-2, 9):
        with pytest.raises(ag.AgzError):
            e.set_symmetry(bad)
    e.close()
    x = ag.Engine(board_size=5, tower_height=0, games=2, num_readouts=8, external_network=1)
    with pytest.raises(ag.AgzError):
        x.set_symmetry("random")
    x.close()


def test_mode_switched_on_mid_game_keeps_the_ordinal():
    """the evaluation counter runs with the mode off too: a game whose root was evaluated plain and whose later
    evaluations are random draws them at e = 1, 2, ... (the oracle's callable: T_0 for e = 0, the draw key after)"""
    N, tower, readouts, games, seed = 9, 1, 16, 2, 6
    eng = peaked_engine(N, tower, games=games, num_readouts=readouts, seed=seed, record_capacity_games=games + 8)
    eng.start(games)
    eng.step(1)                          # every game's root, the only evaluation so far (e = 0), without a symmetry
    eng.set_symmetry("random")
    for _ in range(100000):
        eng.step(8)
        if eng.stats()["games_finished"] >= games:
            break
    recs, st = eng.records(), eng.stats()
    assert len(recs) == games
    fwd = peaked_engine(N, tower, games=1, num_readouts=8, max_nodes_per_game=16)
    evals = 0
    for r in recs:
        net = SymNetForOracle(fwd, seed, int(r["game_id"]), sy.RANDOM, plain_first=1)
        o = oracle_game(N, net, readouts, seed, int(r["game_id"]))
        assert r["num_moves"] == o["num_moves"] and (r["moves"] == o["moves"][: r["num_moves"]]).all()
        assert bits_equal(r["qs"], o["qs"]) and bits_equal(r["pis"], o["pis"])
        evals += o["evals"]
    assert st["evals"] == evals
    fwd.close()
    eng.close()


def test_draw_is_uniform_and_deterministic():
    """1024 games, two random-mode steps: the roots' evaluation (e = 0) and one select phase of eight leaves each
    (e = 1..8), so the engine's evaluations are exactly the keys (game id < 1024, e <= 8) -- the predicted s over them must be
    uniform.  That the engine evaluated each leaf under the predicted s is read back from the device: the priors a
    root child received must be the network's output under one of the s its game drew for e = 1..8."""
    N, tower, G, seed = 9, 1, 1024, 9
    eng = peaked_engine(N, tower, games=G, num_readouts=32, seed=seed, record_capacity_games=16)
    eng.set_symmetry("random")
    eng.start(G)
    eng.step(2)
    st = eng.stats()
    assert st["evals"] == 9 * G          # no terminal leaf on an empty board: every game evaluated e = 0..8
    counts = np.bincount([sy.draw_symmetry(seed, g, e) for g in range(G) for e in range(9)], minlength=8)
    frac = counts / counts.sum()
    assert (counts > 0).all() and (np.abs(frac - 1 / 8) <= 0.02).all(), frac
    # the device's draws: root children of the first 128 games against the eight candidate evaluations of each
    P, A = N * N, N * N + 1
    n = informative = 0
    for g in range(128):
        gid = int(eng.debug_live_record(g)[0])      # slots claim game ids in the order they reach the counter
        root = eng.tree_root(g)
        rows, boards = [], []
        for a, c in enumerate(eng.node_children(g, root)):
            if c >= 0 and eng.node_info(g, int(c)).is_expanded:
                rows.append(eng.node_floats(g, int(c), 2)[:A])
                boards.append(eng.node_board(g, int(c)).reshape(P))
        m = len(rows)
        b = np.stack(boards).astype(np.int8)
        deltas = np.zeros((m, 7, P), np.int8)
        deltas[:, 0] = b                      # one move played on the empty board
        feats = eng.features(b, deltas, np.ones(m, np.int32), -np.ones(m, np.int8))
        cand, _ = eng.forward_features_sym(np.repeat(feats, 8, axis=0), np.tile(np.arange(8, dtype=np.int32), m))
        cand = cand.reshape(m, 8, A)
        drawn = {sy.draw_symmetry(seed, gid, e) for e in range(1, 9)}
        for k in range(m):
            match = {s for s in range(8) if bits_equal(cand[k, s], rows[k])}
            assert match and match & drawn, (gid, match, drawn)
            informative += len(match) < 8 and not drawn <= match
        n += m
    assert n >= 4 * 128 and informative >= n // 4
    eng.close()
    out = []
    for _ in range(2):
        e = peaked_engine(5, 1, games=3, num_readouts=16, seed=seed, record_capacity_games=16)
        e.set_symmetry("random")
        out.append(run(e, 3)[0])
        e.close()
    same_records(out[0], out[1])


def test_replay_buffer_augment():
    """ReplayBuffer.sample(augment=True): the same samples as without, sample b under the s the caller's rng draws
    right after them"""
    N, B = 9, 16
    eng = peaked_engine(N, 1, games=2, num_readouts=16, seed=5, record_capacity_games=10)
    recs, _ = run(eng, 2)
    buf = ag.ReplayBuffer(ag.GoEnv(N))
    buf.extend(recs)
    f0, p0, r0 = buf.sample(B, np.random.default_rng(3), eng)
    f1, p1, r1 = buf.sample(B, np.random.default_rng(3), eng, augment=True)
    rng = np.random.default_rng(3)
    buf.sample_indices(B, rng)
    sym = rng.integers(0, 8, size=B)
    assert len(set(sym.tolist())) > 1
    for b in range(B):
        assert (f1[b] == sy.apply_features(f0[b], int(sym[b]), N)).all()
        assert (p1[:, b] == sy.apply_policy(p0[:, b], int(sym[b]), N)).all()
    assert (r1 == r0).all()
    with pytest.raises(ValueError):
        buf.sample(B, np.random.default_rng(3), eng, out=object(), augment=True)
    eng.close()

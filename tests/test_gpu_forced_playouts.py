"""Forced playouts and policy target pruning on the device (agz_selfplay_set_forced_playouts, agz_tree_pruned_pi,
DESIGN.md §5i).

Every self-play game must be, bit for bit, the twin's game (tests/selfplay_twin.py: the reference's loop with the forced
root descent in its full searches and the pruned target in their pi rows) on the engine's own forward -- under the
playout cap, from a table of starts, with drawn symmetries.  The single-tree calls reach the rule with hand-made rows at
the four register-row widths of the descent and at the two boards the widest one runs rounded up.  Off is the engine that never made the call, byte for byte; analysis never
forces; train(..., forced_playouts=...) plays the twin's games on the weights of each round."""
import numpy as np
import pytest

import alphago_jl_amd as ag
import orc
import selfplay_twin as tw
from alphago_jl_amd import symmetry as sy
from gpu_common import GpuNetForOracle
from gpu_options import SymNetForOracle, assert_game_equals_twin, assert_train_equals_twin, host_schedule, peaked_engine, play
from test_hostsim_selfplay import bits_equal

pytestmark = pytest.mark.gpu
L = orc.lib()
BAD_ARGUMENT = ag._lib.BAD_ARGUMENT
CAP = (8, 0.5)
THR = -0.1


def check_set(eng, recs, st, twins):
    for r, o in zip(recs, twins):
        assert_game_equals_twin(r, o, int(r["game_id"]), o["full"])
    for o in twins:           # the condition of the comparison set
        assert o["forced_sel"] >= 1, "a game of the set has no forced selection"
        assert o["pruned_rows"].any(), "a game of the set has no row that pruning changed"
    nforced, nrows = sum(o["forced_sel"] for o in twins), sum(int(o["pruned_rows"].sum()) for o in twins)
    print(f"{len(recs)} games: {nforced} forced selections, {nrows} rows changed, evals {st['evals']}")
    assert eng.forced_counts() == (nforced, nrows)
    assert st["evals"] == sum(o["evals"] for o in twins)
    assert st["positions"] == sum(o["num_moves"] for o in twins)
    assert eng.playout_cap_counts() == (sum(int(o["full"].sum()) for o in twins),
                                        sum(int((~o["full"]).sum()) for o in twins))


# ---------------------------------------------------------------- bit-exact games

@pytest.mark.parametrize("N,tower,R,k,games,slots,seed,plies", [
    (9, 2, 32, 2.0, 6, 32, 4, (6, 11, 2)),
    (9, 2, 32, 16.0, 6, 32, 4, (6, 11, 2)),
    (5, 1, 16, 2.0, 6, 32, 3, (4, 7, 1)),
    (5, 1, 16, 16.0, 5, 32, 3, (4, 7, 1)),
])
def test_games_equal_the_twin(N, tower, R, k, games, slots, seed, plies):
    starts = tw.random_starts(N, plies, seed=0)
    eng = ag.Engine(board_size=N, tower_height=tower, games=slots, num_readouts=R, seed=seed,
                    record_capacity_games=games + 8, resign_threshold=THR, resign_disable_fraction=0.0)
    eng.init_synthetic(0)
    b, i, h = tw.opos_arrays(starts)
    eng.set_starts(boards=b, info=i, history=h)
    eng.set_playout_cap(*CAP)
    eng.set_forced_playouts(k)
    recs, st = play(eng, games)
    fwd = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=8, max_nodes_per_game=16)
    fwd.init_synthetic(0)
    cb = GpuNetForOracle(fwd).cb
    twins = [tw.twin_selfplay(N, cb, R, seed, int(r["game_id"]), starts[int(r["game_id"]) % len(starts)], THR, 0.0,
                              cap=CAP, forced=(k, True)) for r in recs]
    check_set(eng, recs, st, twins)
    eng.close()
    fwd.close()


def test_games_with_random_symmetry_equal_the_twin():
    N, tower, R, k, games, seed = 9, 1, 32, 2.0, 3, 4
    starts = tw.random_starts(N, (6, 11, 2), seed=0)
    eng = peaked_engine(N, tower, games=games, num_readouts=R, seed=seed, record_capacity_games=games + 8,
                        resign_threshold=THR, resign_disable_fraction=0.0)
    b, i, h = tw.opos_arrays(starts)
    eng.set_starts(boards=b, info=i, history=h)
    eng.set_symmetry("random")
    eng.set_playout_cap(*CAP)
    eng.set_forced_playouts(k)
    recs, st = play(eng, games)
    fwd = peaked_engine(N, tower, games=1, num_readouts=8, max_nodes_per_game=16)
    twins = []
    for r in recs:
        gid = int(r["game_id"])
        net = SymNetForOracle(fwd, seed, gid, sy.RANDOM)
        twins.append(tw.twin_selfplay(N, net.cb, R, seed, gid, starts[gid % 3], THR, 0.0, cap=CAP, forced=(k, True)))
    check_set(eng, recs, st, twins)
    eng.close()
    fwd.close()


# ---------------------------------------------------------------- the single-tree known answers

EX_N = [60, 20, 12, 1, 6]
EX_P = [0.50, 0.20, 0.10, 0.05, 0.15]
EX_W = [30.5, 0, 6.25, 0, 3.5]


def set_rows(eng, N, at, rootN, n):
    """a fresh single tree on slot 0 whose expanded root holds the example's children at actions `at`"""
    A = N * N + 1
    root = eng.tree_init(0, np.zeros(N * N, np.int8), n=n)
    assert eng.select_leaf(0, root) == root
    assert eng.incorporate_results(0, root, np.full(A, 1.0 / A, np.float32), 0.0, root) == 0
    rows = []
    for field, vals in ((ag._lib.F_CHILD_N, EX_N), (ag._lib.F_CHILD_W, EX_W), (ag._lib.F_CHILD_PRIOR, EX_P)):
        row = np.zeros(A, np.float32)
        row[list(at)] = np.asarray(vals, np.float32)
        eng.node_set_floats(0, root, field, row)
        rows.append(row)
    eng.node_set_N(0, root, rootN)
    return root, rows


@pytest.mark.parametrize("N", [5, 9, 13, 15, 17, 19])
def test_single_tree_known_answers(N):
    """N = 5, 9, 13, 19: the descent at its row widths 1, 2, 3, 6; N = 15, 17 (4 and 5 row elements per lane): the
    width 6 rounded up, whose last rows lie past AP.  The under-forced child sits at action A - 2 (the last point) and,
    separately, at the pass: the last register row in use and its lane mapping"""
    A = N * N + 1
    tau = ((N * N // 12) // 2) * 2
    eng = ag.Engine(board_size=N, tower_height=1, games=1, num_readouts=8, max_nodes_per_game=64, c_puct=1.0, seed=1)
    eng.init_synthetic(0)
    for u in (A - 2, A - 1):
        at = (0, A // 3, A // 2, u, (2 * A) // 3)
        assert len(set(at)) == 5
        for n in (tau + 1, 0):                      # plain and squashed rows
            root, rows = set_rows(eng, N, at, 99.0, n)
            for k in (2.0, 0.0, 16.0):
                got = eng.tree_pruned_pi(0, root, k)
                want, changed = tw.pruned_pi(*rows, 1, 99.0, 1.0, k, n <= tau)
                assert changed == (k > 0) and bits_equal(got, want), (N, u, n, k)
            want2, _ = tw.pruned_pi(*rows, 1, 99.0, 1.0, 2.0, n <= tau)
            assert want2[u] == 0.0 and abs(float(want2.astype(np.float64).sum()) - 1.0) < 1e-6
        # the forced pick, and the PUCT arg-max with the setting off
        score, _, scale = tw.action_scores(rows[0], rows[1], rows[2], 1, 99.0, 1.0)
        assert scale == 10.0
        best = int(np.argmax(score))
        assert best == at[4]
        assert list(np.flatnonzero(tw.under_forced(2.0, rows[0], rows[2], 99.0))) == [u]
        for k, want_pick, counted in ((2.0, u, 1), (0.0, best, 0)):
            eng.set_forced_playouts(k)
            root, rows = set_rows(eng, N, at, 98.0, tau + 1)
            before = eng.forced_counts()
            leaf = eng.select_leaf(0, root)
            pick = np.flatnonzero(eng.node_children(0, root) == leaf)
            assert list(pick) == [want_pick], (N, u, k, pick)
            assert eng.forced_counts() == (before[0] + counted, before[1])
            assert eng.node_info(0, root).N == 99.0
        eng.set_forced_playouts(0.0)
    eng.close()


def test_node_view_pruned_pi():
    env = ag.GoEnv(5)
    nn = ag.NeuralNet(env, tower_height=1, seed=0)
    pl = ag.MCTSPlayer(env, nn, num_readouts=16)
    pl.initialize_game()
    for _ in range(5):
        pl.tree_search(8)
    cn = pl.root.child_N
    want, _ = tw.pruned_pi(cn, pl.root.child_W, pl.root.child_prior, 1, pl.root.N, pl.engine.cfg.c_puct, 2.0, True)
    assert bits_equal(pl.root.pruned_pi(2.0), want)
    assert bits_equal(pl.root.pruned_pi(0.0), tw.pi_of(cn.astype(np.float64), True))


# ---------------------------------------------------------------- off is off

def test_off_is_the_engine_that_never_made_the_call():
    N, tower, R, games = 9, 1, 16, 4
    out = []
    for how in ("never", "zero", "reset", "on"):
        eng = ag.Engine(board_size=N, tower_height=tower, games=games, num_readouts=R, seed=2,
                        record_capacity_games=games + 8)
        eng.init_synthetic(0)
        eng.set_playout_cap(*CAP)
        if how == "zero":
            eng.set_forced_playouts(0.0, False)
        if how in ("reset", "on"):
            eng.set_forced_playouts(2.0, True)
        if how == "reset":
            eng.set_forced_playouts(0.0)
        recs, st = play(eng, games)
        out.append((eng.records_packed().copy(), st, eng.forced_counts(), eng.debug_counters().copy()))
        eng.close()
    for packed, st, fc, raw in out[1:3]:
        assert packed.tobytes() == out[0][0].tobytes()
        assert st == out[0][1]
        assert fc == (0, 0) and (raw == out[0][3]).all()
    assert out[3][0].tobytes() != out[0][0].tobytes() and out[3][2][0] > 0 and out[3][2][1] > 0


# ---------------------------------------------------------------- refusals

def test_refusals():
    N, R = 5, 16

    def refused(fn, word):
        with pytest.raises(ag.AgzError) as e:
            fn()
        assert e.value.status == BAD_ARGUMENT and word in str(e.value), str(e.value)

    arena = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=R, arena_mode=1)
    refused(lambda: arena.set_forced_playouts(2.0), "arena")
    arena.close()
    eng = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=R, seed=1, record_capacity_games=8,
                    resign_threshold=-2.0, resign_disable_fraction=0.0)
    eng.init_synthetic(0)
    for bad in (-0.5, 1024.5, float("nan"), float("inf")):
        refused(lambda: eng.set_forced_playouts(bad), "k =")
    assert eng.L.agz_selfplay_set_forced_playouts(eng.h, 0.0, 1) == BAD_ARGUMENT      # pruning without forcing
    eng.set_forced_playouts(1024.0)
    eng.set_forced_playouts(2.0, False)
    eng.set_forced_playouts(16.0, True)
    eng.start(2)
    eng.set_forced_playouts(16.0, True)          # started, not stepped: no game claimed yet
    eng.step(3)
    refused(lambda: eng.set_forced_playouts(0.0), "still being played")
    refused(lambda: eng.set_forced_playouts(2.0), "still being played")
    while eng.records_count() < 2:
        eng.step(8)
    assert eng.forced_counts()[0] > 0            # the refused calls left (16, prune) in force
    eng.set_forced_playouts(0.0)                 # the run is over
    with pytest.raises(ag.AgzError):
        eng.tree_pruned_pi(0, 0, -1.0)
    eng.close()


# ---------------------------------------------------------------- analysis never forces

def test_analysis_is_untouched():
    N, R = 5, 16
    starts = tw.random_starts(N, (4, 7, 1, 9), seed=0)
    b, i, h = tw.opos_arrays(starts)
    res = []
    for k in (0.0, 16.0):
        eng = ag.Engine(board_size=N, tower_height=1, games=4, num_readouts=R, seed=5)
        eng.init_synthetic(0)
        if k:
            eng.set_forced_playouts(k)
        eng.analyze_start(b, i, h, game_id_base=7)
        for _ in range(4000):
            eng.step(4)
            if eng.analyze_progress() >= len(starts):
                break
        res.append((eng.analyze_results(), eng.forced_counts()))
        eng.close()
    assert sorted(res[0][0]) == sorted(res[1][0])
    for key in res[0][0]:
        assert np.asarray(res[0][0][key]).tobytes() == np.asarray(res[1][0][key]).tobytes(), key
    assert res[1][1] == (0, 0)


# ---------------------------------------------------------------- train(..., forced_playouts=...)

TRAIN = dict(N=5, TOWER=1, R=16, k=2.0, SEED=3, num_games=8, slots=4, memory=40, B=8, start_after=8)


def configure_train(eng):
    eng.set_playout_cap(*CAP)
    eng.set_forced_playouts(TRAIN["k"], True)


def test_train_with_forced_playouts_plays_the_twins_games():
    c = TRAIN
    env = ag.GoEnv(c["N"])
    nn0 = ag.NeuralNet(env, tower_height=c["TOWER"], seed=1)
    ref, snaps, start_step, counts = host_schedule(nn0, c, configure_train, targets_only=True)
    twins, _ = assert_train_equals_twin(
        env, nn0, c, (ref, snaps, start_step),
        lambda cb, gid, on_round: tw.twin_selfplay(c["N"], cb, c["R"], c["SEED"], gid, None, -0.9, 0.05, on_round=on_round,
                                                   cap=CAP, forced=(c["k"], True)),
        masked=True, playout_cap=CAP, forced_playouts=c["k"])
    nforced, nrows = sum(o["forced_sel"] for o in twins), sum(int(o["pruned_rows"].sum()) for o in twins)
    assert nforced >= 3 and nrows >= 3 and counts["forced"] == (nforced, nrows)


def test_selfplay_takes_the_keywords():
    N, R, k = 5, 16, 2.0
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=0)
    kw = dict(games=3, seed=2, game_id_base=0, playout_cap=CAP, resign_threshold=-2.0, resign_disable_fraction=0.0)
    cb = GpuNetForOracle(nn.engine).cb
    for prune in (True, False):
        players = ag.selfplay(env, nn, R, forced_playouts=k, prune_targets=prune, **kw)
        for gid, pl in enumerate(players):
            o = tw.twin_selfplay(N, cb, R, 2, gid, None, -2.0, 0.0, cap=CAP, forced=(k, prune))
            assert [ag.to_flat(m, env) for m in pl.moves] == list(o["moves"]) and pl.result == o["result"]
            assert pl.full_search == list(o["full"])
            assert bits_equal(np.stack(pl.searches_pi), o["pis"])

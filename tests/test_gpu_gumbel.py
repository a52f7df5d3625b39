"""The Gumbel root search on the device (agz_selfplay_set_gumbel, agz_tree_gumbel_pi).

Every self-play game must be, bit for bit, the twin's game (tests/selfplay_twin.py: the reference's loop with Gumbel-top-k
candidates, Sequential Halving, the best-s move and the softmax(logit + sigma(q)) row in its full searches) on the
engine's own forward -- with the playout cap on and off, from a table of starts, with drawn symmetries.  The
single-tree row call is held to the worked example at the four register-row widths and at the two boards the widest
one runs rounded up.  Off is the engine that never made the call, byte for byte; every refusal; analysis is unchanged;
train(..., gumbel=...) plays the twin's games on the weights of each round."""
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


def check_set(eng, recs, st, twins, cap):
    for r, o in zip(recs, twins):
        assert_game_equals_twin(r, o, int(r["game_id"]), o["full"])
    begun, halved = sum(o["begun"] for o in twins), sum(o["halved"] for o in twins)
    print(f"{len(recs)} games: {begun} searches begun, {halved} halvings, evals {st['evals']}")
    assert begun >= 1 and halved >= 1                   # the condition of the comparison set, on the twin
    assert sum(o["reused"] for o in twins) >= 1
    assert eng.gumbel_counts() == (begun, halved)
    assert st["evals"] == sum(o["evals"] for o in twins)
    assert st["positions"] == sum(o["num_moves"] for o in twins)
    if cap:
        assert eng.playout_cap_counts() == (sum(int(o["full"].sum()) for o in twins),
                                            sum(int((~o["full"]).sum()) for o in twins))
    assert eng.forced_counts() == (0, 0)


# ---------------------------------------------------------------- bit-exact games

@pytest.mark.parametrize("N,tower,R,m,cap,games,slots,seed,plies", [
    (9, 2, 32, 16, None, 4, 32, 4, (6, 11, 2)),
    (9, 2, 32, 4, CAP, 6, 32, 4, (6, 11, 2)),
    (5, 1, 32, 4, None, 5, 32, 3, (4, 7, 1)),
    (5, 1, 32, 16, CAP, 6, 32, 3, (4, 7, 1)),
])
def test_games_equal_the_twin(N, tower, R, m, cap, games, slots, seed, plies):
    starts = tw.random_starts(N, plies, seed=0)
    eng = ag.Engine(board_size=N, tower_height=tower, games=slots, num_readouts=R, seed=seed,
                    record_capacity_games=games + 8, resign_threshold=THR, resign_disable_fraction=0.0)
    eng.init_synthetic(0)
    b, i, h = tw.opos_arrays(starts)
    eng.set_starts(boards=b, info=i, history=h)
    if cap:
        eng.set_playout_cap(*cap)
    eng.set_gumbel(m)
    recs, st = play(eng, games)
    fwd = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=8, max_nodes_per_game=16)
    fwd.init_synthetic(0)
    cb = GpuNetForOracle(fwd).cb
    r, p = cap if cap else (0, 1.0)
    twins = [tw.twin_selfplay(N, cb, R, seed, int(rec["game_id"]), starts[int(rec["game_id"]) % len(starts)], THR, 0.0,
                              cap=(r, p), gumbel=(m, 50.0, 1.0)) for rec in recs]
    check_set(eng, recs, st, twins, cap)
    eng.close()
    fwd.close()


def test_games_with_random_symmetry_equal_the_twin():
    N, tower, R, m, games, seed = 9, 1, 32, 16, 3, 4
    starts = tw.random_starts(N, (6, 11, 2), seed=0)
    eng = peaked_engine(N, tower, games=games, num_readouts=R, seed=seed, record_capacity_games=games + 8,
                        resign_threshold=THR, resign_disable_fraction=0.0)
    b, i, h = tw.opos_arrays(starts)
    eng.set_starts(boards=b, info=i, history=h)
    eng.set_symmetry("random")
    eng.set_playout_cap(*CAP)
    eng.set_gumbel(m, 50.0, 0.5)
    recs, st = play(eng, games)
    fwd = peaked_engine(N, tower, games=1, num_readouts=8, max_nodes_per_game=16)
    twins = []
    for r in recs:
        gid = int(r["game_id"])
        net = SymNetForOracle(fwd, seed, gid, sy.RANDOM)
        twins.append(tw.twin_selfplay(N, net.cb, R, seed, gid, starts[gid % 3], THR, 0.0, cap=CAP, gumbel=(m, 50.0, 0.5)))
    check_set(eng, recs, st, twins, CAP)
    eng.close()
    fwd.close()


# ---------------------------------------------------------------- the worked row on a single tree

EX_N = [60, 20, 12, 1, 6, 0]
EX_P = [0.50, 0.20, 0.10, 0.05, 0.10, 0.05]
EX_W = [30.5, 0, 6.25, 0, 3.5, 0.45]
EX_PI = [0.672112, 0.017187, 0.120931, 0.004297, 0.134422, 0.051052]
EX_PI_MINUS = [0.106663, 0.667399, 0.023713, 0.166850, 0.021333, 0.014043]


def set_rows(eng, N, at, to_play=1, board=None):
    """a fresh single tree on slot 0 whose expanded root holds the example's children at actions `at`"""
    A = N * N + 1
    tau = ((N * N // 12) // 2) * 2
    root = eng.tree_init(0, np.zeros(N * N, np.int8) if board is None else board, n=tau + 1, to_play=to_play)
    assert eng.select_leaf(0, root) == root
    assert eng.incorporate_results(0, root, np.full(A, 1.0 / A, np.float32), 0.0, root) == 0
    rows = []
    for field, vals in ((ag._lib.F_CHILD_N, EX_N), (ag._lib.F_CHILD_W, EX_W), (ag._lib.F_CHILD_PRIOR, EX_P)):
        row = np.zeros(A, np.float32)
        row[list(at)] = np.asarray(vals, np.float32)
        eng.node_set_floats(0, root, field, row)
        rows.append(row)
    return root, rows


@pytest.mark.parametrize("N", [5, 9, 13, 15, 17, 19])
def test_single_tree_worked_row(N):
    """N = 5, 9, 13, 19: row widths 1, 2, 3, 6; N = 15, 17: 4 and 5 row elements per lane, run at width 6.  The example's
    a0 (the largest entry) and a5 (the unvisited child) sit at action A - 2 (the last point) and at the pass, and the
    other way round"""
    A = N * N + 1
    eng = ag.Engine(board_size=N, tower_height=1, games=1, num_readouts=8, max_nodes_per_game=64, c_puct=1.0, seed=1)
    eng.init_synthetic(0)
    eng.set_gumbel(16, 3.0, 7.0)                        # the row call does not look at the setting
    for hi, lo in ((A - 2, A - 1), (A - 1, A - 2)):
        at = (hi, 1, A // 3, A // 2, (2 * A) // 3, lo)
        assert len(set(at)) == 6
        legal = np.ones(A, np.int8)
        root, rows = set_rows(eng, N, at)
        for cs, table in ((0.1, EX_PI), (1.0, None)):
            got = eng.tree_gumbel_pi(0, root, 50.0, cs)
            want, _ = tw.gumbel_pi(*rows, legal, 1, 50.0, cs)
            assert bits_equal(got, want), (N, hi, cs)
            if table:
                assert np.abs(got[list(at)].astype(np.float64) - table).max() < 1e-6
            else:
                assert abs(float(got[hi]) - 0.783795) < 1e-6 and abs(float(got[lo]) - 0.00501063) < 1e-6
            rest = np.setdiff1d(np.arange(A), at)
            assert (got[rest] == 0).all() and abs(float(got.astype(np.float64).sum()) - 1.0) < 1e-6
        root, rows = set_rows(eng, N, at, to_play=-1)
        got = eng.tree_gumbel_pi(0, root, 50.0, 0.1)
        want, _ = tw.gumbel_pi(*rows, legal, -1, 50.0, 0.1)
        assert bits_equal(got, want)
        assert np.abs(got[list(at)].astype(np.float64) - EX_PI_MINUS).max() < 1e-6
        # an occupied point is illegal: no mass there, the rest renormalised
        board = np.zeros(N * N, np.int8)
        board[1] = 1
        legal[1] = 0
        root, rows = set_rows(eng, N, at, board=board)
        got = eng.tree_gumbel_pi(0, root, 50.0, 0.1)
        want, _ = tw.gumbel_pi(*rows, legal, 1, 50.0, 0.1)
        assert bits_equal(got, want) and got[1] == 0.0 and got[hi] > EX_PI[0]
    assert eng.gumbel_counts() == (0, 0)
    eng.close()


def test_node_view_gumbel_pi_and_single_trees_do_not_follow_the_setting():
    env = ag.GoEnv(5)
    nn = ag.NeuralNet(env, tower_height=1, seed=0)
    out = []
    for m in (0, 4):
        pl = ag.MCTSPlayer(env, nn, num_readouts=16)
        pl.engine.set_gumbel(m)
        pl.initialize_game()
        for _ in range(5):
            pl.tree_search(8)
        root = pl.root
        legal = np.ones(26, np.int8)
        want, _ = tw.gumbel_pi(root.child_N, root.child_W, root.child_prior, legal, 1, 50.0, 1.0)
        assert bits_equal(root.gumbel_pi(), want)
        want, _ = tw.gumbel_pi(root.child_N, root.child_W, root.child_prior, legal, 1, 20.0, 0.25)
        assert bits_equal(root.gumbel_pi(20.0, 0.25), want)
        out.append((root.child_N.copy(), root.child_W.copy(), pl.engine.gumbel_counts()))
    assert bits_equal(out[0][0], out[1][0]) and bits_equal(out[0][1], out[1][1])     # a single tree is plain PUCT
    assert out[1][2] == (0, 0)


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
            eng.set_gumbel(0)
        if how in ("reset", "on"):
            eng.set_gumbel(4, 50.0, 1.0)                # R = 16, m = 4: (4,8), (2,8) -- a halving in every full search
        if how == "reset":
            eng.set_gumbel(0)
        recs, st = play(eng, games)
        out.append((eng.records_packed().copy(), st, eng.gumbel_counts(), eng.debug_counters().copy()))
        eng.close()
    for packed, st, gc, raw in out[1:3]:
        assert packed.tobytes() == out[0][0].tobytes()
        assert st == out[0][1]
        assert gc == (0, 0) and (raw == out[0][3]).all()
    assert out[3][0].tobytes() != out[0][0].tobytes() and out[3][2][0] > 0 and out[3][2][1] > 0


# ---------------------------------------------------------------- refusals

def test_refusals():
    N, R = 5, 16

    def refused(fn, word):
        with pytest.raises(ag.AgzError) as e:
            fn()
        assert e.value.status == BAD_ARGUMENT and word in str(e.value), str(e.value)

    arena = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=R, arena_mode=1)
    refused(lambda: arena.set_gumbel(4), "arena")
    arena.close()
    eng = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=R, seed=1, record_capacity_games=8,
                    resign_threshold=-2.0, resign_disable_fraction=0.0)
    eng.init_synthetic(0)
    for bad in (1, -1, 17, 64):
        refused(lambda: eng.set_gumbel(bad), "m =")
    for bad in (-0.5, float("nan")):
        refused(lambda: eng.set_gumbel(4, bad, 1.0), "c_visit")
    for bad in (0.0, -1.0, float("nan")):
        refused(lambda: eng.set_gumbel(4, 50.0, bad), "c_scale")
    # the two root rules are not composed, either way round
    eng.set_forced_playouts(2.0)
    refused(lambda: eng.set_gumbel(4), "forced")
    eng.set_gumbel(0)                                # off is no conflict
    eng.set_forced_playouts(0.0)
    eng.set_gumbel(2, 0.0, 1.0)
    refused(lambda: eng.set_forced_playouts(2.0), "Gumbel")
    eng.set_forced_playouts(0.0)                     # off is no conflict
    eng.set_gumbel(16, 50.0, 1.0)
    eng.start(2)
    eng.set_gumbel(16, 50.0, 1.0)                    # started, not stepped: no game claimed yet
    eng.step(3)
    refused(lambda: eng.set_gumbel(0), "still being played")
    refused(lambda: eng.set_gumbel(4), "still being played")
    while eng.records_count() < 2:
        eng.step(8)
    assert eng.gumbel_counts()[0] > 0                # the refused calls left m = 16 in force
    eng.set_gumbel(0)                                # the run is over
    for cv, cs in ((-1.0, 1.0), (50.0, 0.0), (float("nan"), 1.0)):
        with pytest.raises(ag.AgzError):
            eng.tree_gumbel_pi(0, 0, cv, cs)
    eng.close()
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=0)
    with pytest.raises(ValueError):
        ag.selfplay(env, nn, R, games=1, gumbel=4, forced_playouts=2.0)
    with pytest.raises(ValueError):
        ag.train(env, num_games=2, readouts=R, model=nn, gumbel=4, forced_playouts=2.0, callback=None)


# ---------------------------------------------------------------- analysis is unchanged

def test_analysis_is_untouched():
    N, R = 5, 16
    starts = tw.random_starts(N, (4, 7, 1, 9), seed=0)
    b, i, h = tw.opos_arrays(starts)
    res = []
    for m in (0, 16):
        eng = ag.Engine(board_size=N, tower_height=1, games=4, num_readouts=R, seed=5)
        eng.init_synthetic(0)
        if m:
            eng.set_gumbel(m)
        eng.analyze_start(b, i, h, game_id_base=7)
        for _ in range(4000):
            eng.step(4)
            if eng.analyze_progress() >= len(starts):
                break
        res.append((eng.analyze_results(), eng.gumbel_counts()))
        eng.close()
    assert sorted(res[0][0]) == sorted(res[1][0])
    for key in res[0][0]:
        assert np.asarray(res[0][0][key]).tobytes() == np.asarray(res[1][0][key]).tobytes(), key
    assert res[1][1] == (0, 0)


# ---------------------------------------------------------------- train(..., gumbel=...)

TRAIN = dict(N=5, TOWER=1, R=16, m=4, SEED=3, num_games=8, slots=4, memory=40, B=8, start_after=8)


def configure_train(eng):
    eng.set_playout_cap(*CAP)
    eng.set_gumbel(TRAIN["m"])


def test_train_with_gumbel_plays_the_twins_games():
    c = TRAIN
    env = ag.GoEnv(c["N"])
    nn0 = ag.NeuralNet(env, tower_height=c["TOWER"], seed=1)
    ref, snaps, start_step, counts = host_schedule(nn0, c, configure_train, targets_only=True)
    twins, _ = assert_train_equals_twin(
        env, nn0, c, (ref, snaps, start_step),
        lambda cb, gid, on_round: tw.twin_selfplay(c["N"], cb, c["R"], c["SEED"], gid, None, -0.9, 0.05, on_round=on_round,
                                                   cap=CAP, gumbel=(c["m"], 50.0, 1.0)),
        masked=True, playout_cap=CAP, gumbel=c["m"])
    begun, halved = sum(o["begun"] for o in twins), sum(o["halved"] for o in twins)
    assert begun >= 3 and halved >= 3 and counts["gumbel"] == (begun, halved)


def test_selfplay_takes_the_keywords():
    N, R, m = 5, 16, 4
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=0)
    kw = dict(games=3, seed=2, game_id_base=0, playout_cap=CAP, resign_threshold=-2.0, resign_disable_fraction=0.0)
    cb = GpuNetForOracle(nn.engine).cb
    players = ag.selfplay(env, nn, R, gumbel=m, gumbel_c_visit=20.0, gumbel_c_scale=0.5, **kw)
    for gid, pl in enumerate(players):
        o = tw.twin_selfplay(N, cb, R, 2, gid, None, -2.0, 0.0, cap=CAP, gumbel=(m, 20.0, 0.5))
        assert [ag.to_flat(mv, env) for mv in pl.moves] == list(o["moves"]) and pl.result == o["result"]
        assert pl.full_search == list(o["full"])
        assert bits_equal(np.stack(pl.searches_pi), o["pis"])

"""Root exploration and the move temperature on the device (agz_selfplay_set_root_policy_temperature,
agz_selfplay_set_root_noise, agz_search_set_move_temperature): the rows of agz_tree_explore_rows and
what agz_tree_inject_noise stores against the numpy restatement of tests/explore_twin.py, agz_tree_pick_move on
hand-made rows, device self-play of the CPU game sets against the twin on the engine's own forward with the four
counters, an external-network run, train(), analyze and review against the single-tree MCTSPlayer loop, off against the
engine that never made the calls, and every refusal keeping the setting in force.  Tower 1 everywhere."""
import functools

import numpy as np
import pytest

import alphago_jl_amd as ag
import explore_twin as ex
import orc
import selfplay_twin as tw
from gpu_common import GpuNetForOracle
from explore_twin import COMPOSE, GAME_SETS, GAME_SETTING, SETTINGS, pick_rows, positions, starts_of
from gpu_options import (api_game, api_positions, apply, assert_game_equals_twin, assert_train_equals_twin, configure,
                         host_schedule, peaked_engine, play, same_game, sharpen)
from test_hostsim_selfplay import bits_equal

pytestmark = pytest.mark.gpu
f32 = np.float32
BAD_ARGUMENT, OK = ag._lib.BAD_ARGUMENT, ag._lib.OK
F_N, F_P = ag._lib.F_CHILD_N, ag._lib.F_CHILD_PRIOR


def root_of(eng, pos, game_id):
    """slot 0 as a single tree on oracle position pos, its root expanded by the engine's network"""
    _, infos, hist = tw.opos_arrays([pos])
    f = infos[0]
    root = eng.tree_init(0, pos.board_np(), n=f.n, to_play=f.to_play, ko=f.ko, caps=(f.caps_black, f.caps_white),
                         last_move=f.last_move, komi=f.komi, history=hist[0][: f.history_len] if f.history_len else None)
    eng.set_draw(0, game_id, 0)
    assert eng.tree_search(0, 8) >= 1        # (the unexpanded root, collected again and again: duplicates are reverted)
    return root


# ---------------------------------------------------------------- rows

@pytest.mark.parametrize("N", [5, 9, 13, 19])
def test_rows_equal_the_restatement_and_inject_noise_stores_them(N):
    seed, game, w = 11, 6, 0.25
    A = N * N + 1
    eng = ag.Engine(board_size=N, tower_height=1, games=1, num_readouts=8, max_nodes_per_game=16, seed=seed)
    eng.init_synthetic(0)
    for pname, pos in positions(N).items():
        root = root_of(eng, pos, game)
        legal = orc.legal_moves(pos)
        kinds = ex.prior_kinds(A, legal, 7 * N)
        kinds["net"] = eng.node_floats(0, root, F_P)
        for kname, P in kinds.items():
            for sname, st in SETTINGS.items():
                what = (N, pname, kname, sname)
                eng.node_set_floats(0, root, F_P, P)
                apply(eng, st)
                t, al, nz = eng.tree_explore_rows(0, root)
                wt, wal, wnz, did = ex.explore_rows(P, legal, pos.n, seed, game, w, st, N)
                assert (ex.bits32(t) == ex.bits32(wt)).all(), (what, "tempered")
                assert (ex.bits64(al) == ex.bits64(wal)).all(), (what, "alpha")
                assert (ex.bits32(nz) == ex.bits32(wnz)).all(), (what, "noised")
                assert (ex.bits32(eng.node_floats(0, root, F_P)) == ex.bits32(P)).all(), (what, "the read wrote the tree")
                assert eng.explore_counts() == (0, 0, 0, 0)
                eng.inject_noise(0, root)
                assert (ex.bits32(eng.node_floats(0, root, F_P)) == ex.bits32(wnz)).all(), (what, "stored")
                assert eng.explore_counts() == (int(did), int(st["noise"][0] > 0), 0, 0), what
    # any output may be left out
    assert eng.L.agz_tree_explore_rows(eng.h, 0, root, None, None, None) == OK
    assert eng.L.agz_tree_explore_rows(eng.h, 0, eng.cfg.max_nodes_per_game, None, None, None) == BAD_ARGUMENT
    eng.close()


def test_temperature_on_the_host():
    for n in (0, 1, 7, 300):
        for sch in ((1.25, 1.1, 19.0), (0.75, 0.15, 9.0), (0.75, 0.0, 2.0)):
            assert ag.explore_temperature(n, *sch) == ex.temperature(n, *sch)


# ---------------------------------------------------------------- picks

@pytest.mark.parametrize("N", [5, 19])
def test_picks_equal_the_restatement(N):
    seed, mt = 5, (0.75, 0.0, 2.0)
    eng = ag.Engine(board_size=N, tower_height=1, games=1, num_readouts=8, max_nodes_per_game=16, seed=seed)
    eng.init_synthetic(0)
    root = root_of(eng, orc.make_pos(N), 0)
    sampled = off_max = 0
    tau = ((N * N // 12) // 2) * 2
    for name, row in pick_rows(N * N + 1, N).items():
        eng.node_set_floats(0, root, F_N, row)
        for key in range(64):
            n = key % 13 if key < 52 else max(13, tau) + key % 20      # T(12) = 0.0117 samples, T(13) = 0.0083 does not
            eng.node_set_n(0, root, n)
            eng.set_draw(0, key, 0)
            eng.set_move_temperature(mt)
            st, a = eng.pick_move(0)
            ok, wa, smp, om = ex.pick_move(row, n, seed, key, mt, N)
            assert ok and st == OK and a == wa, (name, key, n, a, wa)
            assert eng.explore_counts() == (0, 0, int(smp), int(om))
            sampled += smp
            off_max += om
            if not smp:                       # T <= 0.01: the arg-max branch, which n >= tau is with the rule off
                assert n >= tau
                eng.set_move_temperature(None)
                assert eng.pick_move(0) == (OK, a), (name, key)
    assert sampled > 0 and off_max > 0
    eng.node_set_floats(0, root, F_N, np.zeros(N * N + 1, f32))
    eng.set_move_temperature(mt)
    eng.node_set_n(0, root, 0)
    assert eng.pick_move(0)[0] == ag._lib.ASSERT_SOFTPICK
    eng.close()


# ---------------------------------------------------------------- games

def device_games(N, how, st, external=False):
    c = GAME_SETS[N]
    kw = dict(COMPOSE[how])
    starts = starts_of(N) if kw.pop("starts", False) else None
    cfg = dict(games=c["slots"], num_readouts=c["R"], seed=c["seed"], record_capacity_games=c["games"] + 8)
    fwd = peaked_engine(N, 1, games=1, num_readouts=8, max_nodes_per_game=16)
    if external:
        eng = ag.Engine(board_size=N, tower_height=0, external_network=1, **cfg)
    else:
        eng = peaked_engine(N, 1, **cfg)
    configure(eng, dict(kw, starts=starts, explore=st))
    recs, stats = play(eng, c["games"], network=fwd.forward_features if external else None)
    counts = eng.explore_counts()
    eng.close()
    return recs, stats, counts, fwd, starts, kw


def check_against_twin(N, how, external=False):
    c = GAME_SETS[N]
    recs, stats, counts, fwd, starts, kw = device_games(N, how, GAME_SETTING, external)
    cb = GpuNetForOracle(fwd).cb
    twins = []
    for rec in recs:
        gid = int(rec["game_id"])
        o = ex.twin_selfplay_explore(N, cb, c["R"], c["seed"], gid, GAME_SETTING,
                                     start=starts[gid % len(starts)] if starts else None, **kw)
        assert_game_equals_twin(rec, o, (N, how, gid), o["full"] if "cap" in kw else None)
        twins.append(o)
    fwd.close()
    print(N, how, "counters", counts, "twin", ex.tallies(twins), "argmax plies", sum(o["argmax_plies"] for o in twins))
    assert counts == ex.tallies(twins)
    assert stats["evals"] == sum(o["evals"] for o in twins)
    assert counts[2] > 0 and counts[3] > 0 and counts[0] == counts[1] > 0
    assert sum(o["argmax_plies"] for o in twins) > 0 and sum(o["illegal_roots"] for o in twins) > 0


@pytest.mark.parametrize("how", list(COMPOSE))
@pytest.mark.parametrize("N", [5, 9])
def test_games_equal_the_twin(N, how):
    check_against_twin(N, how)


def test_external_network_games_equal_the_twin():
    check_against_twin(5, "plain", external=True)


@functools.lru_cache(maxsize=None)
def unset_games():
    out = device_games(5, "plain", None)
    out[3].close()
    return out[:3]


def same_records(a, b):
    return len(a) == len(b) and all(same_game(r, o) for r, o in zip(a, b))


def test_off_is_the_engine_that_never_made_the_calls():
    never, nstats, ncounts = unset_games()
    off = device_games(5, "plain", ex.OFF)
    off[3].close()
    assert ncounts == off[2] == (0, 0, 0, 0)
    assert same_records(off[0], never)
    for k in ("positions", "evals", "games_finished", "resigned"):
        assert k not in nstats or off[1][k] == nstats[k], k
    on = device_games(5, "plain", GAME_SETTING)
    on[3].close()
    assert not same_records(on[0], never), "the rules changed no game"


# ---------------------------------------------------------------- train()

TRAIN = dict(N=5, TOWER=1, R=16, SEED=3, num_games=8, slots=4, memory=40, B=8, start_after=8)
TRAIN_SETTING = ex.setting(pt=(1.25, 1.1, 5.0), noise=(10.83, True), mt=(0.75, 0.0, 2.0))


def test_train_plays_the_twins_games():
    c = TRAIN
    env = ag.GoEnv(c["N"])
    nn0 = ag.NeuralNet(env, tower_height=c["TOWER"], seed=1)
    ref, snaps, start_step, _ = host_schedule(nn0, c, lambda eng: apply(eng, TRAIN_SETTING), targets_only=False)
    twins, _ = assert_train_equals_twin(
        env, nn0, c, (ref, snaps, start_step),
        lambda cb, gid, on_round: ex.twin_selfplay_explore(c["N"], cb, c["R"], c["SEED"], gid, TRAIN_SETTING,
                                                           on_round=on_round),
        masked=False, root_policy_temperature=TRAIN_SETTING["pt"], root_noise=TRAIN_SETTING["noise"],
        move_temperature=TRAIN_SETTING["mt"])
    assert ex.tallies(twins)[2] > 0 and ex.tallies(twins)[0] > 0


# ---------------------------------------------------------------- analyze and review

MT = (0.75, 0.0, 2.0)


def test_analyze_equals_the_player_under_the_move_temperature():
    env = ag.GoEnv(9)
    nn = ag.NeuralNet(env, tower_height=1, seed=1)
    sharpen(nn.engine, 9)
    positions = api_positions(env, 4, 4, 10)          # four positions of at most nine moves: T(n) samples below n = 13
    sampled = 0
    res = ag.analyze(env, nn, positions, num_readouts=16, seed=4, game_id_base=100, slots=2, move_temperature=MT)
    plain = ag.analyze(env, nn, positions, num_readouts=16, seed=4, game_id_base=100, slots=2)
    for k, pos in enumerate(positions):
        p = ag.MCTSPlayer(env, nn, num_readouts=16, seed=4, game_id=100 + k, move_temperature=MT)
        p.initialize_game(pos)
        mv = p.suggest_move()
        a = res[k]
        assert a.status == OK and ag.to_flat(a.move, env) == ag.to_flat(mv, env), k
        assert bits_equal(a.child_N, p.root.child_N) and bits_equal(a.child_N, plain[k].child_N), k
        n = p.engine.node_info(0, p.root.id).pos.n
        ok, wa, smp, _ = ex.pick_move(p.root.child_N, n, 4, 100 + k, MT, 9)
        assert ok and wa == ag.to_flat(mv, env), k
        sampled += smp
        p.engine.close()
    assert len(positions) == 4 and sampled > 0, "the sampling branch was compared"


def test_review_equals_the_player_under_the_move_temperature():
    env = ag.GoEnv(9)
    nn = ag.NeuralNet(env, tower_height=1, seed=1)
    sharpen(nn.engine, 9)
    games = [api_game(env, 10 + j, 6) for j in range(2)]
    res = ag.review(env, nn, games, num_readouts=16, seed=4, game_id_base=100, slots=2, two_player_mode=False,
                    move_temperature=MT)
    sampled = 0
    for j, g in enumerate(games):
        p = ag.MCTSPlayer(env, nn, num_readouts=16, seed=4, game_id=100 + j, move_temperature=MT)
        p.initialize_game(None)
        for k, m in enumerate(g):
            mv = p.suggest_move()
            a = res[j][k]
            assert a.status == OK and a.move == mv, (j, k)
            assert bits_equal(a.child_N, p.root.child_N), (j, k)
            n = p.engine.node_info(0, p.root.id).pos.n
            ok, wa, smp, _ = ex.pick_move(p.root.child_N, n, 4, 100 + j, MT, 9)
            assert ok and wa == ag.to_flat(mv, env), (j, k)
            sampled += smp
            assert p.play_move(m)
        p.engine.close()
    assert sampled > 0


# ---------------------------------------------------------------- refusals

def test_refusals_keep_the_setting():
    N = 5
    eng = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=8, seed=1)
    eng.init_synthetic(0)
    kept = ex.setting(pt=(1.3, 0.9, 4.0), noise=(5.0, True), mt=(0.8, 0.2, 3.0))
    apply(eng, kept)
    pos = orc.make_pos(N)
    root = root_of(eng, pos, 3)
    legal = orc.legal_moves(pos)
    P = eng.node_floats(0, root, F_P)
    row = np.zeros(N * N + 1, f32)
    row[[3, 7, 11]] = (5, 9, 2)

    def kept_in_force(what):
        t, al, nz = eng.tree_explore_rows(0, eng.tree_root(0))
        wt, wal, wnz, _ = ex.explore_rows(P, legal, 0, 1, 3, 0.25, kept, N)
        assert (ex.bits32(t) == ex.bits32(wt)).all() and (ex.bits64(al) == ex.bits64(wal)).all(), what
        assert (ex.bits32(nz) == ex.bits32(wnz)).all(), what

    def refused(fn, *args):
        kept_in_force(("before", fn, args))
        assert getattr(eng.L, fn)(eng.h, *args) == BAD_ARGUMENT, (fn, args)
        kept_in_force((fn, args))

    nan = float("nan")
    PT, NZ, MV = "agz_selfplay_set_root_policy_temperature", "agz_selfplay_set_root_noise", "agz_search_set_move_temperature"
    for args in ((2, 1.0, 1.0, 1.0), (-1, 1.0, 1.0, 1.0), (1, nan, 1.0, 1.0), (1, 1.0, nan, 1.0), (1, 1.0, 1.0, nan),
                 (1, 0.0999, 1.0, 1.0), (1, 1.0, 10.001, 1.0), (1, 1.0, 1.0, 0.0), (1, 1.0, 1.0, -1.0),
                 (1, 1.0, 1.0, 1.0000001e6), (0, 0.05, 1.0, 1.0)):
        refused(PT, *args)
    for args in ((2, 1.0, 1.0, 1.0), (1, nan, 1.0, 1.0), (1, -1e-9, 1.0, 1.0), (1, 1.0, 10.001, 1.0), (1, 1.0, 1.0, 0.0),
                 (1, 1.0, 1.0, nan), (1, 1.0, 1.0, 1.0000001e6)):
        refused(MV, *args)
    for args in ((nan, 0), (-1e-9, 0), (1000.001, 0), (1.0, 2), (1.0, -1), (0.0, 1)):
        refused(NZ, *args)
    # the move temperature in force too: the pick is the restatement's under `kept`
    eng.node_set_floats(0, root, F_N, row)
    refused(MV, 1, 11.0, 1.0, 1.0)
    st, a = eng.pick_move(0)
    assert (st, a) == (OK, ex.pick_move(row, 0, 1, 3, kept["mt"], N)[1])
    # the bounds themselves are in range
    for fn, args in ((PT, (1, 0.1, 10.0, 1.0e6)), (MV, (1, 0.0, 10.0, 1.0e6)), (NZ, (1000.0, 1)), (NZ, (0.0, 0))):
        assert getattr(eng.L, fn)(eng.h, *args) == OK, (fn, args)
    apply(eng, kept)
    with pytest.raises(ag.AgzError):
        eng._ck(eng.L.agz_search_explore_counts(eng.h, None))
    # between select and incorporate
    eng.node_set_floats(0, root, F_N, np.zeros(N * N + 1, f32))
    assert eng.tree_search_select(0, 4) > 0
    refused(PT, 1, 1.0, 1.0, 1.0)
    refused(NZ, 0.0, 0)
    refused(MV, 0, 1.0, 1.0, 1.0)
    eng.tree_search_incorporate(0)
    # games in flight
    eng.start(2)
    eng.step(3)
    assert eng.stats()["live_games"] > 0
    for fn, args in ((PT, (0, 1.0, 1.0, 1.0)), (NZ, (0.0, 0)), (MV, (0, 1.0, 1.0, 1.0))):
        assert getattr(eng.L, fn)(eng.h, *args) == BAD_ARGUMENT, fn
    for _ in range(20000):
        eng.step(8)
        if eng.records_count() >= 2:
            break
    c = eng.explore_counts()
    assert c[0] > 0 and c[1] > 0 and c[2] > 0, "the setting stayed in force through the run"
    apply(eng, ex.OFF)                        # between games they are taken, and the counters restart
    assert eng.explore_counts() == (0, 0, 0, 0)
    eng.close()


def test_the_arena_refuses_and_evaluate_is_unchanged():
    """an arena engine set up as evaluate() sets its own up refuses all three setters, on and off; the games it then
    plays count nothing and are evaluate()'s games"""
    env = ag.GoEnv(5)
    a, b = ag.NeuralNet(env, tower_height=1, seed=0), ag.NeuralNet(env, tower_height=1, seed=5)
    games = 3
    arena = ag.Engine(board_size=5, tower_height=1, games=2 * games, num_readouts=16, seed=2,
                      record_capacity_games=games + 8, arena_mode=1)
    a.engine.copy_weights_to(arena)
    arena.net_select(1)
    b.engine.copy_weights_to(arena)
    arena.net_select(0)
    for fn, args in (("agz_selfplay_set_root_policy_temperature", (1, 1.0, 1.0, 1.0)),
                     ("agz_selfplay_set_root_noise", (1.0, 0)), ("agz_search_set_move_temperature", (1, 1.0, 1.0, 1.0)),
                     ("agz_selfplay_set_root_policy_temperature", (0, 1.0, 1.0, 1.0)),
                     ("agz_selfplay_set_root_noise", (0.0, 0)), ("agz_search_set_move_temperature", (0, 1.0, 1.0, 1.0))):
        assert getattr(arena.L, fn)(arena.h, *args) == BAD_ARGUMENT, fn
    got, _ = play(arena, games)
    assert arena.explore_counts() == (0, 0, 0, 0)
    arena.close()
    _, st = ag.evaluate(env, a, b, num_games=games, ro=16, seed=2, return_stats=True)
    want = sorted(st.records, key=lambda r: r["game_id"])
    assert len(got) == len(want) == games
    for x, y in zip(got, want):
        assert x["game_id"] == y["game_id"] and x["num_moves"] == y["num_moves"] and x["result"] == y["result"]
        assert (x["moves"] == y["moves"]).all() and bits_equal(x["qs"], y["qs"]), x["game_id"]

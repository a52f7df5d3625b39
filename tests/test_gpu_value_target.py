"""Search-value targets on the device (include/agz.h agz_replay_set_value_target, include/agz_value_target.h, DESIGN.md
§5n): the z of agz_replay_batch, agz_replay_batch_sym and agz_replay_sample against the numpy float64 twin
(tests/value_target_twin.py) applied to the arena's own records, bit for bit, over every (game, ply) of small arenas; the
off path; a targets-only arena under the playout cap; the ring and host entries; the refusals; and train(...,
value_target=...) against the same schedule run by hand."""
import numpy as np
import pytest

import alphago_jl_amd as ag
import value_target_twin as vt
from gpu_options import _twin_pairs, _weights, play, weight_mismatches
from test_hostsim_selfplay import bits_equal

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = ag._lib.BAD_ARGUMENT
N, TOWER, R, GAMES, SLOTS, SEED = 5, 1, 16, 8, 4, 3


def sampled(e, B, call, sym=-1):
    """agz_replay_sample on the host: feats, pi, z, game, ply"""
    import torch
    out = e.replay_sample(B, call, sym)
    torch.cuda.synchronize()
    e.sync()
    return [t.cpu().numpy() for t in out]


@pytest.fixture(scope="module")
def base():
    """5x5, tower 1, R = 16, 8 games on 4 slots under a resign threshold that is easy to hit and a disable coin of one half
    (resigned and scored games both occur), filed by agz_replay_ingest_records.  `eng` is the engine whose setting the
    tests change, `plain` one with the same arena that never makes the call; the twin's y of every ply, computed once"""
    eng = ag.Engine(board_size=N, tower_height=TOWER, games=SLOTS, num_readouts=R, seed=SEED, resign_threshold=-0.05,
                    resign_disable_fraction=0.5, record_capacity_games=GAMES + 8)
    eng.init_synthetic(0)
    recs = sorted(play(eng, GAMES)[0], key=lambda r: r["index"])          # the ring's order: record k is recs[k]
    assert [r["index"] for r in recs] == list(range(GAMES))
    assert eng.replay_ingest_records(0, GAMES) == GAMES
    plain = ag.Engine(board_size=N, tower_height=TOWER, games=1, num_readouts=8, max_nodes_per_game=16, seed=SEED)
    assert plain.replay_ingest(eng.records_packed().copy()) == GAMES
    arena = [eng.replay_record(k) for k in range(GAMES)]
    for a, r in zip(arena, recs):
        assert a["game_id"] == r["game_id"] and bits_equal(a["qs"], r["qs"]) and a["result"] == r["result"]
    print("games:", [(a["num_moves"], a["result"], a["was_resign"]) for a in arena])
    assert any(a["was_resign"] for a in arena) and any(not a["was_resign"] for a in arena)
    game = np.concatenate([np.full(a["num_moves"], k, np.int64) for k, a in enumerate(arena)])
    ply = np.concatenate([np.arange(a["num_moves"], dtype=np.int32) for a in arena])
    z = np.concatenate([np.full(a["num_moves"], a["result"], np.float32) for a in arena])
    y = {p: np.concatenate([vt.value_targets(a["qs"], a["result"], *p) for a in arena]) for p in vt.PAIRS}
    at = {(int(g), int(t)): i for i, (g, t) in enumerate(zip(game, ply))}
    d = dict(eng=eng, plain=plain, recs=recs, arena=arena, game=game, ply=ply, z=z, y=y, at=at, L=len(game))
    yield d
    eng.close()
    plain.close()


def test_off_is_the_result_on_both_engines(base):
    """never set, and set to alpha = 0: z is float(result) bit for bit from all three calls, feats and pi the same"""
    b = base
    b["eng"].replay_set_value_target(0.0, 0.3)
    sym = (np.arange(b["L"]) % 8).astype(np.int32)
    f0, p0, z0 = b["plain"].replay_batch(b["game"], b["ply"])
    f1, p1, z1 = b["eng"].replay_batch(b["game"], b["ply"])
    assert bits_equal(z0, b["z"]) and bits_equal(z1, b["z"]) and bits_equal(f0, f1) and bits_equal(p0, p1)
    f0, p0, z0 = b["plain"].replay_batch_sym(b["game"], b["ply"], sym)
    f1, p1, z1 = b["eng"].replay_batch_sym(b["game"], b["ply"], sym)
    assert bits_equal(z0, b["z"]) and bits_equal(z1, b["z"]) and bits_equal(f0, f1) and bits_equal(p0, p1)
    for B, call, mode in ((2, 1, -1), (32, 2, 8), (b["L"], 3, -1)):
        s0, s1 = sampled(b["plain"], B, call, mode), sampled(b["eng"], B, call, mode)
        want = np.array([b["z"][b["at"][(int(g), int(t))]] for g, t in zip(s0[3], s0[4])], np.float32)
        assert bits_equal(s0[2], want) and bits_equal(s1[2], want)
        assert all(bits_equal(x, y) for x, y in zip(s0, s1))


@pytest.mark.parametrize("alpha,lam", vt.PAIRS)
def test_on_every_ply_equals_the_twin(base, alpha, lam):
    b = base
    e = b["eng"]
    e.replay_set_value_target(alpha, lam)
    want = b["y"][(alpha, lam)]
    f0, p0, _ = b["plain"].replay_batch(b["game"], b["ply"])
    f, p, z = e.replay_batch(b["game"], b["ply"])
    dz = np.abs(z.astype(np.float64) - b["z"])
    print(f"alpha {alpha} lambda {lam}: {b['L']} plies, mean |y - z| {dz.mean():.4f}, max {dz.max():.4f}")
    assert bits_equal(z, want) and bits_equal(f, f0) and bits_equal(p, p0)
    if alpha > 0 and lam < 1:
        assert not bits_equal(z, b["z"]), "the recorded root values moved no target"
    for s in range(8):                                        # a symmetry does not touch y
        _, _, zs = e.replay_batch_sym(b["game"], b["ply"], np.full(b["L"], s, np.int32))
        assert bits_equal(zs, want), s
    for B, call in ((2, 11), (32, 12), (b["L"], 13)):          # the draw, feats and pi are the off call's
        off, on = sampled(b["plain"], B, call), sampled(e, B, call)
        g, t = _twin_pairs(e, call, B)
        assert (on[3] == g).all() and (on[4] == t).all()
        for k in (0, 1, 3, 4):
            assert bits_equal(on[k], off[k]), (B, k)
        assert bits_equal(on[2], np.array([want[b["at"][(int(a), int(c))]] for a, c in zip(g, t)], np.float32)), B
    assert sorted(zip(on[3].tolist(), on[4].tolist())) == sorted(b["at"])      # B = L: every entry of the window
    # device outputs (what agz_train_step reads) go the same way as host outputs
    _, _, zs, _, _ = sampled(e, b["L"], 14, 8)
    g, t = _twin_pairs(e, 14, b["L"])
    assert bits_equal(zs, np.array([want[b["at"][(int(a), int(c))]] for a, c in zip(g, t)], np.float32))


def test_window_inside_a_game_and_clear_keep_the_setting(base):
    """a window that starts inside a game: a live ply sums later plies of its own record only; agz_replay_clear leaves
    the setting alone"""
    b = base
    e = ag.Engine(board_size=N, tower_height=TOWER, games=1, num_readouts=8, max_nodes_per_game=16, seed=SEED)
    packed = b["eng"].records_packed().copy()
    assert e.replay_ingest(packed) == GAMES
    e.replay_set_value_target(0.25, 0.5)
    want = b["y"][(0.25, 0.5)]
    g1 = next(k for k in range(1, GAMES) if b["arena"][k]["num_moves"] > 3)
    live = b["L"] - sum(a["num_moves"] for a in b["arena"][:g1]) - 2      # the window starts at ply 2 of game g1
    e.replay_set_window(live)
    assert e.replay_live_positions() == live
    shift = GAMES - e.replay_count()                          # (dead games may have been dropped: the indices move up)
    s = sampled(e, live, 21)
    assert min(zip((s[3] + shift).tolist(), s[4].tolist())) == (g1, 2)
    assert bits_equal(s[2], np.array([want[b["at"][(int(a) + shift, int(c))]] for a, c in zip(s[3], s[4])], np.float32))
    e.replay_clear()
    assert e.replay_ingest(packed) == GAMES
    _, _, z = e.replay_batch(b["game"], b["ply"])
    assert bits_equal(z, want)
    e.close()


def test_targets_only_arena_sums_the_fast_plies_behind_a_target():
    """9x9, tower 2, playout_cap = (8, 0.5), a targets-only arena: every sampled ply is a target, its y is the twin's over
    ALL the record's qs, and at a target with a fast ply behind it that differs from the twin without that ply's q"""
    alpha, lam = 1.0, 0.9
    e = ag.Engine(board_size=9, tower_height=2, games=4, num_readouts=16, seed=5, record_capacity_games=12)
    e.init_synthetic(5)
    e.set_playout_cap(8, 0.5)
    play(e, 4)
    e.replay_set_targets_only(True)
    assert e.replay_ingest_records(0, 4) == 4
    e.replay_set_value_target(alpha, lam)
    arena = [e.replay_record(k) for k in range(4)]
    full = [(a["pis"] != 0).any(axis=1) for a in arena]
    L = e.replay_live_positions()
    assert L == sum(int(f.sum()) for f in full) and 4 <= L <= 2048 and L < e.replay_positions()
    _, pi, z, game, ply = sampled(e, L, 1)
    assert (pi != 0).any(axis=1).all()
    assert sorted(zip(game.tolist(), ply.tolist())) == [(k, int(t)) for k in range(4) for t in np.flatnonzero(full[k])]
    shown = 0
    for g, t, y in zip(game, ply, z):
        a = arena[int(g)]
        assert full[int(g)][t]
        assert vt.bits(y) == vt.bits(vt.value_target(a["qs"], int(t), a["result"], alpha, lam)), (g, t)
        fast_behind = [k for k in range(int(t) + 1, a["num_moves"]) if not full[int(g)][k]]
        if fast_behind:
            k = fast_behind[0]
            without = vt.value_target(np.delete(a["qs"], k), int(t), a["result"], alpha, lam)
            shown += int((vt.bits(y) != vt.bits(without)).any())
    print(f"{L} targets of {e.replay_positions()} plies; {shown} targets whose y shows the q of a fast ply behind them")
    assert shown >= 1
    e.close()


def test_ring_and_host_entries_agree_with_the_twin(base):
    b = base
    e = b["eng"]
    env = ag.GoEnv(N)
    assert e.records_count() == GAMES
    for k, r in enumerate(b["recs"]):
        pl = ag.SelfPlayPlayer(env, None, R, r)
        pos, pis, res = ag.extract_data(pl)
        assert res == [r["result"]] * r["num_moves"] and all(type(x) is int for x in res)        # today's constant
        for alpha, lam in vt.PAIRS:
            want = vt.value_targets(r["qs"], r["result"], alpha, lam)
            assert bits_equal(e.records_value_targets(k, alpha, lam), want), (k, alpha, lam)
            assert bits_equal(ag.value_targets(r["qs"], r["result"], alpha, lam), want)
            pos2, pis2, res2 = ag.extract_data(pl, value_target=(alpha, lam))
            assert len(pos2) == len(pos) and bits_equal(np.stack(pis2), np.stack(pis))
            assert bits_equal(np.array(res2, np.float32), want)
            assert bits_equal(np.array(pl.extract_data(value_target=(alpha, lam))[2], np.float32), want)
    with pytest.raises(ag.AgzError) as ei:
        e.records_value_targets(GAMES, 0.5, 0.5)              # agz_records_game's numbering and refusal
    assert ei.value.status == BAD_ARGUMENT


def test_live_player_extract_data_takes_the_keyword():
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=0)
    pl = ag.MCTSPlayer(env, nn, num_readouts=8)
    pl.initialize_game()
    for _ in range(4):
        assert pl.play_move(pl.suggest_move())
    pl.set_result(-1, True)
    pos, pis, res = ag.extract_data(pl)
    assert res == [-1] * 4
    pos2, pis2, res2 = ag.extract_data(pl, value_target=(0.5, 0.9))
    assert len(pos2) == 4 and bits_equal(np.stack(pis2), np.stack(pis))
    assert bits_equal(np.array(res2, np.float32), vt.value_targets(np.array(pl.qs, np.float32), -1, 0.5, 0.9))
    assert not bits_equal(np.array(res2, np.float32), np.array(res, np.float32))


def test_refusals_keep_the_setting_in_force(base):
    b = base
    e = b["eng"]
    e.replay_set_value_target(0.5, 0.9)
    for bad in (-0.1, 1.5, float("nan")):
        for alpha, lam in ((bad, 0.5), (0.5, bad)):
            with pytest.raises(ag.AgzError) as ei:
                e.replay_set_value_target(alpha, lam)
            assert ei.value.status == BAD_ARGUMENT and "0..1" in str(ei.value)
            with pytest.raises(ag.AgzError) as ei:
                e.records_value_targets(0, alpha, lam)
            assert ei.value.status == BAD_ARGUMENT
    _, _, z = e.replay_batch(b["game"], b["ply"])
    assert bits_equal(z, np.concatenate([vt.value_targets(a["qs"], a["result"], 0.5, 0.9) for a in b["arena"]]))
    assert not bits_equal(z, b["z"])


# ---------------------------------------------------------------- train(..., value_target=...)

TRAIN = dict(num_games=6, memory=40, B=8, start_after=8, slots=4, seed=3)


def by_hand(env, value_target):
    """train()'s schedule by single calls on an engine of its own: self-play steps, agz_replay_ingest_records,
    agz_replay_set_window, agz_replay_sample, agz_train_step -> (the weights left, trainings done)"""
    import torch
    c = TRAIN
    nn0 = ag.NeuralNet(env, tower_height=TOWER, seed=1)
    eng = ag.Engine(board_size=N, tower_height=TOWER, games=c["slots"], num_readouts=R, seed=c["seed"],
                    record_capacity_games=c["slots"] + 8)
    nn0.engine.copy_weights_to(eng)
    if value_target is not None:
        eng.replay_set_value_target(*value_target)
    dev = torch.device("cuda", eng.cfg.device)
    feats = torch.empty((c["B"], 17 * eng.P), dtype=torch.float32, device=dev)
    pi = torch.empty((c["B"], eng.A), dtype=torch.float32, device=dev)
    z = torch.empty(c["B"], dtype=torch.float32, device=dev)
    eng.set_hold(True)
    eng.start(c["num_games"])
    eng.release()
    i = trained = 0
    for _ in range(200000):
        if i >= c["num_games"]:
            break
        eng.step(1)
        n = eng.records_count()
        if n == 0:
            continue
        for _, k in sorted((eng.record_header(k)["game_id"], k) for k in range(n)):
            assert eng.replay_ingest_records(k, 1) == 1
            eng.replay_set_window(c["memory"])
            i += 1
            if eng.replay_live_positions() >= c["start_after"]:
                eng.replay_sample(c["B"], i, -1, feats, pi, z)
                eng.train_step_device(feats, pi, z, c["B"], eta=0.02, rho=0.9)
                trained += 1
        eng.records_clear()
        eng.release()
    assert i == c["num_games"]
    w = _weights(eng)
    eng.close()
    return w, trained


def test_train_takes_the_value_target():
    """train(..., value_target=(0.5, 0.9), slots=4) leaves, byte for byte, the weights of the same schedule run by hand
    with the setting on -- and those differ from the same run with the setting off"""
    c = TRAIN
    env = ag.GoEnv(N)
    w_on, trained = by_hand(env, (0.5, 0.9))
    w_off, trained_off = by_hand(env, None)
    assert trained >= 3 and trained_off >= 3
    nn = ag.train(env, num_games=c["num_games"], memory_size=c["memory"], batch_size=c["B"], readouts=R,
                  model=ag.NeuralNet(env, tower_height=TOWER, seed=1), start_training_after=c["start_after"],
                  slots=c["slots"], seed=c["seed"], callback=None, value_target=(0.5, 0.9))
    bad = weight_mismatches(nn.engine, w_on)
    assert not bad, bad
    assert weight_mismatches(nn.engine, w_off), "the value target changed no weight"
    nn_off = ag.train(env, num_games=c["num_games"], memory_size=c["memory"], batch_size=c["B"], readouts=R,
                      model=ag.NeuralNet(env, tower_height=TOWER, seed=1), start_training_after=c["start_after"],
                      slots=c["slots"], seed=c["seed"], callback=None)
    assert not weight_mismatches(nn_off.engine, w_off)

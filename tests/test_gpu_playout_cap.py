"""Playout cap randomization on the device (agz_selfplay_set_playout_cap, agz_replay_set_targets_only).

With the cap on, every self-play game must be, bit for bit, the twin's game (tests/selfplay_twin.py: the reference's loop
with the coin u01(draw(seed, game, n, site 11, 0)) < p before each search) on the engine's own forward: full plies with noise,
R readouts and their pi, fast plies without noise, r readouts and an all-zero pi row.  Off -- r = 0, or every search
full -- is today's engine byte for byte.  A targets-only arena counts, keeps and samples the non-zero rows only, as the
numpy restatement of the sampler says; train(..., playout_cap=...) is that schedule."""
import numpy as np
import pytest

import alphago_jl_amd as ag
import orc
import selfplay_twin as tw
from alphago_jl_amd import symmetry as sy
from gpu_common import GpuNetForOracle, pos_soa
from gpu_options import (SymNetForOracle, _twin_pairs, arena_pis, assert_game_equals_twin, assert_train_equals_twin,
                         count_targets, host_schedule, peaked_engine)
from gpu_options import play as play_sorted
from test_hostsim_selfplay import bits_equal

pytestmark = pytest.mark.gpu
L = orc.lib()
BAD_ARGUMENT = ag._lib.BAD_ARGUMENT


def play(eng, games):
    return play_sorted(eng, games, sort=False)


def assert_cap_game_equal(r, o, what):
    assert_game_equals_twin(r, o, what, o["full"])


def assert_mixed(twins):
    nfull = nfast = 0
    for o in twins:
        assert o["full"].any() and (~o["full"]).any(), "a game of the set is all full or all fast"
        nfull += int(o["full"].sum())
        nfast += int((~o["full"]).sum())
    assert nfull >= 3 and nfast >= 3, (nfull, nfast)


def check_against_twins(eng, recs, st, twin_of, seed, p, starts=None):
    twins = []
    for r in recs:
        gid = int(r["game_id"])
        o = twin_of(gid)
        assert_cap_game_equal(r, o, gid)
        n0 = starts[gid % len(starts)].n if starts else 0
        assert (o["full"] == tw.pattern(seed, gid, n0, o["num_moves"], p)).all()
        twins.append(o)
    assert_mixed(twins)
    nfull, nfast = sum(int(o["full"].sum()) for o in twins), sum(int((~o["full"]).sum()) for o in twins)
    print(f"{len(recs)} games: {nfull} full + {nfast} fast moves, evals {st['evals']}")
    resigned = sum(int(o["was_resign"]) for o in twins)
    print(f"{resigned} games ended by resignation, {len(twins) - resigned} by two passes or the length limit")
    assert eng.playout_cap_counts() == (nfull, nfast)
    assert st["positions"] == nfull + nfast
    assert st["evals"] == sum(o["evals"] for o in twins)
    return twins


# ---------------------------------------------------------------- off is off

def test_off_and_all_full_are_the_plain_engine():
    N, tower, R, games = 9, 1, 16, 4
    out = []
    for cap in (None, (0, 0.3), (R, 1.0)):
        eng = ag.Engine(board_size=N, tower_height=tower, games=games, num_readouts=R, seed=2,
                        record_capacity_games=games + 8)
        eng.init_synthetic(0)
        if cap is not None:
            eng.set_playout_cap(*cap)
        recs, st = play(eng, games)
        out.append((eng.records_packed().copy(), st, eng.playout_cap_counts()))
        eng.close()
    for packed, st, _ in out[1:]:
        assert packed.tobytes() == out[0][0].tobytes()
        assert st == out[0][1]
    assert out[0][2] == (0, 0) and out[1][2] == (0, 0)
    assert out[2][2] == (out[0][1]["positions"], 0)


# ---------------------------------------------------------------- bit-exact games

@pytest.mark.parametrize("N,tower,R,r,p,games,slots,seed,resign", [
    (9, 2, 32, 8, 0.3, 32, 32, 4, (-0.9, 0.05)),
    (5, 1, 16, 4, 0.4, 40, 32, 2, (-2.0, 0.0)),
])
def test_games_with_the_cap_equal_the_twin(N, tower, R, r, p, games, slots, seed, resign):
    eng = ag.Engine(board_size=N, tower_height=tower, games=slots, num_readouts=R, seed=seed,
                    record_capacity_games=games + 8, resign_threshold=resign[0], resign_disable_fraction=resign[1])
    eng.init_synthetic(0)
    eng.set_playout_cap(r, p)
    recs, st = play(eng, games)
    fwd = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=8, max_nodes_per_game=16)
    fwd.init_synthetic(0)
    cb = GpuNetForOracle(fwd).cb
    check_against_twins(eng, recs, st, lambda gid: tw.twin_selfplay(N, cb, R, seed, gid, None, *resign, cap=(r, p)), seed, p)
    eng.close()
    fwd.close()


def test_games_with_the_cap_from_a_starts_table_equal_the_twin():
    N, tower, R, r, p, games, slots, seed = 5, 1, 16, 4, 0.4, 12, 4, 3
    starts = tw.random_starts(N, (1, 4, 7, 12, 2, 9), seed=0)
    eng = ag.Engine(board_size=N, tower_height=tower, games=slots, num_readouts=R, seed=seed,
                    record_capacity_games=games + 8, resign_threshold=-2.0, resign_disable_fraction=0.0)
    eng.init_synthetic(0)
    b, i, h = tw.opos_arrays(starts)
    eng.set_starts(boards=b, info=i, history=h)
    eng.set_playout_cap(r, p)
    recs, st = play(eng, games)
    fwd = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=8, max_nodes_per_game=16)
    fwd.init_synthetic(0)
    cb = GpuNetForOracle(fwd).cb
    check_against_twins(eng, recs, st, lambda gid: tw.twin_selfplay(N, cb, R, seed, gid, starts[gid % 6], -2.0, 0.0,
                                                                   cap=(r, p)), seed, p, starts)
    eng.close()
    fwd.close()


def test_games_with_the_cap_and_random_symmetry_equal_the_twin():
    N, tower, R, r, p, games, seed = 9, 1, 16, 4, 0.3, 3, 4
    eng = peaked_engine(N, tower, games=games, num_readouts=R, seed=seed, record_capacity_games=games + 8)
    eng.set_symmetry("random")
    eng.set_playout_cap(r, p)
    recs, st = play(eng, games)
    fwd = peaked_engine(N, tower, games=1, num_readouts=8, max_nodes_per_game=16)
    seen = set()

    def twin_of(gid):
        net = SymNetForOracle(fwd, seed, gid, sy.RANDOM)
        o = tw.twin_selfplay(N, net.cb, R, seed, gid, None, -0.9, 0.05, cap=(r, p))
        seen.update(net.syms)
        return o

    check_against_twins(eng, recs, st, twin_of, seed, p)
    assert seen == set(range(8))
    eng.close()
    fwd.close()


# ---------------------------------------------------------------- noise gating

def test_noise_only_on_full_searches():
    """the root's priors after a fast decision are the network's, bit for bit; after a full one they are not -- at both
    places that decide: behind the pre-expansion (n = 0) and behind a move (n = 1)"""
    N, tower, R, r, p, seed = 5, 1, 8, 2, 0.5, 6
    fwd = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=8, max_nodes_per_game=16)
    fwd.init_synthetic(0)
    seen = {0: set(), 1: set()}
    for gid in range(8):
        eng = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=R, seed=seed, game_id_base=gid,
                        resign_threshold=-2.0, resign_disable_fraction=0.0)
        eng.init_synthetic(0)
        eng.set_playout_cap(r, p)
        eng.start(1)
        eng.step(1)                                             # the pre-expansion and the decision for n = 0
        pos = orc.make_pos(N)
        for n in (0, 1):
            if n == 1:
                for _ in range(64):
                    if eng.slot_status()[2][0] >= 1:
                        break
                    eng.step(1)
                assert eng.slot_status()[2][0] == 1
                move = int(eng.debug_live_record(0, 0)[2])
                rcode, pos = orc.play(pos, move)
                assert rcode == orc.OK
            root = eng.tree_root(0)
            got = eng.node_floats(0, root, 2)
            want, _ = fwd.forward(*pos_soa([pos]))
            full = bool(tw.coin_full(seed, gid, n, p))
            seen[n].add(full)
            print(f"game {gid}, n = {n}: {'full' if full else 'fast'}, max |prior - net| "
                  f"{float(np.abs(got - want[0]).max()):.3e}")
            if full:
                assert not bits_equal(got, want[0]), (gid, n)
            else:
                assert bits_equal(got, want[0]), (gid, n)
        eng.close()
    assert seen[0] == {True, False} and seen[1] == {True, False}, seen
    fwd.close()


# ---------------------------------------------------------------- refusals

def test_refusals():
    N, R = 5, 16

    def refused(fn, word):
        with pytest.raises(ag.AgzError) as e:
            fn()
        assert e.value.status == BAD_ARGUMENT and word in str(e.value), str(e.value)
        assert "AGZ_" not in str(e.value).split(":", 1)[-1]

    arena = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=R, arena_mode=1)
    refused(lambda: arena.set_playout_cap(4, 0.5), "arena")
    arena.close()
    eng = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=R, seed=1, record_capacity_games=8)
    eng.init_synthetic(0)
    refused(lambda: eng.set_playout_cap(R + 1, 0.5), "fast readouts")
    refused(lambda: eng.set_playout_cap(-1, 0.5), "fast readouts")
    for bad in (-0.01, 1.01, float("nan")):
        refused(lambda: eng.set_playout_cap(4, bad), "full_prob")
    eng.set_playout_cap(4, 0.0)
    eng.set_playout_cap(R, 1.0)
    eng.set_playout_cap(4, 0.4)
    eng.start(2)
    eng.set_playout_cap(4, 0.4)                  # started, not stepped: no game claimed yet
    eng.step(3)
    refused(lambda: eng.set_playout_cap(0, 1.0), "still being played")
    refused(lambda: eng.set_playout_cap(4, 0.5), "still being played")
    while eng.records_count() < 2:
        eng.step(8)
    eng.set_playout_cap(4, 0.4)                  # the run is over
    # the arena's mode changes only while it is empty
    eng.replay_set_targets_only(True)
    eng.replay_set_targets_only(False)
    assert eng.replay_ingest_records(0, 2) == 2
    refused(lambda: eng.replay_set_targets_only(True), "replay arena")
    refused(lambda: eng.replay_set_targets_only(False), "replay arena")
    assert eng.replay_live_positions() == eng.replay_positions()
    eng.replay_clear()
    eng.replay_set_targets_only(True)
    eng.close()


# ---------------------------------------------------------------- the targets-only arena

def check_samples(e, live_want, calls_and_B):
    import torch
    from test_train_loop_batched import sample_syms
    pis = arena_pis(e)
    assert e.replay_live_positions() == live_want
    for call, B, sym in calls_and_B:
        feats, pi, z, game, ply = e.replay_sample(B, call, sym)
        torch.cuda.synchronize()
        e.sync()
        want, Lw = tw.sample_targets(e.cfg.seed, call, B, pis, window=live_want)
        assert Lw == live_want
        g = np.array([a for a, _ in want], np.int64)
        q = np.array([b for _, b in want], np.int32)
        assert (game.cpu().numpy() == g).all() and (ply.cpu().numpy() == q).all(), (call, B)
        if sym == -1:
            wf, wp, wz = e.replay_batch(g, q)
        else:
            s = sample_syms(e.cfg.seed, call, B) if sym == 8 else np.full(B, sym, np.int32)
            wf, wp, wz = e.replay_batch_sym(g, q, s)
        got_pi = pi.cpu().numpy()
        assert (got_pi != 0).any(axis=1).all(), "a sampled pi row is all zero"
        assert bits_equal(feats.cpu().numpy(), wf) and bits_equal(got_pi, wp) and bits_equal(z.cpu().numpy(), wz)


def test_targets_only_arena_counts_and_samples_the_nonzero_rows():
    import torch
    N, tower, R, r, p, games, seed = 9, 1, 8, 2, 0.4, 128, 5       # about 25 targets a game: 2048 need more than 84
    eng = ag.Engine(board_size=N, tower_height=tower, games=games, num_readouts=R, seed=seed,
                    record_capacity_games=games + 8)
    eng.init_synthetic(5)
    eng.set_playout_cap(r, p)
    recs, _ = play(eng, games)
    packed = eng.records_packed().copy()
    total = sum(int(x["num_moves"]) for x in recs)
    targets = count_targets([x["pis"] for x in recs])
    print(f"{games} games, {total} plies, {targets} targets")
    assert 2048 <= targets < total
    by_packed = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=8, max_nodes_per_game=16, seed=seed)
    plain = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=8, max_nodes_per_game=16, seed=seed)
    eng.replay_set_targets_only(True)
    by_packed.replay_set_targets_only(True)
    half = games // 2
    assert eng.replay_ingest_records(0, half) == half            # two ingest calls: the index grows
    assert eng.replay_ingest_records(half, games - half) == games - half
    assert by_packed.replay_ingest(packed) == games
    assert plain.replay_ingest(packed) == games
    for e in (eng, by_packed):
        assert e.replay_count() == games and e.replay_positions() == total       # these count every ply
        pis = arena_pis(e)
        assert count_targets(pis) == targets
        check_samples(e, targets, [(1, 8, -1), (2, 2048, -1), (3, 256, 8)])
        # a window that cuts a game in the middle of its targets, then one small enough to drop dead games physically
        per_game = [int((x != 0).any(axis=1).sum()) for x in pis]
        first_big = next(k for k, c in enumerate(per_game) if c >= 4)
        cut = targets - sum(per_game[:first_big]) - 2
        e.replay_set_window(cut)
        check_samples(e, cut, [(4, 64, -1), (5, min(cut, 2048), -1)])
        e.replay_set_window(targets)                               # the window's start never moves back
        assert e.replay_live_positions() == cut
        before = e.replay_count()
        e.replay_set_window(300)
        assert e.replay_count() < before, "dead games were dropped: the target lists moved with them"
        check_samples(e, 300, [(6, 32, -1), (7, 300, 5)])
        # agz_replay_trim counts every ply, and the window lives on in the games it keeps
        # (here the window began in the game that is dropped: every target of the games kept is live again)
        e.replay_trim(e.replay_positions() - len(arena_pis(e)[0]))
        assert e.replay_count() >= 2
        live = count_targets(arena_pis(e))
        check_samples(e, live, [(8, 16, -1)])
        # agz_replay_clear empties the arena and keeps the mode
        e.replay_clear()
        assert e.replay_ingest(packed) == games
        assert e.replay_live_positions() == targets and e.replay_positions() == total
    # targets-only off: the same records sample as they always did
    assert plain.replay_live_positions() == total
    for call, B in ((1, 64), (2, 2048)):
        feats, pi, z, game, ply = plain.replay_sample(B, call)
        torch.cuda.synchronize()
        plain.sync()
        g, q = _twin_pairs(plain, call, B)
        assert (game.cpu().numpy() == g).all() and (ply.cpu().numpy() == q).all()
        wf, wp, wz = plain.replay_batch(g, q)
        assert bits_equal(feats.cpu().numpy(), wf) and bits_equal(pi.cpu().numpy(), wp)
    assert not (pi.cpu().numpy() != 0).any(axis=1).all(), "without the mode, zero rows are sampled too"
    for e in (eng, by_packed, plain):
        e.close()


# ---------------------------------------------------------------- train(..., playout_cap=...)

TRAIN = dict(N=5, TOWER=1, R=16, r=4, p=0.4, SEED=3, num_games=8, slots=4, memory=40, B=8, start_after=8)


def test_train_with_the_cap_plays_the_twins_games_and_counts_targets():
    c = TRAIN
    env = ag.GoEnv(c["N"])
    nn0 = ag.NeuralNet(env, tower_height=c["TOWER"], seed=1)
    ref, snaps, start_step, _ = host_schedule(nn0, c, lambda eng: eng.set_playout_cap(c["r"], c["p"]), targets_only=True)
    twins, log = assert_train_equals_twin(
        env, nn0, c, (ref, snaps, start_step),
        lambda cb, gid, on_round: tw.twin_selfplay(c["N"], cb, c["R"], c["SEED"], gid, None, -0.9, 0.05, on_round=on_round,
                                                   cap=(c["r"], c["p"])),
        masked=True, playout_cap=(c["r"], c["p"]))
    nfull, nfast = sum(int(o["full"].sum()) for o in twins), sum(int((~o["full"]).sum()) for o in twins)
    assert nfull >= 3 and nfast >= 3, (nfull, nfast)          # (a game that resigns early may hold one kind only)
    targets = 0
    for x, y in zip(log, ref):
        targets += count_targets([x["record"]["pis"][: x["record"]["num_moves"]]])
        assert x["live"] == y["live"] == min(c["memory"], targets)
    assert targets < sum(int(x["record"]["num_moves"]) for x in log)


def test_selfplay_takes_the_cap_and_extract_data_drops_fast_plies():
    N, R, r, p = 5, 16, 4, 0.4
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=0)
    players = ag.selfplay(env, nn, R, games=4, seed=2, game_id_base=0, playout_cap=(r, p), resign_threshold=-2.0,
                          resign_disable_fraction=0.0)
    cb = GpuNetForOracle(nn.engine).cb
    for gid, pl in enumerate(players):
        o = tw.twin_selfplay(N, cb, R, 2, gid, None, -2.0, 0.0, cap=(r, p))
        assert [ag.to_flat(m, env) for m in pl.moves] == list(o["moves"]) and pl.result == o["result"]
        assert pl.full_search == list(o["full"])
        pos, pis, res = ag.extract_data(pl)
        assert len(pos) == len(pis) == len(res) == o["num_moves"] and bits_equal(np.stack(pis), o["pis"])
        tpos, tpis, tres = ag.extract_data(pl, targets_only=True)
        keep = np.flatnonzero(o["full"])
        assert len(tpos) == len(tpis) == len(tres) == len(keep) < o["num_moves"]
        assert bits_equal(np.stack(tpis), o["pis"][keep]) and [q.n for q in tpos] == [pos[k].n for k in keep]

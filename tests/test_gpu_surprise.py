"""Policy surprise weighting on the device (include/agz.h agz_replay_score, include/agz_surprise.h): the
scores and weights of agz_replay_score / agz_replay_surprise against the engine-free agz_surprise_weights on the priors
the network gives game by game, bit for bit; agz_replay_sample under rho > 0 against the twin's picks
(tests/surprise_twin.py) over the read-back q, in an all-plies and a targets-only arena under a window that starts inside
a game; the off path against an engine that never made the calls; what ingest, trim, reanalysis and clear do to the
scores; the scan at a size that crosses one tile; games in flight; train(..., surprise=...) against the same schedule by
hand; the refusals."""
import numpy as np
import pytest

import alphago_jl_amd as ag
import surprise_twin as st
from gpu_options import _weights, play, weight_mismatches
from test_hostsim_selfplay import bits_equal

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = ag._lib.BAD_ARGUMENT
N, TOWER, R, GAMES, SLOTS, SEED = 5, 1, 16, 8, 4, 3
UNIT = st.UNIT


def sampled(e, B, call, sym=-1):
    """agz_replay_sample on the host: feats, pi, z, game, ply"""
    import torch
    out = e.replay_sample(B, call, sym)
    torch.cuda.synchronize()
    e.sync()
    return [t.cpu().numpy() for t in out]


def engine(**kw):
    cfg = dict(board_size=N, tower_height=TOWER, games=SLOTS, num_readouts=R, seed=SEED, record_capacity_games=GAMES + 8)
    cfg.update(kw)
    e = ag.Engine(**cfg)
    e.init_synthetic(0)
    return e


def priors(e, k):
    """the network's priors for every ply of arena game k, evaluated for that game alone"""
    n = e.replay_record(k)["num_moves"]
    feats, _, _ = e.replay_batch(np.full(n, k, np.int64), np.arange(n, dtype=np.int32))
    return e.forward_features(feats)[0]


def surprise_all(e):
    return [e.replay_surprise(k) for k in range(e.replay_count())]


@pytest.fixture(scope="module")
def base():
    """5x5, tower 1, R = 16, 8 games on 4 slots under playout_cap = (8, 0.5), so zero pi rows occur.  `eng` holds them in
    an all-plies arena and is scored; `tonly` holds them in a targets-only arena, with the same network; `plain` never
    makes a call of this feature.  The expected (kl, q) of every game under rho = 0, 0.5 and 1 from agz_surprise_weights
    on priors evaluated game by game"""
    eng = engine()
    eng.set_playout_cap(8, 0.5)
    assert len(play(eng, GAMES)[0]) == GAMES
    assert eng.replay_ingest_records(0, GAMES) == GAMES
    packed = eng.records_packed().copy()
    plain = engine()
    assert plain.replay_ingest(packed) == GAMES
    tonly = engine()
    tonly.replay_set_targets_only(True)
    assert tonly.replay_ingest(packed) == GAMES
    arena = [eng.replay_record(k) for k in range(GAMES)]
    targets = [(a["pis"] != 0).any(axis=1) for a in arena]
    print("games (moves, targets):", [(a["num_moves"], int(t.sum())) for a, t in zip(arena, targets)])
    assert any((~t).any() for t in targets) and all(t.sum() >= 3 for t in targets[1:3])
    ps = [priors(eng, k) for k in range(GAMES)]
    want = {rho: [ag.surprise_weights(a["pis"], p, rho) for a, p in zip(arena, ps)] for rho in (0.0, 0.5, 1.0)}
    d = dict(eng=eng, plain=plain, tonly=tonly, packed=packed, arena=arena, targets=targets, ps=ps, want=want,
             lengths=[a["num_moves"] for a in arena], ntargets=int(sum(t.sum() for t in targets)))
    yield d
    for e in (eng, plain, tonly):
        e.close()


def test_scores_equal_the_host_weights_bit_for_bit(base):
    b = base
    e = b["eng"]
    fresh = engine()                                            # unscored: no scores, every ply weighs 1 under any rho
    fresh.replay_ingest(b["packed"])
    fresh.replay_set_surprise(0.5)
    for kl, q, scored in surprise_all(fresh):
        assert not scored and (kl == 0).all() and (q == UNIT).all()
    fresh.close()
    assert e.replay_score() == b["ntargets"]
    for rho in (0.5, 1.0, 0.0):
        e.replay_set_surprise(rho)
        for k, (kl, q, scored) in enumerate(surprise_all(e)):
            wkl, wq = b["want"][rho][k]
            assert scored and (st.bits(kl) == st.bits(wkl)).all() and (q == wq).all(), (rho, k)
            tkl, tq = st.weights(b["arena"][k]["pis"], b["ps"][k], rho)           # and the twin says the same
            assert (st.bits(kl) == st.bits(tkl)).all() and (q == tq).all(), (rho, k)
            assert (kl[~b["targets"][k]] == 0).all() and (q[~b["targets"][k]] == UNIT).all()
    kls = np.concatenate([w[0][t] for w, t in zip(b["want"][0.5], b["targets"])])
    print(f"{len(kls)} target plies: KL min {kls.min():.4f} median {np.median(kls):.4f} max {kls.max():.4f}")
    assert kls.max() > 0
    # a range scored in two calls and in one: the same bits (the chunks of the forward do not show)
    t = b["tonly"]
    assert t.replay_score(0, 3) + t.replay_score(3, GAMES - 3) == b["ntargets"]
    t.replay_set_surprise(0.5)
    for k, (kl, q, scored) in enumerate(surprise_all(t)):
        wkl, wq = b["want"][0.5][k]
        assert scored and (st.bits(kl) == st.bits(wkl)).all() and (q == wq).all(), k
    e.replay_set_surprise(0.0)
    t.replay_set_surprise(0.0)


def _window(e, targets, tonly, g1, skip):
    """the window of e starts `skip` entries into game g1 (entries: the target plies of a targets-only arena, else every
    ply) -> the live entries and the window's first (game, ply)"""
    count = [int(t.sum()) if tonly else len(t) for t in targets]
    live = sum(count[g1:]) - skip
    e.replay_set_window(live)
    assert e.replay_live_positions() == live
    assert e.replay_count() == GAMES                            # (nothing dropped: the dead part is small)
    return live, (g1, int(np.flatnonzero(targets[g1])[skip]) if tonly else skip)


@pytest.mark.parametrize("rho", [0.5, 1.0])
@pytest.mark.parametrize("mode", ["all", "targets_only"])
def test_sampler_equals_the_twin(base, mode, rho):
    b = base
    tonly = mode == "targets_only"
    e = b["tonly"] if tonly else b["eng"]
    if not e.replay_surprise(0)[2]:
        e.replay_score()
    fg, fp = 1, 2
    live, first = _window(e, b["targets"], tonly, fg, fp)
    e.replay_set_surprise(rho)
    qs = [q for _, q, _ in surprise_all(e)]
    tg = b["targets"] if tonly else None
    try:
        for B, call, sym, vt in ((1, 1, -1, None), (64, 2, -1, None), (live + 3, 3, -1, None), (64, 4, 8, None),
                                 (64, 5, -1, (0.5, 0.9))):
            if vt:
                e.replay_set_value_target(*vt)
            f, p, z, game, ply = sampled(e, B, call, sym)
            wg, wp = st.sample_pairs(SEED, call, B, qs, fg, fp, tg)
            assert (game == wg).all() and (ply == wp).all(), (B, call)
            assert min(zip(game.tolist(), ply.tolist())) >= first
            if tonly:
                assert all(b["targets"][g][t] for g, t in zip(game, ply))
            if sym == 8:
                f0, p0, z0 = e.replay_batch_sym(game, ply, st.sample_syms(SEED, call, B))
            else:
                f0, p0, z0 = e.replay_batch(game, ply)
            assert bits_equal(f, f0) and bits_equal(p, p0) and bits_equal(z, z0), (B, call)
            if vt:
                assert not bits_equal(z, np.array([b["arena"][g]["result"] for g in game], np.float32))
            if B > live:
                assert len(set(zip(game.tolist(), ply.tolist()))) < B            # with replacement
    finally:
        e.replay_set_value_target(0.0, 1.0)
        e.replay_set_surprise(0.0)
        e.replay_set_window(-1)


def test_off_path_is_the_parents(base):
    """rho never set (tonly's twin below), and rho set back to 0 on an engine that has scores: agz_replay_sample gives
    what an engine that never made a call of this feature gives"""
    b = base
    e, plain = b["eng"], b["plain"]
    if not e.replay_surprise(0)[2]:
        e.replay_score()
    e.replay_set_surprise(0.5)
    sampled(e, 8, 1)
    e.replay_set_surprise(0.0)
    L = sum(b["lengths"])
    for B, call, mode in ((2, 1, -1), (32, 2, 8), (L, 3, -1)):
        s0, s1 = sampled(plain, B, call, mode), sampled(e, B, call, mode)
        assert all(bits_equal(x, y) for x, y in zip(s0, s1)), (B, call)
    assert len(set(zip(s1[3].tolist(), s1[4].tolist()))) == L                   # the Floyd draw: distinct entries
    with pytest.raises(ag.AgzError):
        sampled(e, L + 1, 4)                                      # and its bound, B <= L
    never = engine()                                              # scored, rho never set
    never.replay_ingest(b["packed"])
    never.replay_score()
    for B, call, mode in ((2, 1, -1), (32, 2, 8)):
        assert all(bits_equal(x, y) for x, y in zip(sampled(plain, B, call, mode), sampled(never, B, call, mode)))
    never.close()


def test_invalidation(base):
    b = base
    recs = ag.distributed.unpack_records(b["packed"], N * N + 1)
    pack = lambda rs: ag.distributed.pack_records(rs, N * N + 1)
    e = engine()
    e.replay_set_surprise(0.5)
    assert e.replay_ingest(pack(recs[:4])) == 4
    e.replay_score()
    before = surprise_all(e)
    assert all(s for _, _, s in before) and any((q != UNIT).any() for _, q, _ in before)
    assert e.replay_ingest(pack(recs[4:])) == 4                   # ingest: the new games are unscored and weigh 1
    now = surprise_all(e)
    for k in range(4):
        assert now[k][2] and (st.bits(now[k][0]) == st.bits(before[k][0])).all() and (now[k][1] == before[k][1]).all()
    for k in range(4, 8):
        assert not now[k][2] and (now[k][1] == UNIT).all() and (now[k][0] == 0).all()
    s = sampled(e, 16, 1)                                         # (a mixed arena samples)
    wg, wp = st.sample_pairs(SEED, 1, 16, [q for _, q, _ in now])
    assert (s[3] == wg).all() and (s[4] == wp).all()
    e.replay_score(4, 2)
    e.replay_trim(sum(b["lengths"][2:]))                          # trim: games 0 and 1 go, the scores move with the rest
    assert e.replay_count() == 6
    after = surprise_all(e)
    for k in (2, 3):
        assert after[k - 2][2] and (st.bits(after[k - 2][0]) == st.bits(before[k][0])).all()
        assert (after[k - 2][1] == before[k][1]).all()
    assert [x[2] for x in after] == [True, True, True, True, False, False]
    wkl, wq = b["want"][0.5][4]
    assert (st.bits(after[2][0]) == st.bits(wkl)).all() and (after[2][1] == wq).all()
    s = sampled(e, 16, 2)
    wg, wp = st.sample_pairs(SEED, 2, 16, [q for _, q, _ in after])
    assert (s[3] == wg).all() and (s[4] == wp).all()
    counts, _ = ag.reanalyze(e, first=1, count=2)                 # reanalysis commit: its games' pi changed
    assert counts["committed"] > 0
    assert [x[2] for x in surprise_all(e)] == [True, False, False, True, False, False]
    assert (e.replay_surprise(1)[1] == UNIT).all()
    assert e.replay_score(1, 2) > 0                               # scored again, on the new rows
    assert [x[2] for x in surprise_all(e)] == [True, True, True, True, False, False]
    e.replay_clear()                                              # clear: everything goes, rho stays
    assert e.replay_count() == 0
    assert e.replay_ingest(pack(recs[:2])) == 2
    assert [x[2] for x in surprise_all(e)] == [False, False]
    e.replay_score()
    got = surprise_all(e)
    for k in range(2):
        assert (st.bits(got[k][0]) == st.bits(b["want"][0.5][k][0])).all() and (got[k][1] == b["want"][0.5][k][1]).all()
    e.close()


def test_prefix_scan_across_a_tile(base):
    """the scan works in tiles of 1024 positions: an arena of the eight games several times over (hand-packed, fresh game
    ids) holds more than one tile and no whole number of them; an arena of one copy holds less than one.  The picks
    over both, and over the large one under a window, against the twin"""
    b = base
    recs = ag.distributed.unpack_records(b["packed"], N * N + 1)
    big = []
    for c in range(1024 // sum(b["lengths"]) + 2):
        for r in recs:
            big.append(dict(r, game_id=int(r["game_id"]) + 100 * c))
    e = engine()
    assert e.replay_ingest(ag.distributed.pack_records(big, N * N + 1)) == len(big)
    npos = e.replay_positions()
    print("positions:", npos)
    assert npos > 1024 and npos % 1024 != 0 and sum(b["lengths"]) < 1024
    e.replay_score(0, len(big) - 3)                               # (the last games stay unscored)
    e.replay_set_surprise(0.5)
    qs = [q for _, q, _ in surprise_all(e)]
    for k in range(GAMES):                                        # a copy of a game scores as the game does
        assert (qs[k] == b["want"][0.5][k][1]).all() and (qs[GAMES + k] == qs[k]).all()
    for B, call in ((64, 1), (2048, 2)):
        _, _, _, game, ply = sampled(e, B, call)
        wg, wp = st.sample_pairs(SEED, call, B, qs)
        assert (game == wg).all() and (ply == wp).all(), (B, call)
    cum = np.concatenate([[0], np.cumsum([len(q) for q in qs])])
    at = cum[game] + ply
    assert at.max() >= 1024 and at.min() < 1024                   # both tiles are reached
    # under a window: one that starts inside the first tile, then one whose dead games are dropped from the arena's
    # front (more than half of its bytes), which moves the scores up with the position prefix
    for start, call in ((300, 3), (1000, 4)):
        old = e.replay_count()
        e.replay_set_window(npos - start)
        shift = old - e.replay_count()
        assert (shift > 0) == (start == 1000)
        now = [q for _, q, _ in surprise_all(e)]
        assert len(now) == len(qs) - shift and all((x == y).all() for x, y in zip(now, qs[shift:]))
        qs = now
        cum = np.concatenate([[0], np.cumsum([len(q) for q in qs])])
        first = int(cum[-1]) - e.replay_live_positions()
        fg = int(np.searchsorted(cum, first, side="right") - 1)
        _, _, _, game, ply = sampled(e, 256, call)
        wg, wp = st.sample_pairs(SEED, call, 256, qs, fg, first - int(cum[fg]))
        assert (game == wg).all() and (ply == wp).all(), start
        assert min(zip(game.tolist(), ply.tolist())) >= (fg, first - int(cum[fg]))
    e.close()


def test_games_in_flight_are_left_alone():
    """a train()-like loop with the hold on: the records are the same, bit for bit, with agz_replay_score running
    between the steps while games are in flight"""
    def run(score):
        e = engine()
        e.set_playout_cap(8, 0.5)
        e.set_hold(True)
        e.start(GAMES)
        e.release()
        done, out, calls = 0, [], 0
        for _ in range(200000):
            if done >= GAMES:
                break
            e.step(1)
            if score and e.replay_count():
                calls += 1
                assert e.replay_score(e.replay_count() - 1, 1) >= 0
            n = e.records_count()
            if n == 0:
                continue
            out += sorted(e.records(), key=lambda r: r["game_id"])
            assert e.replay_ingest_records(0, n) == n
            if score:
                e.replay_score()
            done += n
            e.records_clear()
            e.release()
        e.close()
        return out, calls
    a, calls = run(True)
    c, _ = run(False)
    assert calls > 10 and len(a) == len(c) == GAMES
    for x, y in zip(a, c):
        assert x["game_id"] == y["game_id"] and x["num_moves"] == y["num_moves"] and x["result"] == y["result"]
        assert (x["moves"] == y["moves"]).all() and bits_equal(x["pis"], y["pis"]) and bits_equal(x["qs"], y["qs"])


# ---------------------------------------------------------------- train(..., surprise=...)

TRAIN = dict(num_games=6, memory=40, B=8, start_after=8, slots=4, seed=3)


def by_hand(env, rho):
    """train()'s schedule by single calls on an engine of its own: steps, ingest, score, window, sample, train step
    -> (the weights left, the losses)"""
    import torch
    c = TRAIN
    nn0 = ag.NeuralNet(env, tower_height=TOWER, seed=1)
    eng = ag.Engine(board_size=N, tower_height=TOWER, games=c["slots"], num_readouts=R, seed=c["seed"],
                    record_capacity_games=c["slots"] + 8)
    nn0.engine.copy_weights_to(eng)
    eng.replay_set_surprise(rho)
    dev = torch.device("cuda", eng.cfg.device)
    feats = torch.empty((c["B"], 17 * eng.P), dtype=torch.float32, device=dev)
    pi = torch.empty((c["B"], eng.A), dtype=torch.float32, device=dev)
    z = torch.empty(c["B"], dtype=torch.float32, device=dev)
    eng.set_hold(True)
    eng.start(c["num_games"])
    eng.release()
    i, losses = 0, []
    for _ in range(200000):
        if i >= c["num_games"]:
            break
        eng.step(1)
        n = eng.records_count()
        if n == 0:
            continue
        for _, k in sorted((eng.record_header(k)["game_id"], k) for k in range(n)):
            assert eng.replay_ingest_records(k, 1) == 1
            if rho > 0:
                eng.replay_score(eng.replay_count() - 1, 1)
            eng.replay_set_window(c["memory"])
            i += 1
            if eng.replay_live_positions() >= c["start_after"]:
                eng.replay_sample(c["B"], i, -1, feats, pi, z)
                losses.append(float(eng.train_step_device(feats, pi, z, c["B"], eta=0.02, rho=0.9)[0]))
        eng.records_clear()
        eng.release()
    assert i == c["num_games"]
    w = _weights(eng)
    eng.close()
    return w, losses


def test_train_takes_the_surprise():
    """train(..., surprise=0.5, slots=4) leaves the losses and, byte for byte, the weights of the same schedule run by
    hand -- and those differ from the same run with it off, which is train() without the keyword"""
    c = TRAIN
    env = ag.GoEnv(N)
    w_on, l_on = by_hand(env, 0.5)
    w_off, l_off = by_hand(env, 0.0)
    assert len(l_on) >= 3 and len(l_off) >= 3
    kw = dict(num_games=c["num_games"], memory_size=c["memory"], batch_size=c["B"], readouts=R,
              start_training_after=c["start_after"], slots=c["slots"], seed=c["seed"], callback=None, return_log=True)
    nn, log = ag.train(env, model=ag.NeuralNet(env, tower_height=TOWER, seed=1), surprise=0.5, **kw)
    got = [x["loss"] for x in log if x["loss"] is not None]
    assert bits_equal(np.array(got, np.float64), np.array(l_on, np.float64)), (got, l_on)
    assert not weight_mismatches(nn.engine, w_on)
    assert weight_mismatches(nn.engine, w_off), "the weighted draw changed no weight"
    nn_off, log_off = ag.train(env, model=ag.NeuralNet(env, tower_height=TOWER, seed=1), **kw)
    assert bits_equal(np.array([x["loss"] for x in log_off if x["loss"] is not None], np.float64), np.array(l_off, np.float64))
    assert not weight_mismatches(nn_off.engine, w_off)


def test_refusals(base):
    b = base
    ext = ag.Engine(board_size=N, tower_height=TOWER, games=SLOTS, num_readouts=R, seed=SEED, external_network=1)
    assert ext.replay_ingest(b["packed"]) == GAMES
    with pytest.raises(ag.AgzError) as ei:
        ext.replay_score()
    assert ei.value.status == BAD_ARGUMENT and "external_network" in str(ei.value)
    ext.close()
    e = engine()
    assert e.replay_ingest(b["packed"]) == GAMES
    for first, count in ((-1, 1), (0, GAMES + 1), (GAMES, 1), (3, GAMES - 2), (0, -1)):
        with pytest.raises(ag.AgzError) as ei:
            e.replay_score(first, count)
        assert ei.value.status == BAD_ARGUMENT, (first, count)
    assert not any(s for _, _, s in surprise_all(e))
    assert e.replay_score(GAMES, 0) == 0                          # an empty range at the end is a range
    e.replay_score()
    e.replay_set_surprise(0.5)
    for bad in (float("nan"), -0.1, 1.5):
        with pytest.raises(ag.AgzError) as ei:
            e.replay_set_surprise(bad)
        assert ei.value.status == BAD_ARGUMENT and "0..1" in str(ei.value)
    for k in range(GAMES):                                        # the setting in force is kept
        assert (e.replay_surprise(k)[1] == b["want"][0.5][k][1]).all()
    with pytest.raises(ag.AgzError):
        e.replay_surprise(GAMES)
    with pytest.raises(ag.AgzError):
        sampled(e, 2049, 1)
    e.reanalyze_start(0, 2, 0)                                    # an open reanalysis run
    with pytest.raises(ag.AgzError) as ei:
        e.replay_score()
    assert ei.value.status == BAD_ARGUMENT and "reanalysis" in str(ei.value)
    assert all(s for _, _, s in surprise_all(e))
    e.close()

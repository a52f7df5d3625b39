"""What the GPU tests of the search options share (test_gpu_starts.py, test_gpu_playout_cap.py,
test_gpu_forced_playouts.py, test_gpu_gumbel.py, test_gpu_symmetry.py, test_gpu_puct.py, test_gpu_explore.py,
test_gpu_uncertainty.py, test_gpu_superko.py; test_gpu_train_batched.py takes the arena helpers): engines with a peaked policy, setting the options of an engine or a
simulator from one dict, playing a run to its records, a record against another record or against the twin's game
(tests/selfplay_twin.py), and train() against the same schedule composed of single calls, whose games are the twin's on
the weights in force round by round.  Test infrastructure only."""
import ctypes as C

import numpy as np

import alphago_jl_amd as ag
import explore_twin as ex
import hs
import orc
import selfplay_twin as tw
import superko_twin as sk
from alphago_jl_amd import symmetry as sy
from gpu_common import GpuNetForOracle, pos_soa
from test_gpu_analysis import api_positions        # noqa: F401  (the API positions and games that the option files
from test_gpu_review import api_game               # noqa: F401   give analyze and review)
from test_hostsim_selfplay import bits_equal
from test_train_loop_batched import sample_entries, window_pairs


def sharpen(engine, N):
    """scale the policy FC of the selected network by the smallest power of two k that makes pi max > 0.5 on random
    positions (the synthetic FC bias is zero, so the logits scale by k): with the flat glorot policy a wrong remap
    would hide in the noise"""
    w = engine.get_weights(orc.L_POLICY_FC, 0)
    pi0, _ = engine.forward_features(rand_feats(N, 8, seed=123))
    logp = np.log(pi0.astype(np.float64))
    for k in (2.0 ** i for i in range(1, 10)):
        z = k * logp - (k * logp).max(axis=1, keepdims=True)
        if (np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)).max(axis=1).min() > 0.5:
            break
    engine.set_weights(orc.L_POLICY_FC, 0, (w * k).astype(np.float32))


def peaked_engine(N, tower, **kw):
    e = ag.Engine(board_size=N, tower_height=tower, **kw)
    e.init_synthetic(0)
    sharpen(e, N)
    return e


def rand_feats(N, B, seed=0):
    x = (np.random.RandomState(seed).rand(B, 17 * N * N) < 0.3).astype(np.float32)
    x[:, 16 * N * N:] = 1.0
    return x


class SymNetForOracle:
    """an or_net_fn for ONE game (or one arena player): evaluation e of the game is made under T_s with s predicted by
    the mirror of the draw key (or fixed): features of the oracle's positions, host transform, the plain GPU forward,
    host un-permute"""

    def __init__(self, engine, seed, game_id, mode, plain_first=0):
        self.engine, self.seed, self.game_id, self.mode = engine, seed, game_id, mode
        self.plain_first = plain_first      # evaluations made before the mode was switched on: T_0
        self.e = 0
        self.syms = []
        N = engine.N

        def _fn(ctx, positions, B, pi, v):
            plist = [positions[b].contents for b in range(B)]
            feats = engine.features(*pos_soa(plist))
            sym = []
            for _ in range(B):
                if self.e < self.plain_first:
                    sym.append(0)
                else:
                    sym.append(self.mode if self.mode != sy.RANDOM else sy.draw_symmetry(self.seed, self.game_id, self.e))
                self.e += 1
            self.syms += sym
            tx = np.stack([sy.apply_features(feats[b], sym[b], N) for b in range(B)])
            gpi, gv = engine.forward_features(tx)
            gpi = np.ascontiguousarray(np.stack([sy.apply_policy(gpi[b], sy.inverse(sym[b]), N) for b in range(B)]),
                                       np.float32)
            C.memmove(pi, gpi.ctypes.data, 4 * B * engine.A)
            C.memmove(v, np.ascontiguousarray(gv, np.float32).ctypes.data, 4 * B)

        self.cb = orc.NET_FN(_fn)


def apply(eng, st):
    """the three exploration setters of an engine from a setting of explore_twin; an off part is set off"""
    sched = lambda t: None if t is None else ex.schedule_of(t, eng.N)
    eng.set_root_policy_temperature(sched(st["pt"]))
    eng.set_root_noise(*st["noise"])
    eng.set_move_temperature(sched(st["mt"]))


def configure(x, opt):
    """the options of ag.Engine or hs.Sim x from opt: starts (oracle positions), cap (fast readouts, full probability),
    forced (k, prune), gumbel (m), symmetry (random), explore (a setting of explore_twin), puct ((r, r_root), c_base),
    lcb (z, min_visits, min_ratio) and pv (k, prior, weight) with moments (left out or None: "a rule is asked for"),
    ko_rule (0 simple, 1 positional, 2 situational).  A key left out -- or, of the last five, None -- is a setter not
    called; a simulator's setter that returns a status is held to OK."""
    sim = isinstance(x, hs.Sim)

    def ok(status):                  # (an engine's setter raises instead)
        assert not sim or status == ag._lib.OK, status
    if opt.get("starts"):
        if sim:
            x.set_starts(opt["starts"])
        else:
            b, i, h = tw.opos_arrays(opt["starts"])
            x.set_starts(boards=b, info=i, history=h)
    if "cap" in opt:
        x.set_playout_cap(*opt["cap"])
    if "forced" in opt:
        x.set_forced_playouts(*opt["forced"])
    if "gumbel" in opt:
        x.set_gumbel(opt["gumbel"], 50.0, 1.0)
    if "symmetry" in opt:
        x.set_symmetry(8 if sim else "random")
    if opt.get("explore") is not None:
        x.apply(opt["explore"]) if sim else apply(x, opt["explore"])
    if opt.get("puct") is not None:
        fpu, c_base = opt["puct"]
        x.set_puct(1, *fpu, c_base) if sim else x.set_puct(fpu, c_base)
    lcb, pv = opt.get("lcb"), opt.get("pv")
    if (lcb is not None or pv is not None) if opt.get("moments") is None else opt["moments"]:
        ok(x.set_value_moments(True))
    if lcb is not None:
        ok(x.set_lcb(*lcb) if sim else x.set_lcb(lcb))
    if pv is not None:
        ok(x.set_puct_variance(*pv) if sim else x.set_puct_variance(pv))
    if opt.get("ko_rule") is not None:
        ok(x.set_ko_rule(opt["ko_rule"] if sim else sk.RULE_NAMES[opt["ko_rule"]]))


def play(eng, games, network=None, white=None, chunk=8, sort=True):
    """a run of `games` games to its records (sort: by game id, else in the ring's order) and stats; network / white:
    the callbacks of an external_network engine (white: an arena's second network)"""
    eng.start(games)
    for _ in range(400000):
        if network is None:
            eng.step(chunk)
        elif white is None:
            eng.step_external(network)
        else:
            eng.step_external(network, white)
        if eng.records_count() >= games:
            break
    recs, st = eng.records(), eng.stats()
    assert len(recs) == games and st["pool_exhausted"] == 0 and st["pool_short_searches"] == 0
    return (sorted(recs, key=lambda r: r["game_id"]) if sort else recs), st


RECORD = ("game_id", "num_moves", "moves", "result", "was_resign", "pis", "qs")


def same_game(r, o, fields=RECORD):
    """records r and o agree in `fields`: floats and float rows bit for bit"""
    def same(k):
        if k in ("pis", "qs"):
            return bits_equal(r[k], o[k])
        if k == "final_score":
            return np.float32(r[k]) == np.float32(o[k])
        return (r[k] == o[k]).all() if k == "moves" else r[k] == o[k]
    return all(same(k) for k in fields)


def assert_game_equals_twin(r, o, what, full=None):
    """record r is the twin's game o, bit for bit.  full (the twin's mask of fully searched plies, under the playout
    cap): the pi row of a fast ply is all-zero bits, the full rows are the twin's and none of them is all zero"""
    extra = {k: o[k] for k in ("forced_sel", "begun", "halved", "off_max", "dups", "cuts") if k in o}
    print(f"game {what}: start {r.get('start')}, {r['num_moves']} moves{'' if full is None else f' ({int(full.sum())} full)'}, "
          f"result {r['result']}, resign {r['was_resign']}, score {r['final_score']}; twin {o['num_moves']} / {o['result']} / "
          f"{o['was_resign']} / {o['final_score']}, evals {o['evals']} {extra}")
    assert r["num_moves"] == o["num_moves"], what
    assert (r["moves"] == o["moves"]).all(), what
    assert r["result"] == o["result"] and r["was_resign"] == o["was_resign"], what
    assert r["resign_disabled"] == o["resign_disabled"], what
    assert np.float32(r["final_score"]) == np.float32(o["final_score"]), what
    assert bits_equal(r["qs"], o["qs"]), what
    if full is None:
        assert bits_equal(r["pis"], o["pis"]), what
    elif r["num_moves"]:
        got = np.ascontiguousarray(r["pis"], np.float32)
        assert (got[~full].view(np.uint32) == 0).all(), (what, "a fast row is not all zero")
        assert bits_equal(got[full], o["pis"][full]), what
        assert (got[full] != 0).any(axis=1).all(), what
    assert r["short_searches"] == 0, what


def weight_mismatches(engine, want):
    """the (layer, kind) arrays of `engine` that are not bit for bit `want`, with the largest difference of each"""
    out = []
    for lk, v in want.items():
        got = engine.get_weights(*lk)
        if not bits_equal(got, v):
            out.append((lk, int((got != v).sum()), float(np.abs(got.astype(np.float64) - v).max())))
    return out


def _weights(eng):
    return {lk: eng.get_weights(*lk) for lk in eng.layers()}


def _lengths(e):
    return [e.replay_record(k)["num_moves"] for k in range(e.replay_count())]


def _twin_pairs(e, call, B):
    """what agz_replay_sample must draw: the twin's entries mapped through the arena's current window"""
    lengths = _lengths(e)
    live = e.replay_live_positions()
    first = sum(lengths) - live
    cum = np.concatenate([[0], np.cumsum(lengths)])
    fg = int(np.searchsorted(cum, first, side="right") - 1)
    return window_pairs(lengths, fg, first - int(cum[fg]), sample_entries(e.cfg.seed, call, live, B))


def arena_pis(e):
    return [e.replay_record(k)["pis"][: e.replay_record(k)["num_moves"]] for k in range(e.replay_count())]


def count_targets(pis):
    return int(sum((np.asarray(x) != 0).any(axis=1).sum() for x in pis if len(x)))


def host_schedule(nn0, cfg, configure, targets_only):
    """train()'s schedule composed of single calls (the method of tests/test_gpu_train_batched.py) on an engine that
    configure(eng) set the options of, with the weights after every training kept; targets_only: the arena train()
    keeps under the playout cap.  cfg: N, TOWER, R, SEED, num_games, slots, memory, B, start_after
    -> (per game: record, loss, step, live entries; the snapshots; the step each game was claimed in; the option
    counters of the run)"""
    c = cfg
    num_games, slots = c["num_games"], c["slots"]
    eng = ag.Engine(board_size=c["N"], tower_height=c["TOWER"], games=slots, num_readouts=c["R"], seed=c["SEED"],
                    record_capacity_games=slots + 8)
    nn0.engine.copy_weights_to(eng)
    configure(eng)
    if targets_only:
        eng.replay_set_targets_only(True)
    eng.set_hold(True)
    eng.start(num_games)
    eng.release()
    snaps = [_weights(eng)]
    i, claimed, pending, ref, steps, start_step, targets = 0, 0, min(slots, num_games), [], 0, {}, 0
    while i < num_games:
        for k in range(claimed, claimed + pending):
            start_step[k] = steps + 1
        claimed += pending
        eng.step(1)
        steps += 1
        n = eng.records_count()
        for r in sorted(eng.records(), key=lambda r: r["game_id"]):
            assert eng.replay_ingest_records(r["index"], 1) == 1
            eng.replay_set_window(c["memory"])
            i += 1
            live = eng.replay_live_positions()
            if targets_only:
                targets += count_targets([r["pis"][: r["num_moves"]]])
                assert live == min(c["memory"], targets)
            loss = None
            if live >= c["start_after"]:
                if targets_only:
                    pairs, _ = tw.sample_targets(c["SEED"], i, c["B"], arena_pis(eng), window=live)
                    g, p = np.array([a for a, _ in pairs], np.int64), np.array([b for _, b in pairs], np.int32)
                else:
                    g, p = _twin_pairs(eng, i, c["B"])
                f, pi, z = eng.replay_batch(g, p)
                assert not targets_only or (pi != 0).any(axis=1).all()
                loss = float(eng.train_step(f, pi, z, eta=np.float32(0.02), rho=0.9)[0])
                snaps.append(_weights(eng))
            ref.append(dict(i=i, record=r, loss=loss, step=steps, live=live))
        eng.records_clear()
        eng.release()
        pending = min(n, num_games - claimed)
    counts = dict(cap=eng.playout_cap_counts(), forced=eng.forced_counts(), gumbel=eng.gumbel_counts())
    eng.close()
    return ref, snaps, start_step, counts


def assert_train_equals_twin(env, nn0, cfg, schedule, twin_of, masked, **train_kw):
    """schedule = host_schedule(...)[:3].  Every game of it is the twin's game twin_of(cb, gid, on_round) on the weights
    in force round by round: with several slots games overlap training, so round r of a game (engine step start_step +
    r) runs on the weights left by the trainings of the steps before it.  And ag.train(..., **train_kw) is that
    schedule: records, losses, live entries (targets-only arenas) and final weights.  -> (the twins, train()'s log)"""
    c = cfg
    ref, snaps, start_step = schedule
    assert sum(g["loss"] is not None for g in ref) >= 4
    chk = ag.Engine(board_size=c["N"], tower_height=c["TOWER"], games=1, num_readouts=8, max_nodes_per_game=16)
    cb = GpuNetForOracle(chk).cb
    loaded = [None]
    switched = 0
    twins = []
    for gme in ref:
        gid = int(gme["record"]["game_id"])
        rnd = [0]

        def on_round():
            step = start_step[gid] + rnd[0]
            rnd[0] += 1
            t = sum(1 for h in ref if h["step"] < step and h["loss"] is not None)
            if loaded[0] != t:
                for (layer, kind), w in snaps[t].items():
                    chk.set_weights(layer, kind, w)
                loaded[0] = t

        o = twin_of(cb, gid, on_round)
        assert_game_equals_twin(gme["record"], o, gid, o["full"] if masked else None)
        twins.append(o)
        first = sum(1 for h in ref if h["step"] < start_step[gid] and h["loss"] is not None)
        switched += loaded[0] != first
    assert switched > 0, "some game was in flight across a training step"

    nn, log = ag.train(env, num_games=c["num_games"], memory_size=c["memory"], batch_size=c["B"], readouts=c["R"],
                       model=nn0, start_training_after=c["start_after"], slots=c["slots"], seed=c["SEED"], callback=None,
                       return_log=True, epochs=1, **train_kw)
    assert len(log) == len(ref) == c["num_games"]
    for x, y in zip(log, ref):
        a, b = x["record"], y["record"]
        assert a["game_id"] == b["game_id"] and a["num_moves"] == b["num_moves"] and a["result"] == b["result"]
        assert (a["moves"] == b["moves"]).all() and bits_equal(a["pis"], b["pis"]) and bits_equal(a["qs"], b["qs"])
        assert x["loss"] == y["loss"]
        assert not masked or x["live"] == y["live"]
    bad = weight_mismatches(nn.engine, snaps[-1])
    assert not bad, bad
    chk.close()
    return twins, log

"""What the rate tools of the search options share (playout_cap_rate.py, forced_playouts_rate.py, gumbel_rate.py,
starts_rate.py): one engine at the BASELINE.json configs[1] shape, and the modes of an option timed in alternating
windows of the same process on the same box.  An option changes between runs only, so every window is a run of its
own: the slots of the previous window are given up (agz_slot_abandon), the mode is set on a run without a step yet,
the run is started, stepped through its prelude and a warm-up, and then K steps are timed, ending in a synchronise."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--tower", type=int, default=10)
    ap.add_argument("--readouts", type=int, default=400)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--stagger", type=int, default=60, help="the bench stagger (games at mixed stages, as in bench.py)")
    ap.add_argument("--steps", type=int, default=100, help="timed steps per window")
    ap.add_argument("--pairs", type=int, default=3, help="rounds of the windows (the order reverses every round)")
    ap.add_argument("--warmup", type=int, default=10)
    return ap


def engine(args, **cfg):
    import alphago_jl_amd as ag
    eng = ag.Engine(board_size=args.board, tower_height=args.tower, games=args.games, num_readouts=args.readouts,
                    parallel_readouts=8, seed=1, record_capacity_games=2 * args.games + 64, **cfg)
    eng.init_synthetic(0)
    return eng


def set_stagger(eng, moves):
    eng._ck(eng.L.agz_debug_set_stagger(eng.h, moves))


def first_search_steps(args):
    """steps until every game of a fresh run is behind its first search"""
    return (args.readouts + 7) // 8 + 5


def windows_of(eng, args, modes, configure, collect, prelude, counts=None, profile=True):
    """configure(eng, mode) sets the stagger and the mode; counts(eng) reads the option's counter pair;
    collect(s0, s1, c0, c1, dt) gives the option's own columns of a window (stats and counts before and behind it)
    -> {mode: [columns of each of its windows]}"""
    out = {m: [] for m in modes}
    live = False
    for k in range(args.pairs):
        for mode in (modes if k % 2 == 0 else modes[::-1]):
            if live:
                for g in range(args.games):
                    eng.slot_abandon(g)
            eng.records_clear()
            eng.start(0)                      # a run without a step yet: stagger and setting may change here
            configure(eng, mode)
            eng.start(0)
            live = True
            eng.step(prelude + args.warmup)
            eng.sync()
            s0, c0 = eng.stats(), counts(eng) if counts else None
            if profile:
                eng.profile_search(True)
            t0 = time.perf_counter()
            eng.step(args.steps)
            eng.sync()
            dt = time.perf_counter() - t0
            w = dict(ms_per_step=round(1e3 * dt / args.steps, 4))
            if profile:                       # the five search kernels' time per step (bench.py's `search_kernels`)
                search_ms, search_steps = eng.profile_search_read()
                eng.profile_search(False)
                w["search_kernels_ms_per_step"] = round(float(sum(search_ms.values())) / max(search_steps, 1), 4)
                w["k_pre_us_per_step"] = round(1e3 * float(search_ms.get("k_pre", 0.0)) / max(search_steps, 1), 2)
            s1, c1 = eng.stats(), counts(eng) if counts else None
            moves = s1["positions"] - s0["positions"]
            w.update(moves=moves, moves_per_s=round(moves / dt, 1),
                     evals_per_move=round((s1["evals"] - s0["evals"]) / max(moves, 1), 2),
                     pool_short_searches=s1["pool_short_searches"] - s0["pool_short_searches"])
            w.update(collect(s0, s1, c0, c1, dt))
            out[mode].append(w)
    return out


def summary(windows, keys):
    """median and spread (max - min) over a mode's windows of every column in `keys`"""
    res = {}
    for mode, ws in windows.items():
        res[mode] = {}
        for key in keys:
            v = [w[key] for w in ws]
            res[mode][key] = dict(median=round(statistics.median(v), 4), spread=round(max(v) - min(v), 4))
    return res


def on_minus_off(res, key):
    return round(res["on"][key]["median"] - res["off"][key]["median"], 4)


def measured(res):
    """on against off, beside the off windows' own spread"""
    return dict(ms_per_step_on_minus_off=on_minus_off(res, "ms_per_step"),
                search_kernels_on_minus_off=on_minus_off(res, "search_kernels_ms_per_step"),
                off_spread_ms_per_step=res["off"]["ms_per_step"]["spread"],
                off_spread_search_kernels=res["off"]["search_kernels_ms_per_step"]["spread"])

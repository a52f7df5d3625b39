#!/usr/bin/env python3
"""Cost and effect of the Gumbel root search at the BASELINE.json configs[1] shape, off against on in
alternating windows of the same process on the same box (the method of tools/forced_playouts_rate.py).

  search  per window: the previous window's games are given up, the setting is made (it changes between runs only), a
          run is started with the bench stagger, stepped through its prelude and a warm-up, and then K steps are timed,
          ending in a synchronise.  Reported per mode: ms per step, the five search kernels' time per step (bench.py's
          `search_kernels`), moves/s, evaluations per move, the mean leaves per select phase (evaluations over games
          times steps: the phase cuts of Sequential Halving are the expected cost) and, with the setting on, the halvings
          per search (agz_selfplay_gumbel_counts), with the spread over the repeated windows.
  rows    what the records do not show: a small engine with the setting on, stepped one step at a time; before every
          step each slot's root rows are read (agz_tree_node_floats, agz_tree_gumbel_pi), and after it a slot whose
          root moved on gives one sample -- the move played against the most visited child of the rows read, and the
          entropy of the Gumbel target row against that of children_as_pi on the same visits.

Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows_of(eng, args, R):
    modes = ("off", "on")
    out = {m: [] for m in modes}
    live = False
    for k in range(args.pairs):
        for mode in (modes if k % 2 == 0 else modes[::-1]):
            if live:
                for g in range(args.games):
                    eng.slot_abandon(g)
            eng.records_clear()
            eng.start(0)                      # a run without a step yet: stagger and setting may change here
            eng._ck(eng.L.agz_debug_set_stagger(eng.h, args.stagger))
            eng.set_gumbel(args.m if mode == "on" else 0, args.c_visit, args.c_scale)
            eng.start(0)
            live = True
            eng.step(((R + 7) // 8 + 5 if args.stagger > 0 else 0) + args.warmup)
            eng.sync()
            s0, c0 = eng.stats(), eng.gumbel_counts()
            eng.profile_search(True)
            t0 = time.perf_counter()
            eng.step(args.steps)
            eng.sync()
            dt = time.perf_counter() - t0
            search_ms, search_steps = eng.profile_search_read()
            eng.profile_search(False)
            s1, c1 = eng.stats(), eng.gumbel_counts()
            moves = s1["positions"] - s0["positions"]
            evals = s1["evals"] - s0["evals"]
            begun, halved = c1[0] - c0[0], c1[1] - c0[1]
            out[mode].append(dict(
                ms_per_step=round(1e3 * dt / args.steps, 4), moves_per_s=round(moves / dt, 1),
                evals_per_move=round(evals / max(moves, 1), 2), moves=moves,
                leaves_per_select_phase=round(evals / (args.games * args.steps), 3),
                searches_begun=begun, halvings=halved, halvings_per_search=round(halved / max(begun, 1), 3),
                search_kernels_ms_per_step=round(float(sum(search_ms.values())) / max(search_steps, 1), 4),
                pool_short_searches=s1["pool_short_searches"] - s0["pool_short_searches"]))
    return out


def summary(windows):
    res = {}
    for mode, ws in windows.items():
        res[mode] = {}
        for key in ("ms_per_step", "moves_per_s", "evals_per_move", "leaves_per_select_phase",
                    "search_kernels_ms_per_step", "halvings_per_search"):
            v = [w[key] for w in ws]
            res[mode][key] = dict(median=round(statistics.median(v), 4), spread=round(max(v) - min(v), 4))
    return res


def entropy(row):
    p = np.asarray(row, np.float64)
    p = p[p > 0]
    return float(-(p * np.log(p)).sum())


def rows_part(args):
    import alphago_jl_amd as ag
    N, R, S = args.board, args.readouts, args.rows_slots
    eng = ag.Engine(board_size=N, tower_height=args.tower, games=S, num_readouts=R, parallel_readouts=8, seed=1,
                    record_capacity_games=4 * S + 64, resign_threshold=-2.0, resign_disable_fraction=0.0)
    eng.init_synthetic(0)
    eng.set_gumbel(args.m, args.c_visit, args.c_scale)
    eng.start(0)
    eng.step(2)
    off_max, h_gumbel, h_visits, samples = 0, [], [], 0
    for _ in range(args.rows_steps):
        before = []
        for g in range(S):
            root = eng.tree_root(g)
            info = eng.node_info(g, root)
            before.append((root, info.pos.n, info.N, eng.node_floats(g, root, 0), eng.tree_gumbel_pi(g, root, args.c_visit,
                                                                                                   args.c_scale)))
        eng.step(1)
        for g in range(S):
            root0, n0, rootN0, cn, row = before[g]
            root = eng.tree_root(g)
            info = eng.node_info(g, root)
            if info.pos.n != n0 + 1 or not cn.sum() > 0:      # no move, or a new game in the slot
                continue
            a = int(info.pos.last_move)
            samples += 1
            off_max += a != int(np.argmax(cn))
            h_gumbel.append(entropy(row))
            h_visits.append(entropy(cn.astype(np.float64) / float(cn.sum())))
        if samples >= args.rows_samples:
            break
    out = dict(slots=S, samples=samples, moves_off_the_most_visited_child=int(off_max),
               share_off_the_most_visited_child=round(off_max / max(samples, 1), 4),
               mean_entropy_gumbel_row=round(float(np.mean(h_gumbel)), 4) if samples else None,
               mean_entropy_children_as_pi=round(float(np.mean(h_visits)), 4) if samples else None,
               uniform_entropy=round(float(np.log(N * N + 1)), 4))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--tower", type=int, default=10)
    ap.add_argument("--readouts", type=int, default=400)
    ap.add_argument("--m", type=int, default=16, help="root candidates of the Gumbel search")
    ap.add_argument("--c-visit", type=float, default=50.0)
    ap.add_argument("--c-scale", type=float, default=1.0)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--stagger", type=int, default=60)
    ap.add_argument("--steps", type=int, default=100, help="timed steps per window")
    ap.add_argument("--pairs", type=int, default=3, help="rounds of the windows (the order reverses every round)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows-slots", type=int, default=8, help="slots of the engine of the rows part")
    ap.add_argument("--rows-steps", type=int, default=400, help="most steps of the rows part")
    ap.add_argument("--rows-samples", type=int, default=100, help="moves the rows part stops at")
    args = ap.parse_args()

    import alphago_jl_amd as ag

    N, R = args.board, args.readouts
    eng = ag.Engine(board_size=N, tower_height=args.tower, games=args.games, num_readouts=R, parallel_readouts=8, seed=1,
                    record_capacity_games=2 * args.games + 64)
    eng.init_synthetic(0)
    windows = windows_of(eng, args, R)
    eng.close()
    res = summary(windows)
    print(json.dumps(dict(
        shape=dict(board=N, tower=args.tower, readouts=R, m=args.m, c_visit=args.c_visit, c_scale=args.c_scale,
                   games=args.games, stagger=args.stagger),
        steps_per_window=args.steps, windows=windows, summary=res,
        measured=dict(
            ms_per_step_on_minus_off=round(res["on"]["ms_per_step"]["median"] - res["off"]["ms_per_step"]["median"], 4),
            search_kernels_on_minus_off=round(res["on"]["search_kernels_ms_per_step"]["median"]
                                              - res["off"]["search_kernels_ms_per_step"]["median"], 4),
            off_spread_ms_per_step=res["off"]["ms_per_step"]["spread"],
            off_spread_search_kernels=res["off"]["search_kernels_ms_per_step"]["spread"],
            evals_per_move=dict(off=res["off"]["evals_per_move"]["median"], on=res["on"]["evals_per_move"]["median"]),
            leaves_per_select_phase=dict(off=res["off"]["leaves_per_select_phase"]["median"],
                                         on=res["on"]["leaves_per_select_phase"]["median"]),
            halvings_per_search=res["on"]["halvings_per_search"]["median"]),
        rows=rows_part(args))))


if __name__ == "__main__":
    main()

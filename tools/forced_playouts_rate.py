#!/usr/bin/env python3
"""Cost and effect of forced playouts and policy target pruning at the BASELINE.json configs[1] shape,
off against on in alternating windows of the same process on the same box (the method of tools/playout_cap_rate.py).

  search  per window: the previous window's games are given up, the setting is made (it changes between runs only), a
          run is started with the bench stagger, stepped through its prelude and a warm-up, and then K steps are timed,
          ending in a synchronise.  Reported per mode: ms per step, the five search kernels' time per step (bench.py's
          `search_kernels`), moves/s, and with the setting on the forced selections per full search and the share of the
          recorded target rows that pruning changed (agz_selfplay_forced_counts over agz_stats.positions), with the
          spread over the repeated windows.
  mass    what pruning moves, which the records do not show (they hold the pruned row only): one host-driven game on a
          single tree with the setting on -- noise, R readouts, then agz_tree_pruned_pi under k against the same call
          under k = 0 (children_as_pi of the raw visits), the move with the most visits played -- gives per searched
          position the mass moved, half the L1 distance of the two rows.

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
            eng.set_forced_playouts(args.k if mode == "on" else 0.0, True)
            eng.start(0)
            live = True
            eng.step(((R + 7) // 8 + 5 if args.stagger > 0 else 0) + args.warmup)
            eng.sync()
            s0, c0 = eng.stats(), eng.forced_counts()
            eng.profile_search(True)
            t0 = time.perf_counter()
            eng.step(args.steps)
            eng.sync()
            dt = time.perf_counter() - t0
            search_ms, search_steps = eng.profile_search_read()
            eng.profile_search(False)
            s1, c1 = eng.stats(), eng.forced_counts()
            moves = s1["positions"] - s0["positions"]
            evals = s1["evals"] - s0["evals"]
            forced, rows = c1[0] - c0[0], c1[1] - c0[1]
            out[mode].append(dict(
                ms_per_step=round(1e3 * dt / args.steps, 4), moves_per_s=round(moves / dt, 1),
                evals_per_move=round(evals / max(moves, 1), 2), moves=moves, forced_selections=forced, rows_changed=rows,
                # every search is full here (no cap); the stagger's shortened first moves are not in `positions`, so
                # both ratios are slightly high while such games are still about
                forced_per_full_search=round(forced / max(moves, 1), 3), rows_changed_share=round(rows / max(moves, 1), 4),
                search_kernels_ms_per_step=round(float(sum(search_ms.values())) / max(search_steps, 1), 4),
                pool_short_searches=s1["pool_short_searches"] - s0["pool_short_searches"]))
    return out


def summary(windows):
    res = {}
    for mode, ws in windows.items():
        res[mode] = {}
        for key in ("ms_per_step", "moves_per_s", "evals_per_move", "search_kernels_ms_per_step", "forced_per_full_search",
                    "rows_changed_share"):
            v = [w[key] for w in ws]
            res[mode][key] = dict(median=round(statistics.median(v), 4), spread=round(max(v) - min(v), 4))
    return res


def mass_part(args):
    import alphago_jl_amd as ag
    N, R = args.board, args.readouts
    eng = ag.Engine(board_size=N, tower_height=args.tower, games=1, num_readouts=R, parallel_readouts=8, seed=1)
    eng.init_synthetic(0)
    eng.set_forced_playouts(args.k, True)
    eng.tree_init(0, np.zeros(N * N, np.int8))
    eng.set_draw(0, 0, 0)
    moved, changed, forced0 = [], 0, eng.forced_counts()[0]
    for ply in range(args.mass_plies):
        root = eng.tree_root(0)
        if eng.is_done(0, root):
            break
        if not eng.node_info(0, root).is_expanded:
            eng.tree_search(0, 8)
        eng.inject_noise(0, root)
        target = eng.node_info(0, root).N + R
        while eng.node_info(0, root).N < target:
            eng.tree_search(0, 8)
        raw, pruned = eng.tree_pruned_pi(0, root, 0.0), eng.tree_pruned_pi(0, root, args.k)
        m = 0.5 * float(np.abs(pruned.astype(np.float64) - raw.astype(np.float64)).sum())
        moved.append(m)
        changed += m > 0
        if not eng.play_move(0, int(np.argmax(eng.node_floats(0, root, 0)))):
            break
    out = dict(positions=len(moved), rows_changed=int(changed), forced_per_search=round((eng.forced_counts()[0] - forced0)
                                                                                       / max(len(moved), 1), 3),
               mean_mass_moved_per_row=round(float(np.mean(moved)), 5) if moved else None,
               mean_mass_moved_per_changed_row=round(float(np.sum(moved)) / max(changed, 1), 5),
               max_mass_moved=round(float(np.max(moved)), 5) if moved else None)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--tower", type=int, default=10)
    ap.add_argument("--readouts", type=int, default=400)
    ap.add_argument("--k", type=float, default=2.0, help="forced playouts coefficient (KataGo: 2)")
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--stagger", type=int, default=60)
    ap.add_argument("--steps", type=int, default=100, help="timed steps per window")
    ap.add_argument("--pairs", type=int, default=3, help="rounds of the windows (the order reverses every round)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mass-plies", type=int, default=40, help="positions of the single-tree game of the mass part")
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
        shape=dict(board=N, tower=args.tower, readouts=R, k=args.k, prune=True, games=args.games, stagger=args.stagger),
        steps_per_window=args.steps, windows=windows, summary=res,
        measured=dict(
            ms_per_step_on_minus_off=round(res["on"]["ms_per_step"]["median"] - res["off"]["ms_per_step"]["median"], 4),
            search_kernels_on_minus_off=round(res["on"]["search_kernels_ms_per_step"]["median"]
                                              - res["off"]["search_kernels_ms_per_step"]["median"], 4),
            off_spread_ms_per_step=res["off"]["ms_per_step"]["spread"],
            off_spread_search_kernels=res["off"]["search_kernels_ms_per_step"]["spread"],
            forced_per_full_search=res["on"]["forced_per_full_search"]["median"],
            rows_changed_share=res["on"]["rows_changed_share"]["median"]),
        mass=mass_part(args))))


if __name__ == "__main__":
    main()

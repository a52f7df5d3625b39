#!/usr/bin/env python3
"""Cost of random-symmetry leaf evaluation (DESIGN.md "Board symmetries") at the BASELINE.json configs[1] shape:
one engine, steady state as in bench.py (stagger prelude + warm-up), then alternating windows of K steps with the
symmetry off and AGZ_SYMMETRY_RANDOM on the same box, same process, same games.  With the mode on a step launches
k_leaf_features_sym instead of k_leaf_features and one k_pi_unpermute behind the network.  Prints one JSON object:
per-window milliseconds per step, the medians of both modes and their ratio."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--tower", type=int, default=10)
    ap.add_argument("--readouts", type=int, default=400)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--stagger", type=int, default=60)
    ap.add_argument("--steps", type=int, default=20, help="steps per window")
    ap.add_argument("--pairs", type=int, default=4, help="off / random window pairs (order alternates per pair)")
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()

    import alphago_jl_amd as ag

    N, R = args.board, args.readouts
    eng = ag.Engine(board_size=N, tower_height=args.tower, games=args.games, num_readouts=R, parallel_readouts=8, seed=1,
                    stagger_moves=args.stagger, record_capacity_games=2 * args.games + 64)
    eng.init_synthetic(0)
    eng.start(0)
    eng.step((R + 7) // 8 + 5 + args.warmup)
    eng.sync()
    windows = {"off": [], "random": []}
    for k in range(args.pairs):
        order = ("off", "random") if k % 2 == 0 else ("random", "off")
        for mode in order:
            eng.set_symmetry(None if mode == "off" else "random")
            eng.step(2)                       # the first launches under the new mode are not timed
            eng.sync()
            t0 = time.perf_counter()
            eng.step(args.steps)
            eng.sync()
            windows[mode].append(1e3 * (time.perf_counter() - t0) / args.steps)
    eng.records_clear()
    eng.close()
    off, on = statistics.median(windows["off"]), statistics.median(windows["random"])
    print(json.dumps(dict(shape=dict(board=N, tower=args.tower, readouts=R, games=args.games), steps_per_window=args.steps,
                          ms_per_step=windows, median_off_ms=round(off, 3), median_random_ms=round(on, 3),
                          cost=round(on / off - 1.0, 5))))


if __name__ == "__main__":
    main()

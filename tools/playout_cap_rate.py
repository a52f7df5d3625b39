#!/usr/bin/env python3
"""Rate of self-play under playout cap randomization at the BASELINE.json configs[1] shape, cap off
against cap on in alternating windows of the same process on the same box.

  search  per window: the previous window's games are given up, the cap is set (it changes between runs only), a run is
          started with the bench stagger (games at mixed stages and phases, as in bench.py), stepped through its
          prelude and a warm-up, and then K steps are timed, ending in a synchronise.  Reported per mode: ms per step,
          moves/s (agz_stats.positions: moves played on a spent budget), target positions/s (moves of full searches --
          all of them with the cap off), network evaluations per move, the full / fast counts, the five search kernels'
          time per step (bench.py's `search_kernels`) and the spread over the repeated windows.
  arena   over the finished games of a short cap-on run: agz_replay_ingest_records into a plain and into a targets-only
          arena (the difference is the scan kernel and its read-back) and agz_replay_sample from both, ms per call.

Prints one JSON object."""
import json
import statistics
import time

import rate_windows as rw


def arena_part(args):
    import alphago_jl_amd as ag
    import torch
    N, G, B = args.board, args.arena_games, args.arena_batch
    eng = ag.Engine(board_size=N, tower_height=1, games=G, num_readouts=16, seed=1, record_capacity_games=G + 8,
                    resign_threshold=-2.0)
    eng.init_synthetic(0)
    eng.set_playout_cap(4, args.prob)
    eng.start(G)
    while eng.records_count() < G:
        eng.step(32)
    out = {}
    # the first round is a warm-up (the arena's buffers are allocated in it) and is not reported
    for rnd, mode in enumerate(("plain", "targets_only") * (1 + args.arena_rounds)):
        eng.replay_clear()
        eng.replay_set_targets_only(mode == "targets_only")
        eng.sync()
        t0 = time.perf_counter()
        eng.replay_ingest_records(0, G)
        eng.sync()
        ingest = 1e3 * (time.perf_counter() - t0)
        bufs = eng.replay_sample(B, 1)
        eng.sync()
        ms = []
        for rep in range(args.arena_calls):
            t0 = time.perf_counter()
            eng.replay_sample(B, 2 + rep, -1, *bufs)
            eng.sync()
            ms.append(round(1e3 * (time.perf_counter() - t0), 4))
        if rnd < 2:
            del bufs
            continue
        d = out.setdefault(mode, dict(ingest_ms_per_call=[], sample_ms_per_call=[]))
        d["ingest_ms_per_call"].append(round(ingest, 4))
        d["sample_ms_per_call"] += ms
        d["entries"] = eng.replay_live_positions()
        d["positions"] = eng.replay_positions()
        del bufs
    for d in out.values():
        d["ingest_median_ms"] = round(statistics.median(d["ingest_ms_per_call"]), 4)
        d["sample_median_ms"] = round(statistics.median(d["sample_ms_per_call"]), 4)
        d["sample_spread_ms"] = round(max(d["sample_ms_per_call"]) - min(d["sample_ms_per_call"]), 4)
        d["ingest_spread_ms"] = round(max(d["ingest_ms_per_call"]) - min(d["ingest_ms_per_call"]), 4)
        d["sample_ms_per_call"] = d["sample_ms_per_call"][:8]
    out["scan_ms_per_ingest"] = round(out["targets_only"]["ingest_median_ms"] - out["plain"]["ingest_median_ms"], 4)
    eng.close()
    torch.cuda.empty_cache()
    return out


def main():
    ap = rw.parser()
    ap.add_argument("--fast", type=int, default=64, help="readouts of a fast search (r)")
    ap.add_argument("--prob", type=float, default=0.25, help="probability of a full search (p)")
    ap.add_argument("--arena-games", type=int, default=512)
    ap.add_argument("--arena-batch", type=int, default=2048)
    ap.add_argument("--arena-calls", type=int, default=20)
    ap.add_argument("--arena-rounds", type=int, default=3, help="timed ingest rounds per arena mode, behind one warm-up")
    args = ap.parse_args()
    N, R = args.board, args.readouts

    def configure(eng, mode):
        rw.set_stagger(eng, args.stagger)
        eng.set_playout_cap(args.fast if mode == "on" else 0, args.prob)

    def collect(s0, s1, c0, c1, dt):
        moves = s1["positions"] - s0["positions"]
        full, fast = c1[0] - c0[0], c1[1] - c0[1]
        # both modes from the same counter: agz_stats.positions leaves out the stagger's shortened first moves, which
        # the cap counts as full, so the on-mode targets are the counted moves that were not fast
        return dict(target_positions_per_s=round((moves - fast) / dt, 1), full=full, fast=fast,
                    evals_per_step=round((s1["evals"] - s0["evals"]) / args.steps, 1))

    eng = rw.engine(args)
    windows = rw.windows_of(eng, args, ("off", "on"), configure, collect,
                            rw.first_search_steps(args) if args.stagger > 0 else 0, lambda e: e.playout_cap_counts())
    eng.close()
    res = rw.summary(windows, ("ms_per_step", "moves_per_s", "target_positions_per_s", "evals_per_move",
                               "search_kernels_ms_per_step"))
    mean_readouts = args.prob * R + (1 - args.prob) * args.fast
    print(json.dumps(dict(
        shape=dict(board=N, tower=args.tower, readouts=R, fast_readouts=args.fast, full_prob=args.prob, games=args.games,
                   stagger=args.stagger),
        steps_per_window=args.steps, windows=windows, summary=res,
        predicted=dict(mean_readouts_per_move=mean_readouts, moves_per_s_ratio=round(R / mean_readouts, 3)),
        measured=dict(
            moves_per_s_ratio=round(res["on"]["moves_per_s"]["median"] / max(res["off"]["moves_per_s"]["median"], 1e-9), 3),
            target_positions_per_s_ratio=round(res["on"]["target_positions_per_s"]["median"]
                                               / max(res["off"]["target_positions_per_s"]["median"], 1e-9), 3),
            ms_per_step_on_minus_off=rw.on_minus_off(res, "ms_per_step")),
        arena=arena_part(args))))


if __name__ == "__main__":
    main()

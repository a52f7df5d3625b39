#!/usr/bin/env python3
"""Cost and data effect of policy surprise weighting (agz_replay_score / agz_replay_set_surprise).

  train   train() ms per iteration (one finished game: ingest, window, sample, training step, and the self-play steps
          between) with surprise = 0.5, against the same run with it off and (--parent-tree DIR: a built checkout of the
          parent commit) against the parent commit's library.  Two libraries cannot share a process, so every round runs
          one child process per (tree, mode) -- this file, importing the package from that tree -- in an order that
          reverses every round.  Accepted when off minus parent lies inside the spread of the parent's own windows; the
          cost of `on` is reported, not bounded.
  score   the scoring pass in positions/s, and the time of the lazy rebuild (weights kernel + the scan in three launches
          + the read of the total) at an arena of --arena-positions positions, as the difference between a sample call
          that rebuilds (rho changed) and one that does not.
  data    what the weighting does to the draw, on a synthetic network (no strength claim): the distribution of q, and the
          share of draws that land on the top decile of KL against the share a uniform draw gives them.

Writes one JSON object to --out (default profiles/surprise_rate.json) and prints it."""
import argparse
import json
import os
import sys
import time

import rate_windows as rw

HERE = os.path.dirname(os.path.abspath(__file__))
RHO = 0.5


def child(args):
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree]
    import alphago_jl_amd as ag
    env = ag.GoEnv(args.board)
    kw = dict(surprise=RHO) if args.modes == "on" else {}
    windows = []
    for w in range(args.warm + args.windows):
        prof = {}
        ag.train(env, num_games=args.train_games, memory_size=args.memory, batch_size=args.batch, readouts=args.readouts,
                 model=ag.NeuralNet(env, tower_height=args.tower, seed=1), start_training_after=args.start_after,
                 slots=args.slots, seed=3, callback=None, profile=prof, **kw)
        if w >= args.warm:
            windows.append(dict(ms_per_iteration=round(1e3 * prof["wall_s"] / args.train_games, 4),
                                train_ms_per_iteration=round(1e3 * prof["train_s"] / args.train_games, 4),
                                steps=prof["steps"], positions=prof["positions"]))
    print("SURPRISE_RATE_CHILD " + json.dumps(windows))


def run_child(args, tree, mode):
    argv = ["--modes", mode] + rw.child_argv(args, ("board", "tower", "readouts", "train_games", "memory", "batch",
                                                     "start_after", "slots", "windows", "warm"))
    return rw.run_child(__file__, "SURPRISE_RATE_CHILD", tree, argv, args.child_timeout)


def summary(ws, key):
    import numpy as np
    v = np.array([w[key] for w in ws], np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4),
                spread=round(float(v.max() - v.min()), 4), windows=len(v))


def measure(windows):
    """-> (the summary of the windows, on against off and off against the parent)"""
    res = {m: {key: summary(w, key) for key in ("ms_per_iteration", "train_ms_per_iteration")} for m, w in windows.items() if w}
    measured = dict(on_minus_off_ms_per_iteration=round(res["on"]["ms_per_iteration"]["median"]
                                                        - res["off"]["ms_per_iteration"]["median"], 4),
                    off_spread_ms_per_iteration=res["off"]["ms_per_iteration"]["spread"])
    if windows["parent_off"]:
        measured.update(rw.off_against_parent(res, dict(ms_per_iteration=("ms_per_iteration", 4))))
    else:
        measured.update(parent="not measured (no --parent-tree)")
    return res, measured


def train_part(args):
    this = os.path.dirname(HERE)
    windows = rw.parent_rounds(          # (parent off, off, on) children, backwards in the odd rounds
        args.pairs, args.parent_tree, lambda tree: run_child(args, tree, "off"),
        lambda k: {m: run_child(args, this, m) for m in (("off", "on") if k % 2 == 0 else ("on", "off"))})
    res, measured = measure(windows)
    return dict(shape=dict(board=args.board, tower=args.tower, readouts=args.readouts, games=args.train_games,
                           slots=args.slots, memory=args.memory, batch=args.batch, start_after=args.start_after),
                windows=windows, summary=res, measured=measured)


def arena_part(args):
    import numpy as np
    import torch
    import alphago_jl_amd as ag
    A = args.board * args.board + 1
    eng = ag.Engine(board_size=args.board, tower_height=args.tower, games=args.arena_slots, num_readouts=args.readouts,
                    seed=1, record_capacity_games=args.arena_games + 8)
    eng.init_synthetic(0)
    eng.start(args.arena_games)
    while eng.records_count() < args.arena_games:
        eng.step(32)
    packed = eng.records_packed().copy()
    eng.replay_ingest(packed)
    base_games, base_pos = eng.replay_count(), eng.replay_positions()
    # ---- data: the base arena, every game scored
    eng.replay_score()                      # (warm: the first call allocates and loads the kernels)
    eng.sync()
    t0 = time.perf_counter()
    targets = eng.replay_score()
    eng.sync()
    score_s = time.perf_counter() - t0
    eng.replay_set_surprise(RHO)
    sur = [eng.replay_surprise(k) for k in range(base_games)]
    kl = np.concatenate([s[0] for s in sur])
    q = np.concatenate([s[1] for s in sur]).astype(np.float64) / 65536.0
    start = np.concatenate([[0], np.cumsum([len(s[0]) for s in sur])])
    top = kl >= np.percentile(kl, 90)
    B, calls, hits = 2048, args.data_calls, 0
    dev = torch.device("cuda", eng.cfg.device)
    bufs = (torch.empty((B, 17 * eng.P), dtype=torch.float32, device=dev), torch.empty((B, A), dtype=torch.float32, device=dev),
            torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int64, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev))
    for c in range(calls):
        eng.replay_sample(B, c, -1, *bufs)
        eng.sync()
        at = start[bufs[3].cpu().numpy()] + bufs[4].cpu().numpy()
        hits += int(top[at].sum())
    pct = lambda v, p: round(float(np.percentile(v, p)), 4)
    data = dict(games=base_games, positions=base_pos, target_plies=int(targets), rho=RHO,
                kl=dict(min=round(float(kl.min()), 5), p10=pct(kl, 10), median=pct(kl, 50), p90=pct(kl, 90), max=pct(kl, 100)),
                w=dict(min=pct(q, 0), p10=pct(q, 10), median=pct(q, 50), p90=pct(q, 90), p99=pct(q, 99), max=pct(q, 100),
                       share_below_1=round(float((q < 1).mean()), 4), share_zero=round(float((q == 0).mean()), 4)),
                draws=B * calls, top_decile_share_of_positions=round(float(top.mean()), 4),
                top_decile_share_of_draws=round(hits / (B * calls), 4),
                top_decile_share_of_weight=round(float(q[top].sum() / q.sum()), 4),
                note="synthetic network: what the rule does to the draw, no strength claim")
    score = dict(positions=base_pos, forward_batch=args.arena_slots * 8, seconds=round(score_s, 4),
                 positions_per_s=round(base_pos / score_s, 1))
    # ---- the rebuild at a large arena: the base games filed again and again
    copies = max(0, -(-args.arena_positions // base_pos) - 1)
    for _ in range(copies):
        eng.replay_ingest(packed)
    npos = eng.replay_positions()
    eng.replay_sample(B, 0, -1, *bufs)
    eng.sync()
    plain, rebuild = [], []
    for r in range(args.rebuilds):
        eng.replay_set_surprise(0.25 if r % 2 == 0 else RHO)          # rho changed: the next sample call rebuilds
        eng.sync()
        t0 = time.perf_counter()
        eng.replay_sample(B, r, -1, *bufs)
        eng.sync()
        rebuild.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        eng.replay_sample(B, r, -1, *bufs)
        eng.sync()
        plain.append(1e3 * (time.perf_counter() - t0))
    eng.close()
    scan = dict(games=base_games * (copies + 1), positions=npos, scored_games=base_games, sample_batch=B,
                sample_ms_with_rebuild=round(float(np.median(rebuild)), 4), sample_ms_without=round(float(np.median(plain)), 4),
                rebuild_ms=round(float(np.median(rebuild) - np.median(plain)), 4), repeats=args.rebuilds)
    return score, scan, data


def main():
    ap = argparse.ArgumentParser()
    rw.parent_args(ap, child_timeout=600, data=False)      # (a child here runs one mode: --modes off, or on)
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--tower", type=int, default=2)
    ap.add_argument("--readouts", type=int, default=32)
    ap.add_argument("--train-games", type=int, default=96)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--memory", type=int, default=4000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--start-after", type=int, default=512)
    ap.add_argument("--windows", type=int, default=2, help="timed train() runs per child")
    ap.add_argument("--warm", type=int, default=1, help="untimed train() runs per child before them")
    ap.add_argument("--pairs", type=int, default=2, help="rounds of (parent off, off, on) children")
    ap.add_argument("--arena-slots", type=int, default=256)
    ap.add_argument("--arena-games", type=int, default=256)
    ap.add_argument("--arena-positions", type=int, default=500000)
    ap.add_argument("--rebuilds", type=int, default=10)
    ap.add_argument("--data-calls", type=int, default=20)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--no-arena", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "surprise_rate.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    sys.path[:0] = [os.path.dirname(HERE)]
    out = dict(rho=RHO)
    if not args.no_train:                   # first: this process has not opened the GPU yet
        out["train"] = train_part(args)
    if not args.no_arena:
        out["score"], out["scan"], out["data"] = arena_part(args)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

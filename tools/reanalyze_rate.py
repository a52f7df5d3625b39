#!/usr/bin/env python3
"""Rate and data effect of reanalysis at the BASELINE.json configs[1] shape (9x9, tower 10, R = 400, 1024
slots, tools/rate_windows.py): an arena of --games self-play games (played at --gen-readouts readouts on the initial
weights) is reanalysed with the network after --train-steps training steps on batches of that arena.

  1. plies/s of the reanalysis run -- agz_replay_reanalyze_start (the gather), the steps, the rows read back, the commit --
     next to plies/s of a review run over the same games fed from the host (agz_review_start with the moves uploaded) on a
     second engine of the same shape and weights.  The search is the same kernels at the same R; a game's draw key is
     base + its record's id here and base + its index there, so the two runs are statistically, not bitwise, the same
     work.  The difference is the gather in front and the commit behind, both timed on their own as well.
  2. the data effect of the commit: mean KL(pi_old || pi_new) over the committed pi rows (rows where the new row is zero
     on a move the old one holds have an infinite KL and are counted instead), mean |q_new - q_old| over the committed
     rows, and the share of rows skipped.
Prints one JSON object."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rate_windows as rw  # noqa: E402


def run_rows(eng, rows, what):
    """step the review run on eng to its end and read its rows, as alphago_jl_amd.review does; a progress line on stderr
    every 30 s (the same in both runs)"""
    t0 = last = time.perf_counter()
    while True:
        done = eng.review_progress()
        if done >= rows:
            break
        if time.perf_counter() - last > 30.0:
            last = time.perf_counter()
            print(f"{what}: {done} of {rows} rows after {last - t0:.0f} s", file=sys.stderr, flush=True)
        eng.step(16)
    return eng.review_results()


def main():
    ap = rw.parser()
    ap.set_defaults(games=128)
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--gen-readouts", type=int, default=32)
    ap.add_argument("--train-steps", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()

    import torch
    import alphago_jl_amd as ag

    G, N, R = args.games, args.board, args.readouts
    gen = ag.Engine(board_size=N, tower_height=args.tower, games=min(G, 1024), num_readouts=args.gen_readouts, seed=1,
                    record_capacity_games=G + 64)
    gen.init_synthetic(0)
    t0 = time.perf_counter()
    gen.start(G)
    while gen.records_count() < G:
        gen.step(16)
    gen_s = time.perf_counter() - t0
    packed = gen.records_packed().copy()
    gen.close()

    args.games = args.slots                       # rw.engine: `games` is the number of slots
    eng = rw.engine(args)
    assert eng.replay_ingest(packed) == G
    old = [eng.replay_record(k) for k in range(G)]
    plies = sum(int(r["num_moves"]) for r in old)

    # the network after some training steps on this arena
    dev = torch.device("cuda", eng.cfg.device)
    B = min(args.batch, plies)
    feats = torch.empty((B, 17 * eng.P), dtype=torch.float32, device=dev)
    pi = torch.empty((B, eng.A), dtype=torch.float32, device=dev)
    z = torch.empty(B, dtype=torch.float32, device=dev)
    for t in range(args.train_steps):
        eng.replay_sample(B, t + 1, -1, feats, pi, z)
        eng.train_step_device(feats, pi, z, B, eta=0.02, rho=0.9)
    eng.sync()

    rev = rw.engine(args)
    eng.copy_weights_to(rev)
    moves = np.concatenate([r["moves"] for r in old]).astype(np.int16)
    off = np.concatenate([[0], np.cumsum([int(r["num_moves"]) for r in old])]).astype(np.int64)

    # warm-up of both paths (kernel loading, allocation): eight games, nothing committed
    eng.reanalyze_start(0, min(8, G))
    run_rows(eng, int(eng.reanalyze_offsets()[-1]), "warm-up")
    rev.review_start(moves[: off[min(8, G)]], off[: min(8, G) + 1])
    run_rows(rev, int(off[min(8, G)]), "warm-up")

    t0 = time.perf_counter()
    rev.review_start(moves, off)
    r_host = run_rows(rev, plies, "review")
    review_s = time.perf_counter() - t0
    rev.close()

    t0 = time.perf_counter()
    eng.reanalyze_start(0, G)
    eng.sync()
    gather_s = time.perf_counter() - t0
    r_dev = run_rows(eng, plies, "reanalysis")
    t1 = time.perf_counter()
    counts = eng.reanalyze_commit()               # synchronises
    t2 = time.perf_counter()
    commit_s, reanalyze_s = t2 - t1, t2 - t0

    new = [eng.replay_record(k) for k in range(G)]
    status = r_dev["status"]
    kl, infinite, dq = [], 0, []
    for j, (a, b) in enumerate(zip(old, new)):
        for k in range(int(a["num_moves"])):
            if status[off[j] + k] != 0:
                continue
            dq.append(abs(float(b["qs"][k]) - float(a["qs"][k])))
            p, q = a["pis"][k].astype(np.float64), b["pis"][k].astype(np.float64)
            if not (p != 0).any():
                continue
            m = p > 0
            if (q[m] == 0).any():
                infinite += 1
            else:
                kl.append(float((p[m] * np.log(p[m] / q[m])).sum()))
    out = dict(shape=dict(board=N, tower=args.tower, readouts=R, slots=args.slots),
               arena=dict(games=G, plies=plies, gen_readouts=args.gen_readouts, gen_seconds=round(gen_s, 1),
                          train_steps=args.train_steps, batch=B),
               review_from_host=dict(seconds=round(review_s, 3), plies_per_s=round(plies / review_s, 1),
                                     ok_rows=int((r_host["status"] == 0).sum())),
               reanalyze=dict(seconds=round(reanalyze_s, 3), plies_per_s=round(plies / reanalyze_s, 1),
                              gather_start_call_ms=round(1e3 * gather_s, 3), commit_call_ms=round(1e3 * commit_s, 3),
                              counts=counts),
               reanalyze_over_review=round((plies / reanalyze_s) / (plies / review_s), 4),
               data_effect=dict(kl_old_new_mean=round(float(np.mean(kl)), 5) if kl else None, kl_rows=len(kl),
                                kl_infinite_rows=infinite, abs_dq_mean=round(float(np.mean(dq)), 5) if dq else None,
                                skipped_share=round(counts["skipped"] / max(plies, 1), 5)))
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost and data effect of the search-value targets in agz_replay_sample, on an arena filled by self-play
at the BASELINE.json configs[1] shape: the setting off against on (alpha 0.5, lambda 0.9) in alternating windows of the
same process on the same box, at B = 32 and B = 2048.

  fill    one engine of tools/rate_windows.py plays with the bench stagger until --arena-games games have finished and
          the arena holds at least 2 x 2048 plies; they are filed with agz_replay_ingest_records.
  window  --calls calls of agz_replay_sample into the same device buffers, each timed from the call to the end of a
          synchronise; the windows alternate off / on and the order reverses every round (--pairs rounds, behind one
          warm-up round that is not reported).  Off launches what the library launched before the setting existed
          (k_replay_sample, k_replay_arena_batch); on adds k_replay_value_targets behind them.
  data    over every sample of the reported on windows: mean and maximum of |y - z|, z the result of the sampled game
          (formed on the device behind each timed call, in the off windows too, so that both modes run the same loop).

Writes --out (profiles/value_target_configs1.json) and prints the same JSON object."""
import json
import os
import statistics
import time

import numpy as np

import rate_windows as rw


def main():
    ap = rw.parser()
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--lam", type=float, default=0.9)
    ap.add_argument("--arena-games", type=int, default=64)
    ap.add_argument("--calls", type=int, default=200, help="timed agz_replay_sample calls per window")
    ap.add_argument("--max-steps", type=int, default=20000, help="give up filling the arena after this many steps")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "value_target_configs1.json"))
    args = ap.parse_args()
    import torch
    eng = rw.engine(args)
    eng.start(0)
    rw.set_stagger(eng, args.stagger)
    eng.start(0)
    steps = 0
    while steps < args.max_steps:
        eng.step(64)
        steps += 64
        n = eng.records_count()
        if n >= args.arena_games and sum(eng.record_header(k)["num_moves"] for k in range(n)) >= 2 * 2048:
            break
    n = eng.records_count()
    assert eng.replay_ingest_records(0, n) == n
    L = eng.replay_live_positions()
    assert L >= 2048, f"the arena holds {L} plies after {steps} steps: raise --max-steps"
    results = np.array([eng.replay_record(k)["result"] for k in range(n)], np.float64)
    res_dev = torch.tensor(results, device=torch.device("cuda", eng.cfg.device))
    out = dict(shape=dict(board=args.board, tower=args.tower, readouts=args.readouts, games=args.games, stagger=args.stagger),
               alpha=args.alpha, lam=args.lam, arena=dict(games=int(n), plies=int(L), fill_steps=steps),
               calls_per_window=args.calls, batches={})
    call = 0
    for B in (32, 2048):
        bufs = eng.replay_sample(B, 0)
        eng.sync()
        us = {"off": [], "on": []}
        dy_sum, dy_max, dy_n = 0.0, 0.0, 0
        for rnd in range(1 + args.pairs):
            for mode in (("off", "on") if rnd % 2 == 0 else ("on", "off")):
                eng.replay_set_value_target(args.alpha if mode == "on" else 0.0, args.lam)
                t = []
                acc = [torch.zeros((), dtype=torch.float64, device=res_dev.device) for _ in range(2)]
                for _ in range(args.calls):
                    call += 1
                    t0 = time.perf_counter()
                    eng.replay_sample(B, call, -1, *bufs)
                    eng.sync()
                    t.append(1e6 * (time.perf_counter() - t0))
                    d = (bufs[2].double() - res_dev[bufs[3]]).abs()      # y against the sampled games' results
                    acc[0] += d.sum()
                    acc[1] = torch.maximum(acc[1], d.max())
                    torch.cuda.synchronize()
                if rnd == 0:
                    continue
                us[mode].append(round(statistics.median(t), 2))
                if mode == "on":
                    dy_sum, dy_max, dy_n = dy_sum + float(acc[0]), max(dy_max, float(acc[1])), dy_n + B * args.calls
                else:
                    assert float(acc[1]) == 0.0, "off: z is the result"
        out["batches"][str(B)] = dict(
            us_per_call_windows=us,
            us_per_call_off=round(statistics.median(us["off"]), 2), us_per_call_on=round(statistics.median(us["on"]), 2),
            on_minus_off_us=round(statistics.median(us["on"]) - statistics.median(us["off"]), 2),
            off_spread_us=round(max(us["off"]) - min(us["off"]), 2),
            mean_abs_y_minus_z=round(dy_sum / dy_n, 4), max_abs_y_minus_z=round(dy_max, 4), samples=dy_n)
        del bufs
    eng.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

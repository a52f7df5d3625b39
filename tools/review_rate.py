#!/usr/bin/env python3
"""Throughput of the batched game review (DESIGN.md "Batched game review") at the BASELINE.json configs[1] shape (9x9,
tower 10, R = 400, 1024 slots), on --games self-play games:
  1. plies/s of alphago_jl_amd.review over every ply of the games (wall time of the call, engine set-up included), and
     the mean root N per row, which shows how much of each tree the previous ply handed over;
  2. positions/s of alphago_jl_amd.analyze on the same positions (rebuilt on the host, a fresh tree per position);
  3. ms per step of a review run next to ms per self-play step, engines of the same shape, alternating windows;
  4. with --agreement: one review run per precision (f32, f16) over the same games and draws, and per ply whether the
     selected moves agree, whether the arg-max of child_N agrees, and the total variation distance of the two visit
     distributions.
The games come from a self-play run at --gen-readouts readouts (only the moves matter, not their quality).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def agreement(env, a, b):
    """per-ply comparison of two reviews of the same games"""
    same_move = same_top = n = 0
    tv = []
    for ga, gb in zip(a, b):
        for x, y in zip(ga, gb):
            if x.status != 0 or y.status != 0:
                continue
            n += 1
            same_move += x.move == y.move
            same_top += int(np.argmax(x.child_N)) == int(np.argmax(y.child_N))
            px = x.child_N.astype(np.float64) / max(float(x.child_N.sum()), 1.0)
            py = y.child_N.astype(np.float64) / max(float(y.child_N.sum()), 1.0)
            tv.append(0.5 * float(np.abs(px - py).sum()))
    return dict(plies=n, selected_move=round(same_move / max(n, 1), 4), top1_child_N=round(same_top / max(n, 1), 4),
                tv_mean=round(float(np.mean(tv)) if tv else 0.0, 4),
                tv_median=round(float(np.median(tv)) if tv else 0.0, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--tower", type=int, default=10)
    ap.add_argument("--readouts", type=int, default=400)
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--gen-readouts", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10, help="steps per timing window")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--no-analyze", action="store_true", help="skip the analyze() comparison")
    ap.add_argument("--agreement", action="store_true", help="f16-vs-f32 agreement over all plies")
    args = ap.parse_args()

    import alphago_jl_amd as ag
    from analysis_rate import positions_at

    N, R, S = args.board, args.readouts, args.slots
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=args.tower, seed=0)

    t0 = time.perf_counter()
    players = ag.selfplay(env, nn, args.gen_readouts, games=args.games, seed=3, game_id_base=0)
    gen_s = time.perf_counter() - t0
    games = [[ag.to_flat(c, env) for c in p.moves] for p in players]
    plies = sum(len(g) for g in games)

    # 1. review
    ag.review(env, nn, games[:8], num_readouts=R, slots=S)             # warm-up (kernel loading, allocation)
    t0 = time.perf_counter()
    res = ag.review(env, nn, games, num_readouts=R, slots=S)
    rv_s = time.perf_counter() - t0
    rows = [a for g in res for a in g]
    statuses = {int(s): sum(1 for a in rows if a.status == s) for s in {a.status for a in rows}}
    inherited = [float(g[k - 1].child_N[games[j][k - 1]]) for j, g in enumerate(res) for k in range(1, len(g))]
    out = dict(shape=dict(board=N, tower=args.tower, readouts=R, slots=S),
               generation=dict(games=len(games), plies=plies, readouts=args.gen_readouts, seconds=round(gen_s, 1)),
               review=dict(seconds=round(rv_s, 3), plies_per_s=round(plies / rv_s, 1), statuses=statuses,
                           mean_root_N=round(float(np.mean([a.N for a in rows])), 1),
                           mean_inherited_N=round(float(np.mean(inherited)) if inherited else 0.0, 1)))

    # 2. analyze on the same positions, with the two_player_mode review uses
    if not args.no_analyze:
        recs = [dict(moves=g) for g in games]
        positions = positions_at(ag, env, [(r, k) for r in recs for k in range(len(r["moves"]))])
        t0 = time.perf_counter()
        ag.analyze(env, nn, positions, num_readouts=R, slots=S, two_player_mode=True)
        an_s = time.perf_counter() - t0
        out["analyze"] = dict(seconds=round(an_s, 3), positions_per_s=round(len(positions) / an_s, 1))
        out["review_over_analyze"] = round((plies / rv_s) / (len(positions) / an_s), 3)

    # 3. step time: a review run and self-play on engines of the same shape, alternating windows
    shape = dict(board_size=N, tower_height=args.tower, games=S, num_readouts=R, parallel_readouts=8, seed=1)
    er = ag.Engine(two_player_mode=1, **shape)
    nn.engine.copy_weights_to(er)
    moves, off = ag.review_arrays(env, games)
    er.review_start(moves, off)
    es = ag.Engine(stagger_moves=60, record_capacity_games=2 * S + 64, **shape)
    nn.engine.copy_weights_to(es)
    es.start(0)
    es.step((R + 7) // 8 + 15)
    er.step(10)
    er.sync()
    es.sync()
    windows = {"review": [], "selfplay": []}
    for k in range(args.pairs):
        order = (("review", er), ("selfplay", es)) if k % 2 == 0 else (("selfplay", es), ("review", er))
        for name, e in order:
            t0 = time.perf_counter()
            e.step(args.steps)
            e.sync()
            windows[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    busy = er.stats()["live_games"]
    es.records_clear()
    er.close()
    es.close()
    mr, ms = statistics.median(windows["review"]), statistics.median(windows["selfplay"])
    out["step_ms"] = dict(windows=windows, review_median=round(mr, 3), selfplay_median=round(ms, 3),
                          review_over_selfplay=round(mr / ms, 4), review_slots_busy_at_end=busy)

    # 4. f16 vs f32 on every ply of the same games
    if args.agreement:
        f16 = ag.review(env, nn, games, num_readouts=R, slots=S, precision="f16")
        out["f16_vs_f32"] = agreement(env, res, f16)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

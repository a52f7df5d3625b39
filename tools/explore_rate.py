#!/usr/bin/env python3
"""Cost and data effect of root exploration and the move temperature (agz_selfplay_set_root_policy_temperature,
agz_selfplay_set_root_noise, agz_search_set_move_temperature) at the BASELINE.json configs[1] shape, on
rate_windows.py's alternating windows of one box.

  parent  (--parent-tree DIR: a built checkout of the parent commit)  Everything off against the parent commit's library.
          The two libraries cannot share a process, so every round runs one child process per tree -- this file, importing
          the package from that tree -- in an order that reverses every round.  Accepted when the medians of ms per step
          and of the k_pre microseconds lie no further apart than the parent's own max - min; otherwise the exit status is 1.
  on      KataGo's values -- (1.25, 1.1, N), (10.83, shaped), (0.75, 0.15, N) -- against off in alternating windows of
          the same process: ms per step, k_pre, the four counters per step.
  data    the synthetic network has no strength to gain or lose, so this is a record of what the rules do to the data,
          not a claim: finished self-play games at a small shape under off and on -- entropy of the recorded pi, the share
          of moves off the most visited child, game length.

Prints one JSON object."""
import json
import os
import sys

import rate_windows as rw

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("ms_per_step", "steps_per_s", "moves_per_s", "evals_per_move", "search_kernels_ms_per_step", "k_pre_us_per_step")


def katago(board):
    return dict(pt=(1.25, 1.1, float(board)), noise=(10.83, True), mt=(0.75, 0.15, float(board)))


def set_mode(eng, on, board):
    k = katago(board)
    eng.set_root_policy_temperature(k["pt"] if on else None)
    eng.set_root_noise(*(k["noise"] if on else (0.0, False)))
    eng.set_move_temperature(k["mt"] if on else None)


def child(args):
    """one tree's windows, in this process: the modes this tree's library knows"""
    # the windows are this tree's rate_windows.py for both trees (it reports k_pre); the package is the tree's own: it is
    # imported when the engine is made, with the tree in front of the path
    sys.path.insert(0, os.path.abspath(args.tree))
    modes = tuple(args.modes.split(","))
    has = "on" in modes                        # (the parent's library has no such calls)

    def configure(eng, mode):
        rw.set_stagger(eng, args.stagger)
        if has:
            set_mode(eng, mode == "on", args.board)

    def collect(s0, s1, c0, c1, dt):
        out = dict(steps_per_s=round(args.steps / dt, 3))
        if c0 is not None:
            out.update(counts_per_step=[round((b - a) / args.steps, 3) for a, b in zip(c0, c1)])
        return out

    eng = rw.engine(args)
    windows = rw.windows_of(eng, args, modes, configure, collect, rw.first_search_steps(args) if args.stagger > 0 else 0,
                            (lambda e: e.explore_counts()) if has else None)
    eng.close()
    print("EXPLORE_RATE_CHILD " + json.dumps(windows))


def data_part(args):
    import numpy as np
    import alphago_jl_amd as ag
    out = {}
    for mode in ("off", "on"):
        eng = ag.Engine(board_size=args.board, tower_height=args.data_tower, games=args.data_games,
                        num_readouts=args.data_readouts, seed=1, record_capacity_games=args.data_games + 8)
        eng.init_synthetic(0)
        set_mode(eng, mode == "on", args.board)
        eng.start(args.data_games)
        while eng.records_count() < args.data_games:
            eng.step(32)
        recs, st, counts = eng.records(), eng.stats(), eng.explore_counts()
        eng.close()
        rows = np.concatenate([r["pis"][: r["num_moves"]] for r in recs if r["num_moves"]]).astype(np.float64)
        moves = np.concatenate([r["moves"][: r["num_moves"]] for r in recs if r["num_moves"]]).astype(np.int64)
        ent = -(np.where(rows > 0, rows * np.log(np.where(rows > 0, rows, 1.0)), 0.0)).sum(axis=1)
        off_max = rows[np.arange(len(moves)), moves] < rows.max(axis=1)        # by the recorded pi, for both modes
        out[mode] = dict(games=len(recs), positions=int(st["positions"]),
                         pi_entropy_nats=round(float(ent.mean()), 4),
                         moves_off_the_most_visited_child=round(float(off_max.mean()), 4),
                         game_length=round(float(np.mean([r["num_moves"] for r in recs])), 2),
                         resignation_share=round(float(np.mean([bool(r["was_resign"]) for r in recs])), 4),
                         counters=list(counts), pool_short_searches=int(st["pool_short_searches"]))
    return out


def measure(windows):
    """-> (the summary of the windows, on against off and off against the parent)"""
    res = rw.summary({m: w for m, w in windows.items() if w}, KEYS)
    measured = dict(on_minus_off_ms_per_step=rw.on_minus_off(res, "ms_per_step"),
                    on_minus_off_k_pre_us=rw.on_minus_off(res, "k_pre_us_per_step"),
                    off_spread_ms_per_step=res["off"]["ms_per_step"]["spread"])
    if windows["parent_off"]:
        measured.update(rw.off_against_parent(res, dict(ms_per_step=("ms_per_step", 4), k_pre_us=("k_pre_us_per_step", 2))))
    return res, measured


def main():
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    ap = rw.parser()
    rw.parent_args(ap)
    args = ap.parse_args()
    if args.child:
        return child(args)
    windows = rw.window_rounds(__file__, "EXPLORE_RATE_CHILD", args)
    res, measured = measure(windows)
    print(json.dumps(dict(
        shape=dict(board=args.board, tower=args.tower, readouts=args.readouts, games=args.games, stagger=args.stagger),
        setting={k: list(v) for k, v in katago(args.board).items()},
        steps_per_window=args.steps, windows=windows, summary=res, measured=measured,
        data=None if args.no_data else dict(
            shape=dict(board=args.board, tower=args.data_tower, readouts=args.data_readouts, games=args.data_games),
            note="synthetic network: what the rules do to the data, no strength claim", **data_part(args)))))

    # the bar of the off path is part of the tool: outside the parent's own spread is a failure, not a figure
    if windows["parent_off"] and not measured["off_within_parent_spread"]:
        print("off against the parent lies outside the parent's own max - min", file=sys.stderr)
        return 1
    return 0

if __name__ == "__main__":
    sys.exit(main())

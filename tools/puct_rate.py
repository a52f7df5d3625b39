#!/usr/bin/env python3
"""Cost and data effect of the PUCT rule options (agz_search_set_puct) at the BASELINE.json configs[1]
shape, on rate_windows.py's alternating windows of one box.

  parent  (--parent-tree DIR: a built checkout of the parent commit)  Off against the parent commit's library.  The two
          libraries cannot share a process, so every round runs one child process per tree -- this file, importing the
          package and rate_windows from that tree -- in an order that reverses every round; each child times its off
          windows (and, on this tree, the on windows beside them).  Accepted when the difference of the medians lies
          inside the spread the parent's own repeated windows show.
  on      (fpu_on, r, r_root, c_base) = (1, 0.2, 0.0, 19652) against off in alternating windows of the same process:
          ms per step, steps/s, positions/s, the search kernels' time per step, the two counters.
  data    the synthetic network has no strength to gain or lose, so this is a record of what the rule does to the data,
          not a claim: finished self-play games at a small shape under off and on -- root children visited per search,
          entropy of the recorded pi, evaluations per position, game length, resignation share.

Prints one JSON object."""
import json
import os
import sys

import rate_windows as rw

HERE = os.path.dirname(os.path.abspath(__file__))
SETTING = (1, 0.2, 0.0, 19652.0)
KEYS = ("ms_per_step", "steps_per_s", "moves_per_s", "evals_per_move", "search_kernels_ms_per_step")


def child(args):
    """one tree's windows, in this process: the modes this tree's library knows"""
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree, os.path.join(tree, "tools")]
    modes = tuple(args.modes.split(","))

    def configure(eng, mode):
        rw.set_stagger(eng, args.stagger)
        if "on" in modes:                      # (the parent's library has no such call)
            eng.set_puct((SETTING[1], SETTING[2]) if mode == "on" else None, SETTING[3] if mode == "on" else 0.0)

    def collect(s0, s1, c0, c1, dt):
        out = dict(steps_per_s=round(args.steps / dt, 3))
        if c0 is not None:
            out.update(levels_per_step=round((c1[0] - c0[0]) / args.steps, 1),
                       unvisited_share=round((c1[1] - c0[1]) / max(c1[0] - c0[0], 1), 4))
        return out

    eng = rw.engine(args)
    windows = rw.windows_of(eng, args, modes, configure, collect, rw.first_search_steps(args) if args.stagger > 0 else 0,
                            (lambda e: e.puct_counts()) if "on" in modes else None)
    eng.close()
    print("PUCT_RATE_CHILD " + json.dumps(windows))


def data_part(args):
    import numpy as np
    import alphago_jl_amd as ag
    out = {}
    for mode in ("off", "on"):
        eng = ag.Engine(board_size=args.board, tower_height=args.data_tower, games=args.data_games,
                        num_readouts=args.data_readouts, seed=1, record_capacity_games=args.data_games + 8)
        eng.init_synthetic(0)
        if mode == "on":
            eng.set_puct((SETTING[1], SETTING[2]), SETTING[3])
        eng.start(args.data_games)
        while eng.records_count() < args.data_games:
            eng.step(32)
        recs, st, counts = eng.records(), eng.stats(), eng.puct_counts()
        eng.close()
        rows = np.concatenate([r["pis"][: r["num_moves"]] for r in recs if r["num_moves"]]).astype(np.float64)
        ent = -(np.where(rows > 0, rows * np.log(np.where(rows > 0, rows, 1.0)), 0.0)).sum(axis=1)
        out[mode] = dict(games=len(recs), positions=int(st["positions"]),
                         root_children_visited_per_search=round(float((rows > 0).sum(axis=1).mean()), 3),
                         pi_entropy_nats=round(float(ent.mean()), 4),
                         evals_per_position=round(st["evals"] / max(st["positions"], 1), 3),
                         game_length=round(float(np.mean([r["num_moves"] for r in recs])), 2),
                         resignation_share=round(float(np.mean([bool(r["was_resign"]) for r in recs])), 4),
                         levels_scored=counts[0], unvisited_share=round(counts[1] / max(counts[0], 1), 4),
                         pool_short_searches=int(st["pool_short_searches"]))
    return out


def measure(windows):
    """-> (the summary of the windows, on against off and off against the parent)"""
    res = rw.summary({m: w for m, w in windows.items() if w}, KEYS)
    measured = dict(on_minus_off_ms_per_step=rw.on_minus_off(res, "ms_per_step"),
                    on_minus_off_search_kernels_ms=rw.on_minus_off(res, "search_kernels_ms_per_step"),
                    on_over_off_moves_per_s=round(res["on"]["moves_per_s"]["median"]
                                                  / max(res["off"]["moves_per_s"]["median"], 1e-9), 4),
                    off_spread_ms_per_step=res["off"]["ms_per_step"]["spread"])
    if windows["parent_off"]:              # the bar is ms per step; the search kernels are a figure beside it
        measured.update(rw.off_against_parent(res, dict(ms_per_step=("ms_per_step", 4))))
        measured.update(off_minus_parent_search_kernels_ms=round(
            res["off"]["search_kernels_ms_per_step"]["median"] - res["parent_off"]["search_kernels_ms_per_step"]["median"], 4))
    return res, measured


def main():
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    ap = rw.parser()
    rw.parent_args(ap)
    args = ap.parse_args()
    if args.child:
        return child(args)
    windows = rw.window_rounds(__file__, "PUCT_RATE_CHILD", args)
    res, measured = measure(windows)
    print(json.dumps(dict(
        shape=dict(board=args.board, tower=args.tower, readouts=args.readouts, games=args.games, stagger=args.stagger),
        setting=dict(fpu_on=SETTING[0], r=SETTING[1], r_root=SETTING[2], c_base=SETTING[3]),
        steps_per_window=args.steps, windows=windows, summary=res, measured=measured,
        data=None if args.no_data else dict(
            shape=dict(board=args.board, tower=args.data_tower, readouts=args.data_readouts, games=args.data_games),
            note="synthetic network: what the rule does to the data, no strength claim", **data_part(args)))))


if __name__ == "__main__":
    main()

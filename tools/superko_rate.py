#!/usr/bin/env python3
"""Cost and data effect of the superko rules (agz_search_set_ko_rule) at the BASELINE.json configs[1]
shape, on rate_windows.py's alternating windows of one box.

  windows  off (the simple ko), positional, situational in alternating windows of one process -- a child process, as the
           tools with a parent part run theirs: ms per step, k_pre microseconds per step, k_expand's share of the five
           search kernels, the two counters per step.
  data     finished self-play games at a small shape under each rule: the share of initialised nodes that lost a move
           (against the positions searched) and the moves removed per game.  The synthetic network has no strength to
           gain or lose: a record of what the rules do, not a claim.

Off against the parent commit is bench.py's to measure (profiles/superko_bench_ab.json).  Prints one JSON object."""
import json
import os
import sys

import rate_windows as rw

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("ms_per_step", "steps_per_s", "moves_per_s", "evals_per_move", "search_kernels_ms_per_step", "k_pre_us_per_step",
        "k_expand_us_per_step", "k_expand_share")
MODES = ("off", "positional", "situational")
RULE = {"off": "simple", "positional": "positional", "situational": "situational"}


def child(args):
    """the windows of the modes asked for, in this process"""
    sys.path.insert(0, os.path.abspath(args.tree))
    modes = tuple(args.modes.split(","))

    def configure(eng, mode):
        rw.set_stagger(eng, args.stagger)
        eng.set_ko_rule(RULE[mode])

    def collect(s0, s1, c0, c1, dt):
        return dict(steps_per_s=round(args.steps / dt, 3),
                    counts_per_step=[round((b - a) / args.steps, 3) for a, b in zip(c0, c1)])

    eng = rw.engine(args)
    windows = rw.windows_of(eng, args, modes, configure, collect, rw.first_search_steps(args) if args.stagger > 0 else 0,
                            lambda e: e.superko_counts())
    eng.close()
    for ws in windows.values():
        for w in ws:
            w["k_expand_share"] = round(1e-3 * w["k_expand_us_per_step"] / max(w["search_kernels_ms_per_step"], 1e-9), 4)
    print("SUPERKO_RATE_CHILD " + json.dumps(windows))


def data_part(args):
    import numpy as np
    import alphago_jl_amd as ag
    out = {}
    for mode in MODES:
        eng = ag.Engine(board_size=args.board, tower_height=args.data_tower, games=args.data_games,
                        num_readouts=args.data_readouts, seed=1, record_capacity_games=args.data_games + 8)
        eng.init_synthetic(0)
        eng.set_ko_rule(RULE[mode])
        eng.start(args.data_games)
        while eng.records_count() < args.data_games:
            eng.step(32)
        recs, st, counts = eng.records(), eng.stats(), eng.superko_counts()
        eng.close()
        out[mode] = dict(games=len(recs), positions=int(st["positions"]), evals=int(st["evals"]),
                         game_length=round(float(np.mean([r["num_moves"] for r in recs])), 2), counters=list(counts),
                         nodes_that_lost_a_move_per_eval=round(counts[0] / max(int(st["evals"]), 1), 6),
                         moves_removed_per_game=round(counts[1] / max(len(recs), 1), 3),
                         pool_short_searches=int(st["pool_short_searches"]))
    return out


def measure(windows):
    """-> (the summary of the windows, each rule against off beside the off windows' own spread)"""
    res = rw.summary({m: w for m, w in windows.items() if w}, KEYS)
    measured = dict(off_spread_ms_per_step=res["off"]["ms_per_step"]["spread"],
                    off_spread_k_pre_us=res["off"]["k_pre_us_per_step"]["spread"])
    for mode in MODES[1:]:
        for key, name in (("ms_per_step", "ms_per_step"), ("k_pre_us_per_step", "k_pre_us"),
                          ("k_expand_us_per_step", "k_expand_us")):
            measured[f"{mode}_minus_off_{name}"] = round(res[mode][key]["median"] - res["off"][key]["median"], 4)
    return res, measured


def main():
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    ap = rw.parser()
    rw.parent_args(ap)
    ap.set_defaults(modes=",".join(MODES))
    args = ap.parse_args()
    if args.child:
        return child(args)
    this = os.path.dirname(HERE)
    windows = {m: [] for m in MODES}
    for k in range(args.pairs):                         # the order of the modes reverses every round
        order = MODES if k % 2 == 0 else MODES[::-1]
        argv = ["--modes", ",".join(order), "--pairs", "1"] + rw.child_argv(
            args, ("board", "tower", "readouts", "games", "stagger", "steps", "warmup"))
        w = rw.run_child(__file__, "SUPERKO_RATE_CHILD", this, argv, args.child_timeout)
        for m in MODES:
            windows[m] += w[m]
    res, measured = measure(windows)
    print(json.dumps(dict(
        shape=dict(board=args.board, tower=args.tower, readouts=args.readouts, games=args.games, stagger=args.stagger),
        steps_per_window=args.steps, windows=windows, summary=res, measured=measured,
        data=None if args.no_data else dict(
            shape=dict(board=args.board, tower=args.data_tower, readouts=args.data_readouts, games=args.data_games),
            note="synthetic network: what the rules do to the data, no strength claim", **data_part(args)))))
    return 0


if __name__ == "__main__":
    sys.exit(main())

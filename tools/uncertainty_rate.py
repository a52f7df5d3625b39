#!/usr/bin/env python3
"""Cost and data effect of the value uncertainty options (agz_search_set_value_moments, agz_search_set_lcb,
agz_search_set_puct_variance) at the BASELINE.json configs[1] shape, on rate_windows.py's alternating
windows of one box.

  windows  off, moments (the S stores alone), on (moments, the LCB rule and the variance factor with values of the kind
           KataGo ships: z = 5, ratio 0.15, k = 0.85, prior 0.4, weight 2) in alternating windows of one process -- a
           child process, as the tools with a parent part run theirs: ms per step, k_pre microseconds per step, the four
           counters per step.
  data     the synthetic network has no strength to gain or lose, so this is a record of what the rules do to the data,
           not a claim: finished self-play games at a small shape under off and on -- the share of moves off the most
           visited child, the mean variance factor (read from the roots of a sample of searches), game length.

Off against the parent commit is bench.py's to measure (profiles/uncertainty_bench_ab.json).  Prints one JSON object."""
import json
import os
import sys

import rate_windows as rw

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("ms_per_step", "steps_per_s", "moves_per_s", "evals_per_move", "search_kernels_ms_per_step", "k_pre_us_per_step")
MODES = ("off", "moments", "on")
LCB, PUCT_VARIANCE = (5.0, 1, 0.15), (0.85, 0.4, 2.0)


def set_mode(eng, mode):
    eng.set_lcb(None)
    eng.set_puct_variance(None)
    eng.set_value_moments(mode != "off")
    if mode == "on":
        eng.set_lcb(LCB)
        eng.set_puct_variance(PUCT_VARIANCE)


def child(args):
    """the windows of the modes asked for, in this process"""
    sys.path.insert(0, os.path.abspath(args.tree))
    modes = tuple(args.modes.split(","))

    def configure(eng, mode):
        rw.set_stagger(eng, args.stagger)
        set_mode(eng, mode)

    def collect(s0, s1, c0, c1, dt):
        return dict(steps_per_s=round(args.steps / dt, 3),
                    counts_per_step=[round((b - a) / args.steps, 3) for a, b in zip(c0, c1)])

    eng = rw.engine(args)
    windows = rw.windows_of(eng, args, modes, configure, collect, rw.first_search_steps(args) if args.stagger > 0 else 0,
                            lambda e: e.uncertainty_counts())
    eng.close()
    print("UNCERTAINTY_RATE_CHILD " + json.dumps(windows))


def data_part(args):
    import numpy as np
    import alphago_jl_amd as ag
    out = {}
    for mode in ("off", "on"):
        eng = ag.Engine(board_size=args.board, tower_height=args.data_tower, games=args.data_games,
                        num_readouts=args.data_readouts, seed=1, record_capacity_games=args.data_games + 8)
        eng.init_synthetic(0)
        set_mode(eng, mode)
        eng.start(args.data_games)
        factors = []
        while eng.records_count() < args.data_games:
            eng.step(32)
            if mode == "on" and len(factors) < 4096:      # the factor at the roots under search, a sample per pause
                for g in range(0, args.data_games, max(args.data_games // 16, 1)):
                    r = eng.tree_root(g)
                    info = eng.node_info(g, r)
                    factors.append(ag.puct_variance_factor(info.N, info.W, eng.node_S(g, r), *PUCT_VARIANCE))
        recs, st, counts = eng.records(), eng.stats(), eng.uncertainty_counts()
        eng.close()
        rows = np.concatenate([r["pis"][: r["num_moves"]] for r in recs if r["num_moves"]]).astype(np.float64)
        moves = np.concatenate([r["moves"][: r["num_moves"]] for r in recs if r["num_moves"]]).astype(np.int64)
        off_max = rows[np.arange(len(moves)), moves] < rows.max(axis=1)        # by the recorded pi, for both modes
        out[mode] = dict(games=len(recs), positions=int(st["positions"]),
                         moves_off_the_most_visited_child=round(float(off_max.mean()), 4),
                         game_length=round(float(np.mean([r["num_moves"] for r in recs])), 2),
                         resignation_share=round(float(np.mean([bool(r["was_resign"]) for r in recs])), 4),
                         counters=list(counts), pool_short_searches=int(st["pool_short_searches"]))
        if mode == "on":
            out[mode].update(lcb_moves_off_the_most_visited_child=round(counts[1] / max(counts[0], 1), 4),
                             levels_with_factor_above_1=round(counts[3] / max(counts[2], 1), 4),
                             mean_root_factor=round(float(np.mean(factors)), 4), root_factors_sampled=len(factors))
    return out


def measure(windows):
    """-> (the summary of the windows, moments and on against off beside the off windows' own spread)"""
    res = rw.summary({m: w for m, w in windows.items() if w}, KEYS)
    measured = dict(off_spread_ms_per_step=res["off"]["ms_per_step"]["spread"],
                    off_spread_k_pre_us=res["off"]["k_pre_us_per_step"]["spread"])
    for mode in ("moments", "on"):
        for key, name in (("ms_per_step", "ms_per_step"), ("k_pre_us_per_step", "k_pre_us")):
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
        w = rw.run_child(__file__, "UNCERTAINTY_RATE_CHILD", this, argv, args.child_timeout)
        for m in MODES:
            windows[m] += w[m]
    res, measured = measure(windows)
    print(json.dumps(dict(
        shape=dict(board=args.board, tower=args.tower, readouts=args.readouts, games=args.games, stagger=args.stagger),
        setting=dict(lcb=list(LCB), puct_variance=list(PUCT_VARIANCE)),
        steps_per_window=args.steps, windows=windows, summary=res, measured=measured,
        data=None if args.no_data else dict(
            shape=dict(board=args.board, tower=args.data_tower, readouts=args.data_readouts, games=args.data_games),
            note="synthetic network: what the rules do to the data, no strength claim", **data_part(args)))))
    return 0


if __name__ == "__main__":
    sys.exit(main())

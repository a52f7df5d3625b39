#!/usr/bin/env python3
"""Cost and effect of the Gumbel root search at the BASELINE.json configs[1] shape, off against on in
alternating windows of the same process on the same box (the method of tools/forced_playouts_rate.py).

  search  per window: the previous window's games are given up, the setting is made (it changes between runs only), a
          run is started with the bench stagger, stepped through its prelude and a warm-up, and then K steps are timed,
          ending in a synchronise.  Reported per mode: ms per step, the five search kernels' time per step (bench.py's
          `search_kernels`), moves/s, evaluations per move, the mean leaves per select phase (evaluations over games
          times steps: the phase cuts of Sequential Halving are the expected cost) and, with the setting on, the halvings
          per search (agz_selfplay_gumbel_counts), with the spread over the repeated windows.
  rows    what the records do not show: a small engine with the setting on, stepped one step at a time; before every
          step each slot's root rows are read (agz_tree_node_floats, agz_tree_gumbel_pi), and after it a slot whose
          root moved on gives one sample -- the move played against the most visited child of the rows read, and the
          entropy of the Gumbel target row against that of children_as_pi on the same visits.

Prints one JSON object."""
import json

import numpy as np

import rate_windows as rw


def entropy(row):
    p = np.asarray(row, np.float64)
    p = p[p > 0]
    return float(-(p * np.log(p)).sum())


def rows_part(args):
    import alphago_jl_amd as ag
    N, R, S = args.board, args.readouts, args.rows_slots
    eng = ag.Engine(board_size=N, tower_height=args.tower, games=S, num_readouts=R, parallel_readouts=8, seed=1,
                    record_capacity_games=4 * S + 64, resign_threshold=-2.0, resign_disable_fraction=0.0)
    eng.init_synthetic(0)
    eng.set_gumbel(args.m, args.c_visit, args.c_scale)
    eng.start(0)
    eng.step(2)
    off_max, h_gumbel, h_visits, samples = 0, [], [], 0
    for _ in range(args.rows_steps):
        before = []
        for g in range(S):
            root = eng.tree_root(g)
            info = eng.node_info(g, root)
            before.append((root, info.pos.n, info.N, eng.node_floats(g, root, 0), eng.tree_gumbel_pi(g, root, args.c_visit,
                                                                                                   args.c_scale)))
        eng.step(1)
        for g in range(S):
            root0, n0, rootN0, cn, row = before[g]
            root = eng.tree_root(g)
            info = eng.node_info(g, root)
            if info.pos.n != n0 + 1 or not cn.sum() > 0:      # no move, or a new game in the slot
                continue
            a = int(info.pos.last_move)
            samples += 1
            off_max += a != int(np.argmax(cn))
            h_gumbel.append(entropy(row))
            h_visits.append(entropy(cn.astype(np.float64) / float(cn.sum())))
        if samples >= args.rows_samples:
            break
    out = dict(slots=S, samples=samples, moves_off_the_most_visited_child=int(off_max),
               share_off_the_most_visited_child=round(off_max / max(samples, 1), 4),
               mean_entropy_gumbel_row=round(float(np.mean(h_gumbel)), 4) if samples else None,
               mean_entropy_children_as_pi=round(float(np.mean(h_visits)), 4) if samples else None,
               uniform_entropy=round(float(np.log(N * N + 1)), 4))
    eng.close()
    return out


def main():
    ap = rw.parser()
    ap.add_argument("--m", type=int, default=16, help="root candidates of the Gumbel search")
    ap.add_argument("--c-visit", type=float, default=50.0)
    ap.add_argument("--c-scale", type=float, default=1.0)
    ap.add_argument("--rows-slots", type=int, default=8, help="slots of the engine of the rows part")
    ap.add_argument("--rows-steps", type=int, default=400, help="most steps of the rows part")
    ap.add_argument("--rows-samples", type=int, default=100, help="moves the rows part stops at")
    args = ap.parse_args()

    def configure(eng, mode):
        rw.set_stagger(eng, args.stagger)
        eng.set_gumbel(args.m if mode == "on" else 0, args.c_visit, args.c_scale)

    def collect(s0, s1, c0, c1, dt):
        begun, halved = c1[0] - c0[0], c1[1] - c0[1]
        return dict(leaves_per_select_phase=round((s1["evals"] - s0["evals"]) / (args.games * args.steps), 3),
                    searches_begun=begun, halvings=halved, halvings_per_search=round(halved / max(begun, 1), 3))

    eng = rw.engine(args)
    windows = rw.windows_of(eng, args, ("off", "on"), configure, collect,
                            rw.first_search_steps(args) if args.stagger > 0 else 0, lambda e: e.gumbel_counts())
    eng.close()
    res = rw.summary(windows, ("ms_per_step", "moves_per_s", "evals_per_move", "leaves_per_select_phase",
                               "search_kernels_ms_per_step", "halvings_per_search"))
    print(json.dumps(dict(
        shape=dict(board=args.board, tower=args.tower, readouts=args.readouts, m=args.m, c_visit=args.c_visit,
                   c_scale=args.c_scale, games=args.games, stagger=args.stagger),
        steps_per_window=args.steps, windows=windows, summary=res,
        measured=dict(
            rw.measured(res),
            evals_per_move=dict(off=res["off"]["evals_per_move"]["median"], on=res["on"]["evals_per_move"]["median"]),
            leaves_per_select_phase=dict(off=res["off"]["leaves_per_select_phase"]["median"],
                                         on=res["on"]["leaves_per_select_phase"]["median"]),
            halvings_per_search=res["on"]["halvings_per_search"]["median"]),
        rows=rows_part(args))))


if __name__ == "__main__":
    main()

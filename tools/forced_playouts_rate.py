#!/usr/bin/env python3
"""Cost and effect of forced playouts and policy target pruning at the BASELINE.json configs[1] shape,
off against on in alternating windows of the same process on the same box (the method of tools/playout_cap_rate.py).

  search  per window: the previous window's games are given up, the setting is made (it changes between runs only), a
          run is started with the bench stagger, stepped through its prelude and a warm-up, and then K steps are timed,
          ending in a synchronise.  Reported per mode: ms per step, the five search kernels' time per step (bench.py's
          `search_kernels`), moves/s, and with the setting on the forced selections per full search and the share of the
          recorded target rows that pruning changed (agz_selfplay_forced_counts over agz_stats.positions), with the
          spread over the repeated windows.
  mass    what pruning moves, which the records do not show (they hold the pruned row only): one host-driven game on a
          single tree with the setting on -- noise, R readouts, then agz_tree_pruned_pi under k against the same call
          under k = 0 (children_as_pi of the raw visits), the move with the most visits played -- gives per searched
          position the mass moved, half the L1 distance of the two rows.

Prints one JSON object."""
import json

import numpy as np

import rate_windows as rw


def mass_part(args):
    import alphago_jl_amd as ag
    N, R = args.board, args.readouts
    eng = ag.Engine(board_size=N, tower_height=args.tower, games=1, num_readouts=R, parallel_readouts=8, seed=1)
    eng.init_synthetic(0)
    eng.set_forced_playouts(args.k, True)
    eng.tree_init(0, np.zeros(N * N, np.int8))
    eng.set_draw(0, 0, 0)
    moved, changed, forced0 = [], 0, eng.forced_counts()[0]
    for ply in range(args.mass_plies):
        root = eng.tree_root(0)
        if eng.is_done(0, root):
            break
        if not eng.node_info(0, root).is_expanded:
            eng.tree_search(0, 8)
        eng.inject_noise(0, root)
        target = eng.node_info(0, root).N + R
        while eng.node_info(0, root).N < target:
            eng.tree_search(0, 8)
        raw, pruned = eng.tree_pruned_pi(0, root, 0.0), eng.tree_pruned_pi(0, root, args.k)
        m = 0.5 * float(np.abs(pruned.astype(np.float64) - raw.astype(np.float64)).sum())
        moved.append(m)
        changed += m > 0
        if not eng.play_move(0, int(np.argmax(eng.node_floats(0, root, 0)))):
            break
    out = dict(positions=len(moved), rows_changed=int(changed), forced_per_search=round((eng.forced_counts()[0] - forced0)
                                                                                       / max(len(moved), 1), 3),
               mean_mass_moved_per_row=round(float(np.mean(moved)), 5) if moved else None,
               mean_mass_moved_per_changed_row=round(float(np.sum(moved)) / max(changed, 1), 5),
               max_mass_moved=round(float(np.max(moved)), 5) if moved else None)
    eng.close()
    return out


def main():
    ap = rw.parser()
    ap.add_argument("--k", type=float, default=2.0, help="forced playouts coefficient (KataGo: 2)")
    ap.add_argument("--mass-plies", type=int, default=40, help="positions of the single-tree game of the mass part")
    args = ap.parse_args()

    def configure(eng, mode):
        rw.set_stagger(eng, args.stagger)
        eng.set_forced_playouts(args.k if mode == "on" else 0.0, True)

    def collect(s0, s1, c0, c1, dt):
        moves = s1["positions"] - s0["positions"]
        forced, rows = c1[0] - c0[0], c1[1] - c0[1]
        # every search is full here (no cap); the stagger's shortened first moves are not in `positions`, so both ratios
        # are slightly high while such games are still about
        return dict(forced_selections=forced, rows_changed=rows, forced_per_full_search=round(forced / max(moves, 1), 3),
                    rows_changed_share=round(rows / max(moves, 1), 4))

    eng = rw.engine(args)
    windows = rw.windows_of(eng, args, ("off", "on"), configure, collect,
                            rw.first_search_steps(args) if args.stagger > 0 else 0, lambda e: e.forced_counts())
    eng.close()
    res = rw.summary(windows, ("ms_per_step", "moves_per_s", "evals_per_move", "search_kernels_ms_per_step",
                               "forced_per_full_search", "rows_changed_share"))
    print(json.dumps(dict(
        shape=dict(board=args.board, tower=args.tower, readouts=args.readouts, k=args.k, prune=True, games=args.games,
                   stagger=args.stagger),
        steps_per_window=args.steps, windows=windows, summary=res,
        measured=dict(rw.measured(res), forced_per_full_search=res["on"]["forced_per_full_search"]["median"],
                      rows_changed_share=res["on"]["rows_changed_share"]["median"]),
        mass=mass_part(args))))


if __name__ == "__main__":
    main()

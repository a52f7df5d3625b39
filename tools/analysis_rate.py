#!/usr/bin/env python3
"""Throughput of the batched analysis mode (DESIGN.md "Batched analysis") at the BASELINE.json configs[1] shape (9x9,
tower 10, R = 400, 1024 slots), on mid-game positions taken from self-play records:
  1. positions/s of alphago_jl_amd.analyze over --positions positions (wall time of the call, engine set-up included);
  2. positions/s of MCTSPlayer.initialize_game + suggest_move (the single-tree path) on a --sample of them;
  3. ms per step of an analysis run next to ms per self-play step, engines of the same shape, alternating windows.
The records come from a short self-play run at --gen-readouts readouts (only the positions matter, not their quality).
With --lines K (and --pv-depth D) it measures the cost of the analysis lines instead: two analysis runs
over the same positions on engines of the same shape in this process, lines on and lines off, in alternating windows of
--steps steps, then the search kernels of both under the engine's event profile.
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


def positions_from_records(ag, env, recs, count, lo, hi, rng):
    """Position objects (board, board_deltas, recent, ko, caps) at a random ply in [lo, hi) of the games, rebuilt by
    batched agz_go_play replay of their move lists"""
    games = [r for r in recs if int(r["num_moves"]) > lo]
    picks = [(games[rng.randint(len(games))], 0) for _ in range(count)]
    picks = [(r, rng.randint(lo, min(hi, int(r["num_moves"])))) for r, _ in picks]
    return positions_at(ag, env, picks)


def positions_at(ag, env, picks):
    """the Position before ply p of record r for every (r, p) of `picks` (records: dicts with flat "moves"), rebuilt by
    batched agz_go_play replay"""
    N, P = env.N, env.N * env.N
    eng = ag.Engine(board_size=N, tower_height=0, games=1, num_readouts=1, max_nodes_per_game=8)
    B = len(picks)
    boards = np.zeros((B, P), np.int8)
    ko = np.full(B, -1, np.int32)
    tp = np.ones(B, np.int8)
    caps = np.zeros((B, 2), np.int64)
    deltas = [[] for _ in range(B)]
    recent = [[] for _ in range(B)]
    for k in range(max([p for _, p in picks], default=0)):
        live = np.array([b for b in range(B) if k < picks[b][1]])
        mv = np.array([int(picks[b][0]["moves"][k]) for b in live], np.int32)
        nb, nko, ncap, st = eng.go_play(boards[live], tp[live], ko[live], mv)
        assert (st == 0).all()
        for j, b in enumerate(live):
            color = int(tp[b])
            d = np.where(nb[j] != boards[b], color, 0).astype(np.int8).reshape(N, N).T     # [row, col]
            deltas[b] = [d] + deltas[b][:6]
            recent[b].append(ag.PlayerMove(color, ag.from_flat(int(mv[j]), env)))
            caps[b, 0 if color == 1 else 1] += int(ncap[j])
        boards[live], ko[live], tp[live] = nb, nko, -tp[live]
    eng.close()
    out = []
    for b, (_, ply) in enumerate(picks):
        out.append(ag.Position(env, board=boards[b].reshape(N, N).T, n=ply, caps=tuple(int(c) for c in caps[b]),
                               ko=None if ko[b] < 0 else ag.from_flat(int(ko[b]), env), recent=recent[b],
                               board_deltas=np.stack(deltas[b]) if deltas[b] else None, to_play=int(tp[b])))
    return out


def lines_cost(ag, args, env, nn, positions, gen_s):
    """ms per analysis step with lines on against lines off: alternating windows, the runs in step with each other (a
    slot finishes a search about every readouts / 8 steps, so the windows have to span several times that), then the
    search kernels of the runs over further steps.  The allowance is the one DESIGN.md §5f derives: the off median plus
    D + 2 dependent round trips (k_leaf_features reads as three of them) plus the off windows' own spread."""
    N, R, S, K, D = args.board, args.readouts, args.slots, args.lines, args.pv_depth
    P = N * N
    shape = dict(board_size=N, tower_height=args.tower, games=S, num_readouts=R, parallel_readouts=8, seed=1,
                 max_nodes_per_game=2 * R + 256)
    boards = np.zeros((len(positions), P), np.int8)
    hist = np.zeros((len(positions), 7, P), np.int8)
    infos = (ag._lib.PositionInfo * len(positions))()
    for k, p in enumerate(positions):
        boards[k], infos[k], h = ag.position_arrays(p)
        hist[k, :len(h)] = h
    # two engines per arm, created off, on, on2, off2: the second pair is the A/A control that tells an engine-instance
    # effect (where its buffers landed) from the cost of the lines
    names = tuple(args.engine_order.split(","))
    assert sorted(names) == ["off", "off2", "on", "on2"], "--engine-order is a permutation of off,on,on2,off2"
    eng = {}
    for name in names:
        e = eng[name] = ag.Engine(**shape)
        nn.engine.copy_weights_to(e)
        if name.startswith("on"):
            e.analyze_set_lines(K, D, args.pv_min_visits)
        e.analyze_start(boards, infos, hist, 0)
        e.step(10)
        e.sync()
    windows = {name: [] for name in names}
    for k in range(args.pairs):
        for j in range(len(names)):
            name = names[(j + k) % len(names)]
            e = eng[name]
            t0 = time.perf_counter()
            e.step(args.steps)
            e.sync()
            windows[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    done_windows = {name: eng[name].analyze_progress() for name in names}
    kernels, prof_steps = {}, min(512, args.steps * max(1, args.pairs // 2))
    for name, e in eng.items():
        e.profile_search(True)
        e.step(prof_steps)
        ms, n = e.profile_search_read()
        e.profile_search(False)
        kernels[name] = {k: round(1e3 * v / max(n, 1), 2) for k, v in ms.items()}        # us per step
    done_end = {name: eng[name].analyze_progress() for name in names}
    for e in eng.values():
        e.close()
    # One of four engines of one shape in one process has run 1.7-1.9 ms per step slower than the other three in every
    # run so far, whichever arm it belonged to (the second one created: profiles/analysis_lines_configs1.json), so each
    # arm is read off its faster engine, and the A/A differences are quoted beside it.
    med = {name: statistics.median(w) for name, w in windows.items()}
    best_off = min(("off", "off2"), key=lambda n: med[n])
    best_on = min(("on", "on2"), key=lambda n: med[n])
    m_off, m_on = med[best_off], med[best_on]
    spread = max(windows[best_off]) - min(windows[best_off])
    trip_us = kernels[best_off]["k_leaf_features"] / 3
    allowance = m_off + (D + 2) * trip_us / 1e3 + spread
    return dict(
        shape=dict(board=N, tower=args.tower, readouts=R, slots=S), positions=len(positions),
        generation=dict(readouts=args.gen_readouts, seconds=round(gen_s, 1)),
        lines=dict(K=K, pv_depth=D, pv_min_visits=args.pv_min_visits),
        step_ms=dict(steps_per_window=args.steps, engines_in_creation_order=list(names), windows=windows,
                     median_by_engine={n: round(v, 3) for n, v in med.items()},
                     off_vs_off2=round(abs(med["off"] - med["off2"]), 3), on_vs_on2=round(abs(med["on"] - med["on2"]), 3),
                     off_engine=best_off, on_engine=best_on, off_median=round(m_off, 3), on_median=round(m_on, 3),
                     off_spread=round(spread, 3), on_minus_off=round(m_on - m_off, 3),
                     on_over_off=round(m_on / m_off, 4)),
        rows_finished_after_windows=done_windows, rows_finished_at_end=done_end,
        search_kernels_us_per_step=dict(steps=prof_steps, **kernels),
        allowance=dict(round_trip_us=round(trip_us, 2), allowance_ms=round(allowance, 3),
                       within=bool(m_on <= allowance)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--tower", type=int, default=10)
    ap.add_argument("--readouts", type=int, default=400)
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--sample", type=int, default=32, help="positions searched by MCTSPlayer.suggest_move")
    ap.add_argument("--gen-readouts", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10, help="steps per timing window")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--lines", type=int, default=0, help="K > 0: compare analysis steps with K lines on against lines off")
    ap.add_argument("--pv-depth", type=int, default=16)
    ap.add_argument("--pv-min-visits", type=int, default=1)
    ap.add_argument("--engine-order", default="off,on,on2,off2",
                    help="--lines: creation order of the four engines (two with lines on, two off)")
    args = ap.parse_args()

    import alphago_jl_amd as ag

    N, R, S = args.board, args.readouts, args.slots
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=args.tower, seed=0)
    rng = np.random.RandomState(0)

    # self-play records -> mid-game positions
    t0 = time.perf_counter()
    recs = [dict(num_moves=len(p.moves), moves=[ag.to_flat(c, env) for c in p.moves])
            for p in ag.selfplay(env, nn, args.gen_readouts, games=S, seed=3, game_id_base=0)]
    gen_s = time.perf_counter() - t0
    P = N * N
    positions = positions_from_records(ag, env, recs, args.positions, P // 8, P // 2, rng)

    if args.lines > 0:
        print(json.dumps(lines_cost(ag, args, env, nn, positions, gen_s)))
        return

    # 1. analyze
    ag.analyze(env, nn, positions[:S], num_readouts=R, slots=S)        # warm-up (kernel loading, allocation)
    t0 = time.perf_counter()
    res = ag.analyze(env, nn, positions, num_readouts=R, slots=S)
    an_s = time.perf_counter() - t0
    statuses = {int(s): sum(1 for a in res if a.status == s) for s in {a.status for a in res}}

    # 2. the single-tree path
    sample = positions[: args.sample]
    player = ag.MCTSPlayer(env, nn, num_readouts=R, seed=0)
    player.initialize_game(sample[0])
    player.suggest_move()                                              # warm-up
    t0 = time.perf_counter()
    for k, pos in enumerate(sample):
        player._game_id = k                                            # the draw key analyze() gives position k
        player.initialize_game(pos)
        player.suggest_move()
    sm_s = time.perf_counter() - t0
    player.engine.close()

    # 3. step time: an analysis run and self-play on engines of the same shape, alternating windows
    shape = dict(board_size=N, tower_height=args.tower, games=S, num_readouts=R, parallel_readouts=8, seed=1)
    ea = ag.Engine(**shape)
    nn.engine.copy_weights_to(ea)
    boards = np.zeros((len(positions), P), np.int8)
    hist = np.zeros((len(positions), 7, P), np.int8)
    infos = (ag._lib.PositionInfo * len(positions))()
    for k, p in enumerate(positions):
        boards[k], infos[k], h = ag.position_arrays(p)
        hist[k, :len(h)] = h
    ea.analyze_start(boards, infos, hist, 0)
    es = ag.Engine(stagger_moves=60, record_capacity_games=2 * S + 64, **shape)
    nn.engine.copy_weights_to(es)
    es.start(0)
    es.step((R + 7) // 8 + 15)
    ea.step(10)
    ea.sync()
    es.sync()
    windows = {"analysis": [], "selfplay": []}
    for k in range(args.pairs):
        order = (("analysis", ea), ("selfplay", es)) if k % 2 == 0 else (("selfplay", es), ("analysis", ea))
        for name, e in order:
            t0 = time.perf_counter()
            e.step(args.steps)
            e.sync()
            windows[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    busy = ea.stats()["live_games"]
    es.records_clear()
    ea.close()
    es.close()
    ma, ms = statistics.median(windows["analysis"]), statistics.median(windows["selfplay"])
    print(json.dumps(dict(
        shape=dict(board=N, tower=args.tower, readouts=R, slots=S), positions=len(positions),
        generation=dict(games=len(recs), readouts=args.gen_readouts, seconds=round(gen_s, 1)),
        analyze=dict(seconds=round(an_s, 3), positions_per_s=round(len(positions) / an_s, 1), statuses=statuses),
        suggest_move=dict(positions=len(sample), seconds=round(sm_s, 3), positions_per_s=round(len(sample) / sm_s, 2)),
        ratio=round((len(positions) / an_s) / (len(sample) / sm_s), 1),
        step_ms=dict(windows=windows, analysis_median=round(ma, 3), selfplay_median=round(ms, 3),
                     analysis_over_selfplay=round(ma / ms, 4), analysis_slots_busy_at_end=busy))))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of a table of start positions at the BASELINE.json configs[1] shape, alternating windows on
the same box in the same process.  Modes:

  off          no table, no stagger: every game begins on the empty board
  on_empty     a table of `--starts` EMPTY boards: the same games as `off`, bit for bit, through the table's path
  on           a table of `--starts` mid-game positions (N*N/4 .. N*N/2 plies of random play)
  off_stagger  no table, the bench stagger: bench.py's steady state of games at mixed stages

Three parts, each on one engine:

  search    the four modes, K timed steps behind the first search of a run.  No game starts inside these windows (the
            count is reported): they price the positions the games are searched from, NOT the install.
  turnover  off / on_empty / on with a resign threshold no game survives: every game resigns at its first move phase
            and its slot starts the next one in the same step, so a window of K steps holds about 2 game starts per
            slot (reported).  on_empty against off is identical work but for the install through the table.
  replay    agz_replay_sample of `--replay-batch` samples over the finished games of a short self-play run, table off /
            on_empty / on: milliseconds per call and the mean ply of the arena's entries (a sample replays `ply` moves;
            with a table it first loads the entry's board and up to 7 older boards).

A table can be set only while no game is being played and the bench stagger excludes it, so every window is a run of
its own: the slots of the previous window are given up (agz_slot_abandon), the mode is set, the run is started,
stepped through its first search plus a warm-up, and then K steps are timed.  Prints one JSON object."""
import json
import statistics
import time

import numpy as np

import rate_windows as rw


def midgame_starts(eng, S, lo, hi, seed, komi=7.5):
    """S positions after lo..hi plies of uniformly random legal play, all games advanced together through the batched
    rule calls (agz_go_legal / agz_go_play) -> (boards [S][P], info array, history [S][7][P])"""
    import alphago_jl_amd as ag
    rng = np.random.default_rng(seed)
    P = eng.P
    boards = np.zeros((S, P), np.int8)
    tp = np.ones(S, np.int8)
    ko = np.full(S, -1, np.int32)
    caps = np.zeros((S, 2), np.int64)
    last = np.full(S, -1, np.int64)
    prev = np.full(S, -1, np.int64)
    hist = np.zeros((S, 7, P), np.int8)
    hl = np.zeros(S, np.int64)
    n = np.zeros(S, np.int64)
    want = rng.integers(lo, hi + 1, S)
    for _ in range(hi):
        act = n < want
        if not act.any():
            break
        legal = eng.go_legal(boards, tp, ko)[:, :P]
        moves = np.full(S, P, np.int32)
        for i in np.flatnonzero(act):
            cand = np.flatnonzero(legal[i])
            if len(cand):
                moves[i] = int(rng.choice(cand))
            elif last[i] == P:                # a second pass would finish the game: this start stays where it is
                want[i] = n[i]
        act = n < want
        bo, ko_o, nc, st = eng.go_play(boards, tp, ko, moves)
        assert (st[act] == 0).all()
        for i in np.flatnonzero(act):
            hist[i, 1:] = hist[i, :-1]
            hist[i, 0] = boards[i]
            hl[i] = min(hl[i] + 1, 7)
            boards[i] = bo[i]
            caps[i, 0 if tp[i] == 1 else 1] += int(nc[i])
            ko[i] = ko_o[i]
            prev[i], last[i] = last[i], moves[i]
            tp[i] = -tp[i]
            n[i] += 1
    info = (ag._lib.PositionInfo * S)()
    for i in range(S):
        f = info[i]
        f.n, f.to_play, f.ko = int(n[i]), int(tp[i]), int(ko[i])
        f.caps_black, f.caps_white = int(caps[i, 0]), int(caps[i, 1])
        f.last_move, f.prev_move, f.history_len, f.komi = int(last[i]), int(prev[i]), int(hl[i]), komi
    return boards, info, hist


def windows_of(eng, args, modes, tables):
    """alternating timed windows of `modes` on one engine -> (ms per step, games started inside each window, ms of
    each set_starts call)"""
    set_ms = []

    def configure(eng, mode):
        if mode == "off_stagger":
            eng.set_starts(None)
            rw.set_stagger(eng, args.stagger)
            return
        rw.set_stagger(eng, 0)
        t0 = time.perf_counter()
        if mode == "off":
            eng.set_starts(None)
        else:
            tb = tables[mode]
            eng.set_starts(boards=tb[0], info=tb[1], history=tb[2])
        set_ms.append(round(1e3 * (time.perf_counter() - t0), 3))

    ws = rw.windows_of(eng, args, modes, configure,
                       lambda s0, s1, c0, c1, dt: dict(games_started=s1["games_started"] - s0["games_started"]),
                       rw.first_search_steps(args), profile=False)
    return ({m: [w["ms_per_step"] for w in v] for m, v in ws.items()},
            {m: [w["games_started"] for w in v] for m, v in ws.items()}, set_ms)


def summary(windows):
    med = {m: round(statistics.median(v), 4) for m, v in windows.items()}
    spread = {m: round(max(v) - min(v), 4) for m, v in windows.items()}
    return med, spread


def replay_part(args, tables):
    """agz_replay_sample over the games of a short run (R = 16, --replay-games games), table off / on_empty / on"""
    import alphago_jl_amd as ag
    import torch
    N, G, B = args.board, args.replay_games, args.replay_batch
    out = {}
    for mode in ("off", "on_empty", "on"):
        eng = ag.Engine(board_size=N, tower_height=1, games=G, num_readouts=16, seed=1, record_capacity_games=G + 8,
                        resign_threshold=-2.0)
        eng.init_synthetic(0)
        if mode != "off":
            tb = tables[mode]
            eng.set_starts(boards=tb[0], info=tb[1], history=tb[2])
        eng.start(G)
        while eng.records_count() < G:
            eng.step(32)
        eng.replay_ingest_records(0, G)
        entries = eng.replay_positions()
        plies = [eng.replay_record(k)["num_moves"] for k in range(G)]
        mean_ply = sum(n * (n - 1) / 2 for n in plies) / max(entries, 1)
        bufs = eng.replay_sample(B, 1)
        eng.sync()
        ms = []
        for rep in range(args.replay_calls):
            t0 = time.perf_counter()
            eng.replay_sample(B, 2 + rep, -1, *bufs)
            eng.sync()
            ms.append(round(1e3 * (time.perf_counter() - t0), 4))
        out[mode] = dict(entries=entries, mean_ply=round(mean_ply, 2), ms_per_call=ms,
                         median_ms=round(statistics.median(ms), 4), spread_ms=round(max(ms) - min(ms), 4))
        eng.close()
        del bufs
        torch.cuda.empty_cache()
    return out


def main():
    ap = rw.parser()          # --stagger is the off_stagger windows' alone
    ap.add_argument("--starts", type=int, default=1024)
    ap.add_argument("--replay-games", type=int, default=512)
    ap.add_argument("--replay-batch", type=int, default=2048)
    ap.add_argument("--replay-calls", type=int, default=20)
    args = ap.parse_args()

    N, R = args.board, args.readouts
    eng = rw.engine(args)
    t0 = time.perf_counter()
    tables = dict(on=midgame_starts(eng, args.starts, N * N // 4, N * N // 2, seed=7))
    t_gen = time.perf_counter() - t0
    tables["on_empty"] = midgame_starts(eng, args.starts, 0, 0, seed=7)
    search, search_started, set_ms = windows_of(eng, args, ("off", "on_empty", "on", "off_stagger"), tables)
    short = eng.stats()["pool_short_searches"]
    eng.close()
    # no game survives its first move phase: Q_perspective(root) < 2 always (mcts_play.jl:124)
    eng = rw.engine(args, resign_threshold=2.0, resign_disable_fraction=0.0)
    turn, turn_started, _ = windows_of(eng, args, ("off", "on_empty", "on"), tables)
    eng.close()
    rp = replay_part(args, tables)
    med, spread = summary(search)
    tmed, tspread = summary(turn)
    print(json.dumps(dict(
        shape=dict(board=N, tower=args.tower, readouts=R, games=args.games, starts=args.starts, stagger=args.stagger),
        steps_per_window=args.steps,
        search=dict(ms_per_step=search, games_started_in_window=search_started, median_ms=med, spread_ms=spread,
                    on_empty_minus_off_ms=round(med["on_empty"] - med["off"], 4),
                    on_minus_off_ms=round(med["on"] - med["off"], 4),
                    on_minus_off_stagger_ms=round(med["on"] - med["off_stagger"], 4)),
        turnover=dict(ms_per_step=turn, games_started_in_window=turn_started, median_ms=tmed, spread_ms=tspread,
                      on_empty_minus_off_ms=round(tmed["on_empty"] - tmed["off"], 4),
                      on_minus_off_ms=round(tmed["on"] - tmed["off"], 4)),
        replay_sample=dict(batch=args.replay_batch, games=args.replay_games, modes=rp),
        set_starts_ms=set_ms, table_generation_s=round(t_gen, 2), pool_short_searches=short)))


if __name__ == "__main__":
    main()

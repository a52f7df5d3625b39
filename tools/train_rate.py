#!/usr/bin/env python3
"""Rates of the batched train() at the BASELINE.json configs[1] shape by default (9x9, tower 10,
R = 400, 1024 slots), with a small start_training_after so that training runs from the first finished game:
  1. self-play positions/s inside train() and of the same engine shape stepping self-play alone (hold off), in
     alternating windows (--rounds of each; a train() window plays --games games, the self-play window runs as long);
  2. training steps/s (agz_train_step calls per second of the time spent sampling and training);
  3. the share of train()'s wall time spent in sampling + training;
  4. host synchronisations per engine step: the library calls of train()'s loop that synchronise (each at least once).
Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--tower", type=int, default=10)
    ap.add_argument("--readouts", type=int, default=400)
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--games", type=int, default=None, help="games per train() window (default 2 x slots)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--start-after", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    import alphago_jl_amd as ag
    env = ag.GoEnv(a.board)
    nn = ag.NeuralNet(env, tower_height=a.tower)
    games = a.games or 2 * a.slots
    rows = []
    for r in range(a.rounds):
        prof = {}
        ag.train(env, num_games=games, memory_size=500000, batch_size=a.batch, readouts=a.readouts, tower_height=a.tower,
                 model=nn, start_training_after=a.start_after, slots=a.slots, seed=r, game_id_base=r * games,
                 callback=None, profile=prof)
        eng = ag.Engine(board_size=a.board, tower_height=a.tower, games=a.slots, num_readouts=a.readouts, seed=100 + r)
        nn.engine.copy_weights_to(eng)
        eng.start(0)
        eng.step(16)
        p0, t0 = eng.stats()["positions"], time.perf_counter()
        while time.perf_counter() - t0 < prof["wall_s"]:
            eng.step(16)
        p1, t1 = eng.stats()["positions"], time.perf_counter()
        eng.close()
        rows.append(dict(train_positions_per_s=prof["positions"] / prof["wall_s"],
                         selfplay_positions_per_s=(p1 - p0) / (t1 - t0),
                         train_steps_per_s=prof["train_steps"] / max(prof["train_s"], 1e-9),
                         train_share=prof["train_s"] / prof["wall_s"],
                         host_syncs_per_step=prof["host_syncs"] / max(prof["steps"], 1), **prof))
    med = lambda k: statistics.median(x[k] for x in rows)
    print(json.dumps(dict(shape=dict(board=a.board, tower=a.tower, readouts=a.readouts, slots=a.slots, games=games,
                                     batch=a.batch, start_training_after=a.start_after),
                          train_positions_per_s=med("train_positions_per_s"),
                          selfplay_positions_per_s=med("selfplay_positions_per_s"),
                          ratio=med("train_positions_per_s") / med("selfplay_positions_per_s"),
                          train_steps_per_s=med("train_steps_per_s"), train_share=med("train_share"),
                          host_syncs_per_step=med("host_syncs_per_step"), windows=rows)))


if __name__ == "__main__":
    main()

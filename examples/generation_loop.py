#!/usr/bin/env python3
"""One generation of the reference's train() loop (src/train.jl:38-92) on the MI355X:
self-play -> replay arena -> training batches -> optimiser step -> arena match -> checkpoint.

    python examples/generation_loop.py [--board 9] [--tower 2] [--games 32] [--readouts 64] [--reanalyze]
                                       [--surprise RHO] [--explore] [--uncertainty] [--ko-rule RULE]

What runs where:
  selfplay          G concurrent games on the device (one wave per tree, one network batch per step)
  extract_data      finished games come back as (moves, pi, result); multi-GPU: all-gathered over RCCL
  get_replay_batch  (game, ply) pairs are sampled on the host; the device replays the move lists of the replay
                    arena and emits the N x N x 17 x B feature tensor, pi and z (agz_replay_batch)
  explore           (--explore) KataGo's root exploration in self-play: the root prior at temperature 1.25 -> 1.1, shaped
                    Dirichlet noise of total concentration 10.83 over the legal moves, the move sampled at temperature
                    0.75 -> 0.15, each with a halflife of the board size (agz_selfplay_set_root_policy_temperature /
                    _set_root_noise, agz_search_set_move_temperature)
  uncertainty       (--uncertainty) value uncertainty in self-play and in the arena match: a second moment beside every W,
                    the move picked by the lower confidence bound (z = 5 among the children with at least 0.15 of the top
                    visits) and the PUCT scale times 1 + 0.85 (sd / 0.4 - 1) of a node's own values, the expected spread
                    0.4 weighing 2 visits (agz_search_set_value_moments / _set_lcb / _set_puct_variance); values of the
                    kind KataGo ships, quoted from memory
  reanalyze         (--reanalyze) the arena's games are searched again on the current weights and their pi / q
                    targets overwritten in place, moves and results as played (agz_replay_reanalyze_start / _commit)
  surprise          (--surprise RHO) every arena ply is scored by KL(pi || prior) on the current weights and the batches
                    are drawn on the device by weight, with replacement (agz_replay_score / agz_replay_set_surprise)
  _train            agz_train_step: training-mode forward, 0.01 CE + 0.01 MSE + 1e-4 L2, backward, Momentum(0.02)
  evaluate          candidate vs incumbent, both networks resident in one arena engine
  save_model        BSON parameter lists readable by Flux.loadparams!
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the engine: one HIP runtime per process)

import alphago_jl_amd as ag  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--tower", type=int, default=2)
    ap.add_argument("--games", type=int, default=32)
    ap.add_argument("--readouts", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--eval-games", type=int, default=8)
    ap.add_argument("--reanalyze", action="store_true", help="refresh the arena's targets before the training batches")
    ap.add_argument("--surprise", type=float, default=0.0, metavar="RHO",
                    help="policy surprise weighting: draw the training batches by weight, this share of each game's "
                         "sampling mass in proportion to KL(pi || prior)")
    ap.add_argument("--explore", action="store_true",
                    help="KataGo's root policy temperature, shaped root noise and move temperature in self-play")
    ap.add_argument("--uncertainty", action="store_true",
                    help="value moments, the move by lower confidence bound and variance-scaled exploration")
    ap.add_argument("--ko-rule", default=None, choices=["simple", "positional", "situational"], metavar="RULE",
                    help="superko in self-play and in the arena match: positional or situational repetition is refused")
    args = ap.parse_args(argv)

    env = ag.GoEnv(args.board)
    cur = ag.NeuralNet(env, tower_height=args.tower, seed=0)        # Flux-default-equivalent init
    prev = ag.NeuralNet(env, tower_height=args.tower, seed=1)

    explore = {}
    if args.explore:        # KataGo's values; the halflife of both schedules is the board size
        explore = dict(root_policy_temperature=(1.25, 1.1, args.board), root_noise=(10.83, True),
                       move_temperature=(0.75, 0.15, args.board))
    # values of the kind KataGo ships (no strength claim: there is no trained network here)
    uncertainty = dict(lcb=(5.0, 1, 0.15), puct_variance=(0.85, 0.4, 2.0)) if args.uncertainty else {}
    ko = dict(ko_rule=args.ko_rule) if args.ko_rule else {}      # (ours) agz_search_set_ko_rule, DESIGN.md §5x
    records = ag.selfplay(env, cur, args.readouts, games=args.games, seed=1, **explore, **uncertainty, **ko)
    buf = ag.ReplayBuffer(env, memory_size=500000)
    buf.extend(records)
    print(f"self-play: {len(records)} games, {len(buf)} positions, "
          f"results B/W/draw = {sum(r.result == 1 for r in records)}/{sum(r.result == -1 for r in records)}/"
          f"{sum(r.result == 0 for r in records)}")

    B = min(args.batch_size, len(buf))
    feats = torch.empty((B, 17 * env.N * env.N), dtype=torch.float32, device="cuda")
    _, pi, z = buf.sample(B, np.random.default_rng(0), cur.engine, out=feats)       # host-side buffer, device replay
    # the same through the device replay arena + the training step (train.jl:56-70)
    eng = cur.engine
    if args.reanalyze:      # a search needs slots, readouts and a node pool: an engine of that shape holds the arena
        eng = ag.Engine(board_size=env.N, tower_height=args.tower, games=min(args.games, 1024),
                        num_readouts=args.readouts, seed=1)
        cur.engine.copy_weights_to(eng)
    eng.replay_ingest(ag.distributed.pack_records(
        [dict(game_id=r.game_id, result=r.result, was_resign=r.was_resign, moves=[ag.to_flat(c, env) for c in r.moves],
              pis=r.searches_pi, qs=r.qs) for r in records], env.action_space))
    if args.reanalyze:
        counts, _ = ag.reanalyze(eng)
        print(f"reanalyse: {counts['committed']} rows refreshed ({counts['pi_rows']} pi rows), {counts['skipped']} skipped")
    if args.surprise > 0:
        eng.replay_set_surprise(args.surprise)
        print(f"surprise: {eng.replay_score()} target plies scored, rho = {args.surprise}")
    rng = np.random.default_rng(1)
    lens = np.array([eng.replay_record(k)["num_moves"] for k in range(eng.replay_count())])
    losses = []
    for it in range(3):
        if args.surprise > 0:                                                     # drawn on the device, by weight
            f, p, zz, _, _ = eng.replay_sample(B, it)
            losses.append(float(eng.train_step_device(f, p, zz, B)[0]))
            continue
        flat = rng.choice(int(lens.sum()), size=B, replace=False)                 # sample(1:n, B, replace=false)
        game = np.searchsorted(np.cumsum(lens), flat, side="right")
        ply = flat - (np.cumsum(lens) - lens)[game]
        f, p, zz = eng.replay_batch(game, ply)
        losses.append(eng.train_step(f, p, zz)[0])
    print("training: loss", " -> ".join(f"{x:.5f}" for x in losses))
    if args.reanalyze:      # the trained weights go back to the network the match and the checkpoint use
        eng.copy_weights_to(cur.engine)
        eng.close()

    ok, st = ag.evaluate(env, cur, prev, num_games=args.eval_games, ro=args.readouts, seed=2, return_stats=True,
                         **uncertainty, **ko)
    print(f"evaluate: Black (candidate) won {st.games_won}/{st.num_games} -> {'keep' if ok else 'revert'}")

    with tempfile.TemporaryDirectory() as d:
        ag.save_model(cur, d)
        back = ag.load_model(d, env)
        x = (np.random.RandomState(0).rand(1, 17 * env.N * env.N) < 0.3).astype(np.float32)
        same = (back.engine.forward_features(x)[0] == cur.engine.forward_features(x)[0]).all()
        print("checkpoint round trip:", sorted(os.listdir(os.path.join(d, "weights"))), "identical outputs:", bool(same))
        back.engine.close()
    return len(buf), st.num_games, bool(same)


if __name__ == "__main__":
    main()

"""Batched train() on the device: agz_replay_sample against its host twin and agz_replay_batch; train()
against a loop composed in this file from single ABI calls (step, hold / release, agz_replay_ingest_records, the twin's
indices, agz_replay_batch, agz_train_step); with slots = 1 every game is the oracle's game on the weights of that moment;
the hold changes nothing while it is off; checkpoints load back."""
import numpy as np
import pytest

import alphago_jl_amd as ag
from alphago_jl_amd import Engine, GoEnv, NeuralNet, load_model, train
from gpu_common import GpuNetForOracle
from gpu_options import _lengths, _twin_pairs, _weights
from test_hostsim_selfplay import bits_equal, oracle_game
from test_train_loop_batched import sample_syms

pytestmark = pytest.mark.gpu
N, TOWER, R, SEED = 5, 1, 16, 3


def _arena(N, games, slots, R, tower=1, seed=1):
    e = Engine(board_size=N, tower_height=tower, games=slots, num_readouts=R, seed=seed, record_capacity_games=games + 8)
    e.init_synthetic(5)
    e.start(games)
    while e.records_count() < games:
        e.step(16)
    assert e.replay_ingest_records(0, games) == games
    return e


@pytest.mark.parametrize("N,games,slots,R,memory,B", [(5, 3, 3, 8, None, 8), (5, 3, 3, 8, "cut", 16),
                                                      (5, 3, 3, 8, "cut", "all"), (9, 64, 64, 2, 1500, 256)])
def test_sample_equals_twin_and_replay_batch(N, games, slots, R, memory, B):
    import torch
    e = _arena(N, games, slots, R)
    total = e.replay_positions()
    if memory == "cut":
        memory = total - _lengths(e)[0] // 2 - 1                 # the oldest game keeps only its newest plies
    if memory is not None:
        e.replay_set_window(memory)
        assert e.replay_live_positions() == min(memory, total)
    if B == "all":
        B = e.replay_live_positions()
    for call, sym in ((1, -1), (2, 8), (3, 5)):
        feats, pi, z, game, ply = e.replay_sample(B, call, sym)
        torch.cuda.synchronize()
        e.sync()
        g, p = _twin_pairs(e, call, B)
        assert (game.cpu().numpy() == g).all() and (ply.cpu().numpy() == p).all()
        if sym == -1:
            wf, wp, wz = e.replay_batch(g, p)
        else:
            s = sample_syms(e.cfg.seed, call, B) if sym == 8 else np.full(B, sym, np.int32)
            wf, wp, wz = e.replay_batch_sym(g, p, s)
        assert bits_equal(feats.cpu().numpy(), wf) and bits_equal(pi.cpu().numpy(), wp) and bits_equal(z.cpu().numpy(), wz)
    e.close()


def host_loop(env, nn0, num_games, slots, memory, B, start_after, epochs=1, augment=False, on_start=None, on_game=None):
    """train()'s schedule composed from single calls; on_start(game index, engine) when a game is released to start,
    on_game(i, engine) after game i's training"""
    eng = Engine(board_size=env.N, tower_height=nn0.tower_height, games=slots, num_readouts=R, seed=SEED,
                 record_capacity_games=slots + 8)
    nn0.engine.copy_weights_to(eng)
    eng.set_hold(True)
    eng.start(num_games)
    eng.release()
    cuts = list(range(0, B, 32)) + [B]
    if len(cuts) > 2 and cuts[-1] - cuts[-2] == 1:
        del cuts[-2]
    i, claimed, pending, out, steps = 0, 0, min(slots, num_games), [], 0
    while i < num_games:
        for k in range(claimed, claimed + pending):
            if on_start:
                on_start(k, eng)
        claimed += pending
        before = eng.stats()["games_started"]
        eng.step(1)
        steps += 1
        assert eng.stats()["games_started"] - before == pending    # games start only right after a release
        n = eng.records_count()
        recs = sorted(eng.records(), key=lambda r: r["game_id"])
        for r in recs:
            assert eng.replay_ingest_records(r["index"], 1) == 1
            eng.replay_set_window(memory)
            i += 1
            loss = None
            if eng.replay_live_positions() >= start_after:
                g, p = _twin_pairs(eng, i, B)
                if augment:
                    f, pi, z = eng.replay_batch_sym(g, p, sample_syms(SEED, i, B))
                else:
                    f, pi, z = eng.replay_batch(g, p)
                loss = 0.0
                for _ in range(epochs):
                    for lo, hi in zip(cuts[:-1], cuts[1:]):
                        loss += float(eng.train_step(f[lo:hi], pi[lo:hi], z[lo:hi], eta=np.float32(0.02), rho=0.9)[0])
                loss /= epochs
            out.append(dict(i=i, record=r, loss=loss, step=steps))
            if on_game:
                on_game(i, eng)
        eng.records_clear()
        eng.release()
        pending = min(n, num_games - claimed)
    w = _weights(eng)
    eng.close()
    return out, w


def _same_records(a, b):
    for x, y in zip(a, b):
        assert x["game_id"] == y["game_id"] and x["num_moves"] == y["num_moves"] and x["result"] == y["result"]
        assert (x["moves"] == y["moves"]).all() and bits_equal(x["pis"], y["pis"]) and bits_equal(x["qs"], y["qs"])


def test_slots_1_is_the_reference_loop_game_by_game():
    env = GoEnv(N)
    nn0 = NeuralNet(env, tower_height=TOWER)
    chk = NeuralNet(env, tower_height=TOWER)
    want = {}

    def on_start(k, eng):                      # the oracle's game on the weights the engine holds when game k starts
        eng.copy_weights_to(chk.engine)
        want[k] = oracle_game(N, GpuNetForOracle(chk.engine), R, SEED, k)

    ref, w_ref = host_loop(env, nn0, 4, 1, 60, 8, 8, on_start=on_start)
    assert sum(g["loss"] is not None for g in ref) >= 3
    for g in ref:
        r, o = g["record"], want[g["record"]["game_id"]]
        n = o["num_moves"]
        assert r["num_moves"] == n and list(r["moves"]) == list(o["moves"][:n]) and r["result"] == o["result"]
        assert bits_equal(r["pis"], o["pis"]) and bits_equal(r["qs"], o["qs"])
    lines = []
    nn, log = train(env, num_games=4, memory_size=60, batch_size=8, readouts=R, model=nn0, start_training_after=8,
                    slots=1, seed=SEED, callback=lines.append, return_log=True)
    _same_records([g["record"] for g in log], [g["record"] for g in ref])
    assert [g["loss"] for g in log] == [g["loss"] for g in ref]
    assert all(bits_equal(nn.engine.get_weights(*lk), v) for lk, v in w_ref.items())
    assert sum(line.startswith("Episode ") for line in lines) == sum(g["loss"] is not None for g in ref)
    for g in log:                              # sequential: game i + 1 starts after game i's training
        assert g["trained_before_start"] == sum(h["loss"] is not None for h in log if h["i"] < g["i"])


@pytest.mark.parametrize("augment", [False, True])
def test_slots_8_equals_the_host_composed_schedule(augment):
    env = GoEnv(N)
    nn0 = NeuralNet(env, tower_height=TOWER, seed=1)
    ref, w_ref = host_loop(env, nn0, 24, 8, 50, 16, 16, augment=augment)
    nn, log = train(env, num_games=24, memory_size=50, batch_size=16, readouts=R, model=nn0, start_training_after=16,
                    slots=8, seed=SEED, augment=augment, callback=None, return_log=True)
    assert len(log) == len(ref) == 24
    _same_records([g["record"] for g in log], [g["record"] for g in ref])
    assert [g["loss"] for g in log] == [g["loss"] for g in ref]
    assert all(bits_equal(nn.engine.get_weights(*lk), v) for lk, v in w_ref.items())
    assert max(g["live"] for g in log) == 50                     # the window cut games partway
    # no game started before the training of a game that finished in an earlier step
    for g in log:
        earlier = [h for h in log if h["step"] < g["start_step"] and h["loss"] is not None]
        assert g["trained_before_start"] == len(earlier)
    # games overlap training: some game was in flight across a training step
    trained_at = [h["step"] for h in log if h["loss"] is not None]
    assert any(g["start_step"] <= s < g["step"] for g in log for s in trained_at)


def test_hold_off_changes_nothing():
    def run(hold):
        e = Engine(board_size=N, tower_height=TOWER, games=4, num_readouts=R, seed=SEED, record_capacity_games=16)
        e.init_synthetic(2)
        if hold is not None:
            e.set_hold(True)
            e.release()
            e.set_hold(hold)
        e.start(6)
        while e.records_count() < 6:
            e.step(4)
        r = e.records()
        e.close()
        return r
    fresh = run(None)
    _same_records(run(False), fresh)


def test_checkpoints_load_back_with_the_weights_of_that_game(tmp_path):
    env = GoEnv(N)
    nn0 = NeuralNet(env, tower_height=TOWER, seed=4)
    snap = {}

    def on_game(i, eng):
        if i % 2 == 0:
            snap[i] = NeuralNet(env, tower_height=TOWER)
            eng.copy_weights_to(snap[i].engine)

    host_loop(env, nn0, 4, 2, 60, 8, 8, on_game=on_game)
    train(env, num_games=4, memory_size=60, batch_size=8, readouts=R, model=nn0, start_training_after=8, slots=2,
          seed=SEED, ckp_freq=2, checkpoint_dir=str(tmp_path), callback=None)
    pos = [ag.Position(env)]
    pos.append(pos[0].play_move((2, 2)))
    pos.append(pos[1].play_move((1, 3)))
    for i in (2, 4):
        got = load_model(str(tmp_path / f"game_{i}"), env)
        pa, va = got(pos)
        pb, vb = snap[i](pos)
        assert np.allclose(pa, pb, atol=1e-6) and np.allclose(va, vb, atol=1e-6)

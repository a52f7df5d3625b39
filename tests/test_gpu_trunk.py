"""Every form of the HIP tower against the float64 oracle ON THE TRUNK ITSELF, and pi / v on networks whose heads are live.

The pi / v parity tests (test_gpu_nn.py, test_gpu_nn32s.py, test_gpu_nn16.py, test_gpu_tower.py, test_gpu_wino5.py) look at the
tower through a flat softmax and, at the deeper shapes, through a value head that is dead (tests/trunk_probe.py says why and
tests/test_trunk_probe.py measures what slips through).  Here the network gets a probe head (trunk_probe.set_probe): one forward
then returns a random linear functional w.h of the final trunk at every board point, l = log pi[p] - log pi[pass], through heads
that are plain f32 in every form.  K = 4 functionals per case, the same for the oracle and the device.

Bars, on e_gpu = max |l_gpu - l_f64| against e_ref = max |l_directf32oracle - l_f64| over the same samples:
  * exact-f32 forms (direct GEMM, F(3x3,3x3) per layer / persistent / five-pass / on dense blocks, F(4x4,3x3)):
    e_gpu <= 8 e_ref -- twice the top of the 2 .. 4 x that F(4x4,3x3) is expected to lose against direct f32 (VERDICT.md,
    weak point 1);
  * f32s (operands as two f16 halves: 22 significant bits against 24): e_gpu <= 32 e_ref;
  * f16: no closer to its restatement (oracle precision 16) than that restatement is to float64 -- reported, and asserted only
    as e(gpu, restatement) <= e(restatement, f64): on random weights f32 and f64 sums round to different halves now and then,
    and no bar under such a flip exists.  What a flip would hide -- structural defects of the fp16 kernels -- is caught in
    tests/test_gpu_exact_tower.py, where every rounded value is an integer and the trunk has to agree exactly;
  * every form: a row's read-out does not depend on its batch position, to the bit.
tests/test_trunk_probe.py::test_defect_audit shows a dropped tap or tf32-class weight noise at >= 16 e_ref.  No bar here comes from
a device measurement.  Then the ordinary heads, on live networks: |dpi|, |dv| <= 1e-4 against float64, the project's bar.

Board size is what the tower's edge code depends on, so tower 2 (the stem epilogue that emits the first V, a conv1 / conv2 pair
with its residual, the hand-over to the next block, the last layer; in fp16 `w2` on the first and last layer and `q` on the two
between) runs at EVERY size from 3 to 19, under every form the size has (`forms_at`).  The size classes -- T tiles a side, the
boards a tile block holds, and the overhang: the points by which the last tile hangs over the board edge:

         F(3x3,3x3): winograd up to 12, persistent, five-pass,      F(4x4,3x3): winograd from 13
         f32s; from 13 on dense blocks (f33-dense, f32s)
     N    T   boards per block   overhang                            T   boards per block    overhang
     3    1   64                 0
     4    2   16                 2
     5    2   16                 1
     6    2   16                 0
     7    3   7                  2
     8    3   7                  1
     9    3   7                  0
    10    4   4                  2
    11    4   4                  1
    12    4   4                  0
    13    5   dense              2                                   4   4                   3
    14    5   dense              1                                   4   4                   2
    15    5   dense              0                                   4   4                   1
    16    6   dense              2                                   4   4                   0
    17    6   dense              1                                   5   5 per block pair    3
    18    6   dense              0                                   5   5 per block pair    2
    19    7   dense              2                                   5   5 per block pair    1

The batches (trunk_probe.SIZE_BATCH) fill one tile block of every form and leave a partial one; 7 boards at 17 are one block pair
and one block, 8 at 18 a pair and two blocks (75 left-over tiles > 64).  The fp16 kernels have no tiles of the board: they find a
row's board point with float reciprocals of N and P and take a halo of N + 1 rows, which depends on N as well.
tests/test_trunk_probe.py::test_edge_defect_audit shows a lost corner point, one lost channel of it and a last row off by 1e-3
at >= 16 e_ref at sizes of both overhang classes."""
import functools

import numpy as np
import pytest

import alphago_jl_amd as ag
import orc
import trunk_probe as tp
from gpu_common import copy_weights_from_oracle

pytestmark = pytest.mark.gpu
L = orc.lib()
TOL = 1e-4
TOL16, TOLMIX = 5e-4, 1e-2            # test_gpu_nn16.py's two bars; printed against, not asserted, here
EXACT, SPLIT = 8.0, 32.0

FORMS = {
    "winograd": lambda e: None,                               # F(3x3,3x3) per layer up to 12x12, F(4x4,3x3) from 13x13
    "persistent": lambda e: e.set_tower_persistent(True),     # F(3x3,3x3) as one launch
    "five-pass": lambda e: e.set_winograd(3),
    "f33-dense": lambda e: e.set_winograd(2),                 # F(3x3,3x3) on densely packed tile blocks, 13x13 and up
    "direct": lambda e: e.set_winograd(0),
    "f32s": lambda e: e.set_precision("f32s"),
    "f16": lambda e: e.set_precision("f16"),
}
SMALL = ["winograd", "persistent", "five-pass", "direct", "f32s"]
PROBE_CASES = ([(9, 1, f) for f in SMALL] + [(9, 2, f) for f in SMALL + ["f16"]] + [(9, 10, "winograd"), (9, 10, "f32s")]
               + [(13, 2, f) for f in ("winograd", "f33-dense", "direct")]
               + [(19, 2, f) for f in ("winograd", "f33-dense", "direct", "f32s", "f16")])
LIVE_CASES = ([(9, 10, f) for f in SMALL + ["f16"]] + [(13, 2, f) for f in ("winograd", "f33-dense", "direct", "f32s", "f16")]
              + [(19, 2, f) for f in ("winograd", "f33-dense", "direct", "f32s", "f16")])


def forms_at(N):
    """Every tower form a board size has.  The engine refuses none of them at any size: the setters check their argument's
    range only, and the forward takes the form Net::tower_form() names -- persistent and five-pass exist up to 12 (whole-board
    tile blocks; persistent on a 256-CU device, which every MI355X is), F(3x3,3x3) on dense blocks is a form of its own from 13."""
    return SMALL + ["f16"] if N <= 12 else ["winograd", "f33-dense", "direct", "f32s", "f16"]


SIZES = sorted(tp.SIZE_BATCH)          # every size from 3 to 18 that the cases above do not visit
PROBE_CASES += [(N, 2, f) for N in SIZES for f in forms_at(N)]
LIVE_CASES += [(N, 2, f) for N in SIZES for f in ("winograd", "direct", "f32s", "f16")]


def _engine(N, tower, onet, form):
    eng = ag.Engine(board_size=N, games=1, tower_height=tower, num_readouts=8, max_nodes_per_game=16)
    copy_weights_from_oracle(eng, onet, tower)
    FORMS[form](eng)
    return eng


@functools.lru_cache(maxsize=None)
def _probe_ref(N, tower):
    """(onet, feats, ws, l64 [K, B, P], e_ref, l16 or None) of trunk_probe.CASES[(N, tower)], computed once"""
    onet, feats, ws = tp.make_case(N, tower)
    l64 = tp.oracle_probe(onet, feats, ws)
    e_ref = np.abs(tp.oracle_probe(onet, feats, ws, 32) - l64).max()
    l16 = tp.oracle_probe(onet, feats, ws, 16) if (N, tower, "f16") in PROBE_CASES else None
    for a in (feats, ws, l64):
        a.setflags(write=False)
    return onet, feats, ws, l64, e_ref, l16


@functools.lru_cache(maxsize=None)
def _live_ref(N, tower):
    """(onet after live_heads, feats, pi64, v64, pi16, v16)"""
    onet, feats, _ = tp.make_case(N, tower)
    tp.live_heads(onet, feats)
    pi64, v64 = tp.forward64(onet, feats)
    pi16, v16 = tp.forward_prec(onet, feats, 16)
    for a in (feats, pi64, v64):
        a.setflags(write=False)
    return onet, feats, pi64, v64, pi16, v16


def _gpu_probe(eng, N, feats, ws, shifts=(1, 2)):
    """probe logits [K, B, P] of the engine: K x (one set_weights of the policy conv + one forward_features); each read-out
    again with the batch starting `lo` rows later, which must not change a bit"""
    out = []
    for k, w in enumerate(ws):
        tp.set_probe(eng.set_weights, N, w, conv_only=k > 0)
        pi, _ = eng.forward_features(feats)
        assert np.isfinite(pi).all() and (pi > 0).all()
        for lo in shifts:
            spi, _ = eng.forward_features(feats[lo:])
            assert (spi == pi[lo:]).all(), (k, lo, np.argwhere(spi != pi[lo:])[:4])
        out.append(tp.probe_logits(pi))
    return np.stack(out)


def _where(err, N):
    k, b, p = np.unravel_index(np.argmax(err), err.shape)
    return f"worst at probe {k}, row {b}, point (i {p % N}, j {p // N})"


@pytest.mark.parametrize("N,tower,form", PROBE_CASES)
def test_trunk_probe_matches_float64(N, tower, form):
    onet, feats, ws, l64, e_ref, l16 = _probe_ref(N, tower)
    eng = _engine(N, tower, onet, form)
    lg = _gpu_probe(eng, N, feats, ws)
    eng.close()
    err = np.abs(lg - l64)
    e_gpu = err.max()
    tag = f"trunk probe ({N}, t{tower}, B {feats.shape[0]}) {form}:"
    if form == "f16":
        e_rest, e16 = np.abs(lg - l16).max(), np.abs(l16 - l64).max()
        print(f"{tag} e(gpu, fp16 restatement) {e_rest:.2e}, e(restatement, f64) {e16:.2e}, e(gpu, f64) {e_gpu:.2e}")
        assert e_rest <= e16, (e_rest, e16, _where(np.abs(lg - l16), N))
        return
    bar = SPLIT if form == "f32s" else EXACT
    print(f"{tag} e_gpu {e_gpu:.2e}, e_ref {e_ref:.2e}, ratio {e_gpu / e_ref:.2f} (bar {bar:.0f})")
    assert e_gpu <= bar * e_ref, (e_gpu, e_ref, e_gpu / e_ref, _where(err, N))


def test_trunk_probe_two_chains_19x19():
    """(19, t2, B 1400): the F(4x4,3x3) tower on two layer chains reads out bit for bit what one chain does, and both ends of
    the batch -- the first rows of the first chain, the last of the second -- meet the exact-f32 bar"""
    N, tower, B = 19, 2, 1400
    onet, feats, ws = tp.make_case(N, tower, B)
    rows = np.r_[0:3, B - 3:B]
    l64 = tp.oracle_probe(onet, feats[rows], ws)
    e_ref = np.abs(tp.oracle_probe(onet, feats[rows], ws, 32) - l64).max()
    eng = _engine(N, tower, onet, "winograd")
    eng.set_tower_streams(1)
    one = _gpu_probe(eng, N, feats, ws, shifts=())
    eng.set_tower_streams(2)
    two = _gpu_probe(eng, N, feats, ws)
    eng.close()
    L.or_net_free(onet)
    assert (one == two).all(), np.argwhere(one != two)[:4]
    err = np.abs(two[:, rows] - l64)
    print(f"trunk probe ({N}, t{tower}, B {B}) two chains: e_gpu {err.max():.2e}, e_ref {e_ref:.2e}, ratio {err.max() / e_ref:.2f} "
          f"(bar {EXACT:.0f})")
    assert err.max() <= EXACT * e_ref, (err.max(), e_ref, _where(err, N))


@pytest.mark.parametrize("N,tower,form", LIVE_CASES)
def test_live_heads_match_float64(N, tower, form):
    """pi and v on networks whose value plane and both policy planes are positive on half of their entries: the same 1e-4
    against float64 as everywhere, where v is no longer a constant and both halves of the policy FC are read"""
    onet, feats, pi64, v64, pi16, v16 = _live_ref(N, tower)
    eng = _engine(N, tower, onet, form)
    gpi, gv = eng.forward_features(feats)
    eng.close()
    dpi, dv = np.abs(gpi - pi64).max(), np.abs(gv - v64).max()
    tag = f"live heads ({N}, t{tower}, B {feats.shape[0]}) {form}:"
    assert np.isfinite(gpi).all() and np.isfinite(gv).all() and np.allclose(gpi.sum(1), 1, atol=1e-5)
    if form == "f16":
        d16 = max(np.abs(gpi - pi16).max(), np.abs(gv - v16).max())
        print(f"{tag} vs fp16 restatement {d16:.2e} (bar {TOL16:.0e}), vs f64 {max(dpi, dv):.2e} (bar {TOLMIX:.0e}); std v {v64.std():.3f}")
        return
    print(f"{tag} max|dpi| {dpi:.2e}, max|dv| {dv:.2e}; pi max {pi64.max():.3f}, std v {v64.std():.3f}")
    assert dpi <= TOL and dv <= TOL, (dpi, dv)

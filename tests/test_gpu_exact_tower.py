"""The HIP tower, the fp16 tower above all, held to the bit on integer-exact networks (tests/exact_nets.py).

On random weights the fp16 kernels (f32 sums) and their restatement (f64 sums) round values to half that differ in their last
bits, so every fp16 bar elsewhere (TOL16 of test_gpu_nn16.py, the f16 branch of test_gpu_trunk.py) has to let rounding flips
through, and a small structural defect passes with them.  Here every value a kernel rounds or stores is an integer that f32
and f64 both hold exactly: the kernel and the reference round the same number, the final trunk must be the same integers, and
any difference is a defect -- a tap, a halo row, a tile edge, the late flush of the LDS output image, the padded rows, the
rounding mode of a store, a double rounding.

Read-out: probe heads (tests/trunk_probe.py) with +-1 on a block of channels and the scale s, a power of two:
D = l / s = w.h is an integer.  One criterion everywhere: max |l_gpu / s - D_ref| < 0.25.  The cases, s and D_ref come from
tests/exact_nets.py (the oracle, on the CPU); nothing is measured on the device.  tests/test_exact_nets.py asserts, on the
references alone, the conditions under which this means something, and that a dropped weight, a truncating store, a double
rounding or a lost row each move some D_ref by >= 1.

  * family A (nothing rounds; towers 1, 2, 3, 5: every fp16 layer kind): `f16` and `direct` are the point, every other form
    valid at the board runs under the same criterion;
  * family B (halves are rounded, ties included, down to the last block): `f16` against oracle precision 16 at (9, t10) and
    (19, t3) -- and the `direct` f32 read-out of the same network differs, so the fp16 kernels produced it;
  * tile geometry of the persistent fp16 kernels (256-row and 224-row tiles) at their edges.

Family A at tower 2 runs at EVERY board size from 3 to 19 under every form the size has (test_gpu_trunk.forms_at; the batches of
trunk_probe.SIZE_BATCH fill one tile block of every form, leave a partial one and span two fp16 tiles), because the edge code of
every tower form depends on the size: T tiles a side, the boards a tile block holds, and the overhang, the points by which the
last tile hangs over the board edge --

                F(3x3,3x3)                        F(4x4,3x3), from 13
     N    T   boards per block   overhang    T   boards per block    overhang
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
    13    5   dense              2           4   4                   3
    14    5   dense              1           4   4                   2
    15    5   dense              0           4   4                   1
    16    6   dense              2           4   4                   0
    17    6   dense              1           5   5 per block pair    3
    18    6   dense              0           5   5 per block pair    2
    19    7   dense              2           5   5 per block pair    1

-- and because k_conv3x3_f16_w2 and k_conv3x3_f16_q find a row's board point with float reciprocals of N and P and mask their
taps by it: a quotient that is off by one at some size, or a tap mask wrong at an edge, changes an integer here."""
import numpy as np
import pytest

import alphago_jl_amd as ag
import exact_nets as en
import trunk_probe as tp
from gpu_common import copy_weights_from_oracle
from test_gpu_trunk import FORMS, SIZES, SMALL, _where, forms_at

pytestmark = pytest.mark.gpu
BAR = 0.25
LARGE = ["winograd", "f33-dense", "direct", "f32s", "f16"]
A_CASES = ([(n, f) for n in ("a-9-t1", "a-9-t2", "a-9-t3", "a-9-t5") for f in ["f16"] + SMALL]
           + [(n, f) for n in ("a-19-t2", "a-13-t2") for f in LARGE]
           + [(f"a-{N}-t2", f) for N in SIZES for f in forms_at(N)])


def _engine(N, tower, onet, form):
    eng = ag.Engine(board_size=N, games=1, tower_height=tower, num_readouts=8, max_nodes_per_game=16)
    copy_weights_from_oracle(eng, onet, tower)
    FORMS[form](eng)
    return eng


def _gpu_D(eng, N, feats, ws, s, alone=()):
    """l / s [K, B, P] of the engine; each row of `alone`, read as a batch of one, must give the same bits"""
    out = []
    for w in ws:
        tp.set_probe(eng.set_weights, N, w, s)
        pi, _ = eng.forward_features(feats)
        assert np.isfinite(pi).all() and (pi > 0).all()
        for b in alone:
            one, _ = eng.forward_features(feats[b:b + 1])
            assert (one[0] == pi[b]).all(), (b, np.argwhere(one[0] != pi[b])[:4])
        out.append(tp.probe_logits(pi) / s)
    return np.stack(out)


def _check(tag, Dg, D, N):
    err = np.abs(Dg - D)
    print(f"{tag}: max |l / s - D_ref| {err.max():.2e} (bar {BAR}), max |D_ref| {np.abs(D).max():.0f}")
    assert err.max() < BAR, (err.max(), _where(err, N), float(Dg.flat[np.argmax(err)]), float(D.flat[np.argmax(err)]))


@pytest.mark.parametrize("name,form", A_CASES)
def test_family_a_every_form_gives_the_integers(name, form):
    c = en.CASES[name]
    onet, feats, ws, s, D, _ = en.reference(name)
    eng = _engine(c["N"], c["tower"], onet, form)
    Dg = _gpu_D(eng, c["N"], feats, ws, s)
    eng.close()
    _check(f"exact A ({c['N']}, t{c['tower']}, B {c['B']}) {form}", Dg, D, c["N"])


@pytest.mark.parametrize("name", ["b-9-t10", "b-19-t3"])
def test_family_b_f16_rounds_as_the_restatement(name):
    c = en.CASES[name]
    N = c["N"]
    onet, feats, ws, s, D, D64 = en.reference(name)
    eng = _engine(N, c["tower"], onet, "f16")
    Dg = _gpu_D(eng, N, feats, ws, s)
    eng.set_precision("f32")
    eng.set_winograd(0)
    D32 = _gpu_D(eng, N, feats, ws, s)
    eng.close()
    moved = np.round(D32) != np.round(Dg)
    print(f"exact B ({N}, t{c['tower']}, B {c['B']}): direct f32 and f16 read-outs differ on {moved.mean():.2f} of the entries, "
          f"by up to {np.abs(D32 - Dg).max():.0f}; direct f32 against the float64 oracle {np.abs(D32 - D64).max():.2e}")
    _check(f"exact B ({N}, t{c['tower']}, B {c['B']}) f16", Dg, D, N)
    assert moved.any()                     # the fp16 kernels, not a fallback to f32, produced the read-out
    assert np.abs(D32 - D64).max() < BAR   # (and the f32 engine is the unrounded network)


@pytest.mark.parametrize("name", sorted(en.GEOMETRY))
def test_f16_tile_edges(name):
    """k_conv3x3_f16_q works on 256-row tiles, k_conv3x3_f16_w2 on 224-row tiles, workgroups are persistent: batches that end
    exactly on a tile and one row past it (4x4 x 14 / 15 and 16 / 17), 66,420 rows (9x9 x 820: more 256-row tiles than CUs,
    so some workgroups take a second tile and flush the previous tile's LDS image late), and the widest halo (16x16: 17
    rows).  D_ref on the first and last three boards and on the boards around the first multiple of each tile height and the
    first second tile; a row read alone gives the bits it gives in the full batch."""
    N, B = en.GEOMETRY[name]
    onet, feats, ws, s, boards, D, _ = en.geometry_reference(name)
    eng = _engine(N, en.GEOMETRY_TOWER, onet, "f16")
    Dg = _gpu_D(eng, N, feats, ws, s, alone=(0, int(boards[len(boards) // 2]), B - 1))
    eng.close()
    _check(f"exact tile edges ({N}, t{en.GEOMETRY_TOWER}, B {B}; boards {boards.tolist()}) f16", Dg[:, boards], D, N)

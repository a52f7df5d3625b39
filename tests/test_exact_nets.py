"""tests/exact_nets.py on the CPU: for every case of tests/test_gpu_exact_tower.py, the conditions under which its criterion
(|l_gpu / s - D_ref| < 0.25, D_ref an integer) means what it says, asserted on the references alone -- the float64 oracle, the
oracle's precisions 32 and 16, and a torch float64 restatement of the fp16 tower that returns every stored activation.  Then a
defect audit on that restatement: what a dropped weight, a wrong rounding mode, a double rounding and a lost board point do to
the integers the GPU test compares."""
import functools

import numpy as np
import pytest
import torch

import exact_nets as en
import orc
import trunk_probe as tp
from test_oracle_nn import get_param

L = orc.lib()
A_CASES = sorted(n for n, c in en.CASES.items() if c["family"] == "A")
B_CASES = sorted(n for n, c in en.CASES.items() if c["family"] == "B")


@functools.lru_cache(maxsize=None)
def _analysis(name):
    """the case (a geometry case on its reference boards), its restatement's stores and the read-outs of the three oracles"""
    if name in en.GEOMETRY:
        onet, feats, ws, s, boards, D, D64 = en.geometry_reference(name)
        feats, family, tower = feats[boards], "A", en.GEOMETRY_TOWER
    else:
        onet, feats, ws, s, D, D64 = en.reference(name)
        family, tower = en.CASES[name]["family"], en.CASES[name]["tower"]
    h, stored = en.torch_half_trunk(onet, tower, feats)
    Ds = {64: D64, 32: en.oracle_D(onet, feats, ws, s, 32), 16: en.oracle_D(onet, feats, ws, s, 16)}
    return dict(onet=onet, feats=feats, ws=ws, s=s, D=D, family=family, tower=tower, h=h, stored=stored, Ds=Ds)


def _sum_bound(onet, tower, stored):
    """an upper bound of every partial sum of every tower convolution, in any order: k max |input| + |shift| + max |residual|"""
    worst, by = 0.0, {(kind, blk): q for kind, blk, _, q in stored}
    for blk in range(tower):
        for l, x, res in ((1 + 2 * blk, by[("in", blk)], None), (2 + 2 * blk, by[("t", blk)], by[("in", blk)])):
            w = get_param(onet, l, orc.K_WEIGHT).reshape(256, -1)
            k = np.abs(w).sum(1).max()
            worst = max(worst, k * float(x.abs().max()) + 8 + (float(res.abs().max()) if res is not None else 0))
    return worst


@pytest.mark.parametrize("name", A_CASES + sorted(en.GEOMETRY))
def test_family_a_nothing_rounds(name):
    a = _analysis(name)
    for kind, blk, before, after in a["stored"]:
        x = before.numpy()
        assert (x == np.round(x)).all() and np.abs(x).max() <= en.HALF_INT, (kind, blk, np.abs(x).max())
        assert (before == after).all()
    Ds = a["Ds"]
    assert (np.round(Ds[16]) == np.round(Ds[64])).all() and (np.round(Ds[32]) == np.round(Ds[64])).all()
    assert (np.round(Ds[64]) == a["D"]).all() and (en.torch_D(a["h"], a["ws"]) == a["D"]).all()
    # precision 16 and precision 64 to the last bit the ABI returns (under the last probe, and the synthetic value head)
    pi16, v16 = tp.forward_prec(a["onet"], a["feats"], 16)
    pi64, v64 = tp.forward_prec(a["onet"], a["feats"], 64)
    assert (pi16 == pi64).all() and (v16 == v64).all()


@pytest.mark.parametrize("name", B_CASES)
def test_family_b_rounds_exactly(name):
    a = _analysis(name)
    tower = a["tower"]
    for kind, blk, before, after in a["stored"]:
        x = before.numpy()
        assert np.isfinite(x).all() and (x == np.round(x)).all(), (kind, blk)
        if kind != "out":
            assert np.abs(x).max() <= en.HALF_MAX, (kind, blk, np.abs(x).max())
        if blk == 0:
            assert np.abs(x).max() <= en.HALF_INT, (kind, blk, np.abs(x).max())
    bound = _sum_bound(a["onet"], tower, a["stored"])
    assert bound < 2 ** 24, bound
    counts = en.rounding_counts(a["stored"])
    for kind, blk, changed, ties, top in counts:
        print(f"{name} block {blk + 1} {kind:>3}: max {top:.0f}, rounded {changed}, exact ties {ties}")
    changed, ties = sum(c[2] for c in counts), sum(c[3] for c in counts)
    print(f"{name}: rounded {changed} (ties {ties}, others {changed - ties}); sums <= {bound:.0f}")
    assert changed >= 1000 and ties >= 50 and changed - ties >= 50, (changed, ties)
    Ds = a["Ds"]
    differ = np.round(Ds[16]) != np.round(Ds[64])
    print(f"{name}: rounding moves {differ.mean():.2f} of the read-out, by up to {np.abs(Ds[16] - Ds[64]).max():.0f}")
    assert differ.any()
    assert (np.round(Ds[16]) == a["D"]).all()
    Dt = en.torch_D(a["h"], a["ws"])
    assert (Dt == a["D"]).all(), np.argwhere(Dt != a["D"])[:4]


@pytest.mark.parametrize("name", sorted(en.CASES) + sorted(en.GEOMETRY))
def test_networks_are_live_and_resolved(name):
    a = _analysis(name)
    for kind, blk, _, after in a["stored"]:
        share = float((after != 0).double().mean())
        assert share >= 0.25, (kind, blk, share)
    for l in range(1, 1 + 2 * a["tower"]):
        w = get_param(a["onet"], l, orc.K_WEIGHT).reshape(256, 8, 32, 3, 3)            # [cout, cin chunk, cin, b, a]
        assert set(np.unique(w)) == {-1.0, 0.0, 1.0}
        assert (np.abs(w).sum((0, 2)) > 0).all(), l                                      # every (cin chunk, tap)
    assert (np.abs(a["ws"]).sum(0) == 1).all()                                          # the probes touch every channel once
    # the resolution: s is a power of two, |l_ref| <= 8, and 64 times the f32 heads' own error (the trunk is exact in f32
    # too, so oracle precision 32 against float64 is the heads and nothing else) still fits under s
    s, Ds = a["s"], a["Ds"]
    ref = Ds[16] if a["family"] == "B" else Ds[64]
    e_head = np.abs(Ds[32] - Ds[64]).max() * s
    print(f"{name}: s 2^{int(np.log2(s))}, max |D_ref| {np.abs(a['D']).max():.0f}, max |l_ref| {np.abs(ref).max() * s:.2f}, "
          f"e_head {e_head:.2e} = s / {s / e_head:.0f}")
    assert np.log2(s) == int(np.log2(s))
    assert np.abs(ref).max() * s <= en.L_MAX
    assert np.abs(ref - a["D"]).max() < 1 / 64
    assert s >= 64 * e_head, (s, e_head)


def _nonzero_weight(w, rng):
    o = int(rng.randint(256))
    ci, b, a_ = np.argwhere(w[o] != 0)[0]
    return o, int(ci), int(b), int(a_)


@pytest.mark.parametrize("name", ["a-9-t3", "a-19-t2", "b-9-t10", "b-19-t3"])
def test_defect_audit_on_the_restatement(name):
    """Each defect, put into the torch restatement alone, changes some D_ref by at least 1 -- four times the 0.25 of the GPU
    criterion.  A wrong rounding mode and a double rounding exist only where something rounds: family B.  A single weight
    is a defect of the function only if its output channel is alive and read by a later layer (with 4 weights per output
    channel some are not): it is drawn, seeded, until the read-out moves at all, in at most 16 draws; then the bar applies."""
    c = en.CASES[name]
    N, tower = c["N"], c["tower"]
    onet, feats, ws = en.build_case(name)
    D0 = en.torch_D(en.torch_half_trunk(onet, tower, feats)[0], ws)
    assert (D0 == en.reference(name)[4]).all()
    rng = np.random.RandomState(c["seed"])
    set_fn = tp.oracle_setter(onet)
    moved = {}

    def with_weights(layer, w1):
        set_fn(layer, orc.K_WEIGHT, w1)
        return en.torch_D(en.torch_half_trunk(onet, tower, feats)[0], ws)

    for layer in (1, 2 * tower):
        w = get_param(onet, layer, orc.K_WEIGHT).reshape(256, 256, 3, 3)
        for draw in range(16):
            at = _nonzero_weight(w, rng)
            w1 = w.copy()
            w1[at] = 0
            D = with_weights(layer, w1)
            if (D != D0).any():
                break
        moved[f"one weight of layer {layer} dropped (draw {draw + 1})"] = D
        w1 = w.copy()
        w1[:, :, at[2], at[3]] = 0
        moved[f"one tap of layer {layer} dropped"] = with_weights(layer, w1)
        set_fn(layer, orc.K_WEIGHT, w)
    last = tower - 1

    def lost_point(kind, blk, before, after):
        if (kind, blk) == ("t", last):
            after = after.clone()
            after[1, :, N - 1, N - 1] = 0                       # board 1's last point: the last row of its tile image
        return after

    def truncated(kind, blk, before, after):
        return en.to_half_trunc(before) if (kind, blk) == ("t", last) else after

    def double_rounding(kind, blk, before, after):
        return en.to_half(before) if kind == "out" else after

    defects = {"board 1's last point zeroed in the last block's t": lost_point}
    if c["family"] == "B":
        defects["the last block's t truncated, not rounded to nearest even"] = truncated
        defects["the last block's f32 output rounded to half"] = double_rounding
    for what, defect in defects.items():
        moved[what] = en.torch_D(en.torch_half_trunk(onet, tower, feats, defect)[0], ws)
    L.or_net_free(onet)
    for what, D in moved.items():
        d = np.abs(D - D0)
        print(f"{name}: {what}: moves {np.mean(d >= 1):.4f} of the read-out ({int((d >= 1).sum())} entries), by up to {d.max():.0f}")
        assert d.max() >= 1, what

"""tests/trunk_probe.py on the CPU: the probe head reads the trunk exactly, `live_heads` gives networks whose heads see the
tower, and the bar of tests/test_gpu_trunk.py is far below what a defect in a tower weight tensor, or in an activation at a
board edge, does to the read-out."""
import functools

import numpy as np
import pytest
import torch

import orc
import trunk_probe as tp
from test_oracle_nn import get_param, randomize_bn, torch_trunk

L = orc.lib()


@pytest.mark.parametrize("N,tower", [(5, 1), (9, 2)])
def test_probe_reads_the_torch_trunk(N, tower):
    """log pi[p] - log pi[pass] of the float64 oracle under the probe head == w.h of an independent float64 trunk"""
    rng = np.random.RandomState(10 * N + tower)
    P, B = N * N, 3
    net = L.or_net_new(N, tower)
    L.or_net_init_synthetic(net, 5)
    randomize_bn(net, list(range(0, 1 + 2 * tower)) + [orc.L_VALUE_CONV, orc.L_POLICY_CONV], rng)
    feats = tp.make_feats(rng, B, N)
    ws = (rng.randn(2, 256) / 16).astype(np.float32)
    pi_before = tp.forward64(net, feats)[0]
    got = tp.oracle_probe(net, feats, ws)
    x_bcij = feats.reshape(B, 17, N, N).transpose(0, 1, 3, 2)          # feats index i + N * (j + N * c)
    h = torch_trunk(net, tower, np.ascontiguousarray(x_bcij, np.float64))
    for k, w in enumerate(ws):
        want = torch.einsum("c,bcij->bji", torch.tensor(w, dtype=torch.float64), h).reshape(B, P).numpy()   # p = i + N * j
        assert np.abs(want).max() > 0.05                                # the functional is not trivially zero
        assert np.abs(got[k] - want).max() < 1e-12, (k, np.abs(got[k] - want).max())
    # a scale on the policy FC scales the read-out; the heads come back as they were
    with tp.saved_heads(net):
        tp.set_probe(tp.oracle_setter(net), N, ws[0], s=3.0)
        l3 = tp.probe_logits(tp.forward64(net, feats)[0])
    assert np.abs(l3 - 3 * got[0]).max() < 1e-12
    assert (tp.forward64(net, feats)[0] == pi_before).all()
    L.or_net_free(net)


@pytest.mark.parametrize("N,tower", sorted(tp.CASES))
def test_live_heads_conditions(N, tower):
    """every network of tests/test_gpu_trunk.py: after live_heads each head plane is positive on 20 % .. 80 % of its entries and
    v varies over the batch (before it, at the deeper shapes, v is one constant)"""
    onet, feats, ws = tp.make_case(N, tower)
    v_before = tp.forward64(onet, feats)[1]
    live = tp.live_heads(onet, feats)
    pi, v = tp.forward64(onet, feats)
    print(f"({N}, t{tower}, B {feats.shape[0]}): live {live}, std v {v_before.std():.4f} -> {v.std():.4f}, pi max {pi.max():.3f}")
    assert all(0.2 <= f <= 0.8 for f in live), live
    assert v.std() >= 0.02, v.std()
    # the same through the network itself: each plane's BatchNorm output, read back through the probe, has both signs
    for (l, i), f in zip(tp.head_planes(onet), live):
        w = get_param(onet, l, orc.K_WEIGHT).reshape(-1, 256)[i]
        d = tp.oracle_probe(onet, feats, w[None])[0]
        pre = d + float(get_param(onet, l, orc.K_BIAS)[i]) - float(get_param(onet, l, orc.K_BN_MEAN)[i])
        assert abs(np.mean(pre > 0) - f) < 1e-12 and get_param(onet, l, orc.K_BN_BETA)[i] == 0
    L.or_net_free(onet)


TAP = (2, 1)


def _live_pair(onet, layer, feats, ws, l64, rng):
    """A seeded (cout, cin) draw on which the network's function depends at all.  BatchNorm-randomised synthetic networks have
    channels that are zero behind their ReLU on every input; a weight between two of those is no defect of the function, and
    zeroing it moves the float64 read-out by exactly 0.  Decided on the float64 oracle with one probe, before any bar."""
    set_fn = tp.oracle_setter(onet)
    w0 = get_param(onet, layer, orc.K_WEIGHT)
    try:
        for _ in range(16):
            o, ci = int(rng.randint(256)), int(rng.randint(256))
            w = w0.copy().reshape(256, 256, 3, 3)
            w[(o, ci) + TAP] = 0
            set_fn(layer, orc.K_WEIGHT, w)
            if (tp.oracle_probe(onet, feats, ws[:1]) != l64[:1]).any():
                return o, ci
    finally:
        set_fn(layer, orc.K_WEIGHT, w0)
    raise AssertionError("no live (cout, cin) pair in 16 draws")


def _defects(o, ci, rng):
    """name -> function on a tower conv weight tensor [cout, cin, 3, 3]"""
    noise = rng.randn(256, 256, 3, 3).astype(np.float32)

    def corner(w):
        w[o, :, 0, 0] = 0

    def tf32_noise(w):
        w *= 1 + np.float32(1e-3) * noise

    def one_pair_tap(w):
        w[(o, ci) + TAP] = 0

    return {"corner tap of one cout": corner, "weights x (1 + 1e-3 noise)": tf32_noise, "one tap of one (cout, cin)": one_pair_tap}


@functools.lru_cache(maxsize=None)
def _audit_reference(N, tower):
    onet, feats, ws = tp.make_case(N, tower)
    l64 = tp.oracle_probe(onet, feats, ws)
    e_ref = np.abs(tp.oracle_probe(onet, feats, ws, 32) - l64).max()
    pi64 = tp.forward64(onet, feats)[0]
    return onet, feats, ws, l64, e_ref, pi64


@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("N,tower", [(9, 2), (19, 2)])
def test_defect_audit(N, tower, which):
    """Each defect of a tower conv weight tensor, in layer 1 and in the last layer, moves the float64 probe read-out by at
    least 16 e_ref -- twice the exact-f32 bar of tests/test_gpu_trunk.py (e_ref: the direct-f32 oracle against float64 over
    the same probes).  What it does to pi on the ordinary heads is printed: that is what the 1e-4 bar of the pi / v tests sees."""
    onet, feats, ws, l64, e_ref, pi64 = _audit_reference(N, tower)
    layer = 1 if which == "first" else 2 * tower
    rng = np.random.RandomState(1000 * N + layer)
    w0 = get_param(onet, layer, orc.K_WEIGHT)
    set_fn = tp.oracle_setter(onet)
    o, ci = _live_pair(onet, layer, feats, ws, l64, rng)
    try:
        for name, apply in _defects(o, ci, rng).items():
            w = w0.copy().reshape(256, 256, 3, 3)
            apply(w)
            set_fn(layer, orc.K_WEIGHT, w)
            moved = np.abs(tp.oracle_probe(onet, feats, ws) - l64).max()
            dpi = np.abs(tp.forward64(onet, feats)[0] - pi64).max()
            print(f"({N}, t{tower}) layer {layer}, {name}: probe moves {moved:.2e} = {moved / e_ref:.0f} e_ref "
                  f"(e_ref {e_ref:.2e}); ordinary heads |dpi| {dpi:.2e}")
            assert moved >= 16 * e_ref, (name, moved, e_ref)
    finally:
        set_fn(layer, orc.K_WEIGHT, w0)


def _edge_defects(N, c):
    """name -> function on the first block's t [B, 256, i, j], in place.  What a tower kernel gets wrong at a board edge: a
    tile that hangs over the edge and is cut one point short, one channel of it, a last row that comes from the wrong place."""
    def corner(t):
        t[1, :, N - 1, N - 1] = 0

    def corner_channel(t):
        t[1, c, N - 1, N - 1] = 0

    def last_row(t):
        t[1, :, N - 1, :] *= 1 - 1e-3

    return {"board 1's corner point zeroed": corner, f"channel {c} of board 1's corner point zeroed": corner_channel,
            "board 1's last row x (1 - 1e-3)": last_row}


@pytest.mark.parametrize("N", [3, 4, 5, 8, 11, 14, 17])
def test_edge_defect_audit(N):
    """Sizes of both overhang classes (tests/test_gpu_trunk.py has the table), on the network, features and probes of the GPU
    case.  An independent float64 trunk (torch) gives the oracle's probe read-out; then each defect at the board edge, put
    into the first block's t of that trunk, moves the read-out by at least 16 e_ref, as the weight defects above do.  The
    channel is a seeded draw among those alive at the corner point."""
    tower = 2
    onet, feats, ws, l64, e_ref, _ = _audit_reference(N, tower)
    B, P = feats.shape[0], N * N
    x_bcij = np.ascontiguousarray(feats.reshape(B, 17, N, N).transpose(0, 1, 3, 2), np.float64)
    wt = torch.tensor(ws, dtype=torch.float64)

    def read_out(defect=None):
        def store(kind, blk, a):
            if defect is not None and (kind, blk) == ("t", 0):
                a = a.clone()
                defect(a)
            return a
        return torch.einsum("kc,bcij->kbji", wt, torch_trunk(onet, tower, x_bcij, store=store)).reshape(len(ws), B, P).numpy()

    seen = {}
    read_out(lambda t: seen.update(t=t.clone()))
    alive = np.flatnonzero(seen["t"][1, :, N - 1, N - 1].numpy() > 0)
    assert alive.size >= 16, alive.size
    c = int(alive[np.random.RandomState(1000 * N).randint(alive.size)])
    clean = np.abs(read_out() - l64).max()
    print(f"({N}, t{tower}) torch trunk against the oracle's probe: {clean:.1e}; {alive.size} channels alive at the corner")
    assert clean < 1e-12, clean
    for name, defect in _edge_defects(N, c).items():
        moved = np.abs(read_out(defect) - l64).max()
        print(f"({N}, t{tower}) first block's t, {name}: probe moves {moved:.2e} = {moved / e_ref:.0f} e_ref (e_ref {e_ref:.2e})")
        assert moved >= 16 * e_ref, (name, moved, e_ref)

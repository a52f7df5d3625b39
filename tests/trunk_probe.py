"""Reading the trunk through the network's own ABI.

The parity tests of the forward compare pi and v.  On `or_net_init_synthetic` + `randomize_bn` networks the value conv is
negative before its ReLU at every point of every board at the deeper shapes (v is one constant), one policy-conv plane is dead
as well, and the live plane sits behind a flat softmax (pi max 0.02 .. 0.1): a tower defect moves pi by 1e-6 .. 1e-5 and v by
nothing.  Two tools close that, with no new entry point:

  * a PROBE HEAD.  Policy conv: plane 0 = w, plane 1 = -w, BatchNorm the identity (bias 0, beta 0, gamma 1, mean 0, var 1,
    eps 0).  Policy FC (`[in, out]`, in = p + P * plane): fc[p, p] = s, fc[P + p, p] = -s, the pass column and the bias zero.
    Then relu(w.h) - relu(-w.h) = w.h and

        log pi[p] - log pi[pass] = s * sum_c w[c] * h[c, p]:

    one forward reads one linear functional of the final trunk h at every board point.  The heads are plain f32 in every
    tower form, so the read-out costs a few f32 ulps of a 256-term dot product and of one exp / log pair.

  * LIVE HEADS.  `live_heads` reads the three head planes' own conv.h through the probe on the float64 oracle and centres
    each plane's BatchNorm on the median of what it sees (mean = median + bias, beta = 0): every plane is then positive on
    about half of its entries, v varies over the batch, and both heads see the tower.

CPU only: numpy and the oracle.  The GPU tests pass `Engine.set_weights` as the setter."""
import ctypes as C

import numpy as np

import orc
from test_oracle_nn import get_param, randomize_bn

L = orc.lib()
K_PROBES = 4
CONV_KINDS = (orc.K_WEIGHT, orc.K_BIAS, orc.K_BN_BETA, orc.K_BN_GAMMA, orc.K_BN_MEAN, orc.K_BN_VAR, orc.K_BN_EPS)

# (N, tower) -> (batch, seed of the BatchNorm statistics, the features and the probes).  The seeds are chosen so that the
# conditions of tests/test_trunk_probe.py::test_live_heads_conditions hold; that test asserts them for every entry.
CASES = {(9, 1): (9, 91), (9, 2): (9, 29), (9, 10): (9, 100), (13, 2): (9, 132), (19, 2): (7, 192)}
# Every other board size, tower 2.  The batch fills at least one tile block of every tower form (64, 16, 7 and 4 boards for
# T = 1 .. 4 tiles a side, 4 at 13 .. 16, 5 per block pair from 17), leaves a partial last block and spans two of the fp16
# kernels' 224- / 256-row tiles (tests/test_gpu_trunk.py has the size classes).  The seed is 10 N + 2 except at 3 and 5,
# where that one leaves std v at 0.014 and 0.010 under the 0.02 of test_live_heads_conditions.
SIZE_BATCH = {3: 70, 4: 19, 5: 19, 6: 19, 7: 9, 8: 9, 10: 9, 11: 9, 12: 9, 14: 6, 15: 6, 16: 5, 17: 7, 18: 8}
SIZE_SEED = {3: 1032, 5: 1052}
CASES.update({(N, 2): (B, SIZE_SEED.get(N, 10 * N + 2)) for N, B in SIZE_BATCH.items()})


def oracle_setter(onet):
    def set_fn(layer, kind, a):
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        assert L.or_net_set(onet, layer, kind, orc.fptr(a), a.size) == orc.OK
    return set_fn


def set_probe(set_fn, N, w, s=1.0, conv_only=False):
    """Write the probe head for the functional w [256] through set_fn(layer, kind, array).  conv_only: the rest of the probe
    head is already in place and only w changes (one set call)."""
    P = N * N
    w = np.asarray(w, np.float32).reshape(256)
    set_fn(orc.L_POLICY_CONV, orc.K_WEIGHT, np.stack([w, -w]).reshape(-1))
    if conv_only:
        return
    for kind, val, n in ((orc.K_BIAS, 0, 2), (orc.K_BN_BETA, 0, 2), (orc.K_BN_GAMMA, 1, 2), (orc.K_BN_MEAN, 0, 2),
                         (orc.K_BN_VAR, 1, 2), (orc.K_BN_EPS, 0, 1)):
        set_fn(orc.L_POLICY_CONV, kind, np.full(n, val, np.float32))
    fc = np.zeros((2 * P, P + 1), np.float32)
    idx = np.arange(P)
    fc[idx, idx] = s
    fc[P + idx, idx] = -s
    set_fn(orc.L_POLICY_FC, orc.K_WEIGHT, fc.reshape(-1))
    set_fn(orc.L_POLICY_FC, orc.K_BIAS, np.zeros(P + 1, np.float32))


def probe_logits(pi):
    """pi [B, P + 1] -> log pi[:, :P] - log pi[:, P:] in float64: s * w.h at every board point"""
    pi = np.asarray(pi, np.float64)
    return np.log(pi[:, :-1]) - np.log(pi[:, -1:])


def forward64(onet, feats):
    B, A = feats.shape[0], feats.shape[1] // 17 + 1
    pi, v = np.zeros((B, A)), np.zeros(B)
    x = np.ascontiguousarray(feats, np.float64)
    dp = C.POINTER(C.c_double)
    L.or_net_forward_feats_f64(onet, x.ctypes.data_as(dp), B, pi.ctypes.data_as(dp), v.ctypes.data_as(dp))
    return pi, v


def forward_prec(onet, feats, precision):
    """the oracle in float arithmetic: 32 = direct f32, 16 = the restatement of the fp16 tower"""
    B, A = feats.shape[0], feats.shape[1] // 17 + 1
    pi, v = np.zeros((B, A), np.float32), np.zeros(B, np.float32)
    x = np.ascontiguousarray(feats, np.float32)
    L.or_net_forward_feats(onet, orc.fptr(x), B, orc.fptr(pi), orc.fptr(v), precision)
    return pi, v


class saved_heads:
    """the policy conv and the policy FC of an oracle network, put back on exit"""

    def __init__(self, onet):
        self.onet = onet

    def __enter__(self):
        self.kept = [(orc.L_POLICY_CONV, k, get_param(self.onet, orc.L_POLICY_CONV, k)) for k in CONV_KINDS]
        self.kept += [(orc.L_POLICY_FC, k, get_param(self.onet, orc.L_POLICY_FC, k)) for k in (orc.K_WEIGHT, orc.K_BIAS)]
        return self

    def __exit__(self, *exc):
        set_fn = oracle_setter(self.onet)
        for l, k, a in self.kept:
            set_fn(l, k, a)


def head_planes(onet):
    """[(layer, plane index within the layer)] of the three head planes"""
    return [(orc.L_VALUE_CONV, 0), (orc.L_POLICY_CONV, 0), (orc.L_POLICY_CONV, 1)]


def live_heads(onet, feats):
    """Centre the BatchNorm of the value-conv plane and of the two policy-conv planes on the median of their own conv.h over
    feats (read through the probe on the float64 oracle).  Returns the fraction of entries on which each plane is positive
    after that, in the order of head_planes()."""
    N = int(round((feats.shape[1] // 17) ** 0.5))
    set_fn = oracle_setter(onet)
    planes = head_planes(onet)
    ws = [get_param(onet, l, orc.K_WEIGHT).reshape(-1, 256)[i].copy() for l, i in planes]
    with saved_heads(onet):
        dots = []
        for k, w in enumerate(ws):
            set_probe(set_fn, N, w, conv_only=k > 0)
            dots.append(probe_logits(forward64(onet, feats)[0]))
    live = []
    for (l, i), d in zip(planes, dots):
        bias, beta, mean = (get_param(onet, l, k) for k in (orc.K_BIAS, orc.K_BN_BETA, orc.K_BN_MEAN))
        mean[i] = np.float32(np.median(d) + bias[i])
        beta[i] = 0
        set_fn(l, orc.K_BN_MEAN, mean)
        set_fn(l, orc.K_BN_BETA, beta)
        gamma = get_param(onet, l, orc.K_BN_GAMMA)[i]
        live.append(float(np.mean(gamma * (d + np.float64(bias[i]) - np.float64(mean[i])) > 0)))
    return live


def make_feats(rng, B, N):
    """as test_every_tiling_class_of_the_winograd_tower: 16 binary stone planes and a +-1 colour plane"""
    feats = (rng.rand(B, 17 * N * N) < 0.3).astype(np.float32)
    feats[:, 16 * N * N:] = np.where(rng.rand(B, 1) < 0.5, 1.0, -1.0)
    return feats


def make_case(N, tower, B=None):
    """The network, features and probes of CASES[(N, tower)]: (onet, feats [B, 17 P], ws [K, 256]).  The caller frees onet."""
    B0, seed = CASES[(N, tower)]
    rng = np.random.RandomState(seed)
    onet = L.or_net_new(N, tower)
    L.or_net_init_synthetic(onet, 3)
    randomize_bn(onet, list(range(0, 1 + 2 * tower)) + [orc.L_VALUE_CONV, orc.L_POLICY_CONV], rng)
    ws = (rng.randn(K_PROBES, 256) / 16).astype(np.float32)
    feats = make_feats(rng, B0 if B is None else B, N)
    return onet, feats, ws


def oracle_probe(onet, feats, ws, precision=64):
    """probe logits [K, B, P] of the oracle (64: float64; 32, 16: or_net_forward_feats); the oracle's heads are put back"""
    N = int(round((feats.shape[1] // 17) ** 0.5))
    set_fn = oracle_setter(onet)
    out = []
    with saved_heads(onet):
        for k, w in enumerate(ws):
            set_probe(set_fn, N, w, conv_only=k > 0)
            pi = forward64(onet, feats)[0] if precision == 64 else forward_prec(onet, feats, precision)[0]
            out.append(probe_logits(pi))
    return np.stack(out)

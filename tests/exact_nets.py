"""Integer-exact networks: every value the tower rounds or stores is an integer that f32 and f64 both hold exactly.

On random weights the fp16 tower (f32 sums) and its restatement (oracle precision 16, f64 sums) round values to half that differ
in their last bits, so now and then they round to different halves; every fp16 bar has to be wide enough for that, and a small
structural defect passes under it.  Here the two round THE SAME number, so the trunk must agree exactly at any depth:

  * features: `trunk_probe.make_feats` (16 binary planes, a +-1 colour plane);
  * every 3x3 convolution: `k` weights of +-1 per output channel at random (tap, cin) places, 0 elsewhere (exact in half);
  * BatchNorm: gamma 1, var 1, eps 0, and bias, mean, beta small integers -- it folds to scale 1 and an integer shift;
  * the value head as `or_net_init_synthetic` leaves it; the policy head is the probe of tests/trunk_probe.py.

Family A ("no rounding"): every stored activation is an integer of at most 2048: nothing rounds, every tower form computes
the same integers.  Family B ("exact rounding"): stored activations grow past 2048 (but stay within half's range, and every
sum below 2^24), so halves are rounded, ties included -- of one and the same number in f32 and in f64.
Block 1 stays at or under 2048 in family B too: the device's f32 stem is a Winograd convolution whose roundoff (1e-7 beside
an integer) the first half stores snap away, and it must meet no tie before they have.

Read-out: probe k has +-1 on its own 256 / K channels, the policy FC scales by s, a power of two: D = l / s is the integer
w.h.  s comes from the reference alone: the largest power of two with max |l_ref| <= 8 (tests/test_exact_nets.py asserts
that and s >= 64 e_head, e_head the f32 heads' own error on this network).

CPU only: numpy, torch and the oracle."""
import functools

import numpy as np
import torch

import orc
import trunk_probe as tp
from test_oracle_nn import torch_trunk

L = orc.lib()
HALF_INT = 2048                 # integers up to here are halves
HALF_MAX = 32768                # the bound of family B on a stored activation (half's largest finite value is 65504)
S0 = 2.0 ** -20                 # the scale at which the float64 oracle reads D before s is chosen
L_MAX = 8.0

# name -> family, N, tower, B, seed, probes, and the builder's k_tower / shift where they differ from the defaults.
# tests/test_exact_nets.py asserts for every entry the conditions under which tests/test_gpu_exact_tower.py means something.
CASES = {
    "a-9-t1": dict(family="A", N=9, tower=1, B=9, seed=11, probes=8),
    "a-9-t2": dict(family="A", N=9, tower=2, B=9, seed=12, probes=8),
    "a-9-t3": dict(family="A", N=9, tower=3, B=9, seed=13, probes=8),
    "a-9-t5": dict(family="A", N=9, tower=5, B=9, seed=15, probes=8),
    "a-19-t2": dict(family="A", N=19, tower=2, B=3, seed=192, probes=8),
    "a-13-t2": dict(family="A", N=13, tower=2, B=5, seed=132, probes=8),
    "b-9-t10": dict(family="B", N=9, tower=10, B=3, seed=910, probes=16),
    "b-19-t3": dict(family="B", N=19, tower=3, B=2, seed=193, probes=16, k_tower=(24, 24, 48, 48, 48, 4)),
}
# every other board size (family A, tower 2): the batches of trunk_probe.SIZE_BATCH, the geometry cases' shift, seed 500 + N
CASES.update({f"a-{N}-t2": dict(family="A", N=N, tower=2, B=B, seed=500 + N, probes=8, shift=(-2, 1))
              for N, B in tp.SIZE_BATCH.items()})
# tile geometry (family A, tower 3): name -> N, B; D_ref is taken on `geometry_boards` only
GEOMETRY = {"g-4-14": (4, 14), "g-4-15": (4, 15), "g-4-16": (4, 16), "g-4-17": (4, 17), "g-9-820": (9, 820), "g-16-8": (16, 8)}
GEOMETRY_TOWER, GEOMETRY_SEED, GEOMETRY_SHIFT = 3, 77, (-2, 1)    # (the shift: >= 25 % alive on a 4x4 board too)
GEOMETRY_PROBES = {"g-9-820": 4}
TILE_ROWS = (224, 256)          # k_conv3x3_f16_w2's and k_conv3x3_f16_q's tiles
CUS = 256                       # persistent workgroups: tile CUS is the first that is some workgroup's second


def sparse_pm1(rng, cin, k):
    """[256, cin, 3, 3]: per output channel k weights of +-1 at distinct random (cin, tap) places"""
    w = np.zeros((256, cin * 9), np.float32)
    order = rng.rand(256, cin * 9)
    if cin == 256:      # output channel o has a weight at tap o % 9 in cin chunk (o // 9) % 8: every (tap, chunk) is used
        o = np.arange(256)
        order[o, (32 * ((o // 9) % 8) + rng.randint(32, size=256)) * 9 + o % 9] = -1
    at = np.argsort(order, axis=1)[:, :k]
    w[np.arange(256)[:, None], at] = np.where(rng.rand(256, k) < 0.5, -1.0, 1.0)
    return w.reshape(256, cin, 3, 3)


def make_exact(N, tower, seed, B, k_stem=24, k_tower=4, shift=(-3, 1)):
    """(onet, feats [B, 17 P]); deterministic from the seed.  k_tower: one count, or one per tower layer.  The caller frees
    onet.  The policy head is whatever or_net_init_synthetic made until a probe is set."""
    rng = np.random.RandomState(seed)
    onet = L.or_net_new(N, tower)
    L.or_net_init_synthetic(onet, 3)
    set_fn = tp.oracle_setter(onet)
    ks = [k_stem] + (list(k_tower) if np.ndim(k_tower) else [k_tower] * (2 * tower))
    assert len(ks) == 1 + 2 * tower
    for l, k in enumerate(ks):
        set_fn(l, orc.K_WEIGHT, sparse_pm1(rng, 17 if l == 0 else 256, k))
        sh = rng.randint(shift[0], shift[1] + 1, 256)
        bias, beta = rng.randint(-2, 3, 256), rng.randint(-2, 3, 256)
        for kind, a in ((orc.K_BIAS, bias), (orc.K_BN_BETA, beta), (orc.K_BN_MEAN, bias + beta - sh),
                        (orc.K_BN_GAMMA, np.ones(256)), (orc.K_BN_VAR, np.ones(256)), (orc.K_BN_EPS, np.zeros(1))):
            set_fn(l, kind, a)
    return onet, tp.make_feats(rng, B, N)


def make_probes(K, seed):
    """ws [K, 256]: probe k is +-1 on channels k * 256 / K .. and 0 elsewhere; K = 8 is one probe per 32-channel cout block
    of the fp16 kernels.  Together the probes touch every channel."""
    rng = np.random.RandomState(seed + 1000)
    ws = np.zeros((K, 256), np.float32)
    n = 256 // K
    for k in range(K):
        ws[k, k * n:(k + 1) * n] = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    return ws


# ------------------------------------------------------------------------------------------- the torch restatement

def to_half(a):
    """round to nearest even, as the fp16 tower's stores and the oracle's quant_h"""
    return a.to(torch.float16).to(torch.float64)


def to_half_trunc(a):
    """round toward zero: a wrong rounding mode, for the defect audit"""
    q = a.to(torch.float16).numpy()
    up = np.abs(q.astype(np.float64)) > np.abs(a.numpy())
    return torch.tensor(np.where(up, np.nextafter(q, np.float16(0)), q).astype(np.float64))


def x_bcij(feats, N):
    """feats [B, 17 P] (index i + N * (j + N * c)) -> [B, 17, i, j] float64"""
    return np.ascontiguousarray(feats.reshape(-1, 17, N, N).transpose(0, 1, 3, 2), np.float64)


def torch_half_trunk(onet, tower, feats, defect=None):
    """The fp16 tower restated on torch float64: `.to(torch.float16)` at the oracle's three rounding points (the block input on
    load, t, the block output except the last).  Returns (h [B, 256, i, j], stored): stored is a list of
    (kind, blk, value before the store, value after).  defect(kind, blk, before, after) -> after', if given, replaces a store."""
    N = int(round((feats.shape[1] // 17) ** 0.5))
    stored = []

    def store(kind, blk, a):
        q = a if kind == "out" else to_half(a)
        if defect is not None:
            q = defect(kind, blk, a, q)
        stored.append((kind, blk, a, q))
        return q

    h = torch_trunk(onet, tower, x_bcij(feats, N), store=store)
    return h, stored


def torch_D(h, ws):
    """D [K, B, P] = w.h at every board point, p = i + N * j"""
    B = h.shape[0]
    return torch.einsum("kc,bcij->kbji", torch.tensor(ws, dtype=torch.float64), h).reshape(len(ws), B, -1).numpy()


def rounding_counts(stored):
    """per store: (kind, blk, elements the store changed, exact ties among them, max |after|)"""
    out = []
    for kind, blk, a, q in stored:
        a, q = a.numpy(), q.numpy()
        changed = a != q
        h = q.astype(np.float16)
        other = np.where(a > q, np.nextafter(h, np.float16(np.inf)), np.nextafter(h, np.float16(-np.inf))).astype(np.float64)
        ties = changed & (np.abs(a - q) == np.abs(other - a))
        out.append((kind, blk, int(changed.sum()), int(ties.sum()), float(np.abs(q).max())))
    return out


# ------------------------------------------------------------------------------------------- the reference read-out

def oracle_D(onet, feats, ws, s, precision=64):
    """l / s [K, B, P] of the oracle under probes of scale s"""
    N = int(round((feats.shape[1] // 17) ** 0.5))
    set_fn = tp.oracle_setter(onet)
    out = []
    for w in ws:
        tp.set_probe(set_fn, N, w, s)
        pi = tp.forward64(onet, feats)[0] if precision == 64 else tp.forward_prec(onet, feats, precision)[0]
        out.append(tp.probe_logits(pi) / s)
    return np.stack(out)


def choose_s(dmax):
    """the largest power of two s with s * dmax <= L_MAX"""
    return 2.0 ** np.floor(np.log2(L_MAX / dmax))


def read_out(onet, feats, ws, family):
    """(s, D_ref [K, B, P] integers as float64, D64): D_ref is the float64 oracle's (family A) or oracle precision 16's (B);
    D64 is the float64 oracle's l / s as read (at S0: good to 1e-9 of a unit).  s from the reference alone: first D of the float64 oracle at the tiny scale S0, then, for family B, halved until the
    restatement's own |l| <= L_MAX."""
    D64 = oracle_D(onet, feats, ws, S0)
    assert np.abs(D64 - np.round(D64)).max() < 1e-4, np.abs(D64 - np.round(D64)).max()
    s = choose_s(np.abs(D64).max())
    if family == "A":
        return s, np.round(D64), D64
    while True:
        D16 = oracle_D(onet, feats, ws, s, 16)
        if np.abs(D16).max() * s <= L_MAX:
            return s, np.round(D16), D64
        s /= 2


def build_case(name):
    """(onet, feats, ws) of CASES[name], fresh; the caller frees onet"""
    c = CASES[name]
    kw = {k: c[k] for k in ("k_stem", "k_tower", "shift") if k in c}
    onet, feats = make_exact(c["N"], c["tower"], c["seed"], c["B"], **kw)
    return onet, feats, make_probes(c["probes"], c["seed"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(onet, feats, ws, s, D_ref, D64) of CASES[name], computed once; the arrays are read-only and onet is left with the last
    probe set"""
    onet, feats, ws = build_case(name)
    s, D, D64 = read_out(onet, feats, ws, CASES[name]["family"])
    for a in (feats, ws, D, D64):
        a.setflags(write=False)
    return onet, feats, ws, s, D, D64


def geometry_boards(N, B):
    """the first three boards, the last three, and the boards that hold the rows on either side of the first multiple of each
    tile height and of the first tile that is a workgroup's second (CUS tiles in)"""
    P = N * N
    rows = [m for t in TILE_ROWS for m in (t, CUS * t)]
    pick = set(range(min(3, B))) | set(range(max(0, B - 3), B))
    pick |= {r // P for m in rows for r in (m - 1, m) if r // P < B}
    return np.array(sorted(pick))


@functools.lru_cache(maxsize=None)
def geometry_reference(name):
    """(onet, feats [B, 17 P], ws, s, boards, D_ref [K, len(boards), P], D64) of GEOMETRY[name]: boards are independent, so
    the oracle runs on `geometry_boards` only"""
    N, B = GEOMETRY[name]
    onet, feats = make_exact(N, GEOMETRY_TOWER, GEOMETRY_SEED + N, B, shift=GEOMETRY_SHIFT)
    ws = make_probes(GEOMETRY_PROBES.get(name, 8), GEOMETRY_SEED)
    boards = geometry_boards(N, B)
    s, D, D64 = read_out(onet, feats[boards], ws, "A")
    for a in (feats, ws, D, D64):
        a.setflags(write=False)
    return onet, feats, ws, s, boards, D, D64

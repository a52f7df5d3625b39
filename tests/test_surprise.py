"""Policy surprise weighting on the CPU (include/agz_surprise.h): libagz.so's engine-free entry points
(the library loads without a GPU) against the plain-C twin of tests/surprise_twin.py, which is compiled from
include/agz_draws.h alone -- agz_surprise_weights bit for bit (kl as uint64 patterns, q exactly) on games built from the
corner rows, agz_surprise_pick against the Python-integer restatement at every boundary of prefixes that hold zero
weights -- and the surface: the three engine calls, the Python and Julia mirrors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import alphago_jl_amd as ag
import surprise_twin as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHOS = (0.0, 0.5, 1.0)
FLT_MIN = np.float32(1.17549435e-38)


def _rows(A, rng):
    """the corner rows for A actions: name -> (pi, p)"""
    uni = np.full(A, 1.0 / A, np.float32)
    onehot = np.zeros(A, np.float32)
    onehot[A // 3] = 1.0
    soft = rng.dirichlet(np.full(A, 0.3)).astype(np.float32)
    soft2 = rng.dirichlet(np.full(A, 0.3)).astype(np.float32)
    prior = rng.dirichlet(np.full(A, 1.0)).astype(np.float32)
    sparse = soft.copy()
    sparse[rng.rand(A) < 0.6] = 0.0
    sparse[0] = 0.25                                    # never all zero
    holes = prior.copy()
    holes[sparse > 0] = 0.0                             # p = 0 exactly where pi > 0: the FLT_MIN floor
    holes[1] = FLT_MIN / np.float32(4)                  # and a subnormal prior
    zero = np.zeros(A, np.float32)
    return dict(onehot=(onehot, uni), same=(soft, soft.copy()), same2=(prior, prior.copy()), soft=(soft, prior),
                soft2=(soft2, prior), floor=(sparse, holes), zero=(zero, prior), sub=(soft2, holes))


def _games(A):
    rng = np.random.RandomState(100 + A)
    r = _rows(A, rng)
    g = {
        "onehot_vs_uniform": ["onehot", "soft", "soft2"],
        "pi_equals_p_among_others": ["same", "soft", "onehot"],
        "every_score_zero": ["same", "same2", "same"],                 # S = 0: every w = 1
        "zero_row_between_targets": ["soft", "zero", "soft2", "zero", "onehot"],
        "floor": ["floor", "soft", "sub"],
        "single_target": ["soft"],
        "single_target_among_zero_rows": ["zero", "soft2", "zero"],
        "only_zero_rows": ["zero", "zero"],
        "long": ["soft", "soft2", "onehot", "floor", "zero", "same", "sub"] * 5,
    }
    out = {k: (np.stack([r[n][0] for n in v]), np.stack([r[n][1] for n in v]), v) for k, v in g.items()}
    out["T0"] = (np.zeros((0, A), np.float32), np.zeros((0, A), np.float32), [])
    return out


def _lib_weights(pis, ps, rho):
    L = ag.load()
    T, A = pis.shape
    kl = np.full(max(T, 1), 7.0, np.float64)
    q = np.full(max(T, 1), 7, np.uint32)
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert L.agz_surprise_weights(f(np.ascontiguousarray(pis)), f(np.ascontiguousarray(ps)), T, A, rho,
                                  kl.ctypes.data_as(C.POINTER(C.c_double)), q.ctypes.data_as(C.POINTER(C.c_uint32))) == ag._lib.OK
    return kl[:T], q[:T]


@pytest.mark.parametrize("A", [26, 82])
def test_weights_equal_the_twin_bit_for_bit(A):
    for name, (pis, ps, rows) in _games(A).items():
        for rho in RHOS:
            want_kl, want_q = st.weights(pis, ps, rho)
            got_kl, got_q = _lib_weights(pis, ps, rho)
            assert (st.bits(got_kl) == st.bits(want_kl)).all(), (name, rho, got_kl, want_kl)
            assert (got_q == want_q).all(), (name, rho, got_q, want_q)
            kl2, q2 = ag.surprise_weights(pis, ps, rho)                   # the Python mirror
            assert (st.bits(kl2) == st.bits(want_kl)).all() and (q2 == want_q).all(), (name, rho)
            tgt = np.array([n != "zero" for n in rows], bool)
            n = int(tgt.sum())
            assert abs(int(got_q[tgt].astype(np.int64).sum()) - st.UNIT * n) <= n, (name, rho)     # the mass is kept
            assert (got_q[~tgt] == st.UNIT).all() and (got_kl[~tgt] == 0).all()
            assert (got_kl >= 0).all()
            if rho == 0.0:
                assert (got_q == st.UNIT).all()


@pytest.mark.parametrize("A", [26, 82])
def test_what_the_corner_rows_promise(A):
    g = _games(A)
    kl, q = _lib_weights(*g["onehot_vs_uniform"][:2], 0.5)
    assert abs(kl[0] - np.log(A)) < 1e-6                                    # one-hot against uniform: log A
    kl, q = _lib_weights(*g["pi_equals_p_among_others"][:2], 1.0)
    assert st.bits(kl[:1])[0] == 0 and q[0] == 0                            # pi = p: exactly +0.0, and no mass at rho = 1
    for rho in RHOS:
        kl, q = _lib_weights(*g["every_score_zero"][:2], rho)
        assert (kl == 0).all() and (q == st.UNIT).all()
        for name in ("single_target", "single_target_among_zero_rows"):
            kl, q = _lib_weights(*g[name][:2], rho)
            assert (q == st.UNIT).all(), (name, rho, q)
        kl, q = _lib_weights(*g["T0"][:2], rho)
        assert len(kl) == 0 and len(q) == 0
    kl, _ = _lib_weights(*g["floor"][:2], 0.5)
    assert np.isfinite(kl).all() and kl[0] > 10.0                           # -log(FLT_MIN) = 87.3 per unit of pi


def test_weights_range_checks():
    L = ag.load()
    pis, ps, _ = _games(26)["floor"]
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    kl = np.full(3, 7.0)
    q = np.full(3, 7, np.uint32)
    klp, qp = kl.ctypes.data_as(C.POINTER(C.c_double)), q.ctypes.data_as(C.POINTER(C.c_uint32))
    for bad in (-0.1, 1.5, float("nan")):
        assert L.agz_surprise_weights(f(pis), f(ps), 3, 26, bad, klp, qp) == ag._lib.BAD_ARGUMENT
        with pytest.raises(ag.AgzError):
            ag.surprise_weights(pis, ps, bad)
    assert L.agz_surprise_weights(f(pis), f(ps), -1, 26, 0.5, klp, qp) == ag._lib.BAD_ARGUMENT
    assert L.agz_surprise_weights(f(pis), f(ps), 3, 0, 0.5, klp, qp) == ag._lib.BAD_ARGUMENT
    assert L.agz_surprise_weights(None, f(ps), 3, 26, 0.5, klp, qp) == ag._lib.BAD_ARGUMENT
    assert (kl == 7.0).all() and (q == 7).all()
    assert L.agz_surprise_weights(f(pis), f(ps), 3, 26, 0.5, None, None) == ag._lib.OK       # either output may be NULL
    with pytest.raises(ag.AgzError):
        ag.surprise_weights(pis, ps[:2], 0.5)


PREFIXES = [
    [5],
    [0, 0, 3],
    [4, 4, 4, 9, 9],
    [0, 65536, 65536, 131072, 131072 + 7, 131072 + 7],
    list(np.cumsum(np.array([0, 1, 0, 0, 2 ** 31, 0, 3, 2 ** 32 - 1, 0, 1], np.uint64).astype(object))),
    list(np.cumsum((np.random.RandomState(5).randint(0, 3, 300) * np.random.RandomState(6).randint(1, 200000, 300)).astype(object))),
    [2 ** 63, 2 ** 63, 2 ** 64 - 1],
]


def _us_for(r, W):
    """the least and the largest 64-bit u with floor(u * W / 2^64) = r"""
    lo = -((-r << 64) // W)                             # ceil(r * 2^64 / W)
    hi = min(-((-(r + 1) << 64) // W) - 1, 2 ** 64 - 1)
    assert (lo * W) >> 64 == r and (hi * W) >> 64 == r
    return lo, hi


def test_pick_equals_the_restatement_at_every_boundary():
    L = ag.load()
    for cum in PREFIXES:
        cum = [int(c) for c in cum]
        n, W = len(cum), cum[-1]
        arr = (C.c_uint64 * n)(*cum)
        us = {0, 2 ** 64 - 1}
        for c in set(cum):
            for r in (c - 1, c):
                if 0 <= r < W:
                    us.update(_us_for(r, W))
        zero = {i for i in range(n) if cum[i] == (cum[i - 1] if i else 0)}
        seen = set()
        for u in sorted(us):
            got = L.agz_surprise_pick(arr, n, u)
            assert got == st.pick(u, cum), (cum[:8], u, got)
            assert got not in zero, (cum[:8], u, got)
            seen.add(got)
        assert seen == set(range(n)) - zero                               # every index with mass is reached


def test_pick_without_mass():
    L = ag.load()
    z = (C.c_uint64 * 3)(0, 0, 0)
    assert L.agz_surprise_pick(z, 3, 12345) == -1 and st.pick(12345, [0, 0, 0]) == -1
    assert L.agz_surprise_pick(z, 0, 0) == -1
    assert L.agz_surprise_pick((C.c_uint64 * 1)(9), 0, 0) == -1
    assert L.agz_surprise_pick(None, 3, 0) == -1


NAMES = ("agz_replay_score", "agz_replay_set_surprise", "agz_replay_surprise", "agz_surprise_weights", "agz_surprise_pick")


def test_surface_is_declared_everywhere():
    hdr = open(os.path.join(ROOT, "include", "agz.h")).read()
    jl = open(os.path.join(ROOT, "alphago.jl_amd", "julia", "AlphaGoMI.jl")).read()
    lib = ag.load()
    for name in NAMES:
        assert name in hdr and name in lib._agz_signatures and hasattr(lib, name) and ":" + name in jl, name
    assert "agz_surprise.h" in hdr
    assert "AGZ_SITE_REPLAY_WEIGHTED 13u" in open(os.path.join(ROOT, "include", "agz_draws.h")).read()
    for rel in ("alphago.jl_amd/csrc/agz_replay.hip", "alphago.jl_amd/csrc/agz_capi.hip"):        # one arithmetic, included
        assert "include/agz_surprise.h" in open(os.path.join(ROOT, rel)).read()
    assert "surprise::Real = 0.0" in jl
    assert lib.agz_version() == 103


def test_engine_calls_need_an_engine():
    L = ag.load()
    rows = C.c_int64(7)
    assert L.agz_replay_score(None, 0, 1, C.byref(rows)) == ag._lib.BAD_ARGUMENT and rows.value == 7
    assert L.agz_replay_set_surprise(None, 0.5) == ag._lib.BAD_ARGUMENT
    assert L.agz_replay_surprise(None, 0, None, None, None) == ag._lib.BAD_ARGUMENT


def test_python_surface():
    assert "surprise_weights" in ag.__all__ and callable(ag.surprise_weights)
    assert list(inspect.signature(ag.surprise_weights).parameters) == ["pis", "ps", "rho"]
    p = inspect.signature(ag.train).parameters
    assert "surprise" in p and p["surprise"].default == 0.0
    sig = lambda f: [(k, v.default) for k, v in list(inspect.signature(f).parameters.items())[1:]]
    assert sig(ag.Engine.replay_score) == [("first", 0), ("count", None)]
    assert sig(ag.Engine.replay_set_surprise) == [("rho", 0.0)]
    assert [k for k, _ in sig(ag.Engine.replay_surprise)] == ["k"]
    src = open(os.path.join(ROOT, "examples", "generation_loop.py")).read()
    assert "--surprise" in src

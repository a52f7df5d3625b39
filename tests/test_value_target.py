"""Search-value targets on the CPU (include/agz_value_target.h): the header's one function, compiled by gcc
into a shim by this test, and libagz.so's engine-free agz_value_targets (the library loads without a GPU) equal the numpy
float64 twin (tests/value_target_twin.py) bit for bit -- on hand rows, on 2000 random rows and on the worked row of DESIGN
§5n -- and keep the identities of the definition.  The shim is built twice where the host has FMA units: once plainly and
once with -mfma -ffp-contract=fast, the setting under which only the header's own pragma keeps gcc from fusing a product
into the sum behind it (hipcc's default for device code is that setting).  (tools/value_target_check.c is the same
arithmetic as a stand-alone program for a run under the host sanitizers)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import alphago_jl_amd as ag
import value_target_twin as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
TMAX = 60

SHIM = r"""
#include "agz_value_target.h"
float vt_one(const float* qs, int T, int t, int result, double alpha, double lambda) {
  return agz_value_target(qs, T, t, result, alpha, lambda);
}
void vt_rows(const float* qs, int stride, const int* T, const int* t, const int* result, int n, double alpha,
             double lambda, float* out) {
  for (int i = 0; i < n; ++i) out[i] = agz_value_target(qs + (long)i * stride, T[i], t[i], result[i], alpha, lambda);
}
int vt_ok(double alpha, double lambda) { return agz_value_target_params_ok(alpha, lambda); }
"""


def _has_fma():
    try:
        return bool(re.search(r"^flags\s*:.*\bfma\b", open("/proc/cpuinfo").read(), flags=re.M))
    except OSError:
        return False


def _build_shim(td, name, flags):
    src = os.path.join(td, name + ".c")
    out = os.path.join(td, name + ".so")
    open(src, "w").write(SHIM)
    r = subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I", INC] + flags + [src, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    L = C.CDLL(out)
    L.vt_one.restype = C.c_float
    L.vt_one.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    L.vt_rows.restype = None
    L.vt_rows.argtypes = [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                          C.c_double, C.c_double, C.POINTER(C.c_float)]
    L.vt_ok.restype = C.c_int
    L.vt_ok.argtypes = [C.c_double, C.c_double]
    return L


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    """the header compiled by gcc: plainly, and (hosts with FMA units) with contraction asked for on the command line"""
    assert shutil.which("gcc")
    td = str(tmp_path_factory.mktemp("vt"))
    out = {"plain": _build_shim(td, "vt_plain", [])}
    if _has_fma():
        out["fma"] = _build_shim(td, "vt_fma", ["-mfma", "-ffp-contract=fast"])
    return out


def _fp(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def shim_one(L, qs, t, result, alpha, lam):
    q = np.ascontiguousarray(qs, np.float32)
    return np.float32(L.vt_one(_fp(q, C.c_float), len(q), int(t), int(result), alpha, lam))


@pytest.fixture(scope="module")
def random_rows():
    """2000 rows: T in 1..60, q uniform in [-1, 1] with one entry in eight one of +0.0, -0.0, +1, -1, a result of -1, 0
    or +1 and one sampled ply each; the twin's y of every (alpha, lambda) pair, computed once"""
    rng = np.random.RandomState(20260)
    n = 2000
    T = rng.randint(1, TMAX + 1, n).astype(np.int32)
    T[:4] = (1, 1, TMAX, TMAX)
    qs = rng.uniform(-1.0, 1.0, (n, TMAX)).astype(np.float32)
    sp = rng.rand(n, TMAX) < 0.125
    qs[sp] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), int(sp.sum()))
    t = (rng.rand(n) * T).astype(np.int32)
    t[1], t[2], t[3] = 0, 0, TMAX - 1
    result = rng.randint(-1, 2, n).astype(np.int32)
    for i in range(n):
        qs[i, T[i]:] = np.nan                       # whatever lies behind a record must not be read
    want = {p: np.array([vt.value_target(qs[i, :T[i]], t[i], result[i], *p) for i in range(n)], np.float32) for p in vt.PAIRS}
    assert any((np.signbit(qs[i, t[i]]) and qs[i, t[i]] == 0) for i in range(n)), "no -0.0 at a sampled ply"
    return dict(n=n, T=T, qs=qs, t=t, result=result, want=want)


HAND = [(np.array([0.3], np.float32), 0), (np.array([-0.75], np.float32), 0)] + \
       [(np.array([0.2, -0.4, 0.6, -0.1, 0.9], np.float32), t) for t in (0, 2, 4)]


def test_hand_rows_equal_the_twin(shims):
    """T = 1 and T = 5 at t = 0, 2, 4, results +1, -1 and 0 (the draw), every (alpha, lambda) pair"""
    for name, L in shims.items():
        for qs, t in HAND:
            for result in (1, -1, 0):
                for alpha, lam in vt.PAIRS:
                    got, want = shim_one(L, qs, t, result, alpha, lam), vt.value_target(qs, t, result, alpha, lam)
                    assert vt.bits(got) == vt.bits(want), (name, qs, t, result, alpha, lam, got, want)


def test_random_rows_equal_the_twin(shims, random_rows):
    r = random_rows
    for name, L in shims.items():
        for (alpha, lam), want in r["want"].items():
            got = np.zeros(r["n"], np.float32)
            L.vt_rows(_fp(r["qs"], C.c_float), TMAX, _fp(r["T"], C.c_int), _fp(r["t"], C.c_int), _fp(r["result"], C.c_int),
                      r["n"], alpha, lam, _fp(got, C.c_float))
            bad = np.nonzero(vt.bits(got) != vt.bits(want))[0]
            assert bad.size == 0, (name, alpha, lam, bad[:5], got[bad[:5]], want[bad[:5]])


def test_identities(random_rows):
    """what the definition promises without any arithmetic: (1, 0) is q_t itself (its sign of zero too), (1, 1) and
    alpha = 0 are float(result), and no y leaves [-max(1, max|q|), max(1, max|q|)] (a convex combination twice over)"""
    r = random_rows
    qt = r["qs"][np.arange(r["n"]), r["t"]]
    assert (vt.bits(r["want"][(1.0, 0.0)]) == vt.bits(qt)).all()
    assert (vt.bits(r["want"][(1.0, 1.0)]) == vt.bits(r["result"].astype(np.float32))).all()
    assert (vt.bits(r["want"][(0.0, 0.3)]) == vt.bits(r["result"].astype(np.float32))).all()
    for i in range(r["n"]):
        bound = max(1.0, float(np.abs(r["qs"][i, :r["T"][i]]).max()))
        for p in vt.PAIRS:
            assert abs(float(r["want"][p][i])) <= bound, (i, p)


def test_worked_row(shims):
    """the row DESIGN §5n writes out: T = 3, q = (0.2, -0.4, 0.6), z = +1, alpha = 1, lambda = 0.5:
    G_2 = 0.5 * 0.6 + 0.5 * 1 = 0.8,  G_1 = 0.5 * (-0.4) + 0.5 * 0.8 = 0.2,  G_0 = 0.5 * 0.2 + 0.5 * 0.2 = 0.2"""
    qs = np.array([0.2, -0.4, 0.6], np.float32)
    want = vt.value_targets(qs, 1, 1.0, 0.5)
    assert np.abs(want.astype(np.float64) - np.array([0.2, 0.2, 0.8])).max() <= 1e-7
    for name, L in shims.items():
        got = np.array([shim_one(L, qs, t, 1, 1.0, 0.5) for t in range(3)], np.float32)
        assert (vt.bits(got) == vt.bits(want)).all(), (name, got, want)
    assert (vt.bits(ag.value_targets(qs, 1, 1.0, 0.5)) == vt.bits(want)).all()


def test_library_export_equals_the_twin(random_rows):
    """agz_value_targets of libagz.so (the host half of a hipcc translation unit) and its Python mirror: whole records"""
    r = random_rows
    L = ag.load()
    for i in range(0, 120):
        T, qs, res = int(r["T"][i]), np.ascontiguousarray(r["qs"][i, :r["T"][i]]), int(r["result"][i])
        for alpha, lam in vt.PAIRS:
            want = vt.value_targets(qs, res, alpha, lam)
            got = np.zeros(T, np.float32)
            assert L.agz_value_targets(_fp(qs, C.c_float), T, res, alpha, lam, _fp(got, C.c_float)) == ag._lib.OK
            assert (vt.bits(got) == vt.bits(want)).all(), (i, alpha, lam)
            assert (vt.bits(ag.value_targets(qs, res, alpha, lam)) == vt.bits(want)).all()
            assert want[r["t"][i]].view(np.uint32) == r["want"][(alpha, lam)][i].view(np.uint32)
    assert len(ag.value_targets(np.zeros(0, np.float32), 1, 0.5, 0.5)) == 0


def test_range_checks(shims):
    qs = np.array([0.5, -0.5], np.float32)
    out = np.full(2, 7.0, np.float32)
    L = ag.load()
    for bad in (-0.1, 1.5, float("nan")):
        for alpha, lam in ((bad, 0.5), (0.5, bad)):
            assert not shims["plain"].vt_ok(alpha, lam)
            assert L.agz_value_targets(_fp(qs, C.c_float), 2, 1, alpha, lam, _fp(out, C.c_float)) == ag._lib.BAD_ARGUMENT
            assert (out == 7.0).all()
            with pytest.raises(ag.AgzError):
                ag.value_targets(qs, 1, alpha, lam)
    for alpha, lam in ((0.0, 0.0), (1.0, 1.0), (0.0, 1.0)):
        assert shims["plain"].vt_ok(alpha, lam)
    assert L.agz_value_targets(_fp(qs, C.c_float), -1, 1, 0.5, 0.5, _fp(out, C.c_float)) == ag._lib.BAD_ARGUMENT
    assert L.agz_value_targets(None, 2, 1, 0.5, 0.5, _fp(out, C.c_float)) == ag._lib.BAD_ARGUMENT


def test_surface_is_declared_everywhere():
    hdr = open(os.path.join(INC, "agz.h")).read()
    jl = open(os.path.join(ROOT, "alphago.jl_amd", "julia", "AlphaGoMI.jl")).read()
    lib = ag.load()
    for name in ("agz_replay_set_value_target", "agz_records_value_targets", "agz_value_targets"):
        assert name in hdr and name in lib._agz_signatures and hasattr(lib, name) and ":" + name in jl, name
    assert "agz_value_target.h" in hdr
    for rel in ("alphago.jl_amd/csrc/agz_engine.hip", "alphago.jl_amd/csrc/agz_capi.hip"):      # one arithmetic, included
        assert "include/agz_value_target.h" in open(os.path.join(ROOT, rel)).read()
    import inspect
    assert "value_target" in inspect.signature(ag.train).parameters
    assert "value_target" in inspect.signature(ag.extract_data).parameters
    assert "value_target = nothing" in jl

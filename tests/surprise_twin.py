"""The twin of policy surprise weighting (include/agz.h agz_replay_score): a plain-C restatement of the
score and the weights, compiled here from include/agz_draws.h alone (the logarithm and the draw are the shared ones;
include/agz_surprise.h is NOT included), and the pick restated in Python integers.  tests/test_surprise.py holds
libagz.so's engine-free entry points against it; tests/test_gpu_surprise.py the device."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SITE_REPLAY_WEIGHTED, SITE_REPLAY_SYM = 13, 10
UNIT = 65536

_TWIN = r"""
#include <float.h>
#include <stdint.h>
#include "agz_draws.h"
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif
/* one game: pis, ps [T][A] -> kl [T] (0 where the row is all zero), q [T] (65536 there) */
void twin_weights(const float* pis, const float* ps, int T, int A, double rho, double* kl, uint32_t* q) {
  double S = 0.0;
  int n = 0;
  for (int t = 0; t < T; ++t) {
    const float *pi = pis + (long)t * A, *p = ps + (long)t * A;
    int target = 0;
    for (int a = 0; a < A; ++a) target |= pi[a] != 0.f;
    kl[t] = 0.0;
    if (!target) continue;
    double s = 0.0;
    for (int a = 0; a < A; ++a) {
      if (!(pi[a] > 0.f)) continue;
      const float floor_p = p[a] > FLT_MIN ? p[a] : FLT_MIN;
      const double lpi = agz_log((double)pi[a]);
      const double lp = agz_log((double)floor_p);
      const double diff = lpi - lp;
      const double term = (double)pi[a] * diff;
      s = s + term;
    }
    kl[t] = s > 0.0 ? s : 0.0;
    S = S + kl[t];
    ++n;
  }
  for (int t = 0; t < T; ++t) {
    const float* pi = pis + (long)t * A;
    int target = 0;
    for (int a = 0; a < A; ++a) target |= pi[a] != 0.f;
    double w = 1.0;
    if (target && S > 0.0) {
      const double num = kl[t] * (double)n;
      const double share = num / S;
      const double even = 1.0 - rho;
      const double prop = rho * share;
      w = even + prop;
    }
    const double scaled = w * 65536.0;
    q[t] = (uint32_t)(scaled + 0.5);
  }
}
uint64_t twin_draw(uint64_t seed, uint64_t call, uint32_t site, uint64_t idx) {
  return agz_draw_u64(seed, call, 0, site, idx);
}
"""
_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="agz_surprise_twin_")
        src, so = os.path.join(d, "twin.c"), os.path.join(d, "libtwin.so")
        open(src, "w").write(_TWIN)
        subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        src, "-o", so], check=True)
        L = C.CDLL(so)
        L.twin_weights.restype = None
        L.twin_weights.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_double,
                                   C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
        L.twin_draw.restype = C.c_uint64
        L.twin_draw.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64]
        _lib = L
    return _lib


def weights(pis, ps, rho):
    """(kl [T] float64, q [T] uint32) of one game"""
    pi = np.ascontiguousarray(pis, np.float32)
    p = np.ascontiguousarray(ps, np.float32)
    T, A = pi.shape
    kl = np.zeros(max(T, 1), np.float64)
    q = np.zeros(max(T, 1), np.uint32)
    lib().twin_weights(pi.ctypes.data_as(C.POINTER(C.c_float)), p.ctypes.data_as(C.POINTER(C.c_float)), T, A, float(rho),
                       kl.ctypes.data_as(C.POINTER(C.c_double)), q.ctypes.data_as(C.POINTER(C.c_uint32)))
    return kl[:T], q[:T]


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def pick(u, cum):
    """agz_weighted_pick in Python integers: the smallest i with cum[i] > floor(u * cum[-1] / 2^64); -1 without mass"""
    c = [int(x) for x in cum]
    if not c or c[-1] == 0:
        return -1
    r = (int(u) * c[-1]) >> 64
    lo, hi = 0, len(c) - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if c[mid] > r:
            hi = mid
        else:
            lo = mid + 1
    assert c[lo] > r and (lo == 0 or c[lo - 1] <= r)
    return lo


def draw(seed, call, b, site=SITE_REPLAY_WEIGHTED):
    return int(lib().twin_draw(seed, call, site, b))


def sample_pairs(seed, call, B, q_games, first_game=0, first_ply=0, targets=None):
    """what agz_replay_sample must draw under rho > 0: q_games = the per-game q arrays as agz_replay_surprise returns
    them (unmasked), the window's start (first_game, first_ply -- counted in target plies when `targets`, the per-game
    boolean target masks of a targets-only arena, is given) -> (game [B] int64, ply [B] int32)"""
    masked = []
    for g, q in enumerate(q_games):
        q = np.array(q, np.uint64)
        if targets is not None:
            q[~targets[g]] = 0
        if g < first_game:
            q[:] = 0
        elif g == first_game:
            if targets is None:
                q[:first_ply] = 0
            else:
                q[np.nonzero(targets[g])[0][:first_ply]] = 0
        masked.append(q)
    lens = np.array([len(q) for q in masked], np.int64)
    start = np.concatenate([[0], np.cumsum(lens)])
    cum = np.cumsum(np.concatenate(masked).astype(object)) if lens.sum() else []
    cum = [int(x) for x in cum]
    game, ply = np.zeros(B, np.int64), np.zeros(B, np.int32)
    for b in range(B):
        a = pick(draw(seed, call, b), cum)
        g = int(np.searchsorted(start, a, side="right") - 1)
        game[b], ply[b] = g, a - start[g]
    return game, ply


def sample_syms(seed, call, B):
    return np.array([((draw(seed, call, b, SITE_REPLAY_SYM) >> 32) * 8) >> 32 for b in range(B)], np.int32)

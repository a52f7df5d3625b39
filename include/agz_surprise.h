/*
 * agz_surprise.h -- policy surprise weighting of the replay arena: how often a recorded ply is drawn
 * (agz_replay_score, agz_replay_set_surprise, agz_replay_surprise, agz_surprise_weights, agz_surprise_pick;
 * include/agz.h).
 *
 * The score of a ply is the Kullback-Leibler divergence of its search result pi (a recorded row, float[A]) from the
 * network's prior p (float[A]) for the same position:
 *
 *     s = 0
 *     for a = 0 .. A-1 ascending:
 *         if pi[a] > 0:  s = s + (double)pi[a] * (agz_log((double)pi[a]) - agz_log((double)max(p[a], FLT_MIN)))
 *     score = max(s, 0.0)
 *
 * A row that is all zero is "no policy target" (a fast search of the playout cap, an arena record): it has no score.
 *
 * Under rho in [0, 1] a game's target plies T (in ply order, n = |T|, S = the ascending sum of their scores) get
 *
 *     w_t = (1.0 - rho) + rho * ((s_t * (double)n) / S)      when S > 0, else w_t = 1.0
 *
 * so half of the game's n units of sampling mass (rho = 0.5) is spread evenly and half in proportion to the score.
 * Every non-target ply, and every ply of a game that has not been scored, has w = 1.0.  The weight is quantised as
 * q_t = (uint32_t)(w_t * 65536.0 + 0.5); from there on weights are integers, so their prefix sums are exact and do not
 * depend on the order they were added in.
 *
 * The pick over an inclusive prefix C[0..n-1] (uint64, W = C[n-1] > 0) for a 64-bit draw u is r = floor(u * W / 2^64)
 * and the smallest index i with C[i] > r: an index whose q is 0 is never returned.
 *
 * Everything is IEEE-754 double, every multiply, add, subtract and divide rounded on its own (floating-point contraction
 * is switched off for this file), and the logarithm is agz_log of agz_draws.h: gcc on the host and hipcc for gfx950 give
 * the same bits (tests/test_surprise.py, tests/test_gpu_surprise.py).  This is the one place the rule is written.
 *
 * Plain C99; also valid C++ and HIP device code.
 */
#ifndef AGZ_SURPRISE_H
#define AGZ_SURPRISE_H

#include <stdint.h>

#include "agz_draws.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

#define AGZ_SURPRISE_FLT_MIN 1.17549435082228750797e-38f /* FLT_MIN, the floor of a prior entry */
#define AGZ_SURPRISE_UNIT 65536u                          /* q of w = 1.0 */

/* rho inside [0, 1] (a NaN is not) */
static inline AGZ_HD int agz_surprise_rho_ok(double rho) { return rho >= 0.0 && rho <= 1.0; }

/* the row is a policy target: not all zero */
static inline AGZ_HD int agz_surprise_is_target(const float* pi, int32_t A) {
  for (int32_t a = 0; a < A; ++a)
    if (pi[a] != 0.f) return 1;
  return 0;
}

/* one term of the sum, for pi > 0 */
static inline AGZ_HD double agz_surprise_term(float pi, float p) {
  const float pf = p > AGZ_SURPRISE_FLT_MIN ? p : AGZ_SURPRISE_FLT_MIN;
  const double d = agz_log((double)pi) - agz_log((double)pf);
  return (double)pi * d;
}

/* the score of a target row */
static inline AGZ_HD double agz_surprise_score(const float* pi, const float* p, int32_t A) {
  double s = 0.0;
  for (int32_t a = 0; a < A; ++a)
    if (pi[a] > 0.f) s = s + agz_surprise_term(pi[a], p[a]);
  return s > 0.0 ? s : 0.0;
}

/* q of a target ply with score s in a scored game of n targets whose scores sum to S */
static inline AGZ_HD uint32_t agz_surprise_q(double s, int32_t n, double S, double rho) {
  double w = 1.0;
  if (S > 0.0) {
    const double share = (s * (double)n) / S;
    const double even = 1.0 - rho;
    const double prop = rho * share;
    w = even + prop;
  }
  const double scaled = w * 65536.0;
  return (uint32_t)(scaled + 0.5);
}

/* floor(u * W / 2^64) */
static inline AGZ_HD uint64_t agz_mulhi64(uint64_t u, uint64_t W) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(u, W);
#else
  return (uint64_t)(((unsigned __int128)u * W) >> 64);
#endif
}

/* the smallest i with C[i] > r, r = floor(u * C[n-1] / 2^64); n >= 1 and C[n-1] > 0 */
static inline AGZ_HD int64_t agz_weighted_pick(uint64_t u, const uint64_t* C, int64_t n) {
  const uint64_t r = agz_mulhi64(u, C[n - 1]);
  int64_t lo = 0, hi = n - 1;                   /* the answer lies in [lo, hi]: C[n-1] > r */
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (C[mid] > r) hi = mid; else lo = mid + 1;
  }
  return lo;
}

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC pop_options
#endif

#endif /* AGZ_SURPRISE_H */

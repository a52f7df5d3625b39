/*
 * agz_uncertainty.h -- how sure the search is of a value: the statistics of a child from its visit count N, value sum W
 * and sum of squared values S, the lower confidence bound that picks the move, and the factor by which the spread of a
 * node's values scales its exploration (agz_search_set_value_moments, agz_search_set_lcb, agz_search_set_puct_variance,
 * agz_tree_child_lcb, agz_value_lcb, agz_puct_variance_factor; include/agz.h).
 *
 * 1. CHILD STATISTICS of a row entry (N_a, W_a, S_a).  incorporate puts the parent's value into W_a as a pseudo-sample
 *    and its square into S_a; cnt counts it:
 *
 *     cnt = (double)(1.0f + N_a),  mean = (double)W_a / cnt,  m2 = (double)S_a / cnt
 *     var = m2 - mean*mean;  if !(var > 0) var = 0;   sd = agz_sqrt(var)
 *
 * 2. LOWER CONFIDENCE BOUND from the side tp = +-1 to move, z >= 0:
 *
 *     q = mean * (double)tp,   lcb = q - z * agz_sqrt(var / cnt)
 *
 * 3. VARIANCE FACTOR of a node with own stored (n, W_s, S_s), n as puct_scale receives it; k in [0, 1), prior > 0 the
 *    standard deviation expected of a node, pw >= 0 the weight of that expectation in visits:
 *
 *     cnt = (double)(1.0f + n),  mean = (double)W_s / cnt,  m2 = (double)S_s / cnt
 *     var = ((((mean*mean) + (prior*prior)) * pw) + (m2 * cnt)) / (pw + cnt) - (mean*mean);  if !(var > 0) var = 0
 *     factor = 1.0 + k * ((agz_sqrt(var) / prior) - 1.0)
 *
 * Everything is IEEE-754 double unless cast, every multiply, add, subtract and divide rounded on its own (floating-point
 * contraction is switched off for this file); the square root is agz_sqrt of agz_draws.h, so gcc on the host and hipcc
 * for gfx950 give the same bits (tests/test_uncertainty.py, tests/test_gpu_uncertainty.py).  The passes that use these
 * are pick_move, puct_scale and child_lcb_rows of agz_search.h.
 *
 * Plain C99; also valid C++ and HIP device code.
 */
#ifndef AGZ_UNCERTAINTY_H
#define AGZ_UNCERTAINTY_H

#include <stdint.h>

#include "agz_draws.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

typedef struct agz_value_stats {
  double cnt, mean, var, sd;
} agz_value_stats;

/* rule 1 */
static inline AGZ_HD agz_value_stats agz_child_stats(float n, float w, float s) {
  agz_value_stats r;
  r.cnt = (double)(1.0f + n);
  r.mean = (double)w / r.cnt;
  const double m2 = (double)s / r.cnt;
  const double mm = r.mean * r.mean;
  double var = m2 - mm;
  if (!(var > 0.0)) var = 0.0;
  r.var = var;
  r.sd = agz_sqrt(var);
  return r;
}

/* rule 2 */
static inline AGZ_HD double agz_stats_lcb(agz_value_stats st, float tp, double z) {
  const double q = st.mean * (double)tp;
  const double se = agz_sqrt(st.var / st.cnt);
  return q - (z * se);
}
static inline AGZ_HD double agz_child_lcb(float n, float w, float s, float tp, double z) {
  return agz_stats_lcb(agz_child_stats(n, w, s), tp, z);
}

/* rule 3 */
static inline AGZ_HD double agz_variance_factor(float n, float w_s, float s_s, double k, double prior, double pw) {
  const double cnt = (double)(1.0f + n);
  const double mean = (double)w_s / cnt;
  const double m2 = (double)s_s / cnt;
  const double mm = mean * mean;
  const double pp = prior * prior;
  const double num = ((mm + pp) * pw) + (m2 * cnt);
  const double den = pw + cnt;
  double var = (num / den) - mm;
  if (!(var > 0.0)) var = 0.0;
  const double ratio = agz_sqrt(var) / prior;
  return 1.0 + (k * (ratio - 1.0));
}

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC pop_options
#endif

#endif /* AGZ_UNCERTAINTY_H */

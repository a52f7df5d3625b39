/*
 * agz_explore.h -- root exploration and the move that is played: a softmax temperature on the root prior, Dirichlet
 * noise over the legal moves with KataGo's policy-shaped concentration, and a move-selection temperature that decays
 * with the move number (agz_selfplay_set_root_policy_temperature, agz_selfplay_set_root_noise,
 * agz_search_set_move_temperature, agz_tree_explore_rows, agz_explore_temperature; include/agz.h).
 *
 * The schedule both temperatures share, n = position.n of the root (the key its draws use):
 *
 *     T(n) = late + ((early - late) * agz_exp(-(((double)n * 0.6931471805599453) / halflife)))
 *
 * 1. ROOT POLICY TEMPERATURE over the root's stored prior row P, over the legal actions with P_a > 0 only:
 *
 *     x_a = agz_log((double)P_a) / T,  M = max x_a,  e_a = agz_exp(x_a - M),  E = sum e_a,  mass = sum (double)P_a
 *     P_a <- (float)((e_a / E) * mass)
 *
 * 2. ROOT NOISE of total concentration total_alpha > 0 over the L legal actions, u = 1.0 / (double)L:
 *
 *     unshaped: alpha_a = total_alpha * u
 *     shaped:   l_a = agz_log(min(0.01, (double)P_a) + 1e-20),  mean = (sum l_a) / (double)L,
 *               s_a = max(0, l_a - mean),  S = sum s_a,
 *               alpha_a = total_alpha * u when S <= 0, else total_alpha * (0.5 * ((s_a / S) + u))
 *     gamma_a = agz_dirichlet_gamma(seed, game_id, n, a, alpha_a),  G = sum gamma_a,  d_a = G > 0 ? gamma_a / G : u
 *     P_a <- (float)(((double)P_a * (1.0 - w)) + (d_a * w)),  w = dirichlet_noise_weight
 *
 * 3. MOVE TEMPERATURE over the root's visit row N, mx = its maximum over all actions:
 *
 *     w_a = N_a > 0 ? agz_exp(agz_log((double)N_a / (double)mx) / T) : 0,  S = sum w_a,  r = u01 * S
 *     the pick is the first a with w_a > 0 whose running sum exceeds r, else the highest a with w_a > 0
 *
 * Every sum runs in ascending action order.  Everything is IEEE-754 double unless cast, every multiply, add, subtract
 * and divide rounded on its own (floating-point contraction is switched off for this file), and the elementary functions
 * are agz_log and agz_exp of agz_draws.h: gcc on the host and hipcc for gfx950 give the same bits (tests/test_explore.py,
 * tests/test_gpu_explore.py).  This file holds the per-element arithmetic; the sums and the order of the passes are
 * root_explore and pick_move of agz_search.h.
 *
 * Plain C99; also valid C++ and HIP device code.
 */
#ifndef AGZ_EXPLORE_H
#define AGZ_EXPLORE_H

#include <stdint.h>

#include "agz_draws.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

#define AGZ_EXPLORE_ARGMAX_T 0.01 /* a move temperature at or below this is the arg-max */

/* the schedule: early at n = 0, halfway to late at n = halflife */
static inline AGZ_HD double agz_temperature(int32_t n, double early, double late, double halflife) {
  return late + ((early - late) * agz_exp(-(((double)n * 0.6931471805599453) / halflife)));
}

/* rule 1: x_a of a positive prior entry; the new entry from e_a, E and mass */
static inline AGZ_HD double agz_explore_temper_x(float p, double T) { return agz_log((double)p) / T; }
static inline AGZ_HD float agz_explore_temper_p(double e, double E, double mass) { return (float)((e / E) * mass); }

/* rule 2: l_a; s_a; alpha_a (shaped = 0 or S <= 0: the even share); the mixed entry */
static inline AGZ_HD double agz_explore_shape_l(float p) {
  const double q = (double)p;
  return agz_log((q < 0.01 ? q : 0.01) + 1e-20);
}
static inline AGZ_HD double agz_explore_shape_s(double l, double mean) {
  const double d = l - mean;
  return d > 0.0 ? d : 0.0;
}
static inline AGZ_HD double agz_explore_alpha(double total_alpha, double u, int shaped, double s, double S) {
  if (!shaped || S <= 0.0) return total_alpha * u;
  return total_alpha * (0.5 * ((s / S) + u));
}
static inline AGZ_HD float agz_explore_mix(float p, double d, double w) {
  return (float)(((double)p * (1.0 - w)) + (d * w));
}

/* rule 3: w_a of a child with n visits under the row's maximum mx > 0 */
static inline AGZ_HD double agz_explore_pick_weight(float n, float mx, double T) {
  return n > 0.0f ? agz_exp(agz_log((double)n / (double)mx) / T) : 0.0;
}

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC pop_options
#endif

#endif /* AGZ_EXPLORE_H */

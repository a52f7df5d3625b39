/*
 * agz_value_target.h -- the value target of a recorded ply: the game outcome blended with the
 * TD(lambda) return of the root values the search recorded (agz_replay_set_value_target,
 * agz_records_value_targets, agz_value_targets; include/agz.h).
 *
 * A record has T = num_moves recorded plies, q_k = qs[k] (k = 0..T-1, float, Black-absolute: the
 * root's W / (1 + N) when move k was chosen) and z = (double)result.  For the sample at ply t
 * (0 <= t < T) and parameters alpha, lambda in [0, 1]:
 *
 *     acc = z
 *     for k = T-1 down to t:                     backward Horner, in this order
 *         acc = ((1.0 - lambda) * (double)q_k) + (lambda * acc)
 *     G_t = acc                                  = (1-lambda) sum_{k=t}^{T-1} lambda^(k-t) q_k + lambda^(T-t) z
 *     y_t = (float)(((1.0 - alpha) * z) + (alpha * G_t))
 *
 * lambda = 0: G_t = q_t (the plain z/q mix).  lambda = 1: G_t = z.  y is Black-absolute, as z is.  Two corners are
 * returned as they stand, not through the arithmetic:
 *   alpha = 0               y_t = (float)result, the target without this header;
 *   alpha = 1, lambda = 0   y_t = q_t, bit for bit.  (The arithmetic gives the same value; it would only turn a
 *                           q_t of -0.0 into +0.0, by adding the +0.0 of a term whose weight is zero.)
 *
 * Everything is IEEE-754 double, every multiply and add rounded on its own: floating-point
 * contraction is switched off for this file, so gcc on the host, hipcc for gfx950 and numpy float64
 * give the same bits (tests/test_value_target.py, tests/test_gpu_value_target.py).  This is the one
 * place the rule is written; the replay kernel, the host loops and the language mirrors call it.
 *
 * Plain C99; also valid C++ and HIP device code.
 */
#ifndef AGZ_VALUE_TARGET_H
#define AGZ_VALUE_TARGET_H

#include <stdint.h>

#ifndef AGZ_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define AGZ_HD __host__ __device__
#else
#define AGZ_HD
#endif
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

/* both parameters inside [0, 1] (a NaN is not) */
static inline AGZ_HD int agz_value_target_params_ok(double alpha, double lambda) {
  return alpha >= 0.0 && alpha <= 1.0 && lambda >= 0.0 && lambda <= 1.0;
}

/* y_t of the record (qs[0..T-1], result); 0 <= t < T */
static inline AGZ_HD float agz_value_target(const float* qs, int32_t T, int32_t t, int32_t result, double alpha,
                                            double lambda) {
  const double z = (double)result;
  if (alpha == 0.0) return (float)result;
  if (alpha == 1.0 && lambda == 0.0) return qs[t];
  double acc = z;
  for (int32_t k = T - 1; k >= t; --k) {
    const double a = (1.0 - lambda) * (double)qs[k];
    const double b = lambda * acc;
    acc = a + b;
  }
  const double c = (1.0 - alpha) * z;
  const double d = alpha * acc;
  return (float)(c + d);
}

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC pop_options
#endif

#endif /* AGZ_VALUE_TARGET_H */

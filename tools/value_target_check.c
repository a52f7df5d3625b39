/*
 * value_target_check.c -- include/agz_value_target.h as a stand-alone program, for a run under the host sanitizers
 * (DESIGN.md 5n):
 *     gcc -std=c99 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
 *         tools/value_target_check.c -o value_target_check && ./value_target_check
 * 2000 generated rows (T in 1..60, q in [-1, 1] with +-0.0 and +-1 mixed in, result -1 / 0 / +1) in buffers of exactly T
 * entries, every ply, every (alpha, lambda) pair of tests/test_value_target.py.  The program checks the identities that
 * need no twin -- (1, 0) returns q_t bit for bit, (1, 1) and alpha = 0 return (float)result, |y| <= 1 -- and leaves the
 * memory and overflow checks to the sanitizers.  Exit status 0: nothing found.
 */
#include "agz_value_target.h"

static void vt_rows(const float* qs, int stride, const int* T, const int* t, const int* result, int n, double alpha,
                    double lambda, float* out) {
  for (int i = 0; i < n; ++i) out[i] = agz_value_target(qs + (long)i * stride, T[i], t[i], result[i], alpha, lambda);
}

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static unsigned long long s = 0x9E3779B97F4A7C15ull;
static unsigned next(void) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); }
int main(void) {
  static const double pairs[6][2] = {{1, 0}, {1, 1}, {0.5, 0}, {1, 0.9}, {0.25, 0.5}, {0, 0.3}};
  static const float special[4] = {0.0f, -0.0f, 1.0f, -1.0f};
  long bad = 0, done = 0;
  for (int row = 0; row < 2000; ++row) {
    const int T = 1 + (int)(next() % 60), result = (int)(next() % 3) - 1;
    float* qs = (float*)malloc(sizeof(float) * (size_t)T);      /* exactly T entries: a read past them is caught */
    float* out = (float*)malloc(sizeof(float) * (size_t)T);
    int* tt = (int*)malloc(sizeof(int) * (size_t)T);
    int* TT = (int*)malloc(sizeof(int) * (size_t)T);
    int* rr = (int*)malloc(sizeof(int) * (size_t)T);
    for (int k = 0; k < T; ++k) {
      const unsigned u = next();
      qs[k] = (u % 8 == 0) ? special[(u >> 3) % 4] : (float)((double)(u >> 3) / (double)(1u << 28) * 2.0 - 1.0);
      tt[k] = k; TT[k] = T; rr[k] = result;
    }
    for (int p = 0; p < 6; ++p) {
      vt_rows(qs, 0, TT, tt, rr, T, pairs[p][0], pairs[p][1], out);
      for (int t = 0; t < T; ++t, ++done) {
        if (!(out[t] >= -1.0f && out[t] <= 1.0f)) ++bad;
        if (p == 0 && memcmp(&out[t], &qs[t], 4) != 0) ++bad;
        if ((p == 1 || p == 5) && out[t] != (float)result) ++bad;
      }
    }
    free(qs); free(out); free(tt); free(TT); free(rr);
  }
  printf("rows 2000 targets %ld bad %ld\n", done, bad);
  return bad != 0;
}

// uncertainty_sanitize.cpp -- TEST INFRASTRUCTURE: a program of its own around uncertainty_sim.cpp, for a build under
// -fsanitize=address,undefined (tests/test_uncertainty.py).  A check of memory and undefined behaviour, not of results:
// 5x5 / R = 24 self-play on two slots with the value moments, the LCB rule (5, 3, 0.15) and the variance factor
// (0.85, 0.4, 2) on, on a peaked hash network of its own; every step reads the statistics of every root under search.
#include <cstdio>

#include "uncertainty_sim.cpp"

namespace {

// one board point holds 0.6 of the mass, the rest is spread in four levels; v is spread over +-0.9
void hash_net(const float* feats, int B, int P, int A, std::vector<float>& pi, std::vector<float>& v) {
  pi.assign((size_t)B * A, 0.f);
  v.assign(B, 0.f);
  for (int b = 0; b < B; ++b) {
    uint64_t h = 1469598103934665603ull;
    for (int i = 0; i < 17 * P; ++i) h = (h ^ (uint64_t)(feats[(size_t)b * 17 * P + i] != 0.f ? i + 1 : 0)) * 1099511628211ull;
    double sum = 0.0;
    std::vector<double> rest(A);
    for (int a = 0; a < A; ++a) {
      rest[a] = (double)(agz_mix64(h + (uint64_t)a) & 3u) / 4.0 + 0.05;
      if (a == A - 1) rest[a] *= 0.25;
      sum += rest[a];
    }
    for (int a = 0; a < A; ++a) pi[(size_t)b * A + a] = (float)(0.4 * rest[a] / sum);
    pi[(size_t)b * A + (int)(h % (uint64_t)(A - 1))] += 0.6f;
    v[b] = (float)((double)((h >> 8) % 1801u) / 1000.0 - 0.9);
  }
}

}  // namespace

int main() {
  const int N = 5, P = N * N, A = P + 1, slots = 2, games = 3;
  agz_config c{};
  c.board_size = N;
  c.tower_height = 1;
  c.games = slots;
  c.num_readouts = 24;
  c.parallel_readouts = 8;
  c.komi = 7.5f;
  c.c_puct = 0.96;
  c.dirichlet_noise_weight = 0.25;
  c.resign_threshold = -0.9;
  c.resign_disable_fraction = 0.05;
  c.seed = 31;
  c.game_id_stride = 1;
  c.record_capacity_games = games + 8;
  void* h = hs_create(&c);
  if (hu_set_lcb(h, 5.0, 3, 0.15) != AGZ_BAD_ARGUMENT) { printf("a rule was taken with the moments off\n"); return 1; }
  if (hu_set_value_moments(h, 1) != AGZ_OK || hu_set_lcb(h, 5.0, 3, 0.15) != AGZ_OK ||
      hu_set_puct_variance(h, 0.85, 0.4, 2.0) != AGZ_OK) {
    printf("a setter was refused\n");
    return 1;
  }
  hs_start(h, games);
  std::vector<float> feats, pi, v;
  std::vector<double> mean(A), sd(A), lcb(A);
  unsigned long long ct[64] = {0};
  double sum = 0.0;
  for (long steps = 0; steps < 400000; ++steps) {
    hs_counters(h, ct);
    if (ct[agz::CT_FINISHED] >= (unsigned long long)games) break;
    const int B = hs_pre(h);
    if (B == 0) continue;
    feats.assign((size_t)B * 17 * P, 0.f);
    hs_leaf_features(h, feats.data());
    hash_net(feats.data(), B, P, A, pi, v);
    hs_post(h, pi.data(), v.data());
    for (int g = 0; g < slots; ++g) {
      agz::GameState G;
      hs_game_state(h, g, &G);
      if (G.phase != agz::G_SEARCH) continue;
      hu_child_lcb(h, g, G.root, 5.0, mean.data(), sd.data(), lcb.data());
      sum += (double)hu_node_S(h, g, G.root) + sd[A - 1] + (double)hu_node_row_S(h, g, G.root)[0];
    }
  }
  unsigned long long u[4];
  hu_uncertainty_counts(h, u);
  const long recs = hs_records_count(h);
  printf("%ld records, %llu positions, uncertainty counts %llu %llu %llu %llu (checksum %g)\n", recs, ct[agz::CT_POSITIONS],
         u[0], u[1], u[2], u[3], sum);
  const bool ok = recs == games && u[0] > 0 && u[2] > 0;
  hu_destroy(h);
  if (!ok) {
    printf("the game set did not finish, or a counter stayed at zero\n");
    return 1;
  }
  printf("%ld games played\n", recs);
  return 0;
}

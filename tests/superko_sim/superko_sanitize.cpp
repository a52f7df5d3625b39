// superko_sanitize.cpp -- TEST INFRASTRUCTURE: a program of its own around superko_sim.cpp, for a build under
// -fsanitize=address,undefined (tests/test_superko.py).  A check of memory and undefined behaviour, not of results beyond
// two plain facts: random legal games on 2x2 under each rule, played through the two batched entries, never repeat a key;
// a triple ko on one edge of 19x19, played through its cycle, is refused its sixth move; and 3x3 self-play under the
// positional rule, on a hash network of its own, finishes with both counters positive.
#include <cstdio>
#include <set>

#include "superko_sim.cpp"

namespace {

void* make(int N, int slots, int readouts, int games) {
  agz_config c{};
  c.board_size = N;
  c.tower_height = 1;
  c.games = slots;
  c.num_readouts = readouts;
  c.parallel_readouts = 8;
  c.komi = 0.5f;
  c.c_puct = 0.96;
  c.dirichlet_noise_weight = 0.25;
  c.resign_threshold = -2.0;        // resignation off
  c.resign_disable_fraction = 1.0;
  c.seed = 7;
  c.game_id_stride = 1;
  c.record_capacity_games = games + 8;
  return hs_create(&c);
}

// random legal play on 2x2 under `rule` through hk_go_keys / hk_go_legal_seen / hs_go_play; returns moves removed by the
// rule beyond the simple one, -1 when a game repeats a key
long random_games(void* h, int rule, int games, int plies) {
  const int P = 4, A = 5;
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  long removed = 0;
  for (int g = 0; g < games; ++g) {
    std::vector<int8_t> board(P, 0), next(P, 0);
    int8_t tp = 1;
    int32_t ko = -1;
    std::vector<unsigned long long> seen;
    std::set<unsigned long long> had;
    int passes = 0;
    for (int k = 0; k < plies && passes < 2; ++k) {
      unsigned long long key = 0;
      hk_go_keys(h, board.data(), &tp, 1, rule, &key);
      if (!had.insert(key).second && passes == 0) return -1;
      seen.push_back(key);
      const int64_t off[2] = {0, (int64_t)seen.size()};
      int8_t legal[A], simple[A];
      hk_go_legal_seen(h, board.data(), &tp, &ko, seen.data(), off, 1, rule, legal);
      hs_go_legal(h, board.data(), &tp, &ko, 1, simple);
      int cnt = 0;
      for (int a = 0; a < P; ++a) { cnt += legal[a]; removed += simple[a] - legal[a]; }
      rng = agz_mix64(rng + (uint64_t)k);
      int32_t move = P;
      if (cnt > 0 && rng % 10u != 0) {
        int pick = (int)((rng >> 8) % (uint64_t)cnt);
        for (int a = 0; a < P; ++a)
          if (legal[a] && pick-- == 0) move = a;
      }
      passes = move == P ? passes + 1 : 0;
      int32_t nko = -1, ncap = 0, st = 0;
      hs_go_play(h, board.data(), &tp, &ko, &move, 1, next.data(), &nko, &ncap, &st);
      if (st != AGZ_OK) return -1;
      board = next;
      ko = nko;
      tp = (int8_t)-tp;
    }
  }
  return removed;
}

// three edge kos on rows 0..1 of 19x19 (tests/superko_twin.py edge_ko), columns c .. c + 3 for c = 0, 5, 10
bool triple_ko(void* h, int rule) {
  const int N = 19, P = N * N, A = P + 1;
  std::vector<int8_t> board(P, 0), next(P, 0);
  auto at = [&](int row, int col) -> int8_t& { return board[row + N * col]; };
  const int cs[3] = {0, 5, 10};
  for (int i = 0; i < 3; ++i) {
    const int c = cs[i];
    at(0, c) = 1; at(1, c + 1) = 1; at(0, c + 3) = -1; at(1, c + 2) = -1;
    if (i < 2) at(0, c + 1) = -1; else at(0, c + 2) = 1;
  }
  auto take = [&](int i) { return 0 + N * (cs[i] + 2); };
  auto retake = [&](int i) { return 0 + N * (cs[i] + 1); };
  const int32_t cycle[6] = {take(0), retake(2), take(1), retake(0), take(2), retake(1)};
  int8_t tp = 1;
  int32_t ko = -1;
  std::vector<unsigned long long> seen;
  std::vector<int8_t> legal(A);
  for (int k = 0; k < 6; ++k) {
    unsigned long long key = 0;
    hk_go_keys(h, board.data(), &tp, 1, rule, &key);
    seen.push_back(key);
    const int64_t off[2] = {0, (int64_t)seen.size()};
    hk_go_legal_seen(h, board.data(), &tp, &ko, seen.data(), off, 1, rule, legal.data());
    if (k == 5) return legal[cycle[k]] == 0;
    if (!legal[cycle[k]]) return false;
    int32_t nko = -1, ncap = 0, st = 0;
    hs_go_play(h, board.data(), &tp, &ko, &cycle[k], 1, next.data(), &nko, &ncap, &st);
    if (st != AGZ_OK || ncap != 1) return false;
    board = next;
    ko = nko;
    tp = (int8_t)-tp;
  }
  return false;
}

void hash_net(const float* feats, int B, int P, int A, std::vector<float>& pi, std::vector<float>& v) {
  pi.assign((size_t)B * A, 0.f);
  v.assign(B, 0.f);
  for (int b = 0; b < B; ++b) {
    uint64_t hsh = 1469598103934665603ull;
    for (int i = 0; i < 17 * P; ++i) hsh = (hsh ^ (uint64_t)(feats[(size_t)b * 17 * P + i] != 0.f ? i + 1 : 0)) * 1099511628211ull;
    for (int a = 0; a < A; ++a) pi[(size_t)b * A + a] = (a == A - 1 ? 0.02f : 0.98f / (float)P);
    v[b] = (float)((double)((hsh >> 8) % 1801u) / 1000.0 - 0.9);
  }
}

}  // namespace

int main() {
  void* h2 = make(2, 2, 16, 6);
  for (int rule = AGZ_KO_POSITIONAL; rule <= AGZ_KO_SITUATIONAL; ++rule) {
    const long removed = random_games(h2, rule, 40, 60);
    printf("2x2 rule %d: %ld moves removed beyond simple ko\n", rule, removed);
    if (removed <= 0) { printf("a game repeated a key, or the rule removed nothing\n"); return 1; }
  }
  void* h19 = make(19, 1, 8, 1);
  for (int rule = AGZ_KO_POSITIONAL; rule <= AGZ_KO_SITUATIONAL; ++rule)
    if (!triple_ko(h19, rule)) { printf("triple ko: the cycle did not run, or its sixth move was allowed\n"); return 1; }
  hk_destroy(h19);
  hk_destroy(h2);
  // 3x3 self-play under the positional rule
  const int P = 9, A = 10, games = 8;
  h2 = make(3, 4, 16, games);
  if (hk_set_ko_rule(h2, 3) != AGZ_BAD_ARGUMENT || hk_set_ko_rule(h2, AGZ_KO_POSITIONAL) != AGZ_OK) {
    printf("the setter\n");
    return 1;
  }
  hs_start(h2, games);
  std::vector<float> feats, pi, v;
  unsigned long long ct[64] = {0};
  for (long steps = 0; steps < 400000; ++steps) {
    hs_counters(h2, ct);
    if (ct[agz::CT_FINISHED] >= (unsigned long long)games) break;
    const int B = hs_pre(h2);
    if (B == 0) continue;
    feats.assign((size_t)B * 17 * P, 0.f);
    hs_leaf_features(h2, feats.data());
    hash_net(feats.data(), B, P, A, pi, v);
    hs_post(h2, pi.data(), v.data());
  }
  unsigned long long u[2];
  hk_superko_counts(h2, u);
  const long recs = hs_records_count(h2);
  printf("%ld records, superko counts %llu %llu\n", recs, u[0], u[1]);
  const bool ok = recs == games && u[0] > 0 && u[1] >= u[0];
  hk_destroy(h2);
  if (!ok) { printf("the game set did not finish, or a counter stayed at zero\n"); return 1; }
  printf("%ld games played\n", recs);
  return 0;
}

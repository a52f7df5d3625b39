// hostsim_sanitize.cpp -- TEST INFRASTRUCTURE: a program of its own around hostsim.cpp, for a build under
// -fsanitize=address,undefined (the `sanitize` target of the Makefile).  A check of memory and undefined behaviour, not
// of results.  Three parts, one per argument (none: all three):
//   explore      (tests/test_explore.py) the shapes, options and counts of that test's game sets, not its networks or
//                start positions -- 5x5 / R = 24 and 9x9 / R = 32, eight games each on four slots, under the root policy
//                temperature (1.25, 1.1, N), shaped noise of 10.83 and the move temperature (0.75, 0, 2), plain and
//                composed with the playout cap (8, 0.5), forced playouts (2, pruned) and a table of starts -- on a peaked
//                hash network of its own; the rows of every root are read once.
//   uncertainty  (tests/test_uncertainty.py) 5x5 / R = 24 self-play on two slots with the value moments, the LCB rule
//                (5, 3, 0.15) and the variance factor (0.85, 0.4, 2) on, on the same network; every step reads the
//                statistics of every root under search.
//   superko      (tests/test_superko.py) two plain facts beyond memory: random legal games on 2x2 under each rule, played
//                through the two batched entries, never repeat a key; a triple ko on one edge of 19x19, played through
//                its cycle, is refused its sixth move; and 3x3 self-play under the positional rule, on a flat network
//                with hashed values, finishes with both counters positive.
#include <cstdio>
#include <set>
#include <string>

#include "hostsim.cpp"

namespace {

uint64_t hash_feats(const float* f, int P) {
  uint64_t h = 1469598103934665603ull;
  for (int i = 0; i < 17 * P; ++i) h = (h ^ (uint64_t)(f[i] != 0.f ? i + 1 : 0)) * 1099511628211ull;
  return h;
}
float hash_value(uint64_t h) { return (float)((double)((h >> 8) % 1801u) / 1000.0 - 0.9); }

// one board point holds 0.6 of the mass, the rest is spread in four levels; v is spread over +-0.9
void hash_net(const float* feats, int B, int P, int A, std::vector<float>& pi, std::vector<float>& v) {
  pi.assign((size_t)B * A, 0.f);
  v.assign(B, 0.f);
  for (int b = 0; b < B; ++b) {
    const uint64_t h = hash_feats(feats + (size_t)b * 17 * P, P);
    double sum = 0.0;
    std::vector<double> rest(A);
    for (int a = 0; a < A; ++a) {
      rest[a] = (double)(agz_mix64(h + (uint64_t)a) & 3u) / 4.0 + 0.05;
      if (a == A - 1) rest[a] *= 0.25;
      sum += rest[a];
    }
    for (int a = 0; a < A; ++a) pi[(size_t)b * A + a] = (float)(0.4 * rest[a] / sum);
    pi[(size_t)b * A + (int)(h % (uint64_t)(A - 1))] += 0.6f;
    v[b] = hash_value(h);
  }
}

// a flat policy with a rare pass; v as above
void flat_net(const float* feats, int B, int P, int A, std::vector<float>& pi, std::vector<float>& v) {
  pi.assign((size_t)B * A, 0.f);
  v.assign(B, 0.f);
  for (int b = 0; b < B; ++b) {
    for (int a = 0; a < A; ++a) pi[(size_t)b * A + a] = (a == A - 1 ? 0.02f : 0.98f / (float)P);
    v[b] = hash_value(hash_feats(feats + (size_t)b * 17 * P, P));
  }
}

// `superko`: the settings of that part -- komi 0.5, resignation off
void* make(int N, int slots, int readouts, int games, uint64_t seed, bool superko = false) {
  agz_config c{};
  c.board_size = N;
  c.tower_height = 1;
  c.games = slots;
  c.num_readouts = readouts;
  c.parallel_readouts = 8;
  c.komi = superko ? 0.5f : 7.5f;
  c.c_puct = 0.96;
  c.dirichlet_noise_weight = 0.25;
  c.resign_threshold = superko ? -2.0 : -0.9;
  c.resign_disable_fraction = superko ? 1.0 : 0.05;
  c.seed = seed;
  c.game_id_stride = 1;
  c.record_capacity_games = games + 8;
  return hs_create(&c);
}

// self-play of `games` games to the end on `net`; each(g, G) after every step for every slot under search.
// ct: the counters as read before the last step
template <class Net, class Each>
void selfplay(void* h, int N, int slots, int games, Net net, Each each, unsigned long long* ct) {
  const int P = N * N, A = P + 1;
  std::vector<float> feats, pi, v;
  hs_start(h, games);
  for (long steps = 0; steps < 400000; ++steps) {
    hs_counters(h, ct);
    if (ct[agz::CT_FINISHED] >= (unsigned long long)games) break;
    const int B = hs_pre(h);
    if (B == 0) continue;
    feats.assign((size_t)B * 17 * P, 0.f);
    hs_leaf_features(h, feats.data());
    net(feats.data(), B, P, A, pi, v);
    hs_post(h, pi.data(), v.data());
    for (int g = 0; g < slots; ++g) {
      agz::GameState G;
      hs_game_state(h, g, &G);
      if (G.phase == agz::G_SEARCH) each(g, G);
    }
  }
}

// ---------------------------------------------------------------- explore

// a start position: `plies` moves of a fixed walk over the empty points, none of them a capture or a suicide
void walk_start(void* h, int N, int plies, std::vector<int8_t>& board, agz_position_info& info) {
  const int P = N * N;
  board.assign(P, 0);
  info = agz::empty_position_info(7.5f);
  std::vector<int8_t> tp(1), out(P);
  int32_t ko = -1, nko = -1, ncap = 0, status = 0;
  int placed = 0;
  for (int p = 0; p < P && placed < plies; p += 3) {
    tp[0] = (int8_t)info.to_play;
    int32_t mv = p;
    hs_go_play(h, board.data(), tp.data(), &ko, &mv, 1, out.data(), &nko, &ncap, &status);
    if (status != AGZ_OK) continue;
    board.assign(out.begin(), out.end());
    ko = nko;
    info.prev_move = info.last_move;
    info.last_move = p;
    info.to_play = -info.to_play;
    if (info.to_play == 1) info.caps_white += ncap; else info.caps_black += ncap;
    ++placed;
  }
  info.n = placed;
  info.ko = ko;
  info.history_len = 0;
}

long explore_play(int N, int R, uint64_t seed, int mode) {
  const int games = 8, slots = 4, A = N * N + 1;
  void* h = make(N, slots, R, games, seed);
  if (mode == 1) hs_set_playout_cap(h, 8, 0.5);
  if (mode == 2) hs_set_forced_playouts(h, 2.0, 1);
  if (mode == 3) {
    std::vector<int8_t> boards;
    std::vector<agz_position_info> infos;
    for (int plies : {4, 7, 1}) {
      std::vector<int8_t> b;
      agz_position_info f;
      walk_start(h, N, plies, b, f);
      boards.insert(boards.end(), b.begin(), b.end());
      infos.push_back(f);
    }
    hs_set_starts(h, boards.data(), infos.data(), nullptr, 3);
  }
  hs_set_root_policy_temperature(h, 1, 1.25, 1.1, (double)N);
  hs_set_root_noise(h, 10.83, 1);
  hs_set_move_temperature(h, 1, 0.75, 0.0, 2.0);
  std::vector<float> t(A), nz(A);
  std::vector<double> al(A);
  unsigned long long ct[64] = {0};
  selfplay(h, N, slots, games, hash_net,
           [&](int g, const agz::GameState& G) { hs_explore_rows(h, g, G.root, t.data(), al.data(), nz.data()); }, ct);
  unsigned long long ex[4];
  hs_explore_counts(h, ex);
  hs_counters(h, ct);
  const long recs = hs_records_count(h);
  printf("N %d mode %d: %ld records, %llu positions, explore counts %llu %llu %llu %llu\n", N, mode, recs,
         ct[agz::CT_POSITIONS], ex[0], ex[1], ex[2], ex[3]);
  const bool ok = recs == games && ex[0] > 0 && ex[1] == ex[0] && ex[2] > 0;
  hs_destroy(h);
  return ok ? recs : -1;
}

int explore() {
  long total = 0;
  for (int mode = 0; mode < 4; ++mode) {
    const long a = explore_play(5, 24, 21, mode), b = explore_play(9, 32, 22, mode);
    if (a < 0 || b < 0) {
      printf("a game set did not finish, or a counter stayed at zero\n");
      return 1;
    }
    total += a + b;
  }
  printf("%ld games played\n", total);
  return 0;
}

// ---------------------------------------------------------------- uncertainty

int uncertainty() {
  const int N = 5, A = N * N + 1, slots = 2, games = 3;
  void* h = make(N, slots, 24, games, 31);
  if (hs_set_lcb(h, 5.0, 3, 0.15) != AGZ_BAD_ARGUMENT) { printf("a rule was taken with the moments off\n"); return 1; }
  if (hs_set_value_moments(h, 1) != AGZ_OK || hs_set_lcb(h, 5.0, 3, 0.15) != AGZ_OK ||
      hs_set_puct_variance(h, 0.85, 0.4, 2.0) != AGZ_OK) {
    printf("a setter was refused\n");
    return 1;
  }
  std::vector<double> mean(A), sd(A), lcb(A);
  unsigned long long ct[64] = {0};
  double sum = 0.0;
  selfplay(h, N, slots, games, hash_net, [&](int g, const agz::GameState& G) {
    hs_child_lcb(h, g, G.root, 5.0, mean.data(), sd.data(), lcb.data());
    sum += (double)hs_node_S(h, g, G.root) + sd[A - 1] + (double)hs_node_row_S(h, g, G.root)[0];
  }, ct);
  unsigned long long u[4];
  hs_uncertainty_counts(h, u);
  const long recs = hs_records_count(h);
  printf("%ld records, %llu positions, uncertainty counts %llu %llu %llu %llu (checksum %g)\n", recs, ct[agz::CT_POSITIONS],
         u[0], u[1], u[2], u[3], sum);
  const bool ok = recs == games && u[0] > 0 && u[2] > 0;
  hs_destroy(h);
  if (!ok) {
    printf("the game set did not finish, or a counter stayed at zero\n");
    return 1;
  }
  printf("%ld games played\n", recs);
  return 0;
}

// ---------------------------------------------------------------- superko

// random legal play on 2x2 under `rule` through hs_go_keys / hs_go_legal_seen / hs_go_play; returns moves removed by the
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
      hs_go_keys(h, board.data(), &tp, 1, rule, &key);
      if (!had.insert(key).second && passes == 0) return -1;
      seen.push_back(key);
      const int64_t off[2] = {0, (int64_t)seen.size()};
      int8_t legal[A], simple[A];
      hs_go_legal_seen(h, board.data(), &tp, &ko, seen.data(), off, 1, rule, legal);
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
    hs_go_keys(h, board.data(), &tp, 1, rule, &key);
    seen.push_back(key);
    const int64_t off[2] = {0, (int64_t)seen.size()};
    hs_go_legal_seen(h, board.data(), &tp, &ko, seen.data(), off, 1, rule, legal.data());
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

int superko() {
  void* h2 = make(2, 2, 16, 6, 7, true);
  for (int rule = AGZ_KO_POSITIONAL; rule <= AGZ_KO_SITUATIONAL; ++rule) {
    const long removed = random_games(h2, rule, 40, 60);
    printf("2x2 rule %d: %ld moves removed beyond simple ko\n", rule, removed);
    if (removed <= 0) { printf("a game repeated a key, or the rule removed nothing\n"); return 1; }
  }
  void* h19 = make(19, 1, 8, 1, 7, true);
  for (int rule = AGZ_KO_POSITIONAL; rule <= AGZ_KO_SITUATIONAL; ++rule)
    if (!triple_ko(h19, rule)) { printf("triple ko: the cycle did not run, or its sixth move was allowed\n"); return 1; }
  hs_destroy(h19);
  hs_destroy(h2);
  // 3x3 self-play under the positional rule
  const int games = 8, slots = 4;
  h2 = make(3, slots, 16, games, 7, true);
  if (hs_set_ko_rule(h2, 3) != AGZ_BAD_ARGUMENT || hs_set_ko_rule(h2, AGZ_KO_POSITIONAL) != AGZ_OK) {
    printf("the setter\n");
    return 1;
  }
  unsigned long long ct[64] = {0};
  selfplay(h2, 3, slots, games, flat_net, [](int, const agz::GameState&) {}, ct);
  unsigned long long u[2];
  hs_superko_counts(h2, u);
  const long recs = hs_records_count(h2);
  printf("%ld records, superko counts %llu %llu\n", recs, u[0], u[1]);
  const bool ok = recs == games && u[0] > 0 && u[1] >= u[0];
  hs_destroy(h2);
  if (!ok) { printf("the game set did not finish, or a counter stayed at zero\n"); return 1; }
  printf("%ld games played\n", recs);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string part = argc > 1 ? argv[1] : "";
  if (part != "" && part != "explore" && part != "uncertainty" && part != "superko") {
    printf("usage: %s [explore | uncertainty | superko]\n", argv[0]);
    return 2;
  }
  if ((part == "" || part == "explore") && explore() != 0) return 1;
  if ((part == "" || part == "uncertainty") && uncertainty() != 0) return 1;
  if ((part == "" || part == "superko") && superko() != 0) return 1;
  return 0;
}

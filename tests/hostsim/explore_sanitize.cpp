// explore_sanitize.cpp -- TEST INFRASTRUCTURE: a program of its own around hostsim.cpp, for a build under
// -fsanitize=address,undefined (tests/test_explore.py).  A check of memory and undefined behaviour, not of results: it
// plays the shapes, options and counts of that test's game sets, not its networks or start positions -- 5x5 / R = 24 and 9x9 /
// R = 32, eight games each on four slots, under the root policy temperature (1.25, 1.1, N), shaped noise of 10.83 and the
// move temperature (0.75, 0, 2), plain and composed with the playout cap (8, 0.5), forced playouts (2, pruned) and a
// table of starts -- on a peaked hash network of its own, and reads the rows of every root once.
#include <cstdio>

#include "hostsim.cpp"

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

agz_config config(int N, int R, int slots, int games, uint64_t seed) {
  agz_config c{};
  c.board_size = N;
  c.tower_height = 1;
  c.games = slots;
  c.num_readouts = R;
  c.parallel_readouts = 8;
  c.komi = 7.5f;
  c.c_puct = 0.96;
  c.dirichlet_noise_weight = 0.25;
  c.resign_threshold = -0.9;
  c.resign_disable_fraction = 0.05;
  c.seed = seed;
  c.game_id_stride = 1;
  c.record_capacity_games = games + 8;
  return c;
}

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

long play(int N, int R, uint64_t seed, int mode) {
  const int games = 8, slots = 4, P = N * N, A = P + 1;
  agz_config c = config(N, R, slots, games, seed);
  void* h = hs_create(&c);
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
  hs_start(h, games);
  std::vector<float> feats, pi, v, t(A), nz(A);
  std::vector<double> al(A);
  unsigned long long ct[64] = {0};
  long steps = 0;
  for (; steps < 400000; ++steps) {
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
      if (G.phase == agz::G_SEARCH) hs_explore_rows(h, g, G.root, t.data(), al.data(), nz.data());
    }
  }
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

}  // namespace

int main() {
  long total = 0;
  for (int mode = 0; mode < 4; ++mode) {
    const long a = play(5, 24, 21, mode), b = play(9, 32, 22, mode);
    if (a < 0 || b < 0) {
      printf("a game set did not finish, or a counter stayed at zero\n");
      return 1;
    }
    total += a + b;
  }
  printf("%ld games played\n", total);
  return 0;
}

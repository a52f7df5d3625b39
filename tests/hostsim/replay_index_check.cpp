// TEST INFRASTRUCTURE: the replay arena's host-side game index (alphago.jl_amd/csrc/agz_replay_index.h) against a naive
// model, on the CPU: a few thousand seeded random operations -- what ReplayArena does with the index at ingest, window,
// trim, clear, targets-only, score and upload -- are applied to a ReplayIndex and to a plain list of games, from which
// everything the index keeps incrementally is recomputed from scratch after every operation and compared.  A program of
// its own (tests/test_replay_index.py builds it plain and under -fsanitize=address,undefined and runs both).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../alphago.jl_amd/csrc/agz_replay_index.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {                                  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }

struct Game {
  uint64_t id;
  int moves, targets;
  int64_t bytes;
  bool scored;
};

// the model: the games, the window as (first game, first entry inside it), the mode, the counters
struct Model {
  std::vector<Game> games;
  int64_t first_game = 0, first_ply = 0;
  bool targets_only = false;
  uint64_t change = 0;
  size_t uploaded = 0;

  int64_t entries(const Game& g) const { return targets_only ? g.targets : g.moves; }
  int64_t entries_before(size_t k) const {
    int64_t s = 0;
    for (size_t i = 0; i < k; ++i) s += entries(games[i]);
    return s;
  }
  int64_t bytes_before(size_t k) const {
    int64_t s = 0;
    for (size_t i = 0; i < k; ++i) s += games[i].bytes;
    return s;
  }
  int64_t positions_from(size_t k) const {
    int64_t s = 0;
    for (size_t i = k; i < games.size(); ++i) s += games[i].moves;
    return s;
  }
  int64_t positions() const { return positions_from(0); }
  int64_t live() const { return entries_before(games.size()) - entries_before((size_t)first_game) - first_ply; }
  void clear() {
    games.clear();
    first_game = first_ply = 0;
    uploaded = 0;
    ++change;
  }
  void drop_front(size_t n) {
    games.erase(games.begin(), games.begin() + n);
    if (first_game >= (int64_t)n) first_game -= (int64_t)n;
    else first_game = first_ply = 0;
    uploaded = 0;
  }
  // -> the dead games in front and whether they are dropped now
  void set_window(int64_t max_entries, int64_t* dead, bool* drop) {
    ++change;
    *dead = 0;
    *drop = false;
    if (max_entries < 0) { first_game = first_ply = 0; return; }
    const int64_t total = entries_before(games.size());
    int64_t start = entries_before((size_t)first_game) + first_ply;
    if (total - max_entries > start) start = total - max_entries;
    size_t k = (size_t)first_game;                 // the first game from there on that holds an entry behind `start`
    while (k < games.size() && entries_before(k + 1) <= start) ++k;
    if (k == games.size()) { clear(); return; }
    first_game = (int64_t)k;
    first_ply = start - entries_before(k);
    *dead = (int64_t)k;
    *drop = k > 0 && bytes_before(k) > bytes_before(games.size()) / 2;
  }
  size_t trim(int64_t max_positions) {
    ++change;
    size_t drop = 0;                               // the fewest oldest games whose loss leaves at most max_positions
    while (drop < games.size() && positions_from(drop) > max_positions) ++drop;
    if (drop > 0 && drop == games.size()) { clear(); return 0; }
    return drop;
  }
};

int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAILED op %d: %s: ", op_no, #cond);    \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      if (++failures > 20) std::exit(1);                  \
    }                                                     \
  } while (0)

int op_no = 0;

void compare(const agz::ReplayIndex& ix, const Model& m) {
  const size_t n = m.games.size();
  CHECK(ix.count() == (int64_t)n, "%lld games, model %zu", (long long)ix.count(), n);
  CHECK(ix.off().size() == n && ix.hdr().size() == n && ix.scored().size() == n && ix.cum().size() == n + 1, "sizes");
  CHECK(ix.tcum().size() == (m.targets_only ? n + 1 : 1), "tcum has %zu entries", ix.tcum().size());
  if (failures) return;
  int64_t off = 0, cum = 0, tcum = 0;
  for (size_t k = 0; k < n; ++k) {
    const Game& g = m.games[k];
    CHECK(ix.off()[k] == off && ix.cum()[k] == cum, "game %zu: off %lld cum %lld", k, (long long)ix.off()[k], (long long)ix.cum()[k]);
    CHECK(ix.hdr()[k].game_id == g.id && ix.hdr()[k].num_moves == g.moves, "game %zu: header", k);
    CHECK((ix.scored()[k] != 0) == g.scored, "game %zu: scored", k);
    if (m.targets_only) CHECK(ix.tcum()[k] == tcum, "game %zu: tcum %lld", k, (long long)ix.tcum()[k]);
    off += g.bytes;
    cum += g.moves;
    tcum += g.targets;
  }
  CHECK(ix.cum()[n] == cum && ix.positions() == cum && ix.used() == off, "totals");
  CHECK(ix.tcum().back() == (m.targets_only ? tcum : 0), "tcum total");
  CHECK(ix.first_game() == m.first_game && ix.first_ply() == m.first_ply, "window (%lld, %lld), model (%lld, %lld)",
        (long long)ix.first_game(), (long long)ix.first_ply(), (long long)m.first_game, (long long)m.first_ply);
  CHECK(ix.live() == m.live(), "live %lld, model %lld", (long long)ix.live(), (long long)m.live());
  CHECK(ix.targets_only() == m.targets_only && ix.change() == m.change, "mode / change %llu, model %llu",
        (unsigned long long)ix.change(), (unsigned long long)m.change);
  const agz::ReplayIndex::Slice s = ix.pending();
  CHECK(s.from == m.uploaded && s.to == n && (size_t)ix.uploaded() == m.uploaded, "pending [%zu, %zu), model [%zu, %zu)",
        s.from, s.to, m.uploaded, n);
}

int64_t record_bytes(int A, int nm) {
  const int64_t head = (32 + 2 * (int64_t)nm + 3) / 4 * 4;
  return (head + 4 * (int64_t)nm * (A + 1) + 7) / 8 * 8;
}

}  // namespace

int main() {
  const int kOps = 6000, A = 26;
  agz::ReplayIndex ix;
  Model m;
  std::vector<int64_t> dev_off, dev_cum, dev_tcum;      // what the uploads have left on the "device"
  uint64_t next_id = 0;
  int nonempty = 0, half_drops = 0, window_calls = 0, trims = 0, clears = 0, flips = 0, uploads = 0;
  for (op_no = 0; op_no < kOps && !failures; ++op_no) {
    const int64_t what = below(100);
    if (what < 46) {                                    // ingest of 1..4 games
      const int add = 1 + (int)below(4);
      const size_t first_new = (size_t)ix.count();
      std::vector<int32_t> counts;
      ix.touch();
      ++m.change;
      for (int i = 0; i < add; ++i) {
        Game g;
        g.id = next_id++;
        g.moves = (int)below(41);
        g.targets = (int)below(g.moves + 1);
        g.bytes = record_bytes(A, g.moves);
        g.scored = false;
        agz_game_header h{};
        h.game_id = g.id;
        h.num_moves = g.moves;
        ix.append(h, ix.used(), g.bytes);
        counts.push_back(g.targets);
        m.games.push_back(g);
      }
      if (ix.targets_only()) ix.set_targets(first_new, counts);
    } else if (what < 72) {                             // window
      const int64_t total = m.entries_before(m.games.size());
      const int64_t max_entries = below(12) == 0 ? -1 : below(total + 8);
      int64_t dead;
      bool drop;
      m.set_window(max_entries, &dead, &drop);
      const agz::ReplayIndex::Dead d = ix.set_window(max_entries);
      CHECK(d.games == dead && d.drop == drop, "set_window(%lld): dead %lld drop %d, model %lld %d", (long long)max_entries,
            (long long)d.games, (int)d.drop, (long long)dead, (int)drop);
      if (d.drop) {
        ix.drop_front((size_t)d.games);
        m.drop_front((size_t)dead);
        ++half_drops;
      }
      ++window_calls;
    } else if (what < 80) {                             // trim
      const int64_t max_positions = below(m.positions() + 8);
      const size_t want = m.trim(max_positions), got = ix.trim(max_positions);
      CHECK(got == want, "trim(%lld): drop %zu, model %zu", (long long)max_positions, got, want);
      if (got) {
        ix.drop_front(got);
        m.drop_front(want);
      }
      ++trims;
    } else if (what < 82) {                             // clear
      ix.clear();
      m.clear();
      ++clears;
    } else if (what < 90) {                             // scores come and go for a range of games
      if (!m.games.empty()) {
        const int64_t first = below((int64_t)m.games.size()), cnt = 1 + below((int64_t)m.games.size() - first);
        const bool on = below(3) != 0;
        ix.set_scored(first, cnt, on);
        for (int64_t k = first; k < first + cnt; ++k) m.games[(size_t)k].scored = on;
      }
    } else {                                            // upload what is pending; now and then the tables are replaced
      if (below(6) == 0) {
        ix.reset_upload();
        m.uploaded = 0;
        dev_off.clear();
        dev_cum.clear();
        dev_tcum.clear();
      }
      const agz::ReplayIndex::Slice s = ix.pending();
      CHECK(s.from == m.uploaded && s.to == m.games.size(), "pending before the upload");
      dev_off.resize(s.to);
      dev_cum.resize(s.to + 1);
      dev_tcum.resize(s.to + 1);
      if (s.from < s.to) {
        for (size_t k = s.from; k < s.to; ++k) dev_off[k] = ix.off()[k];
        for (size_t k = s.from; k <= s.to; ++k) dev_cum[k] = ix.cum()[k];
        if (ix.targets_only())
          for (size_t k = s.from; k <= s.to; ++k) dev_tcum[k] = ix.tcum()[k];
        ix.mark_uploaded();
        m.uploaded = s.to;
      }
      bool same = true;                                 // the device now holds the whole index
      for (size_t k = 0; k < s.to; ++k) same = same && dev_off[k] == ix.off()[k];
      for (size_t k = 0; k <= s.to && s.to > 0; ++k)
        same = same && dev_cum[k] == ix.cum()[k] && (!ix.targets_only() || dev_tcum[k] == ix.tcum()[k]);
      CHECK(same, "the uploaded tables differ from the index");
      ++uploads;
    }
    if (m.games.empty() && below(3) == 0) {             // the mode changes only while the index is empty
      const bool on = below(2) != 0;
      ix.set_targets_only(on);
      m.targets_only = on;
      m.first_game = m.first_ply = 0;
      ++m.change;
      ++flips;
    }
    compare(ix, m);
    if (!m.games.empty()) ++nonempty;
  }
  std::printf("%d operations: %d window calls (%d physical drops by the half-the-bytes rule), %d trims, %d clears, %d mode "
              "changes, %d uploads; non-empty after %d\n", kOps, window_calls, half_drops, trims, clears, flips, uploads,
              nonempty);
  if (2 * nonempty < kOps) { std::printf("FAILED: the index was non-empty after fewer than half of the operations\n"); ++failures; }
  if (half_drops < 20) { std::printf("FAILED: fewer than 20 half-the-bytes drops\n"); ++failures; }
  std::printf(failures ? "replay index check FAILED\n" : "replay index check passed\n");
  return failures ? 1 : 0;
}

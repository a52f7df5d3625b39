// superko_sim.cpp -- TEST INFRASTRUCTURE: the host simulator of tests/hostsim/hostsim.cpp with the exports of the superko
// rules added (agz_search_set_ko_rule).  A translation unit of its own around hostsim.cpp, built into
// tests/superko_sim/libsuperko_sim.so and loaded by tests/superko_twin.py only; it exports every hs_* call as well, so one
// library serves a whole Sim.
#include <map>

#include "../hostsim/hostsim.cpp"

namespace {

// what the Sim of hostsim.cpp has no place for: the key arrays once allocated (they live as long as the Sim)
struct Extra {
  uint64_t* key = nullptr;
  uint64_t* log = nullptr;
  int32_t* len = nullptr;
};
std::map<void*, Extra>& extras() {
  static std::map<void*, Extra> m;
  return m;
}

}  // namespace

extern "C" {

void hk_destroy(void* h) {
  extras().erase(h);
  hs_destroy(h);
}

// the setter: AGZ_OK, or AGZ_BAD_ARGUMENT with the setting in force kept -- an unknown rule, a call inside a select /
// incorporate window of a single tree (leaves recorded and not yet incorporated), a call while games are being played.
// The two counters restart at every call that is taken.
int hk_set_ko_rule(void* h, int rule) {
  Sim* s = (Sim*)h;
  agz::View& V = s->V;
  if (!agz_ko_rule_valid(rule)) return AGZ_BAD_ARGUMENT;
  for (int g = 0; g < V.games; ++g) {
    const agz::GameState& G = V.gs[g];
    if (G.phase == agz::G_MANUAL && G.nleaves > 0) return AGZ_BAD_ARGUMENT;
    if (G.phase != agz::G_MANUAL && G.phase != agz::G_RETIRED && G.phase != agz::G_IDLE) return AGZ_BAD_ARGUMENT;
  }
  Extra& x = extras()[h];
  if (rule != AGZ_KO_SIMPLE && !x.key) {
    alloc_one(s, x.key, (size_t)V.games * V.cap);
    alloc_one(s, x.log, (size_t)V.games * agz::sk_log_stride(V));
    alloc_one(s, x.len, (size_t)V.games);
  }
  const bool on = rule != AGZ_KO_SIMPLE;
  V.ko_rule = rule;
  V.sk_key = on ? x.key : nullptr;
  V.sk_log = on ? x.log : nullptr;
  V.sk_len = on ? x.len : nullptr;
  V.counters[agz::CT_SK_NODES] = 0;
  V.counters[agz::CT_SK_MOVES] = 0;
  return AGZ_OK;
}

int hk_ko_rule(void* h) { return ((Sim*)h)->V.ko_rule; }

// out[0] = nodes that lost at least one move, out[1] = moves removed
void hk_superko_counts(void* h, unsigned long long* out) {
  const agz::View& V = ((Sim*)h)->V;
  out[0] = V.counters[agz::CT_SK_NODES];
  out[1] = V.counters[agz::CT_SK_MOVES];
}

// a node's key under the rule in force; its position key with none
unsigned long long hk_node_key(void* h, int g, int node) {
  Sim* s = (Sim*)h;
  const long ni = agz::node_index(s->V, g, node);
  if (s->V.sk_key) return s->V.sk_key[ni];
  return agz_position_key(s->V.board + ni * s->V.PP, s->V.P, 1, AGZ_KO_SIMPLE);
}

// the key log of slot g into out [7 + max_game_length]; returns its length (0 with no rule)
int hk_game_log(void* h, int g, unsigned long long* out) {
  const agz::View& V = ((Sim*)h)->V;
  if (!V.sk_key) return 0;
  const int n = V.sk_len[g];
  for (int i = 0; i < n; ++i) out[i] = V.sk_log[(long)g * agz::sk_log_stride(V) + i];
  return n;
}

// the flags of every node slot of game g: out uint8[cap] (NF_ALLOC = 4: the node is live)
void hk_node_flags(void* h, int g, uint8_t* out) {
  const agz::View& V = ((Sim*)h)->V;
  for (int i = 0; i < V.cap; ++i) out[i] = V.meta[agz::node_index(V, g, i)].flags;
}

// ---- the two batched entries, run on SimWave
void hk_go_keys(void* h, const int8_t* boards, const int8_t* to_play, int B, int rule, unsigned long long* out) {
  Sim* s = (Sim*)h;
  SimWave w;
  for (int b = 0; b < B; ++b) {
    uint64_t k = 0;
    agz::go_key_one(w, s->V, boards + (size_t)b * s->V.P, to_play[b], rule, &k);
    out[b] = k;
  }
}
void hk_go_legal_seen(void* h, const int8_t* boards, const int8_t* to_play, const int32_t* ko,
                      const unsigned long long* seen_keys, const int64_t* seen_off, int B, int rule, int8_t* out) {
  Sim* s = (Sim*)h;
  SimWave w;
  for (int b = 0; b < B; ++b)
    agz::go_legal_seen_one(w, s->V, s->S, boards + (size_t)b * s->V.P, to_play[b], ko[b],
                           (const uint64_t*)seen_keys + seen_off[b], (int)(seen_off[b + 1] - seen_off[b]), rule,
                           out + (size_t)b * s->V.A);
}

// the header's arithmetic, for the restatement of tests/test_superko.py
unsigned long long hk_zobrist(int point, int colour) { return agz_zobrist(point, colour); }
unsigned long long hk_white_to_play() { return AGZ_ZOBRIST_WHITE_TO_PLAY; }
unsigned long long hk_position_key(const int8_t* board, int P, int to_play, int rule) {
  return agz_position_key(board, P, to_play, rule);
}

}  // extern "C"

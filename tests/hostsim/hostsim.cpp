// hostsim.cpp -- TEST INFRASTRUCTURE: a host "wave simulator" for alphago.jl_amd/csrc/agz_search.h.
//
// The search / rules logic of the engine is written once as wave-level templates.  The product
// instantiates them with agz::HipWave inside HIP kernels (agz_engine.hip).  This file
// instantiates the very same source with a lane-serial SimWave so that, in a container without
// a GPU, the tree / rules / lifecycle logic can be diffed bit-for-bit against the CPU oracle
// (tests/test_hostsim_*.py).  That includes select_leaf: there is one descent, the register-row
// form the kernels run, and SimWave runs it as a wave of one lane (kLanes = 1, which needs no
// shuffle) at the one row width that covers the largest board.  It is built into
// tests/hostsim/libhostsim.so, is loaded only by tests, and is never linked into or loaded by
// libagz.so.  It contains no network: pi/v always come from the caller.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../alphago.jl_amd/csrc/agz_layout.h"
#include "../../alphago.jl_amd/csrc/agz_search.h"

namespace {

struct SimWave {
  static constexpr int kLanes = 1;                // a wave of one lane: the descent keeps a whole row in that lane
  template <class F>
  void for_each(int n, F f) const { for (int i = 0; i < n; ++i) f(i); }
  void sync() const {}
  bool leader() const { return true; }
  int reduce_sum(int v) const { return v; }
  int reduce_min(int v) const { return v; }
  int reduce_max(int v) const { return v; }
  double reduce_max(double v) const { return v; }
  float reduce_sum_f(float v) const { return v; }
  float reduce_max_f(float v) const { return v; }
  bool any(bool v) const { return v; }
  template <class F>
  int push_desc(int n, F get, int32_t* base, int sp) const {
    for (int i = 0; i < n; ++i) {
      const int c = get(i);
      if (c >= 0) base[--sp] = c;
    }
    return sp;
  }
  void amin(int32_t* p, int v) const { if (v < *p) *p = v; }
  void amax(int32_t* p, int v) const { if (v > *p) *p = v; }
  void aor(int32_t* p, int v) const { *p |= v; }
  void count(unsigned long long* p, unsigned long long v) const { *p += v; }
  unsigned long long clock() const { return 0; }
  void count_max(unsigned long long* p, unsigned long long v) const { if (v > *p) *p = v; }
  unsigned long long fetch_add(unsigned long long* p, unsigned long long v) const {
    const unsigned long long old = *p;
    *p += v;
    return old;
  }
};

struct Sim {
  agz::View V{};
  agz::View made{};                    // V's dimensions, and the arrays of the optional groups (agz_layout.h) once made:
                                       // V's own pointers to them are null while the option is off
  std::vector<void*> bufs;
  std::vector<int8_t> sb;
  std::vector<int32_t> label, minlib, maxlib, path;
  std::vector<int8_t> flag;
  std::vector<double> dbuf;
  std::vector<float> pi, v;
  agz::Scratch S{};
  int batch = 0;
  long long an_rows = 0;               // result rows of the analysis / review run (hs_analysis_start)
};

template <class T>
void alloc_one(Sim* s, T*& p, size_t n) {
  p = (T*)calloc(n ? n : 1, sizeof(T));
  s->bufs.push_back(p);
}

// the counters [first, first + n) of an option restart at its setters (hs_start clears the enum's counters only)
void clear_counts(agz::View& V, int first, int n) {
  for (int i = 0; i < n; ++i) V.counters[first + i] = 0;
}

}  // namespace

extern "C" {

void* hs_create(const agz_config* cfg) {
  Sim* s = new Sim();
  agz::fill_dims(s->V, *cfg);
  s->made = s->V;
  agz::for_each_buffer(s->V, [&](auto*& p, size_t n) { alloc_one(s, p, n); });
  s->sb.resize(s->V.PP);
  s->label.resize(s->V.PP + 64);
  s->minlib.resize(s->V.PP);
  s->maxlib.resize(s->V.PP);
  s->flag.resize(s->V.AP);
  s->dbuf.resize(s->V.AP);
  s->path.resize(s->V.maxd);
  s->S = agz::Scratch{s->sb.data(), s->label.data(), s->minlib.data(), s->maxlib.data(),
                      s->flag.data(), s->dbuf.data(), s->path.data()};
  for (int g = 0; g < s->V.games; ++g) s->V.gs[g].phase = agz::G_RETIRED;
  return s;
}

void hs_destroy(void* h) {
  Sim* s = (Sim*)h;
  for (void* p : s->bufs) free(p);
  delete s;
}

void hs_dims(void* h, int32_t* out /*N,P,A,AP,cap,games,par,mgl,tau,maxd*/) {
  const agz::View& V = ((Sim*)h)->V;
  int32_t v[10] = {V.N, V.P, V.A, V.AP, V.cap, V.games, V.par, V.max_game_length, V.tau, V.maxd};
  memcpy(out, v, sizeof(v));
}

void hs_start(void* h, int64_t total_games) {
  Sim* s = (Sim*)h;
  s->V.total_games = total_games;
  s->V.analysis = 0;                   // back to self-play, as Engine::start
  memset(s->V.counters, 0, sizeof(unsigned long long) * agz::CT_COUNT);
  memset(s->V.ar_hdr, 0, sizeof(int32_t) * 5 * (s->V.games / 2 + 1));
  for (int g = 0; g < s->V.games; ++g) {
    memset(&s->V.gs[g], 0, sizeof(agz::GameState));
    s->V.gs[g].phase = agz::G_IDLE;
  }
}

// phase A+B for every slot, then the prefix scan that assigns batch rows
int hs_pre(void* h) {
  Sim* s = (Sim*)h;
  SimWave w;
  for (int g = 0; g < s->V.games; ++g) agz::game_pre(w, s->V, s->S, g);
  int base = 0;
  if (s->V.arena) {   // rows: [Black players' leaves | White players' leaves]
    for (int c = 0; c < 2; ++c) {
      const int before = base;
      for (int g = c; g < s->V.games; g += 2) {
        s->V.gs[g].leaf_base = base;
        base += s->V.gs[g].nleaves;
      }
      s->V.batch_count[c] = base - before;
    }
    s->batch = base;
    s->V.counters[agz::CT_STEPS] += 1;
    return base;
  }
  for (int g = 0; g < s->V.games; ++g) {
    s->V.gs[g].leaf_base = base;
    base += s->V.gs[g].nleaves;
  }
  s->batch = base;
  *s->V.batch_count = base;
  s->V.counters[agz::CT_STEPS] += 1;
  return base;
}

void hs_leaf_features(void* h, float* whcn) {
  Sim* s = (Sim*)h;
  SimWave w;
  const agz::View& V = s->V;
  for (int g = 0; g < V.games; ++g)
    for (int k = 0; k < V.gs[g].nleaves; ++k)
      agz::leaf_features(w, V, g, k, (float*)nullptr, whcn + (size_t)(V.gs[g].leaf_base + k) * 17 * V.P);
}

void hs_post(void* h, const float* pi, const float* v) {
  Sim* s = (Sim*)h;
  SimWave w;
  s->V.pi = pi;
  s->V.v = v;
  for (int g = 0; g < s->V.games; ++g) agz::game_post(w, s->V, s->S, g);
}

void hs_arena_counts(void* h, int32_t* out) {
  out[0] = ((Sim*)h)->V.batch_count[0];
  out[1] = ((Sim*)h)->V.batch_count[1];
}

void hs_counters(void* h, unsigned long long* out) {
  memcpy(out, ((Sim*)h)->V.counters, sizeof(unsigned long long) * agz::CT_COUNT);
}

int hs_live_games(void* h) {
  Sim* s = (Sim*)h;
  int n = 0;
  for (int g = 0; g < s->V.games; ++g) n += s->V.gs[g].phase != agz::G_RETIRED && s->V.gs[g].phase != agz::G_IDLE;
  return n;
}

long hs_records_count(void* h) {
  Sim* s = (Sim*)h;
  const unsigned long long f = s->V.counters[agz::CT_RECORDED];
  return (long)(f < (unsigned long long)s->V.fin_cap ? f : s->V.fin_cap);
}
void hs_record_header(void* h, long k, agz_game_header* out) { *out = ((Sim*)h)->V.fin_hdr[k]; }
void hs_record_game(void* h, long k, int16_t* moves, float* pis, float* qs) {
  const agz::View& V = ((Sim*)h)->V;
  const int nm = V.fin_hdr[k].num_moves, mgl = V.max_game_length;
  memcpy(moves, V.fin_moves + (size_t)k * mgl, sizeof(int16_t) * nm);
  memcpy(qs, V.fin_q + (size_t)k * mgl, sizeof(float) * nm);
  memcpy(pis, V.fin_pi + (size_t)k * mgl * V.A, sizeof(float) * (size_t)nm * V.A);
}

// ---- Go rules, batched
void hs_go_play(void* h, const int8_t* boards, const int8_t* to_play, const int32_t* ko, const int32_t* moves,
                int B, int8_t* boards_out, int32_t* ko_out, int32_t* ncap_out, int32_t* status_out) {
  Sim* s = (Sim*)h;
  SimWave w;
  const int P = s->V.P;
  for (int b = 0; b < B; ++b)
    agz::go_play_one(w, s->V, s->S, boards + (size_t)b * P, to_play[b], ko[b], moves[b], boards_out + (size_t)b * P,
                     ko_out + b, ncap_out + b, status_out + b);
}
void hs_go_legal(void* h, const int8_t* boards, const int8_t* to_play, const int32_t* ko, int B, int8_t* out) {
  Sim* s = (Sim*)h;
  SimWave w;
  for (int b = 0; b < B; ++b)
    agz::go_legal_one(w, s->V, s->S, boards + (size_t)b * s->V.P, to_play[b], ko[b], out + (size_t)b * s->V.A);
}
void hs_go_score(void* h, const int8_t* boards, const float* komi, int B, float* out) {
  Sim* s = (Sim*)h;
  SimWave w;
  for (int b = 0; b < B; ++b) agz::go_score_one(w, s->V, s->S, boards + (size_t)b * s->V.P, komi[b], out + b);
}

// ---- single-tree compat ops
int hs_tree_op(void* h, const agz::TreeArgs* args, int32_t* r0_out) {
  Sim* s = (Sim*)h;
  SimWave w;
  int32_t iout[4] = {0, 0, 0, 0};
  agz::TreeArgs T = *args;
  T.iout = iout;
  s->V.pi = s->pi.data();
  s->V.v = s->v.data();
  agz::tree_op(w, s->V, s->S, T);
  if (r0_out) *r0_out = iout[1];
  return iout[0];
}
void hs_set_batch_outputs(void* h, const float* pi, const float* v, int B) {
  Sim* s = (Sim*)h;
  s->pi.assign(pi, pi + (size_t)B * s->V.A);
  s->v.assign(v, v + B);
}
void hs_tree_leaf_features(void* h, int g, float* whcn) {
  Sim* s = (Sim*)h;
  SimWave w;
  for (int k = 0; k < s->V.gs[g].nleaves; ++k)
    agz::leaf_features(w, s->V, g, k, (float*)nullptr, whcn + (size_t)k * 17 * s->V.P);
}
void hs_game_state(void* h, int g, agz::GameState* out) { *out = ((Sim*)h)->V.gs[g]; }
void hs_game_set(void* h, int g, int field, double value) {
  agz::GameState& G = ((Sim*)h)->V.gs[g];
  if (field == 0) G.game_id = (uint64_t)value;
  if (field == 1) G.sel = (int32_t)value;
  if (field == 2) G.rootN = (float)value;
  if (field == 3) G.resign_threshold = value;
}
void hs_node_meta(void* h, int g, int node, agz::NodeMeta* out) {
  Sim* s = (Sim*)h;
  *out = s->V.meta[agz::node_index(s->V, g, node)];
}
void hs_node_set_n(void* h, int g, int node, int n) {
  Sim* s = (Sim*)h;
  s->V.meta[agz::node_index(s->V, g, node)].n = n;
}
float hs_node_N(void* h, int g, int node) { Sim* s = (Sim*)h; return *agz::slotN(s->V, g, node); }
float hs_node_W(void* h, int g, int node) { Sim* s = (Sim*)h; return *agz::slotW(s->V, g, node); }
void hs_node_set_N(void* h, int g, int node, float v) { Sim* s = (Sim*)h; *agz::slotN(s->V, g, node) = v; }
float* hs_node_row(void* h, int g, int node, int field) {
  Sim* s = (Sim*)h;
  const long ni = agz::node_index(s->V, g, node);
  float* base = field == 0 ? s->V.childN : field == 1 ? s->V.childW : s->V.childP;
  return base + ni * s->V.AP;
}
int32_t* hs_node_children(void* h, int g, int node) {
  Sim* s = (Sim*)h;
  return s->V.child + agz::node_index(s->V, g, node) * s->V.AP;
}
int8_t* hs_node_board(void* h, int g, int node) {
  Sim* s = (Sim*)h;
  return s->V.board + agz::node_index(s->V, g, node) * s->V.PP;
}
void hs_node_legal(void* h, int g, int node, int8_t* out) {
  Sim* s = (Sim*)h;
  const long ni = agz::node_index(s->V, g, node);
  for (int a = 0; a < s->V.A; ++a) out[a] = agz::legal_bit(s->V, ni, a);
}

// ---- the settings of self-play (agz_selfplay_set_*) and single-node entries of what they add
// the table of start positions (View::st_*, agz_selfplay_set_starts):
// boards int8[S][P], info[S], history int8[S][7][P] or NULL; S = 0 clears.  The copies live as long as the Sim.
void hs_set_starts(void* h, const int8_t* boards, const agz_position_info* info, const int8_t* history, int S) {
  Sim* s = (Sim*)h;
  agz::View& V = s->V;
  V.st_count = 0;
  V.st_board = nullptr;
  V.st_hist = nullptr;
  V.st_info = nullptr;
  if (S <= 0) return;
  const size_t P = (size_t)V.P;
  int8_t *b = nullptr, *hh = nullptr;
  agz_position_info* f = nullptr;
  alloc_one(s, b, (size_t)S * P);
  alloc_one(s, hh, (size_t)S * 7 * P);
  alloc_one(s, f, (size_t)S);
  memcpy(b, boards, (size_t)S * P);
  if (history) memcpy(hh, history, (size_t)S * 7 * P);
  memcpy(f, info, sizeof(agz_position_info) * (size_t)S);
  V.st_count = S;
  V.st_board = b;
  V.st_hist = hh;
  V.st_info = f;
}

int hs_starts_count(void* h) { return ((Sim*)h)->V.st_count; }

// root_board_valid of one candidate entry (what k_starts_valid runs per entry on the device)
int hs_start_board_valid(void* h, const int8_t* board, int ko) {
  Sim* s = (Sim*)h;
  SimWave w;
  return agz::root_board_valid(w, s->V, s->S, board, ko) ? 1 : 0;
}

// the playout cap (View::cap_fast / cap_full_prob, agz_selfplay_set_playout_cap):
// fast_readouts = 0 switches the cap off
void hs_set_playout_cap(void* h, int fast_readouts, double full_prob) {
  agz::view_set_playout_cap(((Sim*)h)->V, fast_readouts, full_prob);
}

// forced playouts and policy target pruning (View::forced_k / forced_prune, agz_selfplay_set_forced_playouts):
// k = 0 switches both rules off
void hs_set_forced_playouts(void* h, double k, int prune) {
  agz::view_set_forced_playouts(((Sim*)h)->V, k, prune);
}

// pruned_pi of node `node` of game slot g under k, whatever the setting: the scale of the node's own N, the squash of
// its own n <= tau.  out float[A]; returns whether pruning changed the row.
int hs_pruned_pi(void* h, int g, int node, double k, float* out) {
  Sim* s = (Sim*)h;
  SimWave w;
  agz::View V = s->V;
  V.forced_k = k;
  const long ni = agz::node_index(V, g, node);
  return agz::pruned_pi(w, V, s->S, ni, *agz::slotN(V, g, node), V.meta[ni].n <= V.tau, out) ? 1 : 0;
}

// the Gumbel root search (View::gumbel_m / gumbel_cvisit / gumbel_cscale, agz_selfplay_set_gumbel):
// m = 0 switches the rule off.  The two counters restart here (hs_start clears the enum's counters only).
void hs_set_gumbel(void* h, int m, double c_visit, double c_scale) {
  agz::View& V = ((Sim*)h)->V;
  agz::view_set_gumbel(V, m, c_visit, c_scale);
  clear_counts(V, agz::CT_GUMBEL_BEGUN, 2);
}

// out[0] = Gumbel searches begun, out[1] = halvings made
void hs_gumbel_counts(void* h, unsigned long long* out) {
  const agz::View& V = ((Sim*)h)->V;
  out[0] = V.counters[agz::CT_GUMBEL_BEGUN];
  out[1] = V.counters[agz::CT_GUMBEL_HALVED];
}

void hs_gumbel_state(void* h, int g, agz::GumbelState* out) { *out = ((Sim*)h)->V.gumbel[g]; }

// gumbel_pi of node `node` of game slot g under the constants given, whatever the setting.  out float[A].
void hs_gumbel_pi(void* h, int g, int node, double c_visit, double c_scale, float* out) {
  Sim* s = (Sim*)h;
  SimWave w;
  agz::View V = s->V;
  V.gumbel_cvisit = c_visit;
  V.gumbel_cscale = c_scale;
  agz::gumbel_pi(w, V, s->S, agz::node_index(V, g, node), out);
}

// The root level of a Gumbel descent on a single tree (hand rows): slot g's state becomes the `cnt` survivors `act` of
// its root, in that order, and one select_leaf runs from the root with gumbel_root_pick's action.  Returns the leaf.
int hs_gumbel_descend(void* h, int g, const int16_t* act, int cnt) {
  Sim* s = (Sim*)h;
  SimWave w;
  agz::View& V = s->V;
  agz::GumbelState& T = V.gumbel[g];
  T.n = V.meta[agz::node_index(V, g, V.gs[g].root)].n;
  T.cnt = cnt;
  for (int i = 0; i < cnt; ++i) T.act[i] = act[i];
  int plen = 0;
  return agz::select_leaf(w, V, s->S, g, V.gs[g].root, &plen, false, false, agz::gumbel_root_pick(V, g));
}

// the schedule of a search of budget n with m0 survivors: (m_p, Q_p) pairs into out, from the functions the search uses
int hs_gumbel_schedule(int n, int m0, int32_t* out, int cap) {
  int P = 1;
  while ((1 << P) < m0) ++P;
  int m = m0, left = n, k = 0;
  while (left > 0 && k < cap) {
    int q = agz::gumbel_quota(n, P, m);
    if (q > left) q = left;
    out[2 * k] = m;
    out[2 * k + 1] = q;
    ++k;
    left -= q;
    m = m == 1 ? 1 : (m / 2 > 2 ? m / 2 : 2);
  }
  return k;
}

// the PUCT rule options (View::fpu_on / fpu_r / fpu_r_root / c_base, agz_search_set_puct):
// (0, 0, 0, 0) switches the rule off.  The two counters restart here (hs_start clears the enum's counters only).
void hs_set_puct(void* h, int fpu_on, double r, double r_root, double c_base) {
  agz::View& V = ((Sim*)h)->V;
  agz::view_set_puct(V, fpu_on, r, r_root, c_base);
  clear_counts(V, agz::CT_PUCT_LEVELS, 2);
}

// out[0] = tree levels scored under an active rule, out[1] = those that picked an unvisited child
void hs_puct_counts(void* h, unsigned long long* out) {
  const agz::View& V = ((Sim*)h)->V;
  out[0] = V.counters[agz::CT_PUCT_LEVELS];
  out[1] = V.counters[agz::CT_PUCT_UNVISITED];
}

// the leaves of slot g's last select phase: nodes [par], plen [par], paths [par][maxd] (root first); returns how many
int hs_leaf_paths(void* h, int g, int32_t* nodes, int32_t* plen, int32_t* paths) {
  const agz::View& V = ((Sim*)h)->V;
  const int n = V.gs[g].nleaves;
  for (int k = 0; k < n; ++k) {
    const long li = (long)g * V.par + k;
    nodes[k] = V.leaf_node[li];
    plen[k] = V.leaf_plen[li];
    for (int i = 0; i < V.leaf_plen[li]; ++i) paths[(long)k * V.maxd + i] = V.leaf_path[li * V.maxd + i];
  }
  return n;
}

// board symmetries of the leaf evaluations (View::symmetry, agz_selfplay_set_symmetry): mode -1 = none, 0..7 = fixed,
// 8 = one drawn T_s per evaluation.  The simulator has no network: the caller evaluates leaf k under hs_leaf_syms()[k]
void hs_set_symmetry(void* h, int mode) { ((Sim*)h)->V.symmetry = mode < 0 ? 0 : mode + 1; }

// the s of every row of the batch hs_pre just assigned (out [batch]); all 0 while the mode is none
void hs_leaf_syms(void* h, int32_t* out) {
  const agz::View& V = ((Sim*)h)->V;
  for (int g = 0; g < V.games; ++g)
    for (int k = 0; k < V.gs[g].nleaves; ++k)
      out[V.gs[g].leaf_base + k] = V.symmetry ? V.leaf_sym[(long)g * V.par + k] : 0;
}

// root exploration and the move temperature (View::pt_* / noise_* / mt_*; agz_selfplay_set_root_policy_temperature,
// agz_selfplay_set_root_noise, agz_search_set_move_temperature).
// The setters check their arguments with the engine's own checks (explore_*_refusal, agz_state.h) and return AGZ_OK, or
// AGZ_BAD_ARGUMENT with the setting in force kept.  The counters restart at every setter that is taken (hs_start clears
// the enum's counters only).
int hs_set_root_policy_temperature(void* h, int on, double early, double late, double halflife) {
  agz::View& V = ((Sim*)h)->V;
  if (agz::explore_schedule_refusal(V, on, early, late, halflife, 0.1)) return AGZ_BAD_ARGUMENT;
  agz::view_set_root_policy_temperature(V, on, early, late, halflife);
  clear_counts(V, agz::CT_EXP_TEMPERED, 4);
  return AGZ_OK;
}

int hs_set_root_noise(void* h, double total_alpha, int shaped) {
  agz::View& V = ((Sim*)h)->V;
  if (agz::explore_noise_refusal(V, total_alpha, shaped)) return AGZ_BAD_ARGUMENT;
  agz::view_set_root_noise(V, total_alpha, shaped);
  clear_counts(V, agz::CT_EXP_TEMPERED, 4);
  return AGZ_OK;
}

int hs_set_move_temperature(void* h, int on, double early, double late, double halflife) {
  agz::View& V = ((Sim*)h)->V;
  if (agz::explore_schedule_refusal(V, on, early, late, halflife, 0.0)) return AGZ_BAD_ARGUMENT;
  agz::view_set_move_temperature(V, on, early, late, halflife);
  clear_counts(V, agz::CT_EXP_TEMPERED, 4);
  return AGZ_OK;
}

// out[4] = roots tempered, roots noised under total_alpha > 0, moves sampled, those off the most visited child
void hs_explore_counts(void* h, unsigned long long* out) {
  const agz::View& V = ((Sim*)h)->V;
  for (int i = 0; i < 4; ++i) out[i] = V.counters[agz::CT_EXP_TEMPERED + i];
}

// what k_tree_explore_rows runs: root_explore of `node` of slot g on a copy of its prior row; tempered float[A], alpha
// double[A], noised float[A], any may be null.  The tree is not written.
void hs_explore_rows(void* h, int g, int node, float* tempered, double* alpha, float* noised) {
  Sim* s = (Sim*)h;
  SimWave w;
  const agz::View& V = s->V;
  const long ni = agz::node_index(V, g, node);
  std::vector<float> row(V.childP + ni * V.AP, V.childP + (ni + 1) * V.AP);
  agz::root_explore(w, V, s->S, g, node, row.data(), tempered, alpha);
  if (noised) memcpy(noised, row.data(), sizeof(float) * (size_t)V.A);
}

double hs_temperature(int n, double early, double late, double halflife) {
  return agz_temperature(n, early, late, halflife);
}

// child_N of `node` of slot g := row [A]; the draw key of the slot's next pick: game id and position.n of the root
void hs_set_pick_case(void* h, int g, const float* child_N, unsigned long long game_id, int n) {
  Sim* s = (Sim*)h;
  agz::View& V = s->V;
  const long ni = agz::node_index(V, g, V.gs[g].root);
  for (int a = 0; a < V.A; ++a) V.childN[ni * V.AP + a] = child_N[a];
  V.gs[g].game_id = game_id;
  V.meta[ni].n = n;
}

// ---- value uncertainty (View::childS / rootS, lcb_* / pv_*; agz_search_set_value_moments / _set_lcb /
// _set_puct_variance).  The three setters: the engine's own checks (agz_state.h), AGZ_OK or
// AGZ_BAD_ARGUMENT with the setting in force kept; the four counters restart at every setter that is taken.  The moment
// arrays are made the first time the option goes on and live as long as the Sim.
int hs_set_value_moments(void* h, int on) {
  Sim* s = (Sim*)h;
  agz::View& V = s->V;
  if (agz::value_moments_refusal(V, on)) return AGZ_BAD_ARGUMENT;
  if (on && !s->made.childS)
    agz::for_each_moment_buffer(s->made, [&](auto*& p, size_t n) { alloc_one(s, p, n); });
  V.childS = on ? s->made.childS : nullptr;
  V.rootS = on ? s->made.rootS : nullptr;
  clear_counts(V, agz::CT_UNC_LCB, 4);
  return AGZ_OK;
}

int hs_set_lcb(void* h, double z, int min_visits, double min_ratio) {
  agz::View& V = ((Sim*)h)->V;
  if (agz::lcb_refusal(V, z, min_visits, min_ratio)) return AGZ_BAD_ARGUMENT;
  agz::view_set_lcb(V, z, min_visits, min_ratio);
  clear_counts(V, agz::CT_UNC_LCB, 4);
  return AGZ_OK;
}

int hs_set_puct_variance(void* h, double k, double prior, double prior_weight) {
  agz::View& V = ((Sim*)h)->V;
  if (agz::puct_variance_refusal(V, k, prior, prior_weight)) return AGZ_BAD_ARGUMENT;
  agz::view_set_puct_variance(V, k, prior, prior_weight);
  clear_counts(V, agz::CT_UNC_LCB, 4);
  return AGZ_OK;
}

// out[8] = moments on, z, min_visits, min_ratio, k, prior, prior_weight, 0: the setting in force
void hs_uncertainty_setting(void* h, double* out) {
  const agz::View& V = ((Sim*)h)->V;
  out[0] = V.childS ? 1.0 : 0.0;
  out[1] = V.lcb_z; out[2] = (double)V.lcb_min_visits; out[3] = V.lcb_min_ratio;
  out[4] = V.pv_k; out[5] = V.pv_prior; out[6] = V.pv_weight; out[7] = 0.0;
}

// out[4] = moves picked under the LCB rule, those off the most visited child, levels scored under a variance factor,
// those with factor > 1
void hs_uncertainty_counts(void* h, unsigned long long* out) {
  const agz::View& V = ((Sim*)h)->V;
  for (int i = 0; i < 4; ++i) out[i] = V.counters[agz::CT_UNC_LCB + i];
}

// a node's own S; the S row of its children (NULL with moments off)
float hs_node_S(void* h, int g, int node) {
  Sim* s = (Sim*)h;
  return s->V.childS ? *agz::slotS(s->V, g, node) : 0.f;
}
float* hs_node_row_S(void* h, int g, int node) {
  Sim* s = (Sim*)h;
  return s->V.childS ? s->V.childS + agz::node_index(s->V, g, node) * s->V.AP : nullptr;
}

// hand-made own statistics of slot g's root: W, and with moments on S (hs_game_set has the root's N)
void hs_root_set(void* h, int g, float W, float S) {
  Sim* s = (Sim*)h;
  s->V.gs[g].rootW = W;
  if (s->V.rootS) s->V.rootS[g] = S;
}

// what k_tree_child_lcb runs: child_lcb_rows of `node` of slot g under z; mean, sd, lcb double[A] each
int hs_child_lcb(void* h, int g, int node, double z, double* mean, double* sd, double* lcb) {
  Sim* s = (Sim*)h;
  SimWave w;
  if (!s->V.childS) return AGZ_BAD_ARGUMENT;
  agz::child_lcb_rows(w, s->V, g, node, z, mean, sd, lcb);
  return AGZ_OK;
}

// the arithmetic of include/agz_uncertainty.h and its square root, for the restatement of tests/uncertainty_twin.py
double hs_sqrt(double x) { return agz_sqrt(x); }
void hs_value_lcb(float n, float w, float s, int to_play, double z, double* out /* mean, sd, lcb */) {
  const agz_value_stats st = agz_child_stats(n, w, s);
  out[0] = st.mean;
  out[1] = st.sd;
  out[2] = agz_stats_lcb(st, (float)to_play, z);
}
double hs_variance_factor(float n, float w, float s, double k, double prior, double pw) {
  return agz_variance_factor(n, w, s, k, prior, pw);
}

// ---- superko (View::ko_rule / sk_*; agz_search_set_ko_rule).  The setter: AGZ_OK, or AGZ_BAD_ARGUMENT
// with the setting in force kept -- an unknown rule, a call inside a select / incorporate window of a single tree
// (leaves recorded and not yet incorporated), a call while games are being played.  The two counters restart at every
// call that is taken.  The key arrays are made the first time a superko rule is taken and live as long as the Sim.
int hs_set_ko_rule(void* h, int rule) {
  Sim* s = (Sim*)h;
  agz::View& V = s->V;
  if (!agz_ko_rule_valid(rule)) return AGZ_BAD_ARGUMENT;
  for (int g = 0; g < V.games; ++g) {
    const agz::GameState& G = V.gs[g];
    if (G.phase == agz::G_MANUAL && G.nleaves > 0) return AGZ_BAD_ARGUMENT;
    if (G.phase != agz::G_MANUAL && G.phase != agz::G_RETIRED && G.phase != agz::G_IDLE) return AGZ_BAD_ARGUMENT;
  }
  const bool on = rule != AGZ_KO_SIMPLE;
  if (on && !s->made.sk_key)
    agz::for_each_superko_buffer(s->made, [&](auto*& p, size_t n) { alloc_one(s, p, n); });
  V.ko_rule = rule;
  V.sk_key = on ? s->made.sk_key : nullptr;
  V.sk_log = on ? s->made.sk_log : nullptr;
  V.sk_len = on ? s->made.sk_len : nullptr;
  clear_counts(V, agz::CT_SK_NODES, 2);
  return AGZ_OK;
}

int hs_ko_rule(void* h) { return ((Sim*)h)->V.ko_rule; }

// out[0] = nodes that lost at least one move, out[1] = moves removed
void hs_superko_counts(void* h, unsigned long long* out) {
  const agz::View& V = ((Sim*)h)->V;
  out[0] = V.counters[agz::CT_SK_NODES];
  out[1] = V.counters[agz::CT_SK_MOVES];
}

// a node's key under the rule in force; its position key with none
unsigned long long hs_node_key(void* h, int g, int node) {
  Sim* s = (Sim*)h;
  const long ni = agz::node_index(s->V, g, node);
  if (s->V.sk_key) return s->V.sk_key[ni];
  return agz_position_key(s->V.board + ni * s->V.PP, s->V.P, 1, AGZ_KO_SIMPLE);
}

// the key log of slot g into out [7 + max_game_length]; returns its length (0 with no rule)
int hs_game_log(void* h, int g, unsigned long long* out) {
  const agz::View& V = ((Sim*)h)->V;
  if (!V.sk_key) return 0;
  const int n = V.sk_len[g];
  for (int i = 0; i < n; ++i) out[i] = V.sk_log[(long)g * agz::sk_log_stride(V) + i];
  return n;
}

// the flags of every node slot of game g: out uint8[cap] (NF_ALLOC = 4: the node is live)
void hs_node_flags(void* h, int g, uint8_t* out) {
  const agz::View& V = ((Sim*)h)->V;
  for (int i = 0; i < V.cap; ++i) out[i] = V.meta[agz::node_index(V, g, i)].flags;
}

// the two batched entries, run on SimWave
void hs_go_keys(void* h, const int8_t* boards, const int8_t* to_play, int B, int rule, unsigned long long* out) {
  Sim* s = (Sim*)h;
  SimWave w;
  for (int b = 0; b < B; ++b) {
    uint64_t k = 0;
    agz::go_key_one(w, s->V, boards + (size_t)b * s->V.P, to_play[b], rule, &k);
    out[b] = k;
  }
}
void hs_go_legal_seen(void* h, const int8_t* boards, const int8_t* to_play, const int32_t* ko,
                      const unsigned long long* seen_keys, const int64_t* seen_off, int B, int rule, int8_t* out) {
  Sim* s = (Sim*)h;
  SimWave w;
  for (int b = 0; b < B; ++b)
    agz::go_legal_seen_one(w, s->V, s->S, boards + (size_t)b * s->V.P, to_play[b], ko[b],
                           (const uint64_t*)seen_keys + seen_off[b], (int)(seen_off[b + 1] - seen_off[b]), rule,
                           out + (size_t)b * s->V.A);
}

// the arithmetic of include/agz_superko.h, for the restatement of tests/superko_twin.py
unsigned long long hs_zobrist(int point, int colour) { return agz_zobrist(point, colour); }
unsigned long long hs_white_to_play() { return AGZ_ZOBRIST_WHITE_TO_PLAY; }
unsigned long long hs_position_key(const int8_t* board, int P, int to_play, int rule) {
  return agz_position_key(board, P, to_play, rule);
}

// ---- batched analysis and game review (agz_analyze_start / agz_review_start; no lines, no reanalysis)
// B claimable items: positions -- or, with `moves` and `game_offset` [B + 1], the start positions of B recorded games.
// The View is set up as Engine::begin_analysis_run and Engine::review_start set it: the an_* / rv_* tables (host arrays
// here; the copies live as long as the Sim), the claim and progress counters cleared, every slot idle.  history may be
// NULL (every history_len 0).  hs_pre / hs_post step the run through game_pre / game_post.
void hs_analysis_start(void* h, const int8_t* boards, const agz_position_info* info, const int8_t* history, int64_t B,
                       const int16_t* moves, const int64_t* game_offset, uint64_t game_id_base) {
  Sim* s = (Sim*)h;
  agz::View& V = s->V;
  const size_t P = (size_t)V.P, A = (size_t)V.A, nb = (size_t)B;
  const size_t rows = game_offset ? (size_t)game_offset[B] : nb, R = rows ? rows : 1;
  int8_t *b = nullptr, *hh = nullptr;
  agz_position_info* f = nullptr;
  agz_analysis* res = nullptr;
  float* tab = nullptr;
  int16_t* mv = nullptr;
  int64_t* off = nullptr;
  alloc_one(s, b, nb * P);
  alloc_one(s, hh, nb * 7 * P);
  alloc_one(s, f, nb);
  alloc_one(s, res, R);                 // (zeroed, as clear_result_tables leaves them)
  alloc_one(s, tab, 3 * R * A);
  memcpy(b, boards, nb * P);
  if (history) memcpy(hh, history, nb * 7 * P);
  memcpy(f, info, sizeof(agz_position_info) * nb);
  V.review = game_offset ? 1 : 0;
  V.rv_moves = nullptr;
  V.rv_off = nullptr;
  if (game_offset) {
    alloc_one(s, mv, rows);
    alloc_one(s, off, nb + 1);
    memcpy(mv, moves, sizeof(int16_t) * rows);
    memcpy(off, game_offset, sizeof(int64_t) * (nb + 1));
    V.rv_moves = mv;
    V.rv_off = off;
  }
  V.analysis = 1;
  V.an_count = B;
  V.an_id_base = game_id_base;
  V.an_board = b;
  V.an_hist = hh;
  V.an_info = f;
  V.an_res = res;
  V.an_childN = tab;
  V.an_childW = tab + R * A;
  V.an_prior = tab + 2 * R * A;
  V.an_gid = nullptr;
  V.an_pi = nullptr;
  V.an_lines = V.an_pv_depth = V.an_pv_min = 0;
  V.an_line = nullptr;
  V.an_pv = nullptr;
  V.an_pvN = nullptr;
  V.an_ctr[0] = V.an_ctr[1] = 0;
  s->an_rows = (long long)rows;
  for (int g = 0; g < V.games; ++g) {
    memset(&V.gs[g], 0, sizeof(agz::GameState));
    V.gs[g].phase = agz::G_IDLE;
  }
}

// the run's result rows: res [rows], child N / W / prior [rows][A] each; returns an_ctr[1], the rows finished so far
long long hs_analysis_results(void* h, agz_analysis* res, float* child_N, float* child_W, float* prior) {
  Sim* s = (Sim*)h;
  const agz::View& V = s->V;
  const size_t n = (size_t)s->an_rows, A = (size_t)V.A;
  memcpy(res, V.an_res, sizeof(agz_analysis) * n);
  memcpy(child_N, V.an_childN, sizeof(float) * n * A);
  memcpy(child_W, V.an_childW, sizeof(float) * n * A);
  memcpy(prior, V.an_prior, sizeof(float) * n * A);
  return (long long)V.an_ctr[1];
}

// ---- analysis lines
// node_lines on `node` of slot g: out [K], pv [K][D], pv_N [K][D]
void hs_node_lines(void* h, int g, int node, int K, int D, int min_visits, agz_line* out, int16_t* pv, float* pv_N) {
  Sim* s = (Sim*)h;
  SimWave w;
  agz::node_lines(w, s->V, s->S, g, node, K, D, min_visits, out, pv, pv_N);
}

}  // extern "C"

// hostsim_explore.cpp -- TEST INFRASTRUCTURE: hostsim.cpp plus the setters of root exploration and the move temperature
// (View::pt_* / noise_* / mt_*; agz_selfplay_set_root_policy_temperature, agz_selfplay_set_root_noise,
// agz_search_set_move_temperature), their four counters and the rows call (agz_tree_explore_rows), so that the rows, the
// picks and whole games under the rules can be diffed against the Python restatement without a GPU
// (tests/explore_twin.py builds it to a library of its own with the flags of the Makefile next to it).
#include "hostsim.cpp"

namespace {
void clear_explore_counts(agz::View& V) {
  for (int i = 0; i < 4; ++i) V.counters[agz::CT_EXP_TEMPERED + i] = 0;
}
}  // namespace

extern "C" {

// The setters check their arguments with the engine's own checks (explore_*_refusal, agz_state.h) and return AGZ_OK, or
// AGZ_BAD_ARGUMENT with the setting in force kept.  The counters restart at every setter that is taken (hs_start clears
// the enum's counters only).
int hs_set_root_policy_temperature(void* h, int on, double early, double late, double halflife) {
  agz::View& V = ((Sim*)h)->V;
  if (agz::explore_schedule_refusal(V, on, early, late, halflife, 0.1)) return AGZ_BAD_ARGUMENT;
  agz::view_set_root_policy_temperature(V, on, early, late, halflife);
  clear_explore_counts(V);
  return AGZ_OK;
}

int hs_set_root_noise(void* h, double total_alpha, int shaped) {
  agz::View& V = ((Sim*)h)->V;
  if (agz::explore_noise_refusal(V, total_alpha, shaped)) return AGZ_BAD_ARGUMENT;
  agz::view_set_root_noise(V, total_alpha, shaped);
  clear_explore_counts(V);
  return AGZ_OK;
}

int hs_set_move_temperature(void* h, int on, double early, double late, double halflife) {
  agz::View& V = ((Sim*)h)->V;
  if (agz::explore_schedule_refusal(V, on, early, late, halflife, 0.0)) return AGZ_BAD_ARGUMENT;
  agz::view_set_move_temperature(V, on, early, late, halflife);
  clear_explore_counts(V);
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

}  // extern "C"

// uncertainty_sim.cpp -- TEST INFRASTRUCTURE: the host simulator of tests/hostsim/hostsim.cpp with the exports of the value
// uncertainty options added (agz_search_set_value_moments / _set_lcb / _set_puct_variance).  A translation
// unit of its own around hostsim.cpp, built into tests/uncertainty_sim/libuncertainty_sim.so and loaded by
// tests/uncertainty_twin.py only; it exports every hs_* call as well, so one library serves a whole Sim.
#include <map>

#include "../hostsim/hostsim.cpp"

namespace {

// what the Sim of hostsim.cpp has no place for: the moment arrays once allocated (they live as long as the Sim)
struct Extra {
  float* childS = nullptr;
  float* rootS = nullptr;
};
std::map<void*, Extra>& extras() {
  static std::map<void*, Extra> m;
  return m;
}

void clear_uncertainty_counts(agz::View& V) {
  for (int i = 0; i < 4; ++i) V.counters[agz::CT_UNC_LCB + i] = 0;
}

}  // namespace

extern "C" {

void hu_destroy(void* h) {
  extras().erase(h);
  hs_destroy(h);
}

// the three setters: the engine's own checks (agz_state.h), AGZ_OK or AGZ_BAD_ARGUMENT with the setting in force kept;
// the four counters restart at every setter that is taken
int hu_set_value_moments(void* h, int on) {
  Sim* s = (Sim*)h;
  agz::View& V = s->V;
  if (agz::value_moments_refusal(V, on)) return AGZ_BAD_ARGUMENT;
  Extra& x = extras()[h];
  if (on && !x.childS) {
    alloc_one(s, x.childS, (size_t)V.games * V.cap * V.AP);
    alloc_one(s, x.rootS, (size_t)V.games);
  }
  V.childS = on ? x.childS : nullptr;
  V.rootS = on ? x.rootS : nullptr;
  clear_uncertainty_counts(V);
  return AGZ_OK;
}

int hu_set_lcb(void* h, double z, int min_visits, double min_ratio) {
  agz::View& V = ((Sim*)h)->V;
  if (agz::lcb_refusal(V, z, min_visits, min_ratio)) return AGZ_BAD_ARGUMENT;
  agz::view_set_lcb(V, z, min_visits, min_ratio);
  clear_uncertainty_counts(V);
  return AGZ_OK;
}

int hu_set_puct_variance(void* h, double k, double prior, double prior_weight) {
  agz::View& V = ((Sim*)h)->V;
  if (agz::puct_variance_refusal(V, k, prior, prior_weight)) return AGZ_BAD_ARGUMENT;
  agz::view_set_puct_variance(V, k, prior, prior_weight);
  clear_uncertainty_counts(V);
  return AGZ_OK;
}

// out[8] = moments on, z, min_visits, min_ratio, k, prior, prior_weight, 0: the setting in force
void hu_setting(void* h, double* out) {
  const agz::View& V = ((Sim*)h)->V;
  out[0] = V.childS ? 1.0 : 0.0;
  out[1] = V.lcb_z; out[2] = (double)V.lcb_min_visits; out[3] = V.lcb_min_ratio;
  out[4] = V.pv_k; out[5] = V.pv_prior; out[6] = V.pv_weight; out[7] = 0.0;
}

// out[4] = moves picked under the LCB rule, those off the most visited child, levels scored under a variance factor,
// those with factor > 1
void hu_uncertainty_counts(void* h, unsigned long long* out) {
  const agz::View& V = ((Sim*)h)->V;
  for (int i = 0; i < 4; ++i) out[i] = V.counters[agz::CT_UNC_LCB + i];
}

// a node's own S; the S row of its children (NULL with moments off)
float hu_node_S(void* h, int g, int node) {
  Sim* s = (Sim*)h;
  return s->V.childS ? *agz::slotS(s->V, g, node) : 0.f;
}
float* hu_node_row_S(void* h, int g, int node) {
  Sim* s = (Sim*)h;
  return s->V.childS ? s->V.childS + agz::node_index(s->V, g, node) * s->V.AP : nullptr;
}

// hand-made own statistics of slot g's root: W, and with moments on S (hs_game_set has the root's N)
void hu_root_set(void* h, int g, float W, float S) {
  Sim* s = (Sim*)h;
  s->V.gs[g].rootW = W;
  if (s->V.rootS) s->V.rootS[g] = S;
}

// what k_tree_child_lcb runs: child_lcb_rows of `node` of slot g under z; mean, sd, lcb double[A] each
int hu_child_lcb(void* h, int g, int node, double z, double* mean, double* sd, double* lcb) {
  Sim* s = (Sim*)h;
  SimWave w;
  if (!s->V.childS) return AGZ_BAD_ARGUMENT;
  agz::child_lcb_rows(w, s->V, g, node, z, mean, sd, lcb);
  return AGZ_OK;
}

// the header's arithmetic and its square root, for the restatement of tests/uncertainty_twin.py
double hu_sqrt(double x) { return agz_sqrt(x); }
void hu_value_lcb(float n, float w, float s, int to_play, double z, double* out /* mean, sd, lcb */) {
  const agz_value_stats st = agz_child_stats(n, w, s);
  out[0] = st.mean;
  out[1] = st.sd;
  out[2] = agz_stats_lcb(st, (float)to_play, z);
}
double hu_variance_factor(float n, float w, float s, double k, double prior, double pw) {
  return agz_variance_factor(n, w, s, k, prior, pw);
}

}  // extern "C"

// hostsim_gumbel.cpp -- TEST INFRASTRUCTURE: hostsim_forced.cpp (hostsim.cpp + the starts table + the playout cap + forced
// playouts) plus the setter of the Gumbel root search (View::gumbel_m / gumbel_cvisit / gumbel_cscale,
// agz_selfplay_set_gumbel), its two counters, the slot's Sequential Halving state and an entry that runs gumbel_pi on one
// node of a tree (agz_tree_gumbel_pi), so that the search, the move and the target can be diffed against the twin
// without a GPU (tests/gumbel_twin.py builds it with the flags of the Makefile next to it).
#include "hostsim_forced.cpp"

extern "C" {

// m = 0 switches the rule off.  The two counters restart here (hs_start clears the enum's counters only).
void hs_set_gumbel(void* h, int m, double c_visit, double c_scale) {
  agz::View& V = ((Sim*)h)->V;
  V.gumbel_m = m > 0 ? m : 0;
  V.gumbel_cvisit = m > 0 ? c_visit : 0.0;
  V.gumbel_cscale = m > 0 ? c_scale : 0.0;
  V.counters[agz::CT_GUMBEL_BEGUN] = 0;
  V.counters[agz::CT_GUMBEL_HALVED] = 0;
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

}  // extern "C"

// hostsim_puct.cpp -- TEST INFRASTRUCTURE: hostsim.cpp plus the setter of the PUCT rule options (View::fpu_on / fpu_r /
// fpu_r_root / c_base, agz_search_set_puct), its two counters, the leaves of a select phase and the symmetry mode, so
// that the scores, the descents and whole games under the rule can be diffed against the Python restatement without a
// GPU (tests/puct_twin.py builds it to a library of its own with the flags of the Makefile next to it).
#include "hostsim.cpp"

extern "C" {

// (0, 0, 0, 0) switches the rule off.  The two counters restart here (hs_start clears the enum's counters only).
void hs_set_puct(void* h, int fpu_on, double r, double r_root, double c_base) {
  agz::View& V = ((Sim*)h)->V;
  agz::view_set_puct(V, fpu_on, r, r_root, c_base);
  V.counters[agz::CT_PUCT_LEVELS] = 0;
  V.counters[agz::CT_PUCT_UNVISITED] = 0;
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

}  // extern "C"

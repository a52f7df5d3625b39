// hostsim_forced.cpp -- TEST INFRASTRUCTURE: hostsim_cap.cpp (hostsim.cpp + the starts table + the playout cap) plus the
// setter of forced playouts and policy target pruning (View::forced_k / forced_prune, agz_selfplay_set_forced_playouts)
// and an entry that runs pruned_pi on one node of a tree (agz_tree_pruned_pi), so that the forced descent and the pruned
// target can be diffed against the twin without a GPU (tests/forced_twin.py builds it with the flags of the Makefile
// next to it).
#include "hostsim_cap.cpp"

extern "C" {

// k = 0 switches both rules off
void hs_set_forced_playouts(void* h, double k, int prune) {
  agz::View& V = ((Sim*)h)->V;
  V.forced_k = k > 0.0 ? k : 0.0;
  V.forced_prune = (k > 0.0 && prune) ? 1 : 0;
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

}  // extern "C"

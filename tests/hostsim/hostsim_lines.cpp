// hostsim_lines.cpp -- TEST INFRASTRUCTURE: the host wave simulator (hostsim.cpp, included as it is) plus one entry
// point for the analysis-lines templates of agz_search.h (node_lines), so that tests/test_lines.py can hold them
// against a numpy walk over the same rows without a GPU.  Built by that test into libhostsim_lines.so with the flags of
// the Makefile next to it; never linked into or loaded by libagz.so.
#include "hostsim.cpp"

extern "C" {

// node_lines on `node` of slot g: out [K], pv [K][D], pv_N [K][D]
void hs_node_lines(void* h, int g, int node, int K, int D, int min_visits, agz_line* out, int16_t* pv, float* pv_N) {
  Sim* s = (Sim*)h;
  SimWave w;
  agz::node_lines(w, s->V, s->S, g, node, K, D, min_visits, out, pv, pv_N);
}

}  // extern "C"

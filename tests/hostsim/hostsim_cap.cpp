// hostsim_cap.cpp -- TEST INFRASTRUCTURE: hostsim_starts.cpp (hostsim.cpp + the table of start positions) plus one
// entry that sets the playout cap (View::cap_fast / cap_full_prob, agz_selfplay_set_playout_cap) on a Sim, so that the
// full / fast decision of game_post and game_move_phase can be diffed against the oracle twin without a GPU
// (tests/cap_twin.py builds it with the flags of the Makefile next to it).
#include "hostsim_starts.cpp"

extern "C" {

// fast_readouts = 0 switches the cap off
void hs_set_playout_cap(void* h, int fast_readouts, double full_prob) {
  agz::View& V = ((Sim*)h)->V;
  V.cap_fast = fast_readouts > 0 ? fast_readouts : 0;
  V.cap_full_prob = fast_readouts > 0 ? full_prob : 1.0;
}

}  // extern "C"

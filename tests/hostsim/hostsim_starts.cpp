// hostsim_starts.cpp -- TEST INFRASTRUCTURE: hostsim.cpp plus one entry that sets the table of start positions
// (View::st_*, agz_selfplay_set_starts) on a Sim, so that game_start / arena_start from a table can be diffed against
// the oracle without a GPU (tests/test_starts.py builds it with the flags of the Makefile next to it).
#include "hostsim.cpp"

extern "C" {

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

}  // extern "C"

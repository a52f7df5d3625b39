// agz_layout.h -- dimensions and buffer list of the engine state (shared by the HIP engine and
// by the host wave simulator used in tests, so both allocate the same View).
#pragma once
#include <cstddef>
#include <cstdint>

#include "agz_state.h"

#if defined(__HIPCC__)
#define AGZ_SYM_FN __host__ __device__ __forceinline__
#else
#define AGZ_SYM_FN inline
#endif

namespace agz {

// ---- the eight symmetries of the board (DESIGN.md "Board symmetries"), the one definition every kernel uses and
// alphago_jl_amd.symmetry mirrors.  Point p = row + N*col (api.to_flat), p == N*N is pass.  T_s(row, col), s in 0..7:
// (1) s & 4: swap row and col; (2) s & 2: row = N-1-row; (3) s & 1: col = N-1-col.  T_0 is the identity.
// A transformed position has X'[plane][T_s(p)] = X[plane][p]; the prior of move p is net(X').pi[T_s(p)].
AGZ_SYM_FN int sym_point(int s, int N, int p) {
  if (p >= N * N) return p;
  int r = p % N, c = p / N;
  if (s & 4) { const int t = r; r = c; c = t; }
  if (s & 2) r = N - 1 - r;
  if (s & 1) c = N - 1 - c;
  return r + N * c;
}
// T_s^-1 = T_inverse(s): the reflections (s < 4, and the two transposes 4, 7) are their own inverses; the two quarter
// turns 5 and 6 are each other's (undoing "swap, then flip" flips first, and a row flip before the swap is a column
// flip after it)
AGZ_SYM_FN int sym_inverse(int s) { return s < 4 ? s : 4 | ((s & 1) << 1) | ((s >> 1) & 1); }

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

inline void fill_dims(View& V, const agz_config& c) {
  V.N = c.board_size;
  V.P = V.N * V.N;
  V.PP = round_up(V.P, 16);
  V.A = V.P + 1;
  V.AP = round_up(V.A, 16);
  V.LW = (V.A + 31) / 32;
  V.games = c.games;
  V.par = c.parallel_readouts;
  V.R = c.num_readouts;
  V.max_game_length = (V.P * 7) / 5;                      // mcts.jl:21
  V.maxd = V.max_game_length + 8;
  V.tau = ((V.P / 12) / 2) * 2;                           // mcts_play.jl:19
  V.arena = c.arena_mode ? 1 : 0;
  V.two_player = c.two_player_mode || c.arena_mode;       // evaluate(): both players are two_player_mode
  V.stagger = 0;                 // agz_debug_set_stagger (bench / soak tests only)
  // default pool: with subtree reuse a game's tree settles near R / (1 - f), f = the played child's share of the root's
  // visits (16 R covers f < 0.94); a sharp policy over a long game adds to that whatever R is, hence the term in the
  // game length (19x19, 16-32 readouts, 500 moves needed ~8000 nodes: tools/soak_selfplay.py).  A full pool is handled
  // by agz_config.pool_policy, not by stopping.
  V.cap = c.max_nodes_per_game > 0 ? c.max_nodes_per_game : 16 * c.num_readouts + 256 + 16 * V.max_game_length;
  V.pool_policy = c.pool_policy;
  V.fin_cap = c.record_capacity_games > 0 ? c.record_capacity_games : 2 * c.games + 64;
  V.total_games = 0;
  V.seed = c.seed;
  V.id_base = c.game_id_base;
  V.id_stride = c.game_id_stride ? c.game_id_stride : 1;
  V.c_puct = c.c_puct;
  V.noise_w = c.dirichlet_noise_weight;
  V.alpha = (double)(float)(0.03 * 361.0 / (double)V.A);  // mcts.jl:22 with go.jl:24
  V.resign_threshold = c.resign_threshold;
  V.resign_disable_frac = c.resign_disable_fraction;
  V.komi = c.komi;
  V.defer_expand = 0;
  V.cap_fast = 0;                // agz_selfplay_set_playout_cap
  V.cap_full_prob = 1.0;
  V.forced_k = 0.0;              // agz_selfplay_set_forced_playouts
  V.forced_prune = 0;
  V.gumbel_m = 0;                // agz_selfplay_set_gumbel
  V.gumbel_cvisit = 0.0;
  V.gumbel_cscale = 0.0;
  V.fpu_on = 0;                  // agz_search_set_puct
  V.fpu_r = 0.0;
  V.fpu_r_root = 0.0;
  V.c_base = 0.0;
  view_set_root_policy_temperature(V, 0, 0.0, 0.0, 0.0);   // agz_selfplay_set_root_policy_temperature
  view_set_root_noise(V, 0.0, 0);                          // agz_selfplay_set_root_noise
  view_set_move_temperature(V, 0, 0.0, 0.0, 0.0);          // agz_search_set_move_temperature
}

// visits every buffer of the View: f(pointer-reference, element count)
template <class F>
inline void for_each_buffer(View& V, F&& f) {
  const size_t nodes = (size_t)V.games * V.cap;
  const size_t leaves = (size_t)V.games * V.par;
  const size_t mgl = (size_t)V.max_game_length;
  f(V.childN, nodes * V.AP);
  f(V.childW, nodes * V.AP);
  f(V.childP, nodes * V.AP);
  f(V.child, nodes * V.AP);
  f(V.board, nodes * V.PP);
  f(V.meta, nodes);
  f(V.legal, nodes * V.LW);
  f(V.gs, (size_t)V.games);
  f(V.hist, (size_t)V.games * 7 * V.PP);
  f(V.freelist, nodes);
  f(V.leaf_node, leaves);
  f(V.leaf_featsrc, leaves * 8);
  f(V.leaf_tp, leaves);
  f(V.leaf_plen, leaves);
  f(V.leaf_path, leaves * V.maxd);
  f(V.pend_node, (size_t)V.games * kMaxPend);
  f(V.rec_moves, (size_t)V.games * mgl);
  f(V.rec_pi, (size_t)V.games * mgl * V.A);
  f(V.rec_q, (size_t)V.games * mgl);
  f(V.fin_hdr, (size_t)V.fin_cap);
  f(V.fin_moves, (size_t)V.fin_cap * mgl);
  f(V.fin_pi, (size_t)V.fin_cap * mgl * V.A);
  f(V.fin_q, (size_t)V.fin_cap * mgl);
  f(V.counters, (size_t)kCounterSlots);
  f(V.batch_count, (size_t)2);
  f(V.ar_hdr, (size_t)5 * (V.games / 2 + 1));        // 4 header words + 1 abort word per pair (agz_search.h)
  f(V.leaf_sym, leaves);
  f(V.eval_ord, (size_t)V.games);
  f(V.an_ctr, (size_t)2);
  f(V.an_slot, (size_t)V.games);
  f(V.gumbel, (size_t)V.games);
}

// The optional array groups, in the same form.  fill_dims and for_each_buffer leave their pointers null (off); the
// engine's setter and the simulator's allocate a group through its visitor the first time the option goes on, so the
// element counts are stated here only.
// the value moments (agz_search_set_value_moments)
template <class F>
inline void for_each_moment_buffer(View& V, F&& f) {
  f(V.childS, (size_t)V.games * V.cap * V.AP);
  f(V.rootS, (size_t)V.games);
}
// the superko keys (agz_search_set_ko_rule)
template <class F>
inline void for_each_superko_buffer(View& V, F&& f) {
  f(V.sk_key, (size_t)V.games * V.cap);
  f(V.sk_log, (size_t)V.games * sk_log_stride(V));
  f(V.sk_len, (size_t)V.games);
}

}  // namespace agz

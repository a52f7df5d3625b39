// agz_state.h -- HBM-resident state of the batched self-play engine (SoA, one pool per game).
//
// The reference keeps one heap-allocated MCTSNode per tree node, each owning a deep-copied
// GoPosition (src/mcts.jl:41-82, src/game/go/board.jl:271-315).  Here every game slot owns a
// fixed pool of `cap` node records in HBM; a node's statistics are rows of [cap*games][AP]
// arrays so that one wavefront reads a level's child_N / child_W / child_prior / child-index
// rows with fully coalesced loads.  A node stores only its own board (N*N bytes): the eight
// history planes the network needs come from its ancestors' boards (features.jl:8-14 rebuilds
// exactly those boards from deltas), plus a 7-deep per-game ring for boards older than the root.
#pragma once
#include <cstdint>

#include "../../include/agz.h"
#include "../../include/agz_draws.h"
#include "../../include/agz_superko.h"

namespace agz {

constexpr int kMaxPar = 64;        // upper bound on parallel_readouts
constexpr int kWave = 64;

enum GamePhase : int32_t {
  G_IDLE = 0, G_INIT = 1, G_INIT_WAIT = 2, G_SEARCH = 3, G_MANUAL = 4, G_RETIRED = 5,
  G_ARENA_WAIT = 6    // arena: the partner slot (other colour, other network) is to move
};

// the position every game without a start table begins at: the empty board, Black to play, komi as given
AGZ_HD inline agz_position_info empty_position_info(float komi) {
  agz_position_info f{};
  f.to_play = 1; f.ko = -1; f.last_move = -1; f.prev_move = -1; f.komi = komi;   // n, caps and history_len stay 0
  return f;
}

enum NodeFlags : uint8_t { NF_EXPANDED = 1, NF_DONE = 2, NF_ALLOC = 4 };

struct NodeMeta {
  int32_t parent;      // slot-local node id, -1 for a root
  int32_t n;           // position.n
  int32_t ko;          // point or -1
  int32_t caps_b, caps_w;
  int16_t fmove;       // action that led here (-1 for a root)
  int16_t last_move;   // recent[end].move: point, N*N for pass, -1 for none
  int16_t losses;      // losses_applied, mcts.jl:45
  int8_t to_play;
  uint8_t flags;
  int32_t pad;
};
static_assert(sizeof(NodeMeta) == 32, "NodeMeta layout");

struct GameState {
  uint64_t game_id;
  double resign_threshold;
  float rootN, rootW;        // DummyNode entries of the root, mcts.jl:27-39,96-102
  float target;              // current_readouts + readouts, selfplay.jl:24-27
  float komi;
  int32_t root;
  int32_t phase;
  int32_t sel;               // select_leaf calls since the last move (draw-stream index)
  int32_t move_count;        // length(searches_pi)
  int32_t nqs;               // length(qs)
  int32_t hist_len;          // boards of history older than the root (<= 7)
  int32_t free_top;
  int32_t nleaves;
  int32_t leaf_base;
  int32_t resign_disabled;
  int32_t err;
  int32_t result;
  int32_t was_resign;
  int32_t nodes_used;
  int32_t short_first;       // bench stagger: the first search of this game has a shortened budget
  int32_t arena_k;           // arena: games this slot has finished (= local index of the current one)
  int32_t garbage;           // nodes on the deferred-free stack (tail of the slot's free list)
  int32_t npend;             // leaves created by this step's select phase whose board update waits for k_expand
  int32_t short_searches;    // moves of this game played before their budget was spent (full pool, AGZ_POOL_MOVE_EARLY)
  int32_t stalled;           // set by game_pre: the pool is full AND this game could not move early -- it is waiting
                             // (G.err alone also reads EXHAUSTED between a refused allocation and the early move of
                             // the next step: ADVICE r5)
};
static_assert(sizeof(GameState) == 112, "GameState layout (tests/hs.py mirrors it)");

constexpr int kMaxPend = 16;    // deferred leaf expansions per game and step (2 x parallel_readouts at most)

// Gumbel root search (agz_selfplay_set_gumbel): the Sequential Halving state of one game slot's current
// search.  Kept beside GameState, not in it (tests/hs.py mirrors that layout).
constexpr int kGumbelMax = 16;  // upper bound on the root candidates m
struct GumbelState {
  int32_t n;                 // position.n of the root this state belongs to, -1 = none (game_start)
  int32_t cnt;               // survivors m_p
  int32_t budget;            // n of the search: G.target - G.rootN when it began
  int32_t P;                 // phases of the schedule: the smallest P >= 1 with 2^P >= m_0
  float end;                 // the root N at which the current phase ends
  int32_t pad;
  int16_t act[kGumbelMax];   // the survivors' actions, in rank order
};
static_assert(sizeof(GumbelState) == 56, "GumbelState layout");

enum Counter : int {
  CT_STEPS = 0, CT_POSITIONS, CT_STARTED, CT_FINISHED, CT_EVALS, CT_DUP, CT_TERMINAL, CT_ROOTVISITS,
  CT_POOL_EXHAUSTED, CT_RESIGNED, CT_CLAIMED,
  CT_RECORDED,     // records written to the finished-game ring since the last records_clear (CT_FINISHED never resets)
  // k_pre phase clocks (100 MHz ticks summed over games), written only in -DAGZ_TIMING_EXPERIMENTS builds and read
  // through agz_debug_counters (tools/pre_phases.py): games in their per-move phase / all searching games
  CT_T_FREE, CT_T_PICK, CT_T_CHILD, CT_T_REROOT, CT_T_NOISE, CT_T_MOVE_SELECT, CT_N_MOVE, CT_T_SELECT, CT_N_SELECT,
  CT_T_MOVE_MAX,   // max over games of one move phase + its select phase
  CT_T_CREATE, CT_N_CREATE,   // node_create_child (leaf expansion: board update in scratch), all callers
  CT_POOL_SHORT,   // moves played early because the pool was full
  CT_PEAK_NODES,   // max over games of nodes_used at the moment of a move
  CT_CAP_FULL, CT_CAP_FAST,   // playout cap on (View::cap_fast > 0): moves played after a full / a fast search
  // forced playouts on (View::forced_k > 0): root descents the forced rule decided / recorded pi rows that policy target
  // pruning changed (appended here: tests/hs.py pins CT_PEAK_NODES's place)
  CT_FORCED_SEL, CT_PRUNED_ROWS,
  CT_COUNT
};
// Gumbel root search on (View::gumbel_m > 0): searches begun (gumbel_begin) / halvings made (gumbel_halve).  The two
// slots after CT_PRUNED_ROWS, named outside the enum: tests/test_forced_playouts.py pins the enum's last two names.
constexpr int CT_GUMBEL_BEGUN = CT_COUNT, CT_GUMBEL_HALVED = CT_COUNT + 1;
// PUCT rule options on (puct_rule_on): tree levels a descent scored under the rule / those of them that picked an
// unvisited child.  The two slots after the Gumbel ones, outside the enum for the same reason.
constexpr int CT_PUCT_LEVELS = CT_COUNT + 2, CT_PUCT_UNVISITED = CT_COUNT + 3;
// Root exploration and the move temperature (agz_search.h root_explore / pick_move): roots tempered / roots
// noised under total_alpha > 0 / moves picked by the sampling branch of the move temperature / those of them that are
// not a most-visited child.  The four slots after the PUCT ones, outside the enum for the same reason.
constexpr int CT_EXP_TEMPERED = CT_COUNT + 4, CT_EXP_NOISED = CT_COUNT + 5, CT_EXP_SAMPLED = CT_COUNT + 6,
              CT_EXP_OFF_MAX = CT_COUNT + 7;
// Value uncertainty (agz_search.h pick_move / descend): moves picked under the LCB rule / those of them not
// on a most-visited child / tree levels a descent scored under a variance factor / those of them with factor > 1.  The
// four slots after the exploration ones, outside the enum for the same reason.
constexpr int CT_UNC_LCB = CT_COUNT + 8, CT_UNC_LCB_OFF_MAX = CT_COUNT + 9, CT_UNC_LEVELS = CT_COUNT + 10,
              CT_UNC_RAISED = CT_COUNT + 11;
// Superko (agz_search.h superko_filter): nodes that lost at least one move to the rule / moves removed.
// The two slots after the uncertainty ones, outside the enum for the same reason.
constexpr int CT_SK_NODES = CT_COUNT + 12, CT_SK_MOVES = CT_COUNT + 13;
constexpr int kCounterSlots = CT_COUNT + 14;    // what View::counters holds

struct View {
  // dimensions
  int N, P, PP, A, AP, LW, cap, games, par, maxd;
  int R, max_game_length, tau, two_player, stagger;
  int arena;           // evaluate() arena: slots 2i / 2i+1 are Black's / White's player of one game
  int pool_policy;     // AGZ_POOL_MOVE_EARLY / AGZ_POOL_STALL
  int fin_cap;
  int64_t total_games;
  uint64_t seed, id_base, id_stride;
  double c_puct, noise_w, alpha, resign_threshold, resign_disable_frac;
  float komi;
  int32_t defer_expand;   // 1: the select phase only allocates new leaves, k_expand (one wave per leaf) plays the move
  // node pools  [games*cap]
  float* childN;
  float* childW;
  float* childP;
  int32_t* child;
  int8_t* board;
  NodeMeta* meta;
  uint32_t* legal;
  // per game
  GameState* gs;
  int8_t* hist;        // [games][7][PP]
  int32_t* freelist;   // [games][cap]
  // per step leaf bookkeeping  [games][par]
  int32_t* leaf_node;
  int32_t* leaf_featsrc;  // [games][par][8]: node id >= 0, or -(h+1) for history slot h
  int8_t* leaf_tp;
  int32_t* leaf_plen;
  int32_t* leaf_path;     // [games][par][maxd]
  int32_t* pend_node;     // [games][kMaxPend]: nodes of GameState::npend
  // live game records [games][mgl]
  int16_t* rec_moves;
  float* rec_pi;          // [games][mgl][A]
  float* rec_q;
  // finished-game arena [fin_cap]
  agz_game_header* fin_hdr;
  int16_t* fin_moves;
  float* fin_pi;
  float* fin_q;
  // counters / batch
  unsigned long long* counters;
  int32_t* batch_count;   // device scalars: leaves in this step's batch ([0]; arena: [0] Black's, [1] White's players)
  int32_t* ar_hdr;        // arena mailbox [games/2][4]: {local game index, plies played, done, -}
  const float* pi;        // [batch][A]
  const float* v;         // [batch]
  // board symmetries (agz_selfplay_set_symmetry; zero = off, the View{} of the host simulator): 1 + s = every
  // evaluation under T_s, 1 + AGZ_SYMMETRY_RANDOM = one T_s per evaluation from the draw stream (AGZ_SITE_SYMMETRY)
  int32_t symmetry;
  int8_t* leaf_sym;       // [games][par]: s of each recorded leaf (written only while symmetry != 0)
  int32_t* eval_ord;      // [games]: network evaluations the slot's game has requested (the draw index)
  // analysis mode (agz_analyze_start; zero = off, the View{} of the host simulator): every slot searches caller positions
  // i = 0..an_count-1 as MCTSPlayer.suggest_move does, draw-stream game id an_id_base + i (DESIGN.md "Batched analysis")
  int32_t analysis;
  int64_t an_count;
  uint64_t an_id_base;
  unsigned long long* an_ctr;         // [2]: {next position index to claim, positions finished}
  int64_t* an_slot;                   // [games]: the position the slot is searching
  const int8_t* an_board;             // [an_count][P]
  const int8_t* an_hist;              // [an_count][7][P]: older boards newest first (history_len of them are real)
  const agz_position_info* an_info;   // [an_count]
  agz_analysis* an_res;               // [an_count]
  float* an_childN;                   // [an_count][A]: the root's rows when the search ended
  float* an_childW;
  float* an_prior;
  // review sub-mode (agz_review_start; analysis = 1 as well, zero = off): the claimed items are games j = 0..an_count-1,
  // an_board / an_hist / an_info hold their start positions, and game j's plies k write rows rv_off[j] + k of the result
  // tables (DESIGN.md "Batched game review"); G.move_count is the slot's ply k
  int32_t review;
  const int16_t* rv_moves;            // [rv_off[an_count]]: the recorded moves, game after game
  const int64_t* rv_off;              // [an_count + 1]: game j's moves and rows are rv_off[j] .. rv_off[j+1]-1
  // finished-slot hold (agz_selfplay_set_hold; zero = off, the View{} of the host simulator): a slot in G_IDLE claims its
  // next game only when agz_selfplay_release has set its flag, and clears the flag as it claims
  int32_t hold;
  int32_t* released;                  // [games]
  // analysis lines (agz_analyze_set_lines; zero = off, the View{} of the host simulator): analysis_finish also writes
  // the root's top an_lines candidates and their principal variations (node_lines, agz_search.h) into row
  // analysis_row() of three more result tables
  int32_t an_lines, an_pv_depth, an_pv_min;   // K, D, min_visits
  agz_line* an_line;                  // [rows][K]
  int16_t* an_pv;                     // [rows][K][D]
  float* an_pvN;                      // [rows][K][D]
  // start positions (agz_selfplay_set_starts; zero = off, the View{} of the host simulator and of fill_dims): self-play
  // game `gid` begins at entry gid mod st_count, arena game g (ids 2g, 2g + 1) at entry g mod st_count, and every
  // kernel that rebuilds a record's positions begins there too.  Tables of their own: analysis
  // overwrites the an_* ones
  int32_t st_count;                   // S
  const int8_t* st_board;             // [S][P]
  const int8_t* st_hist;              // [S][7][P]: older boards newest first (history_len of them are real)
  const agz_position_info* st_info;   // [S]
  // playout cap randomization (agz_selfplay_set_playout_cap; zero = off, the View{} of the host simulator and of
  // fill_dims): a self-play game about to search the root of ply n is full iff
  // agz_u01(agz_draw_u64(seed, game_id, n, AGZ_SITE_PLAYOUT_CAP, 0)) < cap_full_prob -- noise and R readouts, pi recorded;
  // otherwise fast -- no noise, cap_fast readouts, the ply's pi row all zero
  int32_t cap_fast;                   // r
  double cap_full_prob;               // p
  // forced playouts and policy target pruning (agz_selfplay_set_forced_playouts; zero = off, the View{} of the host
  // simulator and of fill_dims): in a full self-play search (and in the single-tree calls that descend from the tree's
  // root) a visited root child a with N_a^2 < forced_k * P_a * sum N is selected ahead of the PUCT arg-max; with
  // forced_prune the pi row of a full search is written by pruned_pi instead of children_as_pi
  double forced_k;                    // k
  int32_t forced_prune;
  // Gumbel root search (agz_selfplay_set_gumbel; zero = off, the View{} of the host simulator and of fill_dims): a full
  // self-play search samples up to gumbel_m root candidates by Gumbel-top-k, spends its budget on them by Sequential
  // Halving, plays the best s(a) and records softmax(logit + sigma(q)) as the pi row (agz_search.h)
  int32_t gumbel_m;                   // m
  double gumbel_cvisit, gumbel_cscale;
  GumbelState* gumbel;                // [games]
  // reanalysis (agz_replay_reanalyze_start; NULL = off, the View{} of the host simulator): a review run whose games are
  // records of the replay arena.  an_gid[j] is game j's draw-stream game id (NULL: an_id_base + j); with an_pi set,
  // analysis_finish also writes the root's children_as_pi row, the policy target self-play records
  const uint64_t* an_gid;             // [an_count]
  float* an_pi;                       // [rows][A]
  // PUCT rule options (agz_search_set_puct; zero = off, the View{} of the host simulator and of fill_dims), for every
  // level of every descent the engine makes: fpu_on -- an unvisited child's Q is its parent's value less
  // fpu_r * sqrt(visited policy mass) (fpu_r_root at the game's root) instead of 0; c_base > 0 -- c_puct grows with the
  // logarithm of the node's visits (include/agz.h states both operation for operation)
  int32_t fpu_on;
  double fpu_r, fpu_r_root;           // r, r_root
  double c_base;
  // Root exploration and the move temperature (agz_selfplay_set_root_policy_temperature / _set_root_noise,
  // agz_search_set_move_temperature; zero = off, the View{} of the host simulator and of fill_dims; include/agz_explore.h
  // states the arithmetic).  pt_on: the root prior is re-softmaxed at T(n) before the noise; noise_total >
  // 0: Dirichlet noise over the legal actions only, of that total concentration, shaped by the prior with noise_shaped;
  // mt_on: pick_move (two_player off) samples in proportion to N^(1/T(n)), and is the arg-max once T(n) <= 0.01
  int32_t pt_on, mt_on, noise_shaped;
  double pt_early, pt_late, pt_half;
  double mt_early, mt_late, mt_half;
  double noise_total;
  // Value uncertainty (agz_search_set_value_moments / _set_lcb / _set_puct_variance; zero = off, the View{} of the host
  // simulator and of fill_dims; include/agz_uncertainty.h states the arithmetic).  childS: the sum of
  // squared values beside every childW entry, rootS the root's own beside GameState::rootW (a side table: tests/hs.py
  // mirrors GameState); NULL = no moments are kept.  lcb_z > 0: the arg-max branch of pick_move takes the largest
  // lower confidence bound among the children with N_a >= lcb_min_visits and N_a >= lcb_min_ratio * max N.  pv_k > 0:
  // puct_scale is multiplied by the variance factor of the node's own (n, W, S)
  float* childS;                      // [games*cap][AP]
  float* rootS;                       // [games]
  double lcb_z, lcb_min_ratio;
  int32_t lcb_min_visits;
  double pv_k, pv_prior, pv_weight;
  float* an_childS;                   // [rows][A]: the root's S row of an analysis / review run begun with moments on
  float* an_rootS;                    // [rows]
  // Superko (agz_search_set_ko_rule; zero = off, the View{} of the host simulator and of fill_dims; include/agz_superko.h
  // states the keys and the rule).  sk_key: every node's key under the rule, written by
  // node_init_from_scratch.  sk_log: the keys of the positions a slot's game has left behind -- the history boards of the
  // install, then every old root -- and sk_len how many (a side table: tests/hs.py mirrors GameState).  NULL = off
  int32_t ko_rule;                    // AGZ_KO_*
  uint64_t* sk_key;                   // [games*cap]
  uint64_t* sk_log;                   // [games][7 + max_game_length]
  int32_t* sk_len;                    // [games]
};
// the key log of one slot holds the 7 history boards and one key per ply
AGZ_HD inline int sk_log_stride(const View& V) { return 7 + V.max_game_length; }

// option values -> View fields, for the engine's setters (which check the arguments first) and the host simulator's
inline void view_set_playout_cap(View& V, int fast_readouts, double full_prob) {
  V.cap_fast = fast_readouts > 0 ? fast_readouts : 0;
  V.cap_full_prob = fast_readouts > 0 ? full_prob : 1.0;
}
inline void view_set_forced_playouts(View& V, double k, int prune) {
  V.forced_k = k > 0.0 ? k : 0.0;
  V.forced_prune = (k > 0.0 && prune) ? 1 : 0;
}
inline void view_set_gumbel(View& V, int m, double c_visit, double c_scale) {
  V.gumbel_m = m > 0 ? m : 0;
  V.gumbel_cvisit = m > 0 ? c_visit : 0.0;
  V.gumbel_cscale = m > 0 ? c_scale : 0.0;
}
inline void view_set_puct(View& V, int fpu_on, double r, double r_root, double c_base) {
  V.fpu_on = fpu_on ? 1 : 0;
  V.fpu_r = fpu_on ? r : 0.0;
  V.fpu_r_root = fpu_on ? r_root : 0.0;
  V.c_base = c_base > 0.0 ? c_base : 0.0;
}
// The argument checks of those three setters, for the engine and the host simulator alike: null when the values are
// taken, else why not (NaN fails every range).  t_min: 0.1 for the root policy temperature, 0 for the move temperature.
// What only an engine knows -- games in flight, a select phase awaiting its incorporate -- is the engine's to add.
inline const char* explore_schedule_refusal(const View& V, int on, double early, double late, double halflife,
                                            double t_min) {
  if (V.arena) return "an arena_mode engine plays evaluate() games only";
  if (on != 0 && on != 1) return "on is not 0 or 1";
  if (!(early >= t_min && early <= 10.0)) return "early is outside the temperature range";
  if (!(late >= t_min && late <= 10.0)) return "late is outside the temperature range";
  if (!(halflife > 0.0 && halflife <= 1.0e6)) return "halflife is not in (0, 1e6]";
  return nullptr;
}
inline const char* explore_noise_refusal(const View& V, double total_alpha, int shaped) {
  if (V.arena) return "an arena_mode engine plays evaluate() games only";
  if (!(total_alpha >= 0.0 && total_alpha <= 1000.0)) return "total_alpha is not in 0 (off) .. 1000";
  if (shaped != 0 && shaped != 1) return "shaped is not 0 or 1";
  if (shaped && !(total_alpha > 0.0)) return "the shape needs total_alpha > 0";
  return nullptr;
}
inline void view_set_root_policy_temperature(View& V, int on, double early, double late, double halflife) {
  V.pt_on = on ? 1 : 0;
  V.pt_early = on ? early : 0.0;
  V.pt_late = on ? late : 0.0;
  V.pt_half = on ? halflife : 0.0;
}
inline void view_set_root_noise(View& V, double total_alpha, int shaped) {
  V.noise_total = total_alpha > 0.0 ? total_alpha : 0.0;
  V.noise_shaped = (total_alpha > 0.0 && shaped) ? 1 : 0;
}
// value uncertainty: the argument checks of the two rules (the moments' pointers are the caller's) and their stores
inline const char* lcb_refusal(const View& V, double z, int min_visits, double min_ratio) {
  if (!(z >= 0.0 && z <= 100.0)) return "z is not in 0 (off) .. 100";
  if (min_visits < 1) return "min_visits is not >= 1";
  if (!(min_ratio >= 0.0 && min_ratio <= 1.0)) return "min_ratio is not in [0, 1]";
  if (z > 0.0 && !V.childS) return "the value moments are off";
  return nullptr;
}
inline const char* puct_variance_refusal(const View& V, double k, double prior, double prior_weight) {
  if (!(k >= 0.0 && k < 1.0)) return "k is not in [0, 1)";
  if (!(prior >= 0.01 && prior <= 2.0)) return "prior is not in [0.01, 2]";
  if (!(prior_weight >= 0.0 && prior_weight <= 1000.0)) return "prior_weight is not in [0, 1000]";
  if (k > 0.0 && !V.childS) return "the value moments are off";
  return nullptr;
}
inline const char* value_moments_refusal(const View& V, int on) {
  if (on != 0 && on != 1) return "on is not 0 or 1";
  if (!on && (V.lcb_z > 0.0 || V.pv_k > 0.0)) return "a rule that reads the moments is on";
  return nullptr;
}
inline void view_set_lcb(View& V, double z, int min_visits, double min_ratio) {
  V.lcb_z = z > 0.0 ? z : 0.0;
  V.lcb_min_visits = z > 0.0 ? min_visits : 0;
  V.lcb_min_ratio = z > 0.0 ? min_ratio : 0.0;
}
inline void view_set_puct_variance(View& V, double k, double prior, double prior_weight) {
  V.pv_k = k > 0.0 ? k : 0.0;
  V.pv_prior = k > 0.0 ? prior : 0.0;
  V.pv_weight = k > 0.0 ? prior_weight : 0.0;
}
inline void view_set_move_temperature(View& V, int on, double early, double late, double halflife) {
  V.mt_on = on ? 1 : 0;
  V.mt_early = on ? early : 0.0;
  V.mt_late = on ? late : 0.0;
  V.mt_half = on ? halflife : 0.0;
}

}  // namespace agz

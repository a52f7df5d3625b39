/*
 * agz.h -- C ABI of libagz.so, the MI355X-native self-play engine for AlphaGo.jl's hot path.
 *
 * The reference has no FFI of its own: its boundary is the Julia call surface that
 * train()/evaluate()/play() and the test-suite use.  Each entry point below
 * names the reference interface it stands in for (file:line under /root/reference); the thin
 * Julia `ccall` wrapper a maintainer would add is alphago.jl_amd/julia/AlphaGoMI.jl and the
 * binding recipe is INTEGRATION.md.  Everything is extern "C", plain pointers and sizes.
 *
 * Conventions
 *   - all indices are 0-based: board point p = row + N*col (Julia's column-major linear index
 *     minus one, src/game/go/coords.jl:6-7); action a in [0, A), A = N*N + 1, a == N*N = pass.
 *   - colours: BLACK = +1, WHITE = -1, EMPTY = 0 (src/game/go/board.jl:12).
 *   - tensors cross in the layouts Flux stores them: conv [kw,kh,cin,cout] column-major,
 *     dense [out,in] column-major, features N x N x 17 x B (WHCN), pi A x B, v B.
 *   - every function returns an agz_status (0 = OK); agz_last_error() describes the last
 *     failure of that engine.  Pointers are HOST pointers unless the name says _device.
 *   - an engine handle is bound to one HIP device and is not thread-safe (the reference is
 *     single-threaded with mutable module globals, src/mcts.jl:11-13).
 *   - the engine fails loudly (AGZ_HIP_ERROR) when no gfx950 device is present; there is no
 *     CPU fallback anywhere behind this ABI.
 */
#ifndef AGZ_H
#define AGZ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGZ_VERSION 103

typedef int32_t agz_status;
#define AGZ_OK 0
#define AGZ_ILLEGAL_MOVE 1        /* IllegalMove   src/AlphaGo.jl:8, board.jl:265,470        */
#define AGZ_ASSERT_DONE_NODE 2    /* AssertionError src/mcts.jl:196                          */
#define AGZ_HISTORY_INCOMPLETE 3  /* AssertionError board.jl:568, mcts_play.jl:127           */
#define AGZ_BAD_SHAPE 4           /* AssertionError src/mcts.jl:190                          */
#define AGZ_ASSERT_SOFTPICK 5     /* AssertionError src/mcts_play.jl:67                      */
#define AGZ_BAD_ARGUMENT 6
#define AGZ_HIP_ERROR 7
#define AGZ_POOL_EXHAUSTED 8      /* a game's node pool overflowed (ours; no reference analogue) */
#define AGZ_RCCL_ERROR 9
#define AGZ_NOT_READY 10

#define AGZ_POOL_MOVE_EARLY 0
#define AGZ_POOL_STALL 1

typedef struct agz_engine agz_engine;

/* One POD for every knob of the hot path (SURVEY.md section 5 "Config / flags"):
 * GoEnv(board_size) go.jl:10; NeuralNet(env; tower_height) neural_net.jl:13;
 * MCTSPlayer(env, net; num_readouts, two_player_mode, resign_threshold) mcts_play.jl:17-18;
 * tree_search!(player, parallel_readouts) mcts_play.jl:73; komi board.jl:297;
 * c_puct / dirichlet_noise_weight mcts.jl:11-13. */
typedef struct {
  int32_t board_size;              /* N; 19 */
  int32_t tower_height;            /* residual blocks; 19 */
  int32_t games;                   /* concurrent game slots on this GPU */
  int32_t num_readouts;            /* 800 */
  int32_t parallel_readouts;       /* 8 */
  int32_t two_player_mode;         /* 0 */
  float komi;                      /* 7.5 */
  float reserved0;
  double c_puct;                   /* 0.96 */
  double dirichlet_noise_weight;   /* 0.25 */
  double resign_threshold;         /* -0.9 */
  double resign_disable_fraction;  /* 0.05, selfplay.jl:9 */
  uint64_t seed;                   /* draw-stream seed (include/agz_draws.h) */
  uint64_t game_id_base;           /* first global game id played by this engine */
  uint64_t game_id_stride;         /* id increment when a slot is recycled (= total slots) */
  int32_t max_nodes_per_game;      /* 0 = auto: 16*num_readouts + 256 + 16*max_game_length (see pool_policy) */
  int32_t device;                  /* HIP device ordinal */
  int32_t external_network;        /* 1: pi/v are supplied by the caller (duck-typed network) */
  int32_t pool_policy;             /* what a game does when its node pool is full (the reference's tree is garbage-
                                    * collected and unbounded, mcts.jl:140-147): AGZ_POOL_MOVE_EARLY (0, default) ends
                                    * the search of the current move there and plays it from the visits it has -- counted
                                    * in agz_stats.pool_short_searches and in the game's header; AGZ_POOL_STALL (1) never
                                    * shortens a search: the slot waits (agz_slot_status) until the host abandons it
                                    * (agz_slot_abandon).  Other slots keep stepping either way.  (This word was
                                    * reserved1 = 0 until round 4, and a bench-only knob before that.) */
  int32_t record_capacity_games;   /* finished-game record slots kept on the device; 0 = auto */
  int32_t arena_mode;              /* 1: evaluate() arena -- slots 2i / 2i+1 are the Black / White player of one
                                    * game with networks 0 / 1 (agz_net_select); `games` must be even */
} agz_config;

int32_t agz_version(void);
void agz_config_default(agz_config* cfg);
agz_status agz_engine_create(const agz_config* cfg, agz_engine** out);
void agz_engine_destroy(agz_engine* e);
const char* agz_last_error(const agz_engine* e);   /* e may be NULL: last create() failure */
agz_status agz_engine_sync(agz_engine* e);

/* ---------------------------------------------------------------- network ------------- */
/* NeuralNet(env; tower_height), neural_net.jl:13-33.  layer ids: 0 = stem conv+BN;
 * 1..2*tower = tower convs (block b, conv c -> 1 + 2b + c); negative = heads. */
#define AGZ_L_VALUE_CONV (-1)
#define AGZ_L_POLICY_CONV (-2)
#define AGZ_L_VALUE_FC1 (-3)
#define AGZ_L_VALUE_FC2 (-4)
#define AGZ_L_POLICY_FC (-5)
#define AGZ_K_WEIGHT 0
#define AGZ_K_BIAS 1
#define AGZ_K_BN_BETA 2
#define AGZ_K_BN_GAMMA 3
#define AGZ_K_BN_MEAN 4
#define AGZ_K_BN_VAR 5
#define AGZ_K_BN_EPS 6
/* copies `count` floats (caller keeps ownership); Flux layouts, kernel flip done inside */
agz_status agz_net_set_weights(agz_engine* e, int32_t layer, int32_t kind, const float* data,
                               int64_t count);
int64_t agz_net_param_count(const agz_engine* e, int32_t layer, int32_t kind);
/* read a parameter back in the layout it was set in (save_model, train.jl:14-35) */
agz_status agz_net_get_weights(agz_engine* e, int32_t layer, int32_t kind, float* out, int64_t count);
/* evaluate(env, black_net, white_net) neural_net.jl:103-158 needs two networks in one engine
 * (arena_mode): `which` = 0 (Black's, the default) or 1 (White's) selects the network that the
 * agz_net_set_weights / get_weights / init_synthetic / forward* calls after it address. */
agz_status agz_net_select(agz_engine* e, int32_t which);
/* Flux-default-equivalent init from the draw stream (glorot-uniform, zero bias, BN identity,
 * eps 1e-5) -- the synthetic weights of SURVEY.md 8d */
agz_status agz_net_init_synthetic(agz_engine* e, uint64_t seed);
/* (nn)(positions::Vector{Position}) -> (pi A x B, v B), neural_net.jl:57-68.
 * Position SoA: boards int8[B][N*N]; deltas int8[B][7][N*N] newest first; ndeltas int32[B];
 * to_play int8[B]. */
agz_status agz_net_forward(agz_engine* e, const int8_t* boards, const int8_t* deltas,
                           const int32_t* ndeltas, const int8_t* to_play, int32_t B,
                           float* pi_out, float* v_out);
/* same on a feature tensor N x N x 17 x B already in host memory */
agz_status agz_net_forward_features(agz_engine* e, const float* feats, int32_t B, float* pi_out,
                                    float* v_out);
/* Board symmetries (ours; the reference evaluates one orientation, features.jl:3-26).  Point p = row + N*col; for s in
 * 0..7, T_s(row, col) does, in order: s & 4 swap row and col; s & 2 row = N-1-row; s & 1 col = N-1-col.  T_0 is the
 * identity, pass maps to pass; the quarter turns 5 and 6 are each other's inverse, every other T_s is its own.  A row
 * of features under T_s is X'[plane][T_s(p)] = X[plane][p]; the prior of move p is then net(X').pi[T_s(p)].
 * agz_net_forward_features_sym: feature rows as agz_net_forward_features takes them ([plane][p] per row), row b is
 * evaluated under T_sym[b], sym[b] in 0..7, and its pi comes back in board orientation (pi[p] = pi_net[T_s(p)], pass
 * unchanged); v is the network's value of the transformed row. */
agz_status agz_net_forward_features_sym(agz_engine* e, const float* feats, const int32_t* sym, int32_t B, float* pi,
                                        float* v);
/* get_feats(pos) -> N x N x 17 (x B), features.jl:3-26 */
agz_status agz_features(agz_engine* e, const int8_t* boards, const int8_t* deltas,
                        const int32_t* ndeltas, const int8_t* to_play, int32_t B, float* out);
/* micro-benchmark hook: run the network `iters` times on B resident synthetic positions and
 * return the average milliseconds per forward (HIP events on the engine's stream) */
agz_status agz_net_time_forward(agz_engine* e, int32_t B, int32_t iters, float* ms_out);
/* average duration (ms) of the dominant 3x3 256->256 conv launch over the same kind of run */
agz_status agz_net_time_conv(agz_engine* e, int32_t B, int32_t iters, float* ms_out);

/* tower-convolution algorithm: 1 (default) = Winograd on the f32 MFMA -- F(3x3,3x3), and for boards of 13x13 and
 * larger in the exact-f32 arithmetic F(4x4,3x3) (a quarter fewer multiplies at 19x19); 2 = Winograd F(3x3,3x3) on every
 * board size (comparison runs); 0 = direct implicit GEMM on the f32 MFMA; 3 = 1 with the tower layers of boards whose tile
 * blocks hold whole boards (N <= 12) on the five-pass 64-tile x 128-cout form of F(3x3,3x3) (agz_wino5.hip: 25 % fewer
 * operand bytes per flop, the same layer time within 0.5 % on the 9x9 headline -- opt-in, tests/test_gpu_wino5.py).  All
 * are f32 end to end; they differ by rounding only (each within 1e-4 of the float64 network: tests/test_gpu_nn.py,
 * tests/test_gpu_configs.py). */
agz_status agz_net_set_winograd(agz_engine* e, int32_t on);
/* the f32 Winograd tower as one launch per layer (0, default) or as ONE persistent launch over all its layers (1: used
 * wherever it applies -- board sizes whose tile blocks hold whole boards (N <= 12), a 256-CU device).  The same device
 * function does the work either way: outputs are bit-identical (tests/test_gpu_tower.py).  The persistent form needs
 * 3.7 % fewer cycles (no partly filled last workgroup round per layer) and, on a power-limited MI355X, runs at a
 * clock 4 % lower: the same wall time (HISTORY.md 4f). */
agz_status agz_net_set_tower_persistent(agz_engine* e, int32_t on);
/* the Winograd tower of a large batch as n = 1..4 independent layer chains (default 2): ranges of the batch's tile blocks, cut
 * at board boundaries, run their layers on n HIP streams and the hardware interleaves their workgroups (-5 % per forward
 * at 19x19 / 2048 positions, -1.6 % per step at 9x9 / 8192: the CUs stop moving through K loops and store bursts in
 * lockstep).  Same kernels, same rows: outputs are bit-identical for every n (tests/test_gpu_tower.py).  Small batches
 * (fewer than 256 tile blocks per chain) run as one chain. */
agz_status agz_net_set_tower_streams(agz_engine* e, int32_t n);
/* tower arithmetic of the network selected by agz_net_select.  AGZ_PRECISION_F32 (default): exact
 * f32 end to end -- the parity target of BASELINE.json's metric.  AGZ_PRECISION_F16: the "fp16 MFMA
 * path" of BASELINE.json configs[4]: tower activations and weights are rounded to IEEE half, products
 * accumulate in f32 (v_mfma_f32_32x32x16_f16); stem, heads, BatchNorm affine and residual adds stay
 * f32.  Mixed-precision inference: outputs agree with the f32 network to ~1e-3, not 1e-4. */
#define AGZ_PRECISION_F32 0
#define AGZ_PRECISION_F16 1
/* AGZ_PRECISION_F32S: the f32 network of AGZ_PRECISION_F32 -- f32 activations, weights, accumulation, BatchNorm,
 * residuals -- with the OPERANDS of the Winograd GEMMs carried as two IEEE halves each (x ~ hi + lo, 22 mantissa
 * bits instead of 24) so that the products run on the fp16 MFMA (v_mfma_f32_32x32x16_f16, all four cross products,
 * exact in f32) at 4x the f32 MFMA rate.  Opt-in; NOT what bench.py measures by default.  Outputs agree with the
 * float64 oracle to ~1e-6 (bar 1e-4, tests/test_gpu_nn32s.py). */
#define AGZ_PRECISION_F32S 2
agz_status agz_net_set_precision(agz_engine* e, int32_t precision);

/* HIP-event timing of every 3x3 256->256 tower-conv launch issued by subsequent steps /
 * forwards (up to 4096 launches), on the engine's own stream.  read() synchronises and returns
 * the summed launch time, the summed ALGORITHMIC flops (2 * rows * 9 * 256 * 256 with the rows
 * each launch actually processed) and the launch count. */
agz_status agz_profile_conv_enable(agz_engine* e, int32_t on);
agz_status agz_profile_conv_read(agz_engine* e, double* total_ms, double* total_flop, int64_t* launches);
/* The same for the search kernels of agz_selfplay_step (SURVEY.md 8d asks for them as HBM GB/s beside the tower's
 * TFLOP/s): HIP events on the engine's stream around k_pre (select_leaf / pick_move / play_move!, mcts.jl:108-138,
 * mcts_play.jl:52-71,126-139), k_expand (maybe_add_child!'s play_move!, mcts.jl:140-147, board.jl:451-509), k_scan,
 * k_leaf_features (features.jl:3-26) and k_post (incorporate_results! / backup_value!, mcts.jl:186-225) of the next
 * <= 512 steps.  read() synchronises; ms5 = summed milliseconds in that order. */
agz_status agz_profile_search_enable(agz_engine* e, int32_t on);
agz_status agz_profile_search_read(agz_engine* e, double* ms5 /* [5] */, int64_t* steps);

/* ---------------------------------------------------------------- Go rules (batched) --- */
/* play_move!(pos, c), board.jl:451-509 / pass_move! :426-440.  In/out SoA per position:
 * boards int8[B][N*N], to_play int8[B], ko int32[B] (-1 = none), moves int32[B].
 * status_out[b] = AGZ_OK or AGZ_ILLEGAL_MOVE (then the outputs for b repeat the input). */
agz_status agz_go_play(agz_engine* e, const int8_t* boards, const int8_t* to_play, const int32_t* ko,
                       const int32_t* moves, int32_t B, int8_t* boards_out, int32_t* ko_out,
                       int32_t* ncaptured_out, int32_t* status_out);
/* all_legal_moves(pos) -> Int8[A], board.jl:393-424 */
agz_status agz_go_legal(agz_engine* e, const int8_t* boards, const int8_t* to_play, const int32_t* ko,
                        int32_t B, int8_t* legal_out /* [B][A] */);
/* score(pos) board.jl:511-533 (area - komi, Black-positive) */
agz_status agz_go_score(agz_engine* e, const int8_t* boards, const float* komi, int32_t B,
                        float* score_out);

/* ---------------------------------------------------------------- batched self-play ----- */
/* selfplay(env, nn, num_ro) selfplay.jl:1-45, many games at once.  Start (re)initialises
 * every slot; each step is one tree_search! (mcts_play.jl:73-98) for every live game plus the
 * per-move phase for games whose readout budget is spent; finished games are recorded and
 * their slot recycled until `total_games` have been started (0 = recycle forever). */
agz_status agz_selfplay_start(agz_engine* e, int64_t total_games);
agz_status agz_selfplay_step(agz_engine* e, int32_t nsteps);          /* asynchronous */
/* Board symmetries in the engine's own network evaluations (AlphaGo Zero's random-symmetry leaf evaluation; T_s as at
 * agz_net_forward_features_sym).  mode AGZ_SYMMETRY_NONE (-1, the default): one orientation, the reference's search;
 * 0..7: every evaluation under T_mode; AGZ_SYMMETRY_RANDOM (8): evaluation e of a game (0-based, in the order the
 * game sends leaves to the network; terminal leaves are not evaluated and not counted) is made under
 * T_s, s = agz_index(agz_draw_u64(seed, game_id, 0, AGZ_SITE_SYMMETRY, e), 8) (include/agz_draws.h).  The leaf's
 * features are transformed, the network runs, its pi goes back to board orientation before it becomes the leaf's
 * priors.  Covers agz_selfplay_step (arena_mode: both networks) and agz_tree_search / agz_tree_search_incorporate
 * with pi == NULL; a pi the caller hands in is taken as it is.  Takes effect at the next step / select; refused
 * (AGZ_BAD_ARGUMENT) for a mode outside -1..8, with external_network = 1, and between agz_tree_search_select and
 * agz_tree_search_incorporate.  The evaluation counter e counts every leaf the game sends to the network, with the
 * mode on or off (a mode switched on mid-game continues the game's ordinal), and restarts with every game
 * (agz_selfplay_start's games, agz_tree_init). */
#define AGZ_SYMMETRY_NONE (-1)
#define AGZ_SYMMETRY_RANDOM 8
agz_status agz_selfplay_set_symmetry(agz_engine* e, int32_t mode);
/* The hold of train() (ours; train.jl:56-57 plays game i + 1 on the weights _train left after game i).  With the hold
 * on, a slot that finishes a game records it as usual and parks in G_IDLE instead of taking its next game in the same
 * step; agz_selfplay_release lets every slot parked at that moment claim its next game id (game_id_base + k * stride,
 * the usual rule) at the next step, so a host that trains between the two calls starts every later game on the trained
 * weights.  agz_selfplay_start's fresh slots wait for a first release too.  set_hold clears pending releases; it is
 * refused in arena_mode.  Hold off (the default): the step is unchanged. */
agz_status agz_selfplay_set_hold(agz_engine* e, int32_t on);
agz_status agz_selfplay_release(agz_engine* e);                     /* asynchronous */
typedef struct {
  int64_t steps;               /* tree_search! rounds executed                          */
  int64_t positions;           /* self-play moves played (= searches_pi entries)        */
  int64_t games_started;
  int64_t games_finished;
  int64_t evals;               /* network evaluations (leaves sent to the NN)            */
  int64_t duplicate_evals;     /* evaluations discarded by revert_visits! (mcts.jl:173)  */
  int64_t terminal_visits;     /* select_leaf hits on finished positions                */
  int64_t root_visits;         /* sum of N(root) increments                             */
  int64_t nodes_in_use;
  int64_t pool_exhausted;      /* allocations refused by a full pool (see pool_policy)  */
  int64_t resigned_games;
  int64_t live_games;
  int64_t records_dropped;     /* finished games overwritten in the record ring since the last
                                * agz_records_clear (ring = record_capacity_games): drain more often */
  int64_t pool_short_searches; /* moves played before their readout budget was spent because the game's pool was
                                * full (AGZ_POOL_MOVE_EARLY); 0 = every move had the reference's R readouts */
  int64_t peak_nodes_per_game; /* largest tree any slot has held at the moment it moved (of max_nodes_per_game) */
  int64_t stalled_games;       /* slots waiting on a full pool right now (AGZ_POOL_STALL, or no visited child to play) */
  int64_t node_capacity;       /* max_nodes_per_game in effect */
  int64_t abandoned_games;     /* games given up by agz_slot_abandon: they produce no record, so a run started with
                                * agz_selfplay_start(total) is over when games_finished + abandoned_games == total */
} agz_stats;
agz_status agz_engine_stats(agz_engine* e, agz_stats* out);            /* synchronises */
/* Per slot (arrays of `games` int32, any of them may be NULL): status = AGZ_OK or AGZ_POOL_EXHAUSTED (the game is
 * waiting on a full node pool: agz_config.pool_policy), nodes its tree holds, moves it has played.  The reference has
 * no analogue (its tree is unbounded, mcts.jl:140-147, mcts_play.jl:48); synchronises. */
agz_status agz_slot_status(agz_engine* e, int32_t* status_out, int32_t* nodes_out, int32_t* moves_out);
/* give up the game in `slot` without a record (counted in agz_stats.abandoned_games; its game id is not played again); the
 * slot starts the next game id at the next step */
agz_status agz_slot_abandon(agz_engine* e, int32_t slot);
/* external-network mode (MCTSPlayer.network duck typing, mcts_play.jl:5,89): after a step's
 * select phase the caller reads the leaf feature tensor and supplies pi/v. */
agz_status agz_selfplay_select(agz_engine* e, int32_t* nleaves_out);
agz_status agz_selfplay_leaf_features(agz_engine* e, float* feats_out /* N x N x 17 x B */);
agz_status agz_selfplay_incorporate(agz_engine* e, const float* pi /* A x B */, const float* v);

/* finished-game records: extract_data(player), mcts_play.jl:126-139 */
typedef struct {
  uint64_t game_id;
  int32_t num_moves;           /* position.n == length(searches_pi)                      */
  int32_t result;              /* +1 Black, -1 White, 0 draw (Black-absolute)             */
  int32_t was_resign;
  int32_t resign_disabled;
  float final_score;           /* score(position) when not resigned                       */
  int32_t short_searches;      /* moves of this game played on fewer than num_readouts readouts (full node pool,
                                * AGZ_POOL_MOVE_EARLY); 0 for a game that is the reference's game */
} agz_game_header;
int64_t agz_records_count(agz_engine* e);                               /* synchronises */
agz_status agz_records_header(agz_engine* e, int64_t k, agz_game_header* out);
/* moves int16[num_moves] (action index), pis float[num_moves][A], qs float[num_moves] */
agz_status agz_records_game(agz_engine* e, int64_t k, int16_t* moves, float* pis, float* qs);
/* packed export for the replay all-gather: writes every finished record as
 * [header | moves | pis | qs] back to back; returns bytes via nbytes_out. dst may be a host
 * or a device pointer (is_device). */
agz_status agz_records_packed_size(agz_engine* e, int64_t* nbytes_out);
agz_status agz_records_export_packed(agz_engine* e, void* dst, int64_t capacity, int32_t is_device);
agz_status agz_records_clear(agz_engine* e);
/* the value targets y_0 .. y_{num_moves-1} of ring record k under (alpha, lambda) (agz_replay_set_value_target states
 * the rule): out float[num_moves].  Numbering and refusals of agz_records_game; AGZ_BAD_ARGUMENT also for alpha or
 * lambda outside [0, 1] or NaN.  alpha = 0: every entry is (float)result. */
agz_status agz_records_value_targets(agz_engine* e, int64_t k, double alpha, double lambda, float* out);
/* the same for a record the caller holds (no engine, no device): qs float[T], out float[T]; the host loop over
 * agz_value_target of include/agz_value_target.h that the Python and Julia mirrors call */
agz_status agz_value_targets(const float* qs, int32_t T, int32_t result, double alpha, double lambda, float* out);
/* arena_mode with external_network: after agz_selfplay_select, counts_out[0] leaves belong to Black
 * players (network 0) and counts_out[1] to White players (network 1); agz_selfplay_leaf_features
 * and agz_selfplay_incorporate order the rows [Black players' | White players'].  A finished
 * arena game is one record: game_id = 2*game + colour of the player that ended it, moves, qs =
 * Q(root) of the mover, pis zero (two_player_mode records none, mcts_play.jl:33-36), result = what
 * set_result! stored, final_score = score(final position) -- evaluate's tally (:147) is
 * final_score > 0, also for resigned games. */
agz_status agz_arena_counts(agz_engine* e, int32_t* counts_out);
/* replay_position(pos, result) board.jl:557-578 on the device: rebuild the feature tensors of
 * every position of record k: out float[num_moves][N*N*17] (WHC per position) */
agz_status agz_records_features(agz_engine* e, int64_t k, float* out);
/* get_replay_batch(pos_buffer, ...) train.jl:4-12, feature side, for records from ANY rank: the
 * caller keeps games as action lists (moves int16[nmoves], games back to back); sample b is the
 * position before move ply[b] of the game starting at moves[game_offset[b]] (ply 0 = empty board).
 * One wave per sample replays the game on the device (board.jl:557-578) and writes
 * out float[B][N*N*17] (same WHC order as agz_features); out may be a device pointer. */
agz_status agz_replay_features(agz_engine* e, const int16_t* moves, int64_t nmoves,
                               const int32_t* game_offset, const int32_t* ply, int32_t B, float* out,
                               int32_t out_is_device);
/* agz_replay_features for hosts that keep the move lists of games played from a table of start positions
 * (agz_selfplay_set_starts): sample b's move list begins at entry start[b] of the table in force, -1 = the empty
 * board; ply 0 is the start position itself.  start = NULL is agz_replay_features. */
agz_status agz_replay_features_starts(agz_engine* e, const int16_t* moves, int64_t nmoves,
                                      const int32_t* game_offset, const int32_t* ply, const int32_t* start, int32_t B,
                                      float* out, int32_t out_is_device);

/* ---------------------------------------------------------------- replay arena + exchange -- */
/* The replay buffer of train() (pos_buffer / pi_buffer / res_buffer, train.jl:47-66) as a device-resident
 * arena of packed game records: games of EVERY rank, in arrival order, addressed by index 0..count-1.
 * A (game, ply) pair is a training sample: position before move `ply` (rebuilt on the device by
 * replay_position, board.jl:557-578), pi = searches_pi[ply], z = result (extract_data, mcts_play.jl:126-139). */
/* append packed records ([header | moves | pis | qs] as written by agz_records_export_packed) from a host or
 * device buffer, e.g. games loaded from disk or received by other means; added_out may be NULL */
agz_status agz_replay_ingest_packed(agz_engine* e, const void* packed, int64_t nbytes, int32_t is_device,
                                    int64_t* added_out);
/* the same for the receive buffer of a padded all-gather the HOST performed with its own communication library
 * (MPI.jl, Distributed): `world` chunks of `chunk_stride` bytes, chunk r holding counts[2r] records in its first
 * counts[2r+1] bytes (what agz_records_count / agz_records_packed_size said on rank r).  This is also the second
 * half of agz_allgather_records (which does the gather itself over RCCL). */
agz_status agz_replay_ingest_gathered(agz_engine* e, const void* buf, int32_t is_device, int32_t world,
                                      int64_t chunk_stride, const int64_t* counts, int64_t* added_out);
int64_t agz_replay_count(agz_engine* e);                 /* games in the arena                       */
int64_t agz_replay_positions(agz_engine* e);             /* sum of num_moves = length(pos_buffer)    */
agz_status agz_replay_header(agz_engine* e, int64_t k, agz_game_header* out);
agz_status agz_replay_game(agz_engine* e, int64_t k, int16_t* moves, float* pis, float* qs);
/* `shrink` (train.jl:52): forget the oldest games until at most max_positions positions remain */
agz_status agz_replay_trim(agz_engine* e, int64_t max_positions);
agz_status agz_replay_clear(agz_engine* e);
/* get_replay_batch (train.jl:4-12) for B sampled (game, ply) pairs, ply < num_moves(game):
 * feats float[B][N*N*17] (order of agz_features), pi float[B][A], z float[B]; pi / z may be NULL;
 * the three outputs are host pointers, or device pointers when out_is_device != 0 */
agz_status agz_replay_batch(agz_engine* e, const int64_t* game, const int32_t* ply, int32_t B, float* feats,
                            float* pi, float* z, int32_t out_is_device);
/* the same with sample b under the board symmetry T_sym[b], sym[b] in 0..7 (agz_net_forward_features_sym): feats
 * X'[plane][T_s(p)] = X[plane][p], pi'[T_s(p)] = pi[p] with pass unchanged, z unchanged.  Symmetry augmentation of
 * training samples; device outputs feed agz_train_step directly. */
agz_status agz_replay_batch_sym(agz_engine* e, const int64_t* game, const int32_t* ply, const int32_t* sym, int32_t B,
                                float* feats, float* pi, float* z, int32_t out_is_device);
/* push_data (train.jl:51,60-61) for this engine's own records k = first .. first+count-1 (agz_records_header's
 * numbering), device to device, in that order; the agz_allgather_records watermark does not move.  added_out may be
 * NULL.  AGZ_BAD_ARGUMENT when the range is outside the ring or the ring has wrapped. */
agz_status agz_replay_ingest_records(agz_engine* e, int64_t first, int64_t count, int64_t* added_out);
/* shrink (train.jl:52-53: keep exactly the last memory_size entries) as a sampling window: the entries before the newest
 * max_entries are dead -- also part of a game -- and the window's start never moves back (max_entries < 0: every entry
 * still in the arena live again).  Dead whole games are dropped physically only when they hold more than half of the
 * arena's bytes, so the copy is amortised.  agz_replay_clear resets the window; agz_replay_trim keeps the part of it
 * that lies in the games it keeps (all of them live when the window's start was dropped); agz_replay_count,
 * _positions, _header, _game, _batch keep counting every game still in the arena. */
agz_status agz_replay_set_window(agz_engine* e, int64_t max_entries);
int64_t agz_replay_live_positions(agz_engine* e);        /* entries in the window = length(pos_buffer) after shrink */
/* get_replay_batch (train.jl:4-12: sample(1:length(pos_buffer), B, replace=false)) drawn and built on the device.  With
 * L = agz_replay_live_positions and window entry e = 0..L-1 (oldest first), sample b = 0..B-1 is Floyd's algorithm:
 * j = L - B + b, t = agz_index(agz_draw_u64(agz_config.seed, call, 0, AGZ_SITE_REPLAY_SAMPLE, j), j + 1); sample b is
 * entry t unless an earlier sample took t, then entry j.  Entry e is ply (first live ply + e) counted through the arena's
 * games.  sym_mode -1: as agz_replay_batch; 0..7: every sample under T_sym_mode; AGZ_SYMMETRY_RANDOM (8): sample b under
 * T_s, s = agz_index(agz_draw_u64(seed, call, 0, AGZ_SITE_REPLAY_SYM, b), 8), as agz_replay_batch_sym.  feats float[B]
 * [N*N*17], pi float[B][A], z float[B], game_out int64[B] (arena game index), ply_out int32[B]: DEVICE pointers; pi, z,
 * game_out, ply_out may be NULL.  1 <= B <= min(L, 2048).  Asynchronous on the engine's stream (agz_train_step with
 * inputs_are_device reads the outputs in order). */
agz_status agz_replay_sample(agz_engine* e, int32_t B, uint64_t call, int32_t sym_mode, float* feats, float* pi, float* z,
                             int64_t* game_out, int32_t* ply_out);
/* Targets-only arena: with on != 0 an arena ENTRY is a ply whose pi row is not all zero -- a policy target.  Zero rows
 * are the convention for "no policy target": the fast searches of agz_selfplay_set_playout_cap write them, and so do
 * arena (evaluate) records.  agz_replay_set_window, agz_replay_live_positions and agz_replay_sample then count, keep and
 * draw target plies only: L is the number of live target plies, entry e the (first live target + e)-th target ply counted
 * through the arena's games, and the Floyd draw over 0..L-1 is the one stated above, unchanged.  A sampled (game, ply) is
 * built as always, by replaying every move of the game up to that ply.  Each ingest call indexes the games it files on
 * the device (one wave per game scans the pi rows).  agz_replay_count, _positions, _header, _game, _batch and _trim
 * keep counting every ply.  The mode can be changed only while the arena is empty (AGZ_BAD_ARGUMENT otherwise);
 * agz_replay_clear empties the arena and leaves the mode as it is.  Off (the default): every call is what it is without
 * this one. */
agz_status agz_replay_set_targets_only(agz_engine* e, int32_t on);
/* Search-value targets (include/agz_value_target.h holds the arithmetic): the z of agz_replay_batch,
 * agz_replay_batch_sym and agz_replay_sample becomes the outcome blended with the TD(lambda) return of the root values
 * the search recorded.  For a record of T = num_moves plies with q_k = qs[k] (Black-absolute, as result is) and
 * z = (double)result, the sample at ply t gets, all in double with every multiply and add rounded on its own:
 *     acc = z;  for k = T-1 down to t:  acc = ((1.0 - lambda) * (double)q_k) + (lambda * acc);      G_t = acc
 *     y_t = (float)(((1.0 - alpha) * z) + (alpha * G_t))
 * lambda = 0: G_t = q_t; lambda = 1: G_t = z; alpha = 1, lambda = 0: y_t = q_t bit for bit (returned as it stands: the
 * arithmetic would turn a q_t of -0.0 into +0.0).  alpha = 0 (the default)
 * is OFF: z = (float)result by the code that runs without this call, and no further kernel is launched.  With
 * alpha > 0 one small kernel (one lane per sample) follows the batch kernel on the engine's stream and overwrites z;
 * feats, pi, game_out, ply_out and the draw are untouched, a symmetry does not touch y, and y stays Black-absolute.
 * In a targets-only arena a sampled target ply sums the q of the fast plies behind it; with a window that starts inside
 * a game the sum reads later plies of the same record only.  The pair is kept on the host and read at the next batch
 * call: it may be set at any time, and agz_replay_clear leaves it as it is.  AGZ_BAD_ARGUMENT, with the setting in
 * force kept, when alpha or lambda is a NaN or outside [0, 1]. */
agz_status agz_replay_set_value_target(agz_engine* e, double alpha, double lambda);
/* Policy surprise weighting (include/agz_surprise.h holds the arithmetic): how often agz_replay_sample
 * draws a ply.  The score of a target ply (pi row not all zero) is KL(pi || p) of its recorded pi from the prior p the
 * network gives for its position, summed in double in ascending action order over pi[a] > 0, p floored at FLT_MIN, logs
 * by agz_log.  Under rho a scored game's n target plies with scores s_t summing (in ply order) to S weigh
 *     w_t = (1.0 - rho) + rho * ((s_t * (double)n) / S)   (S > 0; else 1.0),     q_t = (uint32_t)(w_t * 65536.0 + 0.5)
 * and every other ply (no target, or a game without scores) weighs 1.0, q = 65536.
 *
 * agz_replay_score scores arena games first .. first + count - 1 on the network chosen by agz_net_select, at the
 * precision in force: in chunks of at most the engine's forward batch it rebuilds the features of every ply of the games
 * on the device, runs the forward and keeps one score per ply on the device, next to the arena, plus a "scored" flag per
 * game; rows_out (may be NULL) = target plies scored.  A score is as of the network it was computed on: weight updates
 * leave it alone, a second call replaces it.  It runs on the engine's stream between steps and leaves the games in
 * flight as they are.  AGZ_BAD_ARGUMENT on an external_network engine, for a range outside the arena and while a
 * reanalysis run is open (started, not committed).  Games filed later are unscored; agz_replay_trim and the window move
 * the scores with their games; agz_replay_clear drops them; agz_replay_reanalyze_commit marks its games unscored (their
 * pi changed).
 *
 * agz_replay_set_surprise: rho = 0 (the default) is OFF -- agz_replay_sample is the call stated above, the Floyd draw bit
 * for bit, and nothing is launched or allocated for this feature.  With rho > 0 sample b of agz_replay_sample is position
 *     agz_weighted_pick(agz_draw_u64(seed, call, 0, AGZ_SITE_REPLAY_WEIGHTED, b), C, positions)
 * of the arena, C the inclusive prefix (uint64) of q over all arena positions in arena order with q forced to 0 for the
 * plies in front of the window and, in a targets-only arena, for the plies that are no targets; the pick is
 * r = floor(draw * C[last] / 2^64) and the smallest index with C[i] > r.  The draw is WITH replacement: 1 <= B <= 2048,
 * L >= 1, B may exceed L (AGZ_BAD_ARGUMENT if every live q is 0).  The symmetry draw, the value target, game_out /
 * ply_out and the batch kernels are the same.  C is rebuilt on the device (one wave per game, then a scan in three
 * launches) at the first sample call after the arena, the scores or rho changed.  rho is kept on the host and read at
 * the next sample call: it may be set at any time, and agz_replay_clear leaves it alone.  AGZ_BAD_ARGUMENT, with the
 * setting in force kept, when rho is a NaN or outside [0, 1].
 *
 * agz_replay_surprise: for arena game k, kl_out double[num_moves] (0 for a ply that is no target and for a game without
 * scores), q_out uint32[num_moves] under the rho in force (without the window and targets-only masks) and scored_out;
 * each may be NULL.
 *
 * agz_surprise_weights (host only, no engine): the same score and q for one game the caller holds, pis and ps float[T][A]
 * (the game counts as scored).  agz_surprise_pick (host only): agz_weighted_pick over cum[0..n-1], -1 when cum is NULL,
 * n < 1 or cum[n-1] = 0. */
agz_status agz_replay_score(agz_engine* e, int64_t first, int64_t count, int64_t* rows_out);
agz_status agz_replay_set_surprise(agz_engine* e, double rho);
agz_status agz_replay_surprise(agz_engine* e, int64_t k, double* kl_out, uint32_t* q_out, int32_t* scored_out);
agz_status agz_surprise_weights(const float* pis, const float* ps, int32_t T, int32_t A, double rho, double* kl_out,
                                uint32_t* q_out);
int64_t agz_surprise_pick(const uint64_t* cum, int64_t n, uint64_t u);
/* device memory on the engine's GPU for a host without its own allocator (the Julia stub's train): agz_replay_sample's
 * outputs, agz_train_step's device inputs.  Freed by agz_device_free (after the engine's stream has used it). */
agz_status agz_device_alloc(agz_engine* e, int64_t bytes, void** out);
agz_status agz_device_free(agz_engine* e, void* p);

/* ---------------------------------------------------------------- training step --------- */
/* One optimisation step of `_train` (neural_net.jl:75-101; optimiser Momentum(2f-2), train.jl:54; call
 * train.jl:67-74) on the network selected by agz_net_select, entirely on the device:
 *   training-mode forward (BatchNorm normalises with the batch's statistics; its running statistics move by
 *   momentum 0.1), loss = 0.01 * crossentropy(p, pi) + 0.01 * mse(v, z) + 1e-4 * sum(theta^2), backward,
 *   vel = rho * vel - eta * grad; theta += vel for every parameter (Flux Momentum: eta 0.02, rho 0.9).
 * `_train` does not run at the reference's HEAD; this is its intended step, pinned against a
 * float64 autograd twin.  feats float[B][N*N*17] (agz_features / agz_replay_batch order), pi float[B][A],
 * z float[B]: three host pointers, or three device pointers when inputs_are_device != 0 (the outputs of
 * agz_replay_batch with out_is_device).  losses_out float[4] = {total, policy, value, regulariser} BEFORE the
 * update; may be NULL.  B >= 2.  The optimiser state lives in the engine until agz_train_reset. */
agz_status agz_train_step(agz_engine* e, const float* feats, const float* pi, const float* z, int32_t B,
                          int32_t inputs_are_device, float eta, float rho, float* losses_out);
agz_status agz_train_reset(agz_engine* e);

/* The one exchange step of the path: RCCL over xGMI, one rank per GPU.  Rank 0 calls
 * agz_comm_unique_id and hands the 128 bytes to the other ranks by whatever means the host has (Julia:
 * Distributed / a shared file; Python: torch.distributed / gloo); every rank then calls agz_comm_create with
 * the engine that lives on its GPU.  RCCL is bound at run time (dlopen librccl.so.1); a missing library or a
 * failing collective returns AGZ_RCCL_ERROR with the RCCL error string in agz_last_error. */
#define AGZ_COMM_ID_BYTES 128
typedef struct agz_comm agz_comm;
agz_status agz_comm_unique_id(uint8_t* id_out /* [AGZ_COMM_ID_BYTES] */);
agz_status agz_comm_create(agz_engine* e, int32_t rank, int32_t world, const uint8_t* id, agz_comm** out);
void agz_comm_destroy(agz_comm* c);
/* all-gather the finished records of every rank (what agz_records_* shows on each) into THIS rank's replay
 * arena, rank 0's games first: this rank's unsent records are packed on the device, then a count exchange and one
 * padded ncclAllGather, device to device.  Records a completed payload collective has carried are not sent again,
 * whether or not this rank's own ingest then succeeded (a second call without new finished games adds nothing);
 * agz_records_clear empties the record ring and resets that mark.  comm == NULL: single-GPU run, files the
 * engine's own records.  added_out (may be NULL) = games appended.  Collective: every rank of the
 * communicator must call it.  Everything that can fail on one rank alone (counting, packing) happens BEFORE the
 * first collective; such a rank announces {-1, its status} in the count collective and EVERY rank, the failing
 * one included, returns AGZ_RCCL_ERROR (its message names the rank; the failing rank's also carries its own
 * reason) -- nobody is left waiting in ncclAllGather. */
agz_status agz_allgather_records(agz_engine* e, agz_comm* comm, int64_t* added_out);
/* The host logic between the two collectives of that exchange, for a host that carries the bytes with its own
 * library (MPI.jl, Distributed, torch.distributed/gloo) and finishes with agz_replay_ingest_gathered:
 * counts[2r], counts[2r+1] = {agz_records_count, agz_records_packed_size} of rank r as gathered (a rank that could
 * not pack sends {-1, its agz_status}).  Checks every pair and returns the chunk stride (largest rank, padded to
 * 256 B) each rank pads its packed export to; total_records_out may be NULL.  AGZ_RCCL_ERROR names the
 * offending rank (text via agz_last_error(NULL)).  Pure host code: needs no engine and no GPU. */
agz_status agz_gather_plan(const int64_t* counts, int32_t world, int64_t* chunk_stride_out, int64_t* total_records_out);
/* overwrite every rank's weight replica with rank `root`'s parameters of the selected network (after a
 * training step on one rank); nfloats_out may be NULL.  Collective. */
agz_status agz_broadcast_weights(agz_engine* e, agz_comm* comm, int32_t root, int64_t* nfloats_out);

/* ---------------------------------------------------------------- ABI self-description --- */
/* sizeof and field offsets of the PODs above as this library was compiled, so that a host mirror (ctypes
 * Structure, Julia struct) can be checked against them: name in {"agz_config", "agz_stats",
 * "agz_game_header", "agz_position_info", "agz_node_info", "agz_analysis", "agz_line"}; out[0] = sizeof, out[1..n] = offsetof of the n
 * fields in declaration order; returns n, or -1 for an unknown name / too small a buffer. */
int32_t agz_abi_layout(const char* name, int32_t* out, int32_t cap);

/* ---------------------------------------------------------------- single-tree compat ---- */
/* The reference's MCTSPlayer / MCTSNode API on game slot g (tests drive these one call at a
 * time exactly like test/test_mcts.jl and test/test_mcts_player.jl).  Node handles are
 * slot-local int32 ids; the root is whatever agz_tree_root returns. */
typedef struct {
  int32_t n;                   /* moves played so far                                   */
  int32_t to_play;
  int32_t ko;                  /* -1 none                                               */
  int32_t caps_black, caps_white;
  int32_t last_move;           /* -1 none, N*N pass  (recent[end].move)                 */
  int32_t prev_move;           /* -1 none            (recent[end-1].move)               */
  int32_t history_len;         /* boards of real history available before this one (<=7) */
  float komi;
} agz_position_info;
/* initialize_game!(player, pos) mcts_play.jl:110-118; history = int8[history_len][N*N] older
 * boards newest first (NULL when history_len == 0) */
agz_status agz_tree_init(agz_engine* e, int32_t g, const int8_t* board, const agz_position_info* info,
                         const int8_t* history);
agz_status agz_tree_root(agz_engine* e, int32_t g, int32_t* node_out);
agz_status agz_tree_select_leaf(agz_engine* e, int32_t g, int32_t from_node, int32_t* leaf_out);
agz_status agz_tree_maybe_add_child(agz_engine* e, int32_t g, int32_t node, int32_t a, int32_t* child_out);
agz_status agz_tree_add_virtual_loss(agz_engine* e, int32_t g, int32_t node, int32_t up_to);
agz_status agz_tree_revert_virtual_loss(agz_engine* e, int32_t g, int32_t node, int32_t up_to);
agz_status agz_tree_incorporate(agz_engine* e, int32_t g, int32_t node, const float* probs,
                                int32_t nprobs, float value, int32_t up_to);
agz_status agz_tree_inject_noise(agz_engine* e, int32_t g, int32_t node);
/* tree_search!(player, parallel_readouts): select phase then (with an internal network) the
 * evaluation and incorporate phases; returns the number of leaves */
agz_status agz_tree_search(agz_engine* e, int32_t g, int32_t parallel_readouts, int32_t* nleaves_out);
/* the same split at the network call, for a caller-supplied network (DummyNet, a Flux model):
 * select -> read the leaves' feature tensor (N x N x 17 x nleaves) -> hand back pi (A x nleaves)
 * and v (nleaves); pi == NULL makes the engine evaluate the leaves with its own network */
agz_status agz_tree_search_select(agz_engine* e, int32_t g, int32_t parallel_readouts, int32_t* nleaves_out);
agz_status agz_tree_leaf_features(agz_engine* e, int32_t g, float* feats_out);
/* ... or read the leaves as the `Vector{Position}` the reference hands its network (`mcts_player.network([leaf.position
 * for leaf in leaves])`, mcts_play.jl:89; DummyNet sizes its answer by length(positions), test/test_mcts_player.jl:25-32):
 * per collected leaf, in collection order, the GoPosition fields of board.jl:271-306 -- nodes_out int32[B] (the leaf's
 * node handle), boards_out int8[B][N*N], deltas_out int8[B][7][N*N] (board_deltas newest first, zero beyond ndeltas),
 * ndeltas_out int32[B], to_play_out int8[B] (together the SoA agz_net_forward / agz_features take), info_out[B] (n, ko,
 * caps, last two moves, komi; history_len = ndeltas).  Any output may be NULL.  Valid between agz_tree_search_select and
 * agz_tree_search_incorporate. */
agz_status agz_tree_leaf_positions(agz_engine* e, int32_t g, int32_t* nodes_out, int8_t* boards_out, int8_t* deltas_out,
                                   int32_t* ndeltas_out, int8_t* to_play_out, agz_position_info* info_out);
agz_status agz_tree_search_incorporate(agz_engine* e, int32_t g, const float* pi, const float* v);
agz_status agz_tree_pick_move(agz_engine* e, int32_t g, int32_t* a_out);
agz_status agz_tree_play_move(agz_engine* e, int32_t g, int32_t a, int32_t* ok_out);
agz_status agz_tree_should_resign(agz_engine* e, int32_t g, int32_t* out);
agz_status agz_tree_is_done(agz_engine* e, int32_t g, int32_t node, int32_t* out);
typedef struct {
  float N, W, Q;
  int32_t parent, fmove, is_expanded, losses_applied, done;
  agz_position_info pos;
} agz_node_info;
agz_status agz_tree_node_info(agz_engine* e, int32_t g, int32_t node, agz_node_info* out);
#define AGZ_F_CHILD_N 0
#define AGZ_F_CHILD_W 1
#define AGZ_F_CHILD_PRIOR 2
#define AGZ_F_ACTION_SCORE 3     /* Float64 scores narrowed to double[A] */
#define AGZ_F_CHILD_S 4          /* the sums of squared values; needs agz_search_set_value_moments on */
agz_status agz_tree_node_floats(agz_engine* e, int32_t g, int32_t node, int32_t field, float* out);
agz_status agz_tree_node_scores(agz_engine* e, int32_t g, int32_t node, double* out);
agz_status agz_tree_node_set_floats(agz_engine* e, int32_t g, int32_t node, int32_t field, const float* in);
agz_status agz_tree_node_set_N(agz_engine* e, int32_t g, int32_t node, float value);
agz_status agz_tree_node_set_n(agz_engine* e, int32_t g, int32_t node, int32_t n);
agz_status agz_tree_node_children(agz_engine* e, int32_t g, int32_t node, int32_t* out /* [A] */);
/* the pruned pi row (agz_selfplay_set_forced_playouts, PRUNED TARGET) of one node of single tree g under the k given
 * here, whatever the engine's setting: the node's rows, scale from the node's own N, squashed iff the node's n <= tau.
 * out float[A].  k = 0 gives children_as_pi's row.  One small kernel; synchronises. */
agz_status agz_tree_pruned_pi(agz_engine* e, int32_t g, int32_t node, double k, float* out);
/* the improved-policy row of the Gumbel root search (agz_selfplay_set_gumbel, TARGET) of one node of single tree g under
 * the constants given here, whatever the engine's setting: the node's rows, legal mask and to_play.  out float[A].
 * c_visit >= 0, c_scale > 0.  One small kernel; synchronises. */
agz_status agz_tree_gumbel_pi(agz_engine* e, int32_t g, int32_t node, double c_visit, double c_scale, float* out);
agz_status agz_tree_node_board(agz_engine* e, int32_t g, int32_t node, int8_t* out /* [N*N] */);
agz_status agz_tree_pending_vlosses(agz_engine* e, int32_t g, int32_t* out);
agz_status agz_tree_set_draw(agz_engine* e, int32_t g, uint64_t game_id, uint32_t sel);

/* ---------------------------------------------------------------- batched analysis ------ */
/* suggest_move over many caller positions in one device run (ours; the reference analyses one position per MCTSPlayer,
 * mcts_play.jl:110-118,144-151).  Position i (0-based) gives exactly what
 *   MCTSPlayer(env, nn; num_readouts, two_player_mode) with draw-stream seed agz_config.seed and game id
 *   game_id_base + i;  initialize_game!(player, pos_i);  suggest_move(player)
 * gives: tree_search!(player, parallel_readouts) until N(root) >= num_readouts, then pick_move.  No Dirichlet noise, no
 * pre-expansion, soft pick below tau_threshold unless two_player_mode.  The result does not depend on the number of
 * slots or on which slot searches position i.  A slot that finishes a position claims the next one at once, so B may
 * be far larger than agz_config.games.  Board symmetries (agz_selfplay_set_symmetry) apply as in the tree path.
 *
 * agz_analyze_start: boards int8[B][N*N], info[B] and history int8[B][7][N*N] (or NULL: no older boards) in the
 * conventions of agz_tree_init (info[i].history_len of the 7 boards are real).  It copies the positions to the device,
 * resets every slot (the way agz_selfplay_start does) and leaves the records ring and the counters agz_selfplay_start
 * resets as they are.  Scalar fields are checked here: to_play = +-1, history_len in 0..7, n >= 0, ko in -1..N*N-1,
 * last_move / prev_move in -1..N*N; a bad one fails the whole call naming the position.  The board is checked on the
 * device when the position is installed: every point in {-1, 0, +1}, no group without a liberty, the ko point empty;
 * a bad board gives that position AGZ_BAD_ARGUMENT (move -1, nothing searched).  Refused in arena_mode.
 * agz_selfplay_step (internal network) or agz_selfplay_select / _leaf_features / _incorporate (external network) then
 * step the run; agz_analyze_progress (synchronises) says how many positions are finished; agz_analyze_results copies
 * them out (AGZ_NOT_READY until all B are).  A later agz_selfplay_start returns the engine to self-play.
 *
 * status per position: AGZ_OK; AGZ_BAD_ARGUMENT (invalid board); AGZ_POOL_EXHAUSTED (the node pool filled up: under
 * AGZ_POOL_MOVE_EARLY the search ended early, the move and statistics are valid and N < num_readouts; under
 * AGZ_POOL_STALL the slot waits until agz_slot_abandon gives the position up, move -1); AGZ_ASSERT_SOFTPICK (pick_move's
 * assertion, mcts_play.jl:67; move -1).  N, W of the root (the DummyNode, mcts.jl:27-39), Q = W / (1 + N)
 * (mcts.jl:96-102), nodes_used = tree size when the search ended. */
typedef struct {
  int32_t move;                /* action picked, -1 when none */
  int32_t status;
  float N, W, Q;
  int32_t nodes_used;
} agz_analysis;
agz_status agz_analyze_start(agz_engine* e, const int8_t* boards, const agz_position_info* info, const int8_t* history,
                             int64_t B, uint64_t game_id_base);
/* A table of start positions (initialize_game!(player, pos), mcts_play.jl:110-118, for the bulk loops): S >= 1
 * positions in the conventions of agz_analyze_start -- boards int8[S][N*N], info[S], history int8[S][7][N*N] or NULL.
 * While a table is set, self-play game `gid` (game_id_base + k * stride) starts from entry gid mod S and arena game g
 * (its two players have the ids 2g and 2g + 1) from entry g mod S, on any rank and in any slot.  The game is
 * selfplay.jl:1-45 / neural_net.jl:113-148 from that root: komi, to_play, ko, captures and position.n are the entry's,
 * every draw is keyed by position.n as the reference's player keys it, the soft pick holds while position.n < tau, the
 * game ends by two passes or at position.n >= max_game_length, and in the arena the player whose colour is to move
 * searches first.  A record keeps its layout: num_moves, moves, pis and qs cover the plies played from the start,
 * result and final_score are of the final position.  Everything that rebuilds a record's positions finds the start
 * through the record's game_id by the same rule and begins there -- the entry's board, to_play and its history_len
 * older boards as the history planes: agz_records_features, agz_replay_batch(_sym), agz_replay_sample.  S = 0 clears
 * the table; with none set (the default) every path is what it is without this call.  Analysis, review and the
 * single-tree calls ignore the table.  Synchronises.  Refused with the previous table left in force, naming the entry:
 *   - a scalar field agz_analyze_start would refuse;
 *   - a finished start: last_move and prev_move both pass, or n >= max_game_length;
 *   - a board with a point outside {-1, 0, 1}, a group without a liberty or a stone on the ko point (checked on the
 *     device over the whole table, at this call);
 *   - while the record ring or the replay arena holds games, or games of a run are still being played (their positions
 *     are rebuilt through the table): agz_records_clear / agz_replay_clear first;
 *   - together with agz_debug_set_stagger > 0.
 * The games of the next agz_selfplay_start begin on the new table.  A run that has been started and not stepped yet
 * has claimed no game: a table set there is the table of that run.
 * The record-to-start rule reads the game id as the engine that replays it does: an arena_mode engine takes
 * game_id / 2, any other engine game_id.  Records therefore go into the arena of an engine of the kind that played
 * them (self-play records into a self-play engine, evaluate() records into an arena_mode engine), with the same table
 * set; the library cannot tell the two kinds of id apart. */
agz_status agz_selfplay_set_starts(agz_engine* e, const int8_t* boards, const agz_position_info* info,
                                   const int8_t* history, int64_t S);
int64_t agz_selfplay_starts_count(agz_engine* e);                   /* entries of the table in force, 0 = none */
/* Playout cap randomization for self-play: most moves get a small search and are played but not trained on, a random
 * fraction gets the full search and becomes the policy targets.  fast_readouts = r, full_prob = p; r = 0 switches it
 * off (the default), otherwise 1 <= r <= num_readouts and 0 <= p <= 1.  Whenever a self-play game is about to search the
 * root of ply n = position.n (after the pre-expansion of its start, and after every move), the search is
 *   full  iff  agz_u01(agz_draw_u64(agz_config.seed, game_id, n, AGZ_SITE_PLAYOUT_CAP, 0)) < p.
 * A full search is the move without this call: Dirichlet noise on the root, num_readouts readouts, pi recorded.  A fast
 * search adds no noise and runs r readouts; its move is chosen by the same rule (soft pick while n < tau, arg-max
 * after), moves and qs are recorded as usual, and the ply's pi row of the record is ALL ZEROS: "no policy target".
 * A consumer that samples every ply gets no policy loss from such a row (the loss is -sum pi log p); a targets-only
 * arena (agz_replay_set_targets_only) skips them.  The resign check, tree reuse, the pool policy, symmetry, the hold and
 * the starts table (n begins at the start's n) are unchanged; the bench stagger's shortened first search keeps its
 * budget and counts as full.  The arena, analysis, review and the single-tree calls always search num_readouts.
 * Synchronises.  Refused (AGZ_BAD_ARGUMENT, the setting in force kept): an arena_mode engine, r or p out of range,
 * games of a run still being played (as agz_selfplay_set_starts). */
agz_status agz_selfplay_set_playout_cap(agz_engine* e, int32_t fast_readouts, double full_prob);
/* out[0] = moves played after a full search, out[1] = after a fast one, since agz_selfplay_start, counted only while
 * the cap is on.  Synchronises. */
agz_status agz_selfplay_playout_cap_counts(agz_engine* e, int64_t out[2]);
/* Forced playouts and policy target pruning for self-play (KataGo's pair of rules).  k = 0 switches both
 * off (the default); KataGo plays k = 2.  prune != 0 asks for the pruned target as well and needs k > 0.
 * FORCED SELECTION, at the root level of a descent only (depth 0 of a descent that starts at the root).  After the
 * pass-first rule of mcts.jl:119-126, which keeps its precedence: let T = sum over all A actions of the root's child_N
 * (a Float32 sum of integers).  A legal child a is UNDER-FORCED iff child_N[a] > 0 and
 *   (double)N * (double)N < ((double)k * (double)P[a]) * (double)T        (N = child_N[a], P = child_prior)
 * in Float64 in this order.  If any child is under-forced, every under-forced child scores one common value above every
 * real score, and the unchanged tie rule (the lowest index, or the AGZ_SITE_PUCT_TIE draw keyed sel * 1024 + depth)
 * picks among them.  Levels below the root are untouched.
 * PRUNED TARGET, when a move is recorded.  With the root's rows N, W, P, tp = to_play, scale = c_puct * sqrtf(1 + N(root))
 * and T as above: c* = the child with the most visits, the lowest index on ties (no draw); S* = its action score.  For
 * every other a with N_a > 0, in Float64 except q:
 *   nf = sqrt((k * P_a) * T);  q = (W_a / (1.0f + N_a)) * tp in Float32;  gap = S* - q;
 *   N_min = N_a if gap <= 0, else (scale * P_a) / gap - 1;  N'_a = min(N_a, max(N_a - nf, N_min, 0));
 *   if N'_a < N_a and N'_a <= 1 then N'_a = 0.
 * N'_c* = N_c*, and N'_a = 0 where N_a = 0.  The pi row is children_as_pi's transform of N': N'_a (agz_pow(N'_a, 0.98)
 * while n <= tau) over the Float64 sum in ascending index order, narrowed to Float32 last -- bit for bit today's row
 * when no N'_a differs from N_a.  The move played, the recorded q, the resign check and the re-rooting use the raw
 * visits.
 * WHERE.  Self-play full searches only: every search with the playout cap off; with it on the searches the coin made
 * full (the bench stagger's shortened first search counts as full).  Fast searches are neither forced nor recorded, as
 * before.  The arena never forces or prunes; analysis and review, on any engine, never do either.  The single-tree calls
 * agz_tree_select_leaf, agz_tree_search and agz_tree_search_select FOLLOW THE ENGINE'S SETTING whenever the descent starts
 * at the tree's root (agz_tree_select_leaf from another node does not force): that is how a host-driven MCTSPlayer loop
 * equals device self-play, and how hand-made rows reach the rule.  agz_tree_play_move records children_as_pi as before;
 * agz_tree_pruned_pi gives the pruned row of any node.
 * No draw site is added and none moves; records, agz_game_header, agz_config and agz_stats do not change.
 * Synchronises.  Refused (AGZ_BAD_ARGUMENT, the setting in force kept): an arena_mode engine; k negative, NaN or above
 * 1024; prune != 0 with k == 0; games of a run still being played (as agz_selfplay_set_playout_cap). */
agz_status agz_selfplay_set_forced_playouts(agz_engine* e, double k, int32_t prune);
/* out[0] = root descents that the forced rule decided (some child was under-forced), out[1] = recorded pi rows that
 * pruning changed (some N'_a < N_a), since agz_selfplay_start.  Synchronises. */
agz_status agz_selfplay_forced_counts(agz_engine* e, int64_t out[2]);
/* Gumbel root search for self-play ("Policy improvement by planning with Gumbel", Danihelka et al., ICLR 2022; DESIGN.md
 * §5j).  m = 0 switches it off (the default); m in 2..16 is the largest number of root candidates.  c_visit >= 0 (the
 * paper: 50), c_scale > 0 (the paper: 1.0 for q in [0, 1]).
 * SCORES.  For the root with rows N, W, P, tp = to_play, position.n = n_root, and a legal action a:
 *   logit(a) = agz_log((double)P[a]) when P[a] > 0, else -1.0e30
 *   g(a)     = -agz_log(-agz_log(agz_u01(agz_draw_u64(seed, game_id, n_root, AGZ_SITE_GUMBEL, a))))
 *   qs(a)    = (W[a] / (1.0f + N[a])) * tp in Float32 -- an unvisited child's W is the root's own network value
 *   sigma(a) = ((c_visit + (double)maxN) * c_scale) * (0.5 + 0.5 * (double)qs(a)),  maxN = max of N over all A actions
 *   s(a)     = (g(a) + logit(a)) + sigma(a)                               (Float64, in this order)
 * SEARCH.  At the first select phase of a search whose root is expanded: n = target - N(root); the survivors are the
 * m_0 = min(m, #legal) legal actions with the largest g + logit (ties: the lower action), in that order; P = the smallest
 * integer >= 1 with 2^P >= m_0.  Phase p with m_p survivors ends when N(root) reaches its start plus
 * Q_p = max(1, floor(n / (P m_p))) m_p, cut to what remains of n; reverted duplicates do not count.  At the start of a
 * select phase after a phase end with budget left the survivors are ordered by s descending (ties: the lower action)
 * and the first m_{p+1} = max(2, floor(m_p / 2)) stay (1 if m_p = 1).  At the root level of a descent, after the
 * pass-first rule of mcts.jl:119-126, the pick is the survivor with the smallest child_N, visits in flight included, the
 * first in stored order on ties: no score, no tie draw (the select counter of the draw key advances as ever).  Below
 * the root: PUCT, unchanged.  A select phase stops collecting at the phase end, so a search makes exactly n root visits
 * unless the pool fills.  No Dirichlet noise is injected for a Gumbel search.
 * MOVE.  The survivor with the largest s, the lower action on ties; no soft pick and no pick-tie draw at any move
 * number.  (A search whose state was never set up -- the pool filled before the root was expanded -- falls back to
 * pick_move.)  The resign check, the recorded q and the re-rooting are unchanged.
 * TARGET.  Over legal a: x(a) = logit(a) + sigma(a); pi[a] = (float)(agz_exp(x(a) - max x) / sum), the Float64 sum in
 * ascending index order; illegal actions get 0; no 0.98 squash.
 * WHERE.  Self-play full searches only: every search with the playout cap off; with it on the searches the coin made
 * full (the bench stagger's shortened first search counts as full).  Fast searches, the arena, analysis and review are
 * as before, and so are the single-tree calls: a host-driven MCTSPlayer loop does not reproduce Gumbel self-play;
 * agz_tree_gumbel_pi gives the target row of any node.
 * One draw site is added (AGZ_SITE_GUMBEL = 12: move = n_root, idx = action), none moves; records, agz_game_header,
 * agz_config and agz_stats do not change.
 * Synchronises.  Refused (AGZ_BAD_ARGUMENT, the setting in force kept): an arena_mode engine; m outside {0, 2..16};
 * c_visit negative or NaN; c_scale zero, negative or NaN; forced playouts on (agz_selfplay_set_forced_playouts with
 * k > 0 is refused in turn while m > 0: the two rules answer the same question and are not composed); games of a run
 * still being played (as agz_selfplay_set_playout_cap). */
agz_status agz_selfplay_set_gumbel(agz_engine* e, int32_t m, double c_visit, double c_scale);
/* out[0] = Gumbel searches begun, out[1] = halvings made, since agz_selfplay_start.  Synchronises. */
agz_status agz_selfplay_gumbel_counts(agz_engine* e, int64_t out[2]);
/* PUCT rule options (ours): first-play urgency (FPU) reduction as in KataGo / Leela Zero, and the c_puct
 * growth of AlphaZero (2018).  The setting is (fpu_on, r = fpu_reduction, r_root = fpu_reduction_root, c_base); the
 * default (0, 0, 0, 0) is off: the rule of mcts.jl:86-92, an unvisited child's Q = 0 and one constant c_puct.
 * THE RULE.  Where a node s scores its children (rows N, W, P over the A actions): n = the node's own stored N at that
 * moment (what the scale of mcts.jl:91 receives), N_s = n and W_s = the node's own stored W at that moment (virtual
 * losses of other descents in flight included), tp = (float)to_play.
 *   GROWTH (c_base > 0):   c     = c_puct + agz_log(((double)(1.0f + n) + c_base) / c_base)
 *                          scale = c * (double)sqrtf(1.0f + n)           (c_base == 0: scale = c_puct * (double)sqrtf(1.0f + n))
 *   FPU (fpu_on), for a child a whose row value N_a == 0.0f:
 *     M   = sum over b < A with N_b > 0 of (int64)((double)P_b * 1073741824.0)      (integers: order-free and exact)
 *     m   = (double)M * (1.0 / 1073741824.0)                                         (exact)
 *     q_s = W_s / (1.0f + N_s);  qp = q_s * tp                                       (Float32)
 *     f   = (float)((double)qp - rho * agz_sqrt(m)),  rho = r_root when s is the game's root, else r
 *     score_a = (double)f + (scale * (double)P_a) / (double)1.0f
 *   P_b is the row as stored: Dirichlet noise included at a noised root.  (fpu_on, 0, 0, .) is not off: an unvisited
 *   child then has its parent's value.  A visited child's score keeps the arithmetic of mcts.jl:86-92 under `scale`.
 * Everything else keeps its place and precedence: the pass-first rule of mcts.jl:119-126, the arg-max, the tie rule with
 * its draw and key, the forced-playout score (it replaces scores of visited children only) and the given root action
 * of the Gumbel root search.  The scale of the pruned policy target (agz_selfplay_set_forced_playouts) is `scale` too.
 * WHERE.  Every level of every descent of every search the engine runs: self-play (full and fast searches), the arena
 * (both players), analysis, review and reanalysis, and the single-tree calls agz_tree_select_leaf, agz_tree_search and
 * agz_tree_search_select / _incorporate; agz_tree_node_scores reports the scores under the setting.
 * No draw site is added and none moves; records, agz_game_header, agz_config and agz_stats do not change.
 * Synchronises; the two counters of agz_search_puct_counts restart.  Refused (AGZ_BAD_ARGUMENT, the setting in force
 * kept): fpu_on outside {0, 1}; a reduction outside [0, 4] or NaN; c_base neither 0 nor in [1, 1e9], or NaN; games of a
 * run still being played (as agz_selfplay_set_playout_cap); between agz_tree_search_select and
 * agz_tree_search_incorporate.  An arena_mode engine takes it. */
agz_status agz_search_set_puct(agz_engine* e, int32_t fpu_on, double fpu_reduction, double fpu_reduction_root,
                               double c_base);
/* out[0] = tree levels that a descent scored under an active rule (pass-first and given root actions do not count),
 * out[1] = those of them that picked an unvisited child, since the later of agz_search_set_puct and
 * agz_selfplay_start.  Synchronises. */
agz_status agz_search_puct_counts(agz_engine* e, uint64_t* out /* [2] */);
/* Root exploration and the move that is played (ours; the arithmetic is include/agz_explore.h): a softmax
 * temperature on the root prior, Dirichlet noise over the legal moves with KataGo's policy-shaped concentration, and a
 * move-selection temperature that decays with the move number.  All three are off by default: the reference's
 * inject_noise! (one alpha for all A actions, mcts.jl:233-239) and pick_move (mcts_play.jl:52-71).
 * Everything is Float64, every multiply, add and divide rounded on its own, unless cast; every sum runs in ascending
 * action order.  n is position.n of the root, the key its draws use.
 *   SCHEDULE  T(n) = late + ((early - late) * agz_exp(-(((double)n * 0.6931471805599453) / halflife)))
 *   1. agz_selfplay_set_root_policy_temperature(on, early, late, halflife): over the root's stored prior row, over the
 *      legal actions with P_a > 0 only:  x_a = agz_log((double)P_a) / T, M = max x_a, e_a = agz_exp(x_a - M), E = sum e_a,
 *      mass = sum (double)P_a,  P_a <- (float)((e_a / E) * mass).  Illegal and zero entries stay; a row with no positive
 *      legal entry is left alone.  (1, 1, 1, h) is not off: it runs the arithmetic.
 *   2. agz_selfplay_set_root_noise(total_alpha, shaped), total_alpha = 0 off.  L = the legal actions of the root,
 *      u = 1.0 / (double)L.  Unshaped: alpha_a = total_alpha * u.  Shaped (KataGo): l_a = agz_log(min(0.01, (double)P_a)
 *      + 1e-20), mean = (sum l_a) / (double)L, s_a = max(0, l_a - mean), S = sum s_a, alpha_a = total_alpha * u when
 *      S <= 0, else total_alpha * (0.5 * ((s_a / S) + u)).  Then gamma_a = agz_dirichlet_gamma(seed, game_id, n, a,
 *      alpha_a) for legal a (no draw for an illegal one), G = sum gamma_a, d_a = G > 0 ? gamma_a / G : u,
 *      P_a <- (float)(((double)P_a * (1.0 - w)) + (d_a * w)), w = dirichlet_noise_weight.  Illegal entries stay.  With
 *      both rules on the shape reads the row after the temperature.
 *   3. agz_search_set_move_temperature(on, early, late, halflife), in pick_move with two_player_mode off.  T <= 0.01: the
 *      arg-max branch of pick_move with its AGZ_SITE_PICK_TIE draw.  Otherwise mx = max child_N over the A actions
 *      (mx <= 0: AGZ_ASSERT_SOFTPICK), w_a = N_a > 0 ? agz_exp(agz_log((double)N_a / (double)mx) / T) : 0 (pass
 *      included), S = sum w_a, r = agz_u01(agz_draw_u64(seed, game_id, n, AGZ_SITE_SOFTPICK, 0)) * S, and with acc += w_a
 *      in ascending a the pick is the first a with w_a > 0 and acc > r, else the highest a with w_a > 0.  A full pool
 *      under AGZ_POOL_MOVE_EARLY can then move on any visited child.  The recorded pi row (its n <= tau squash), q, the
 *      resign check and the re-rooting do not change.
 * WHERE.  Rules 1 and 2 run exactly where inject_noise! runs, the temperature first: the full self-play searches that are
 * not Gumbel searches, and agz_tree_inject_noise on single trees (so a host-driven MCTSPlayer loop equals device
 * self-play).  Fast searches, Gumbel searches, the arena, analysis, review and reanalysis get neither.  Rule 3 applies at
 * every pick_move with two_player_mode off: self-play, analysis, review, reanalysis and agz_tree_pick_move.
 * No draw site is added or moved; records, agz_game_header, agz_config and agz_stats do not change.
 * The setters synchronise and restart the counters of agz_search_explore_counts.  Refused (AGZ_BAD_ARGUMENT, the setting
 * in force kept): an arena_mode engine; `on` or `shaped` outside {0, 1}; shaped = 1 with total_alpha = 0; a temperature
 * NaN or outside [0.1, 10] (root policy) / [0, 10] (move); halflife NaN, <= 0 or > 1e6; total_alpha NaN, negative or
 * > 1000; games of a run still being played; between agz_tree_search_select and agz_tree_search_incorporate. */
agz_status agz_selfplay_set_root_policy_temperature(agz_engine* e, int32_t on, double early, double late, double halflife);
agz_status agz_selfplay_set_root_noise(agz_engine* e, double total_alpha, int32_t shaped);
agz_status agz_search_set_move_temperature(agz_engine* e, int32_t on, double early, double late, double halflife);
/* out[0] = roots tempered, out[1] = roots noised under total_alpha > 0, out[2] = moves picked by rule 3's sampling
 * branch, out[3] = those of out[2] that are not a most-visited child; since the later of a setter call and
 * agz_selfplay_start.  Synchronises. */
agz_status agz_search_explore_counts(agz_engine* e, uint64_t* out /* [4] */);
/* What agz_tree_inject_noise would do to `node` of single tree g under the engine's setting; the tree is not modified.
 * tempered float[A]: the prior row after rule 1 (the stored row when rule 1 is off); alpha double[A]: alpha_a, 0 for an
 * illegal action (rule 2 off: the reference's one alpha for all A); noised float[A]: the row agz_tree_inject_noise would
 * store.  Any output may be NULL.  One small kernel; synchronises. */
agz_status agz_tree_explore_rows(agz_engine* e, int32_t g, int32_t node, float* tempered, double* alpha, float* noised);
/* *out = T(n) of the schedule above; host only, needs no engine.  AGZ_BAD_ARGUMENT: out is NULL. */
agz_status agz_explore_temperature(int32_t n, double early, double late, double halflife, double* out);
/* Value uncertainty (ours; the arithmetic is include/agz_uncertainty.h): a second moment S beside every W,
 * the move picked by a lower confidence bound (Leela Zero, KataGo), and exploration scaled by the spread of the values
 * seen below a node (KataGo).  All three are off by default, and off is the engine as it was, bit for bit.
 * Everything is Float64, every multiply, add and divide rounded on its own, unless cast.
 *   1. agz_search_set_value_moments(on).  With moments on every store to a W has its S store beside it: 0 where W is
 *      zeroed; value * value (one Float32 product) in every child entry at a node's first expansion; S = S + (value *
 *      value) in Float32 along a backed-up path; S = S + (float)sign along a path of virtual losses (a virtual loss is
 *      a value of +-1); the child's entry into the root's own S at a re-root.  The arrays (a row the size of child_W's,
 *      one float per slot) are allocated the first time the option goes on; an allocation that fails refuses the call
 *      with the option off.  Moments cover trees begun after the call.  Moments alone observe: every record, row,
 *      counter and move is what it is with moments off.
 *      CHILD STATISTICS of a row entry (N_a, W_a, S_a): cnt = (double)(1.0f + N_a), mean = (double)W_a / cnt,
 *      m2 = (double)S_a / cnt, var = m2 - mean*mean, 0 unless var > 0, sd = agz_sqrt(var).  cnt counts the parent's value
 *      that the first expansion puts into W_a and S_a.
 *   2. agz_search_set_lcb(z, min_visits, min_ratio), z = 0 off: in the arg-max branch of pick_move only (two_player_mode,
 *      n >= tau, a move temperature T <= 0.01).  mx = max child_N.  mx < min_visits: that branch as it is, tie draw
 *      included.  Otherwise a is eligible iff N_a >= min_visits and (double)N_a >= min_ratio * (double)mx, and the pick
 *      is the largest  lcb = (mean * (double)tp) - (z * agz_sqrt(var / cnt)),  tp the root's to_play; ties to the larger
 *      N, then to the lower action; no draw is made.  The soft pick, the sampling branch of the move temperature, the
 *      Gumbel move, the recorded pi row, q, the resign check, re-rooting and the pool rules do not change.  Applies to
 *      every pick_move: self-play, the arena (both players), analysis, review, reanalysis, agz_tree_pick_move.
 *   3. agz_search_set_puct_variance(k, prior, prior_weight), k = 0 off: `scale` of the PUCT rule (agz_search_set_puct)
 *      is multiplied by the factor of the node's own stored (n, W_s, S_s), n as the scale itself receives it:
 *      cnt = (double)(1.0f + n), mean = (double)W_s / cnt, m2 = (double)S_s / cnt, pw = prior_weight,
 *      var = ((((mean*mean) + (prior*prior)) * pw) + (m2 * cnt)) / (pw + cnt) - (mean*mean), 0 unless var > 0,
 *      factor = 1.0 + k * ((agz_sqrt(var) / prior) - 1.0).  At every level of every descent, in the scale of the pruned
 *      policy target (the root's own n, W and S) and in agz_tree_node_scores.  It composes with the FPU, c_base, the forced
 *      rule and the Gumbel root search as agz_search_set_puct does.
 * No draw site is added or moved; records, agz_game_header, agz_config and agz_stats do not change.
 * The setters synchronise and restart the counters of agz_search_uncertainty_counts.  Refused (AGZ_BAD_ARGUMENT, the
 * setting in force kept): `on` outside {0, 1}; z NaN, negative or above 100; min_visits < 1; min_ratio outside [0, 1];
 * k outside [0, 1); prior outside [0.01, 2]; prior_weight outside [0, 1000]; either rule while moments are off; moments
 * switched off while a rule is on; games of a run still being played; between agz_tree_search_select and
 * agz_tree_search_incorporate.  An arena_mode engine takes all three. */
agz_status agz_search_set_value_moments(agz_engine* e, int32_t on);
agz_status agz_search_set_lcb(agz_engine* e, double z, int32_t min_visits, double min_ratio);
agz_status agz_search_set_puct_variance(agz_engine* e, double k, double prior, double prior_weight);
/* out[0] = moves picked under the LCB rule, out[1] = those of them not on a most-visited child, out[2] = tree levels a
 * descent scored under a variance factor, out[3] = those of them with factor > 1; since the later of a setter call and
 * agz_selfplay_start.  Synchronises. */
agz_status agz_search_uncertainty_counts(agz_engine* e, uint64_t* out /* [4] */);
/* the child statistics of `node` of single tree g and their lower confidence bounds under the z given here (0 <= z <=
 * 100), from the node's side to move, whatever the setting of rule 2: mean, sd, lcb double[A] each.  Needs moments on.
 * One small kernel; synchronises. */
agz_status agz_tree_child_lcb(agz_engine* e, int32_t g, int32_t node, double z, double* mean, double* sd, double* lcb);
/* a node's own S (the root's: the slot's side entry); needs moments on */
agz_status agz_tree_node_S(agz_engine* e, int32_t g, int32_t node, float* out);
/* child_S [B][A] and root_S [B] of the analysis / review run, filled beside the three rows of agz_analyze_results.
 * AGZ_BAD_ARGUMENT when the run began with moments off. */
agz_status agz_analyze_child_S(agz_engine* e, float* child_S, float* root_S);
/* rules 1 and 2 on one entry (n, w, s) seen by to_play = +-1, and the factor of rule 3; host only, need no engine.
 * AGZ_BAD_ARGUMENT: an output is NULL. */
agz_status agz_value_lcb(float n, float w, float s, int32_t to_play, double z, double* mean, double* sd, double* lcb);
agz_status agz_puct_variance_factor(float n, float w, float s, double k, double prior, double prior_weight, double* out);

/* Superko (ours; the keys and the rule are include/agz_superko.h): beside the simple ko of board.jl, which
 * stays, a move is refused when it recreates a position the game has seen -- the board alone (AGZ_KO_POSITIONAL) or the
 * board with the side to move (AGZ_KO_SITUATIONAL).  AGZ_KO_SIMPLE, the default, is the reference's rule and leaves
 * every output as it was.  The seen set of a node: its own position, its ancestors up to the root, the roots the slot has
 * left behind since its install, and the history_len boards handed to that install (start tables, agz_tree_init,
 * analysis and review starts).  Positions older than a supplied history are unknown to the rule.  Pass is always legal.
 * The rule lives where a node's legal mask is written, so it holds in every search the engine runs: self-play, the
 * arena, analysis, review, reanalysis and single trees.  Records, features and meta.ko are unchanged.
 * Known limit: positions are compared by 64-bit keys, so a key collision forbids a legal move.
 * Review and reanalysis: review_next_ply gives a game up at a recorded move that is not in the root's mask, so under a
 * rule a game recorded without it can be given up from that ply on, with the existing status (AGZ_BAD_ARGUMENT rows)
 * and counters; reanalysis skips and counts such rows as it does other invalid ones.
 * The setter synchronises and restarts the two counters.  Refused (AGZ_BAD_ARGUMENT, the setting in force kept): an
 * unknown rule; games of a run still being played; between agz_tree_search_select and agz_tree_search_incorporate.
 * The key arrays (8 bytes per node, 8 * (7 + max_game_length) bytes per slot) are allocated when a rule is first taken. */
#include "agz_superko.h"
agz_status agz_search_set_ko_rule(agz_engine* e, int32_t rule);
/* out[0] = nodes that lost at least one move to the rule, out[1] = moves removed; since the later of the setter call and agz_selfplay_start.  Synchronises. */
agz_status agz_search_superko_counts(agz_engine* e, uint64_t* out /* [2] */);
/* the key of `node` of single tree g under the rule in force; with no rule set, its position key computed on demand */
agz_status agz_tree_node_key(agz_engine* e, int32_t g, int32_t node, uint64_t* key);
/* the legal mask of `node` as the search reads it: out int8[A] */
agz_status agz_tree_node_legal(agz_engine* e, int32_t g, int32_t node, int8_t* out /* [A] */);
/* the keys of B positions under `rule` (AGZ_KO_SIMPLE: position keys); SoA as agz_go_legal, one launch */
agz_status agz_go_keys(agz_engine* e, const int8_t* boards, const int8_t* to_play, int32_t B, int32_t rule,
                       uint64_t* keys_out /* [B] */);
/* all_legal_moves under `rule`: position b is refused the moves whose resulting key is one of the caller's
 * seen_keys[seen_off[b] .. seen_off[b+1]) (seen_off int64[B + 1], ascending from 0); one launch */
agz_status agz_go_legal_seen(agz_engine* e, const int8_t* boards, const int8_t* to_play, const int32_t* ko,
                             const uint64_t* seen_keys, const int64_t* seen_off, int32_t B, int32_t rule,
                             int8_t* legal_out /* [B][A] */);
/* agz_position_key of include/agz_superko.h; host only, needs no engine.  AGZ_BAD_ARGUMENT: a NULL pointer, an unknown
 * rule, to_play not +-1. */
agz_status agz_go_position_key(const int8_t* board, int32_t P, int32_t to_play, int32_t rule, uint64_t* out);
agz_status agz_analyze_progress(agz_engine* e, int64_t* done_out);
/* out[B], child_N / child_W / prior [B][A] (the root's rows when the search ended); any of them may be NULL */
agz_status agz_analyze_results(agz_engine* e, agz_analysis* out, float* child_N, float* child_W, float* prior);

/* ---------------------------------------------------------------- batched game review --- */
/* play() (src/play.jl:25-77) over many recorded games in one device run (ours; the reference reviews a game with one
 * MCTSPlayer).  Game j (0-based) is a start position and moves m_0 .. m_{n_j-1}; its row k (0-based) gives exactly what
 *   p = MCTSPlayer(env, nn; num_readouts, two_player_mode) with draw-stream seed agz_config.seed and game id
 *   game_id_base + j;  initialize_game!(p, start_j);  for k: suggest_move(p), then play_move!(p, m_k)
 * gives at its k-th suggest_move: the move picked and the root's N, W, Q and rows.  play_move! with the recorded move
 * re-roots the same tree, so the subtree under m_k is kept and ply k + 1 searches until N(root) >= N0 + num_readouts.
 * No Dirichlet noise, no resignation, no record.  The rows do not depend on the number of slots, on which slot takes a
 * game, or on splitting the games over runs with matching game_id_base.  Board symmetries apply as in the tree path.
 *
 * agz_review_start: moves int16[total] (actions 0..N*N, N*N = pass), game j's moves game_offset[j] .. game_offset[j+1]-1
 * (game_offset int64[G+1], 0 first, non-decreasing, total last); boards / info / history: the start positions, in the
 * conventions of agz_analyze_start, one per game, or boards = info = history = NULL for the empty board with
 * agz_config.komi.  Host checks (a bad value fails the call naming the game): the moves' range, the offsets, the
 * agz_position_info fields as agz_analyze_start checks them.  Refused in arena_mode.  The run is stepped as an analysis
 * run and read with agz_analyze_progress / agz_analyze_results, which count and return the total rows: game j's ply k is
 * row game_offset[j] + k.
 *
 * status per row: as agz_analyze_results', and: AGZ_BAD_ARGUMENT (move -1, nothing searched) for every row of a game
 * from the first recorded move that cannot be played (illegal at that root, or after the game ended: two passes or
 * max_game_length) -- or for all its rows when the start board is invalid; the earlier rows and other games are not
 * affected.  AGZ_POOL_EXHAUSTED under AGZ_POOL_MOVE_EARLY is a short but valid row and the game goes on; under
 * AGZ_POOL_STALL the slot waits, and agz_slot_abandon gives up the rest of the game (its current row carries the
 * statistics reached, the later rows none; all move -1). */
agz_status agz_review_start(agz_engine* e, const int16_t* moves, const int64_t* game_offset, const int8_t* boards,
                            const agz_position_info* info, const int8_t* history, int64_t G, uint64_t game_id_base);

/* ---------------------------------------------------------------- reanalysis ------------ */
/* Refresh the targets of games already in the replay arena with the engine's current network (ours; MuZero's
 * Reanalyse): the stored positions are searched again and the records' pi rows and qs overwritten; the moves, the
 * outcome, the headers, the arena's order and its window stay as played.  Off unless called.
 *
 * agz_replay_reanalyze_start starts a review run (see agz_review_start) whose games are arena games first ..
 * first + count - 1, indexed as agz_replay_game indexes them.  Nothing of a record visits the host: a kernel copies its
 * moves into the review tables, takes its start from the start-position table (entry header.game_id mod S by the index
 * rule of agz_selfplay_set_starts; no table: the empty board with agz_config.komi), and keys its draws by game id
 * game_id_base + header.game_id -- so a row depends neither on the arena index of its game nor on first and count, and
 * runs over disjoint ranges, or over the same games ingested in another order, give the same rows per game_id.
 * Everything else is agz_review_start's contract: row k of a game is suggest_move at ply k of
 *   p = MCTSPlayer(env, nn; num_readouts) with draw-stream seed agz_config.seed and that game id;
 *   initialize_game!(p, start);  for k: suggest_move(p), then play_move!(p, m_k)
 * on the selected network (agz_net_select) and the engine's own num_readouts and pool: plain PUCT without noise,
 * resignation or record, whatever playout cap, forced playouts or Gumbel setting self-play has;
 * agz_selfplay_set_symmetry applies.  It takes over the slots (self-play games in flight are dropped; a later
 * agz_selfplay_start plays as a fresh engine does), is stepped with agz_selfplay_step and read with
 * agz_analyze_progress / agz_analyze_results / agz_slot_status, with agz_analyze_set_lines on also agz_analyze_lines;
 * game j's ply k is row (moves of the run's games before j) + k.  Besides the tables of a review run every finished
 * search keeps the row children_as_pi(root, n <= tau_threshold) -- what play_move! appends to searches_pi
 * (mcts_play.jl:26-50), taken before the recorded move re-roots the tree.  A record whose move cannot be played (or is
 * outside 0..N*N) gives AGZ_BAD_ARGUMENT rows from that ply on, as in a review run.
 * Refused (AGZ_BAD_ARGUMENT, nothing changed): first < 0, count < 1, first + count > agz_replay_count, an empty arena,
 * an arena_mode engine.
 *
 * agz_replay_reanalyze_commit writes the run into the arena, one wave per row, on the engine's stream.  A row is
 * committed iff its agz_analysis.status is AGZ_OK: qs[k] = Q (= W / (1 + N) of the root, Black-absolute, the expression
 * self-play records), and the pi row replaces the record's unless that one is all zero.  An all-zero row means "no
 * policy target" (a fast search of agz_selfplay_set_playout_cap, an arena record) and stays all zero, so the
 * targets-only index, the window and the entry numbering of agz_replay_sample hold.  Short rows
 * (AGZ_POOL_EXHAUSTED), invalid rows (AGZ_BAD_ARGUMENT), failed soft picks and given-up rows leave their plies as they
 * were.  counts_out (may be NULL) = {rows committed, pi rows overwritten, rows skipped}.  agz_replay_game, _batch,
 * _batch_sym, _sample and the value targets of agz_replay_set_value_target read the new rows from then on.
 * Synchronises.  The arena is unchanged until commit.  Refused (AGZ_BAD_ARGUMENT, the arena unchanged): no reanalysis
 * run in force (agz_analyze_start, agz_review_start and agz_selfplay_start end one); the run not complete
 * (agz_analyze_progress below its rows); a second commit of one run; any agz_replay_ingest*, agz_replay_trim, _clear,
 * _set_window or _set_targets_only call since the start. */
agz_status agz_replay_reanalyze_start(agz_engine* e, int64_t first, int64_t count, uint64_t game_id_base);
agz_status agz_replay_reanalyze_commit(agz_engine* e, int64_t counts_out[3]);

/* ---------------------------------------------------------------- analysis lines -------- */
/* The top-K candidate moves of a searched node and the principal variation (PV) the search expects behind each: what
 * most_visited_path, mvp_gg and describe of src/mcts.jl:255-327 define (commented out there; their text is the
 * definition followed here).  All values are exact reads of the node rows child_N / child_W / child_prior / children,
 * no arithmetic.  For a node X:
 *   candidates of X: the actions a with child_N[a] > 0, by child_N descending, then child_prior descending, then a
 *     ascending; the first K are the lines.  (describe's second key is the action score; the prior is a stored value,
 *     so the order is reproducible bit for bit by anyone who reads the rows.)
 *   PV of candidate a, depth limit D >= 1, min_visits >= 1: pv[0] = a, c = child of X under a.  While pv_len < D and c
 *     is a node: m = max of c's child_N; stop if m < min_visits; b = the lowest action with child_N == m (findmax, no
 *     draw); append b; c = child of c under b.  min_visits 1 is most_visited_path, 2 is mvp_gg (maximum(child_N) > 1).
 *   pv_N[d] = the child_N entry pv[d] was chosen by (pv_N[0] = the candidate's N).  Per line: the candidate's N, W and
 *     prior at X, end_W = the child_W entry of the last PV move (Q of the line's end = end_W / (1 + pv_N[pv_len-1])).
 *   Unused line slots: move -1, pv_len 0, the floats 0; pv entries beyond pv_len: -1, pv_N 0.
 * Off by default; with it off every table, record and counter of a run is what it is without this section. */
typedef struct {
  int32_t move, pv_len;
  float N, W, prior, end_W;
} agz_line;
/* K = 0 switches lines off (default).  0 <= K <= 16, 1 <= D <= 64, min_visits >= 1.  Takes effect at the next
 * agz_analyze_start / agz_review_start: every finished search then also writes the lines of its root, taken when the
 * search ended (in a review run: before the recorded move re-roots the tree).  Rows that are never searched keep K
 * unused slots. */
agz_status agz_analyze_set_lines(agz_engine* e, int32_t K, int32_t D, int32_t min_visits);
/* lines [rows][K], pv [rows][K][D], pv_N [rows][K][D]; any may be NULL.  AGZ_NOT_READY until every row is
 * finished; AGZ_BAD_ARGUMENT when the run was started with lines off. */
agz_status agz_analyze_lines(agz_engine* e, agz_line* lines, int16_t* pv, float* pv_N);
/* the same for any node of single tree g (the MCTSPlayer path): one launch, one copy */
agz_status agz_tree_lines(agz_engine* e, int32_t g, int32_t node, int32_t K, int32_t D, int32_t min_visits,
                          agz_line* lines, int16_t* pv, float* pv_N);

/* Test hooks (device-side evaluation of the draw stream, single-tree introspection setters) are declared in
 * include/agz_debug.h: exported by the library for the parity tests, not part of the drop-in surface. */

#ifdef __cplusplus
}
#endif
#endif /* AGZ_H */

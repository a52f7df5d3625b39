// agz_engine.h -- host-side engine object behind the C ABI (include/agz.h).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "agz_common.h"
#include "agz_layout.h"
#include "agz_nn.h"
#include "agz_replay.h"
#include "agz_state.h"

namespace agz {

struct TreeArgs;

class Engine {
 public:
  explicit Engine(const agz_config& cfg);
  ~Engine();

  const agz_config& config() const { return cfg_; }
  const View& view() const { return V_; }
  Net& net() { return (net_sel_ && net2_) ? *net2_ : *net_; }   // the network agz_net_* calls address
  void net_select(int which);
  void arena_counts(int32_t* out) const;
  hipStream_t stream() const { return stream_; }
  void sync();

  // batched self-play
  void start(int64_t total_games);
  void step(int nsteps);
  void stats(agz_stats* out);
  int debug_counters(uint64_t* out, int cap);
  void debug_live_record(int g, int k, uint64_t* game_id, int32_t* num_moves, int32_t* move, float* pi, float* q);
  void debug_set_stagger(int moves);
  int select_external();
  // batched analysis (agz_analyze_*): suggest_move over B caller positions, stepped by step() / the external split
  void analyze_start(const int8_t* boards, const agz_position_info* info, const int8_t* history, int64_t B,
                     uint64_t game_id_base);
  // batched game review (agz_review_start): play() over G recorded games on reused trees, rows read as in analysis
  void review_start(const int16_t* moves, const int64_t* game_offset, const int8_t* boards, const agz_position_info* info,
                    const int8_t* history, int64_t G, uint64_t game_id_base);
  // reanalysis (agz_replay_reanalyze_start / _commit): a review run over arena games [first, first + count) gathered on
  // the device, then its finished rows written over the records' pi and q targets
  void replay_reanalyze_start(int64_t first, int64_t count, uint64_t game_id_base);
  void replay_reanalyze_commit(int64_t counts_out[3]);
  // start positions of self-play / arena games and of everything that replays their records (agz_selfplay_set_starts)
  void set_starts(const int8_t* boards, const agz_position_info* info, const int8_t* history, int64_t S);
  int64_t starts_count() const { return V_.st_count; }
  // playout cap randomization of self-play (agz_selfplay_set_playout_cap): fast_readouts = 0 is off
  void set_playout_cap(int fast_readouts, double full_prob);
  void playout_cap_counts(int64_t out[2]);
  // forced playouts and policy target pruning of self-play (agz_selfplay_set_forced_playouts): k = 0 is off
  void set_forced_playouts(double k, int prune);
  void forced_counts(int64_t out[2]);
  void tree_pruned_pi(int g, int node, double k, float* out);
  // Gumbel root search of self-play (agz_selfplay_set_gumbel): m = 0 is off
  void set_gumbel(int m, double c_visit, double c_scale);
  void gumbel_counts(int64_t out[2]);
  void tree_gumbel_pi(int g, int node, double c_visit, double c_scale, float* out);
  // PUCT rule options of every search (agz_search_set_puct): (0, 0, 0, 0) is off
  void set_puct(int fpu_on, double r, double r_root, double c_base);
  void puct_counts(int64_t out[2]);
  // root exploration and the move temperature (agz_selfplay_set_root_policy_temperature / _set_root_noise,
  // agz_search_set_move_temperature): off by default
  void set_root_policy_temperature(int on, double early, double late, double halflife);
  void set_root_noise(double total_alpha, int shaped);
  void set_move_temperature(int on, double early, double late, double halflife);
  void explore_counts(uint64_t out[4]);
  void tree_explore_rows(int g, int node, float* tempered, double* alpha, float* noised);
  // value uncertainty (agz_search_set_value_moments / _set_lcb / _set_puct_variance): off by default
  void set_value_moments(int on);
  void set_lcb(double z, int min_visits, double min_ratio);
  void set_puct_variance(double k, double prior, double prior_weight);
  void uncertainty_counts(uint64_t out[4]);
  // superko (agz_search_set_ko_rule): AGZ_KO_SIMPLE by default
  void set_ko_rule(int rule);
  void superko_counts(uint64_t out[2]);
  void tree_child_lcb(int g, int node, double z, double* mean, double* sd, double* lcb);
  void analyze_child_S(float* child_S, float* root_S);
  int64_t analyze_progress();
  void analyze_results(agz_analysis* out, float* child_N, float* child_W, float* prior);
  // analysis lines (agz_analyze_set_lines / agz_analyze_lines / agz_tree_lines): top-K candidates with their PVs
  void analyze_set_lines(int K, int D, int min_visits);
  void analyze_lines(agz_line* lines, int16_t* pv, float* pv_N);
  void tree_lines(int g, int node, int K, int D, int min_visits, agz_line* lines, int16_t* pv, float* pv_N);
  void leaf_features_external(float* feats_out);
  void incorporate_external(const float* pi, const float* v);

  // records
  int64_t records_count();
  void record_header(int64_t k, agz_game_header* out);
  void record_game(int64_t k, int16_t* moves, float* pis, float* qs);
  int64_t records_packed_size(int64_t first = 0, int64_t last = -1);    // last = -1: records_count()
  void records_export_packed(void* dst, int64_t capacity, bool is_device);
  void records_clear();
  int64_t pack_records_device(uint8_t* dst, int64_t capacity, int64_t* nbytes, int64_t first = 0, int64_t last = -1);
  // records [0, records_exchanged()) have been filed by agz_allgather_records since the last agz_records_clear
  int64_t records_exchanged() const { return rec_sent_; }
  void records_mark_exchanged(int64_t upto) { rec_sent_ = upto; }
  void record_features(int64_t k, float* out);
  // the value targets y_t of ring record k under (alpha, lambda) (agz_records_value_targets, include/agz_value_target.h)
  void record_value_targets(int64_t k, double alpha, double lambda, float* out);

  // device replay arena (agz_replay.h): what is the arena's alone is called on replay(); here is what joins it to the
  // record ring (the ingest entry points stage a host buffer or pack the ring, then file the bytes), to the network
  // (agz_replay_score: one KL(pi || p) per ply of arena games [first, first + count) on the selected network) and to the
  // engine's staging buffers (replay_batch)
  ReplayArena& replay() { return *replay_; }
  int64_t replay_ingest(const void* packed, int64_t nbytes, bool is_device);
  int64_t replay_ingest_local();
  // records [first, first + count) of this engine's ring into the arena, device to device (agz_replay_ingest_records)
  int64_t replay_ingest_records(int64_t first, int64_t count);
  int64_t replay_ingest_gathered(const void* buf, bool is_device, size_t nbytes, const std::vector<int64_t>& coff,
                                 const std::vector<int64_t>& cbytes, const std::vector<int64_t>& cnrec);
  int64_t replay_score(int64_t first, int64_t count);
  // sym != NULL: sample b under the board symmetry T_sym[b] (agz_replay_batch_sym)
  void replay_batch(const int64_t* game, const int32_t* ply, int B, float* feats, float* pi, float* z,
                    bool out_is_device, const int32_t* sym = nullptr);
  DevBuf<uint8_t>& pack_scratch() { return s_pack_; }
  // one optimisation step on the selected network (agz_train.hip)
  void train_step(const float* feats, const float* pi, const float* z, int B, bool is_device, float eta, float rho,
                  float* losses_out);
  void train_reset();
  // flat parameter vector of the selected network in layers() order (broadcast_weights)
  std::vector<float> weights_flat();
  void weights_set_flat(const std::vector<float>& w);
  // start != NULL: sample b's move list begins at table entry start[b], -1 = the empty board (agz_replay_features_starts)
  void replay_batch_features(const int16_t* moves, int64_t nmoves, const int32_t* off, const int32_t* ply, int B,
                             float* out, bool out_is_device, const int32_t* start = nullptr);

  // network
  void net_forward_positions(const int8_t* boards, const int8_t* deltas, const int32_t* ndeltas,
                             const int8_t* to_play, int B, float* pi_out, float* v_out);
  void net_forward_features(const float* feats, int B, float* pi_out, float* v_out);
  void net_forward_features_sym(const float* feats, const int32_t* sym, int B, float* pi_out, float* v_out);
  // board symmetry of the engine's own evaluations (agz_selfplay_set_symmetry): AGZ_SYMMETRY_NONE, 0..7, RANDOM
  void set_symmetry(int mode);
  // finished-slot hold of train() (agz_selfplay_set_hold / agz_selfplay_release)
  void set_hold(bool on);
  void release();
  void features(const int8_t* boards, const int8_t* deltas, const int32_t* ndeltas, const int8_t* to_play,
                int B, float* out);
  float time_forward(int B, int iters);
  // HIP events around the five search kernels of the next steps (bench.py's `search_kernels`)
  void profile_search_enable(bool on);
  void profile_search_read(double* ms5, int64_t* steps);
  float time_conv(int B, int iters);
  void slot_status(int32_t* status, int32_t* nodes, int32_t* moves);
  void slot_abandon(int g);

  void debug_draws(uint64_t seed, uint64_t game, uint32_t move, int n, double alpha, double* out);
  void debug_math(int op, const double* x, const double* y, int n, double* out);

  // Go rules
  void go_play(const int8_t* boards, const int8_t* to_play, const int32_t* ko, const int32_t* moves, int B,
               int8_t* boards_out, int32_t* ko_out, int32_t* ncap_out, int32_t* status_out);
  void go_legal(const int8_t* boards, const int8_t* to_play, const int32_t* ko, int B, int8_t* out);
  void go_keys(const int8_t* boards, const int8_t* to_play, int B, int rule, uint64_t* out);
  void go_legal_seen(const int8_t* boards, const int8_t* to_play, const int32_t* ko, const uint64_t* seen_keys,
                     const int64_t* seen_off, int B, int rule, int8_t* out);
  void go_score(const int8_t* boards, const float* komi, int B, float* out);

  // single-tree compat
  int tree_op(TreeArgs& T, int32_t* r0);           // returns the op's agz_status
  int tree_search_select(int g, int par, int* nleaves);
  void tree_leaf_features(int g, float* feats_out);
  void tree_leaf_positions(int g, int32_t* nodes, int8_t* boards, int8_t* deltas, int32_t* ndeltas, int8_t* to_play,
                           agz_position_info* info);
  int tree_search_incorporate(int g, const float* pi, const float* v);   // pi == NULL: engine's own network
  void game_state(int g, GameState* out);
  void game_patch(int g, const GameState& s);
  void node_meta(int g, int node, NodeMeta* out);
  void node_meta_set(int g, int node, const NodeMeta& m);
  void node_row_get(int g, int node, int field, float* out);
  void node_row_set(int g, int node, int field, const float* in);
  void node_children(int g, int node, int32_t* out);
  void node_board(int g, int node, int8_t* out);
  uint64_t node_key(int g, int node);              // under the rule in force; the position key with none
  void node_legal(int g, int node, int8_t* out);   // the node's mask, [A]
  float node_stat(int g, int node, int which);     // 0 = N, 1 = W, 2 = S (moments on)
  void node_set_N(int g, int node, float v);

  std::string last_error;

 private:
  void upload_view_outputs();
  void fill_synthetic_inputs(int B);
  void check_game(int g) const;
  void check_node(int g, int node) const;
  // shared by the option setters and their readers (`what` is the error text's prefix)
  void require_selfplay_engine(const char* what) const;
  void require_between_games(const char* what);
  template <class Write>
  void set_option(const char* what, bool single_trees, Write write, int first, int n);
  template <class Visit, class... T>
  void alloc_group(Visit visit, DevBuf<T>&... own);
  template <class T>
  void read_counters(int first, int n, T* out);
  template <class Launch>
  void read_tree_pi_row(float* out, Launch launch);
  void set_all_slots(int phase);
  void idle_all_slots();
  // host <-> device staging on stream_ (the primitives and their rules: agz_common.h)
  template <class T> T* stage(DevBuf<T>& b, const T* host, size_t n) { return agz::stage(b, host, n, stream_); }
  template <class T> void up(T* dev, const T* host, size_t n) { agz::upload(dev, host, n, stream_); }
  template <class T> void down(T* host, const T* dev, size_t n) { agz::download(host, dev, n, stream_); }
  template <class T> T fetch(const T* dev) { return agz::fetch(dev, stream_); }
  template <class T> void put(T* dev, const T& v) { agz::put(dev, v, stream_); }
  void wait() { AGZ_HIP(hipStreamSynchronize(stream_)); }
  // the shared steps of the ABI calls (agz_engine.hip)
  void stage_positions(const int8_t* boards, const int8_t* deltas, const int32_t* ndeltas, const int8_t* to_play, int B);
  float* stage_forward(const int& B);
  void forward_x32(int B);
  void forward_staged(int B, const int32_t* d_sym, float* pi_out, float* v_out);
  template <class Launch>
  float time_launches(int iters, Launch launch);
  size_t packed_layout(int64_t first, int64_t last, std::vector<int64_t>& off);

  agz_config cfg_;
  View V_{};
  hipStream_t stream_ = nullptr;
  std::unique_ptr<Net> net_, net2_;   // net2_: White's network in arena mode
  std::unique_ptr<Trainer> trainer_, trainer2_;
  int net_sel_ = 0;
  static constexpr int kSearchProfMax = 512;      // steps whose search kernels are timed after profile_search_enable(true)
  bool sprof_on_ = false;
  int sprof_n_ = 0;
  std::vector<hipEvent_t> sprof_ev_;              // [step][7]: before k_pre, behind k_pre / k_expand / k_scan / k_leaf_features, in front of / behind k_post
  int external_batch2_ = 0;
  std::vector<void*> bufs_;
  size_t state_bytes_ = 0;
  int bcap_ = 0;
  DevBuf<float> d_x32_, d_pi_, d_v_, d_whcn_;
  DevBuf<int32_t> d_count_;
  // staging for ABI calls
  DevBuf<int8_t> s_boards_, s_deltas_, s_tp_, s_boards_out_, s_legal_, s_leafb_;
  DevBuf<uint8_t> s_leafrows_;
  DevBuf<int32_t> s_i32a_, s_i32b_, s_i32c_, s_i32d_;
  DevBuf<float> s_f32a_, s_f32b_;
  DevBuf<float> s_symf_, s_symp_;     // feature / policy rows before their symmetry transform
  DevBuf<int32_t> s_sym_;
  DevBuf<int16_t> s_i16a_;
  DevBuf<int64_t> s_i64a_;
  DevBuf<double> s_f64_;
  DevBuf<int32_t> s_iout_;
  int external_batch_ = 0;
  int tree_batch_ = 0;
  int64_t abandoned_ = 0;       // games dropped by slot_abandon since the last selfplay_start
  // analysis mode: the caller's positions and the result tables of the last agz_analyze_start (View::an_*)
  DevBuf<int8_t> an_board_, an_hist_;
  DevBuf<agz_position_info> an_info_;
  DevBuf<agz_analysis> an_res_;
  DevBuf<float> an_rows_;       // [3][B][A]: child_N, child_W, prior
  DevBuf<float> an_s_;          // [B][A] child_S, then [B] root_S: a run begun with moments on (View::an_childS / an_rootS)
  DevBuf<float> child_s_, root_s_;   // View::childS / rootS once agz_search_set_value_moments has switched them on
  DevBuf<uint64_t> sk_key_, sk_log_;   // View::sk_key / sk_log / sk_len once agz_search_set_ko_rule has taken a superko rule
  DevBuf<int32_t> sk_len_;
  DevBuf<uint64_t> s_u64_;
  int64_t an_count_ = 0;         // rows of the current run
  DevBuf<int16_t> rv_moves_;    // review mode: the recorded moves and game offsets (View::rv_*)
  DevBuf<int64_t> rv_off_;
  std::vector<int64_t> rv_off_host_;
  int lines_k_ = 0, lines_d_ = 16, lines_min_ = 1;   // agz_analyze_set_lines: what the next start call switches on
  DevBuf<agz_line> an_line_;    // [rows][K]       the lines tables of the current run (View::an_line / an_pv / an_pvN)
  DevBuf<int16_t> an_pv_;       // [rows][K][D]
  DevBuf<float> an_pvN_;        // [rows][K][D]
  DevBuf<uint8_t> s_lines_;     // agz_tree_lines: lines, pv_N, pv of one node behind one another
  void check_positions(const char* mode, const char* item, const agz_position_info* info, const int8_t* history,
                       int64_t B);
  void upload_position_table(DevBuf<int8_t>& board, DevBuf<int8_t>& hist, DevBuf<agz_position_info>& inf,
                             const int8_t* boards, const agz_position_info* info, const int8_t* history, int64_t B);
  void upload_positions(const int8_t* boards, const agz_position_info* info, const int8_t* history, int64_t B,
                        int64_t rows);
  void clear_result_tables(int64_t rows);
  void begin_analysis_run(int64_t B, int64_t rows, uint64_t game_id_base);
  // reanalysis: the run in force (begin_analysis_run ends it), its first arena game and the arena's change counter at
  // its start; the per-game draw ids and the pi rows of the run (View::an_gid / an_pi); the commit's three counts
  bool ra_on_ = false, ra_committed_ = false;
  int64_t ra_first_ = 0;
  uint64_t ra_stamp_ = 0;
  DevBuf<uint64_t> an_gid_;
  DevBuf<float> an_pi_;
  DevBuf<unsigned long long> ra_counts_;
  std::unique_ptr<ReplayArena> replay_;     // made behind stream_, which it enqueues on
  DevBuf<uint8_t> s_pack_;          // packed records on their way out of the ring or into the arena
  DevBuf<int32_t> hold_rel_;        // View::released
  DevBuf<int8_t> st_board_, st_hist_;       // the start-position table in force (View::st_*)
  DevBuf<agz_position_info> st_info_;
  int64_t rec_sent_ = 0;
  bool stepped_ = false;           // a step has run since the last start(): agz_debug_set_stagger is refused
};

// RCCL exchange (agz_comm.hip)
struct Comm;
void comm_unique_id(uint8_t* out);
Comm* comm_create(Engine& E, int rank, int world, const uint8_t* id);
void comm_destroy(Comm* c);
int64_t comm_allgather_records(Engine& E, Comm* c);
// host logic of the exchange between its two collectives (also the C ABI's agz_gather_plan): checks the gathered
// {records, bytes} pairs, returns the padded per-rank chunk size; throws AGZ_RCCL_ERROR naming the offending rank
int64_t gather_plan(const int64_t* counts, int world, int64_t* total_records);
int64_t comm_broadcast_weights(Engine& E, Comm* c, int root);

}  // namespace agz

// agz_engine.h -- host-side engine object behind the C ABI (include/agz.h).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "agz_common.h"
#include "agz_layout.h"
#include "agz_nn.h"
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

  // device replay arena: finished games of every rank, packed, resident in HBM
  int64_t replay_ingest(const void* packed, int64_t nbytes, bool is_device);
  int64_t replay_ingest_local();
  // records [first, first + count) of this engine's ring into the arena, device to device (agz_replay_ingest_records)
  int64_t replay_ingest_records(int64_t first, int64_t count);
  int64_t replay_ingest_gathered(const void* buf, bool is_device, size_t nbytes, const std::vector<int64_t>& coff,
                                 const std::vector<int64_t>& cbytes, const std::vector<int64_t>& cnrec);
  int64_t replay_ingest_chunks(const uint8_t* dbuf, const std::vector<int64_t>& coff,
                               const std::vector<int64_t>& cbytes, const std::vector<int64_t>& cnrec);
  int64_t replay_count() const { return (int64_t)rp_hdr_.size(); }
  int64_t replay_positions() const { return rp_positions_; }
  int64_t replay_bytes() const { return (int64_t)rp_used_; }
  void replay_header(int64_t k, agz_game_header* out) const;
  void replay_game(int64_t k, int16_t* moves, float* pis, float* qs);
  void replay_trim(int64_t max_positions);
  void replay_clear();
  // the sampling window of train(): the newest max_entries entries stay live (agz_replay_set_window)
  void replay_set_window(int64_t max_entries);
  int64_t replay_live_positions() const {
    return rp_entry_cum().back() - rp_entry_cum()[(size_t)rp_first_game_] - rp_first_ply_;
  }
  // targets-only arena (agz_replay_set_targets_only): an entry is a ply whose pi row is not all zero
  void replay_set_targets_only(bool on);
  // the z of the batch calls is y_t under (alpha, lambda) (agz_replay_set_value_target); alpha = 0 (the default) is off
  void replay_set_value_target(double alpha, double lambda);
  // policy surprise weighting (agz_replay_score / _set_surprise / _surprise, include/agz_surprise.h): one KL(pi || p)
  // per ply of arena games [first, first + count) on the selected network; rho = 0 (the default) is off
  int64_t replay_score(int64_t first, int64_t count);
  void replay_set_surprise(double rho);
  void replay_surprise(int64_t k, double* kl_out, uint32_t* q_out, int32_t* scored_out);
  // get_replay_batch without the host: B distinct live entries drawn on the device (agz_replay_sample)
  void replay_sample(int B, uint64_t call, int sym_mode, float* feats, float* pi, float* z, int64_t* game_out,
                     int32_t* ply_out);
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
  float node_stat(int g, int node, int which);     // 0 = N, 1 = W
  void node_set_N(int g, int node, float v);

  std::string last_error;

 private:
  void replay_reserve(size_t bytes);
  void replay_drop_front(size_t drop);
  void replay_scan_targets(size_t first_new);
  void replay_index_to_device();
  // the prefix the window and the sampler count entries by: every ply, or target plies only
  const std::vector<int64_t>& rp_entry_cum() const { return rp_targets_only_ ? rp_tcum_ : rp_cum_; }
  void upload_view_outputs();
  void fill_synthetic_inputs(int B);
  void check_game(int g) const;
  void check_node(int g, int node) const;
  // shared by the option setters and their readers (`what` is the error text's prefix)
  void require_selfplay_engine(const char* what) const;
  void require_between_games(const char* what);
  template <class Write>
  void set_option(const char* what, bool single_trees, Write write, int first, int n);
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
  void emit_replay_batch(int B, const int64_t* off, const int32_t* ply, const int32_t* sym, int8_t* boards, float* feats,
                         float* pi, float* z);
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
  // replay arena
  DevBuf<uint8_t> rp_buf_, s_pack_;
  size_t rp_used_ = 0;
  int64_t rp_positions_ = 0;
  std::vector<int64_t> rp_off_;
  std::vector<agz_game_header> rp_hdr_;
  std::vector<int64_t> rp_cum_{0};  // [count + 1]: positions of the games before game k
  int64_t rp_first_game_ = 0;       // the window (agz_replay_set_window): entries before ply rp_first_ply_ of game
  int64_t rp_first_ply_ = 0;        // rp_first_game_ are dead
  DevBuf<int64_t> d_rp_cum_, d_rp_off_;   // device copies of rp_cum_ / rp_off_ for the sampler
  int64_t rp_dev_n_ = 0;            // games whose rp_cum_ / rp_off_ entries are on the device
  uint64_t rp_change_ = 0;          // bumped by every ingest, trim, clear, window and targets-only call (reanalysis commit)
  // targets-only mode: rp_tcum_[k] = target plies of the games before game k (next to rp_cum_; the window's
  // rp_first_ply_ is then an index into rp_first_game_'s target list); d_rp_tply_[rp_cum_[k] + i] = the i-th target ply
  // of game k, written by k_replay_targets at ingest
  bool rp_targets_only_ = false;
  std::vector<int64_t> rp_tcum_{0};
  DevBuf<int64_t> d_rp_tcum_;
  DevBuf<int16_t> d_rp_tply_;
  DevBuf<int64_t> tgt_idx_;         // replay_scan_targets: offsets and position prefix of the games just filed
  DevBuf<int32_t> tgt_cnt_;         // ... and their target counts
  double vt_alpha_ = 0.0, vt_lambda_ = 1.0;   // agz_replay_set_value_target; alpha = 0: off, z stays the result
  // policy surprise weighting: rp_scored_[k] = game k has scores; d_sp_kl_ / d_sp_tgt_[rp_cum_[k] + t] = the score and the
  // target flag of ply t of a scored game (laid out by the position prefix, as d_rp_tply_ is; what lies under an unscored
  // game is never read).  d_sp_q_ / d_sp_qcum_ = q and its inclusive prefix over all positions, rebuilt by
  // replay_weights_to_device when the arena (rp_change_), the scores (sp_epoch_) or rho changed since they were built
  double sp_rho_ = 0.0;
  std::vector<uint8_t> rp_scored_;
  DevBuf<double> d_sp_kl_;
  DevBuf<uint8_t> d_sp_tgt_, d_sp_scored_;
  DevBuf<uint32_t> d_sp_q_;
  DevBuf<uint64_t> d_sp_qcum_, d_sp_tiles_;
  DevBuf<int64_t> sp_off_;
  DevBuf<int32_t> sp_ply_;
  DevBuf<unsigned long long> sp_count_;
  uint64_t sp_epoch_ = 0, sp_built_change_ = 0, sp_built_epoch_ = 0, sp_total_ = 0;
  double sp_built_rho_ = 0.0;
  bool sp_built_ = false;
  void replay_scores_reserve();
  void replay_scored_to_device();
  void replay_weights_to_device();
  DevBuf<int64_t> smp_off_, smp_game_;
  DevBuf<int32_t> smp_ply_, smp_sym_;
  DevBuf<int8_t> smp_boards_;
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

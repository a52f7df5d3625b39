// agz_replay.h -- the device replay arena (agz_replay_*): finished games of
// every rank, packed (agz_wave.h: PackedRecord), resident in HBM, with the sampler, the targets-only index, the value
// targets and the policy surprise weights that read them.  The search never touches it; from the engine it takes the
// stream, the View (board sizes, seed, the start table; a reference, since st_count changes under set_starts), packed
// bytes on the device and, for scoring, one network forward.
#pragma once
#include <functional>
#include <vector>

#include "agz_common.h"
#include "agz_replay_index.h"
#include "agz_state.h"

namespace agz {

// the one thing scoring lacks: the engine's network on rows the arena has written
struct ReplayForward {
  int cap;                // rows per forward
  float* whcn;            // room for cap rows of 17 P features (WHCN)
  // forward rows [0, B) of whcn; returns the policy rows [B][A] on the device.  B must live until the next wait
  std::function<const float*(const int& B)> run;
  std::function<void()> check;      // behind the wait: raise what the forward reported
};

class ReplayArena {
 public:
  ReplayArena(hipStream_t stream, const View& V) : stream_(stream), V_(V) {}

  const ReplayIndex& index() const { return ix_; }
  int64_t count() const { return ix_.count(); }
  int64_t positions() const { return ix_.positions(); }
  int64_t bytes() const { return ix_.used(); }
  int64_t live_positions() const { return ix_.live(); }
  int64_t ingest_chunks(const uint8_t* dbuf, const std::vector<int64_t>& coff, const std::vector<int64_t>& cbytes,
                        const std::vector<int64_t>& cnrec);
  void header(int64_t k, agz_game_header* out) const;
  void game(int64_t k, int16_t* moves, float* pis, float* qs);
  void trim(int64_t max_positions);
  void clear() { ix_.clear(); }
  // the sampling window of train(): the newest max_entries entries stay live (agz_replay_set_window)
  void set_window(int64_t max_entries);
  // targets-only arena (agz_replay_set_targets_only): an entry is a ply whose pi row is not all zero
  void set_targets_only(bool on);
  // the z of the batch calls is y_t under (alpha, lambda) (agz_replay_set_value_target); alpha = 0 (the default) is off
  void set_value_target(double alpha, double lambda);
  // policy surprise weighting (agz_replay_score / _set_surprise / _surprise, include/agz_surprise.h): one KL(pi || p)
  // per ply of arena games [first, first + count) on the network behind `fwd`; rho = 0 (the default) is off
  int64_t score(int64_t first, int64_t count, const ReplayForward& fwd);
  void set_surprise(double rho);
  void surprise(int64_t k, double* kl_out, uint32_t* q_out, int32_t* scored_out);
  // get_replay_batch without the host: B distinct live entries drawn on the device (agz_replay_sample)
  void sample(int B, uint64_t call, int sym_mode, float* feats, float* pi, float* z, int64_t* game_out, int32_t* ply_out);
  void emit(int B, const int64_t* off, const int32_t* ply, const int32_t* sym, int8_t* boards, float* feats, float* pi,
            float* z);
  // what reanalysis reads and writes (Engine::replay_reanalyze_start / _commit): the packed bytes, the device offset
  // table from game `first` on (index_to_device() first), the commit of a run's rows into the records of games
  // [first, first + G) and "the scores of games [first, first + n) are of old pi rows"
  const uint8_t* buffer() const { return buf_.p; }
  void index_to_device();
  const int64_t* offsets_device(int64_t first) const { return d_off_.p + first; }
  void refresh(int64_t first, const int64_t* rv_off, int64_t G, int64_t rows, const agz_analysis* res, const float* an_pi,
               unsigned long long* counts);
  void forget_scores(int64_t first, int64_t n);

 private:
  void wait() { AGZ_HIP(hipStreamSynchronize(stream_)); }
  void reserve(size_t bytes);
  void drop_front(size_t drop);
  void scan_targets(size_t first_new);
  void scores_reserve();
  void scored_to_device();
  void weights_to_device();

  hipStream_t stream_;
  const View& V_;
  ReplayIndex ix_;
  DevBuf<uint8_t> buf_;                   // the packed records, ix_.used() bytes of them
  DevBuf<int64_t> d_cum_, d_off_, d_tcum_;   // device copies of ix_.cum() / off() / tcum() for the sampler
  // targets-only mode: d_tply_[cum[k] + i] = the i-th target ply of game k, written by k_replay_targets at ingest
  DevBuf<int16_t> d_tply_;
  DevBuf<int64_t> tgt_idx_;         // scan_targets: offsets and position prefix of the games just filed
  DevBuf<int32_t> tgt_cnt_;         // ... and their target counts
  double vt_alpha_ = 0.0, vt_lambda_ = 1.0;   // agz_replay_set_value_target; alpha = 0: off, z stays the result
  // policy surprise weighting: d_sp_kl_ / d_sp_tgt_[cum[k] + t] = the score and the target flag of ply t of a scored
  // game (laid out by the position prefix, as d_tply_ is; what lies under an unscored game is never read).  d_sp_q_ /
  // d_sp_qcum_ = q and its inclusive prefix over all positions, rebuilt by weights_to_device when the arena
  // (ix_.change()), the scores (sp_epoch_) or rho changed since they were built
  double sp_rho_ = 0.0;
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
  DevBuf<int64_t> smp_off_;         // the sampler's draw: record offset, ply and symmetry per sample
  DevBuf<int32_t> smp_ply_, smp_sym_;
  DevBuf<int8_t> boards_;           // replay scratch of the sampler and of scoring, [rows][8][PP]
  DevBuf<float> symf_, symp_;       // emit: feature / policy rows before their symmetry transform
};

}  // namespace agz

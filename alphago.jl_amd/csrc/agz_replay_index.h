// agz_replay_index.h -- the host-side game index of the device replay arena (agz_replay.h), free of HIP: per game its
// byte offset, header, scored flag and the two prefixes entries are counted by, with the sampling window, the change
// counter and the watermark of what has been uploaded.  Nothing outside the struct writes its vectors: ReplayArena does
// the device side of each step and calls here for the host side, and tests/hostsim/replay_index_check.cpp drives it
// against a naive model on the CPU.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/agz.h"

namespace agz {

class ReplayIndex {
 public:
  int64_t count() const { return (int64_t)hdr_.size(); }
  const std::vector<int64_t>& off() const { return off_; }           // [count]: where game k begins in the buffer
  const std::vector<agz_game_header>& hdr() const { return hdr_; }
  const std::vector<uint8_t>& scored() const { return scored_; }     // [count]: game k has surprise scores
  const std::vector<int64_t>& cum() const { return cum_; }           // [count + 1]: positions of the games before game k
  // targets-only mode: tcum()[k] = target plies of the games before game k (next to cum(); the window's first_ply is
  // then an index into first_game's target list); {0} while the mode is off
  const std::vector<int64_t>& tcum() const { return tcum_; }
  int64_t positions() const { return positions_; }
  int64_t used() const { return used_; }                              // bytes of the buffer the games fill
  // the window (agz_replay_set_window): entries before ply first_ply of game first_game are dead
  int64_t first_game() const { return first_game_; }
  int64_t first_ply() const { return first_ply_; }
  bool targets_only() const { return targets_only_; }
  // bumped by every ingest, trim, clear, window and targets-only call (reanalysis commit, the sampler's weights)
  uint64_t change() const { return change_; }
  void touch() { ++change_; }

  // the prefix the window and the sampler count entries by: every ply, or target plies only
  const std::vector<int64_t>& entry_cum() const { return targets_only_ ? tcum_ : cum_; }
  int64_t window_start() const { return entry_cum()[(size_t)first_game_] + first_ply_; }
  int64_t live() const { return entry_cum().back() - window_start(); }

  // a game of `bytes` bytes filed at byte `offset`; it has no surprise scores (agz_replay_score)
  void append(const agz_game_header& h, int64_t offset, int64_t bytes) {
    off_.push_back(offset);
    hdr_.push_back(h);
    scored_.push_back(0);
    positions_ += h.num_moves;
    cum_.push_back(positions_);
    used_ += bytes;
  }
  // targets-only: the target counts of games [first_new, count), which have just been appended
  void set_targets(size_t first_new, const std::vector<int32_t>& counts) {
    tcum_.resize(first_new + 1);
    for (int32_t c : counts) tcum_.push_back(tcum_.back() + c);
  }
  void set_scored(int64_t first, int64_t n, bool on) {
    for (int64_t k = first; k < first + n; ++k) scored_[(size_t)k] = on ? 1 : 0;
  }
  // forget the oldest n games (0 < n < count): offsets and prefixes are rebased, a window that began in a dropped game
  // begins at the first game kept, and everything is to be uploaded again
  void drop_front(size_t n) {
    const int64_t cut = off_[n], c0 = cum_[n];
    if (targets_only_) {
      const int64_t t0 = tcum_[n];
      tcum_.erase(tcum_.begin(), tcum_.begin() + n);
      for (auto& c : tcum_) c -= t0;
    }
    scored_.erase(scored_.begin(), scored_.begin() + n);
    off_.erase(off_.begin(), off_.begin() + n);
    hdr_.erase(hdr_.begin(), hdr_.begin() + n);
    for (auto& o : off_) o -= cut;
    cum_.erase(cum_.begin(), cum_.begin() + n);
    for (auto& c : cum_) c -= c0;
    used_ -= cut;
    positions_ -= c0;
    if (first_game_ >= (int64_t)n) {
      first_game_ -= (int64_t)n;
    } else {
      first_game_ = 0;
      first_ply_ = 0;
    }
    dev_n_ = 0;
  }
  // (the targets-only mode is a setting of the arena, not part of its contents: it stays as it is)
  void clear() {
    ++change_;
    off_.clear();
    hdr_.clear();
    scored_.clear();                // (the surprise scores go with their games)
    cum_.assign(1, 0);
    tcum_.assign(1, 0);
    used_ = 0;
    positions_ = 0;
    first_game_ = 0;
    first_ply_ = 0;
    dev_n_ = 0;
  }
  // only while the index is empty (the caller checks): the index of target plies is built as games are filed
  void set_targets_only(bool on) {
    targets_only_ = on;
    ++change_;
    first_game_ = 0;
    first_ply_ = 0;
  }

  // the window of train() (shrink, train.jl:52, per entry): entries before the newest max_entries are dead; the window's
  // start never moves back.  max_entries < 0: every entry live again (nothing dropped comes back).  With nothing left
  // live the index is cleared.  Returns the dead games in front, which may be dropped physically, and whether they should
  // be now: only once they hold more than half of the bytes, so that the copy is amortised over many calls
  struct Dead {
    int64_t games;
    bool drop;
  };
  Dead set_window(int64_t max_entries) {
    ++change_;
    if (max_entries < 0) {
      first_game_ = 0;
      first_ply_ = 0;
      return {0, false};
    }
    const std::vector<int64_t>& ec = entry_cum();
    const int64_t first = window_start() > ec.back() - max_entries ? window_start() : ec.back() - max_entries;
    int64_t k = first_game_;
    const int64_t n = count();
    while (k < n && ec[(size_t)k + 1] <= first) ++k;
    first_game_ = k;
    first_ply_ = first - ec[(size_t)k];
    if (k == n) {                   // nothing live
      clear();
      return {0, false};
    }
    return {k, k > 0 && off_[(size_t)k] > used_ / 2};
  }
  // the FIFO window of train() (`shrink`, train.jl:52): the oldest games to forget until at most max_positions remain;
  // when that is all of them the index is cleared and 0 returned
  size_t trim(int64_t max_positions) {
    ++change_;
    size_t drop = 0;
    int64_t pos = positions_;
    while (drop < hdr_.size() && pos > max_positions) pos -= hdr_[drop++].num_moves;
    if (drop == hdr_.size() && drop > 0) {
      clear();
      return 0;
    }
    return drop;
  }

  // the upload watermark: off() / cum() / tcum() of games [0, uploaded()) are on the device.  drop_front and clear reset
  // it, and so does the owner of the device tables when it replaces them (reset_upload).  What is to be sent is games
  // [pending().from, pending().to) of off() and one entry more of each prefix; mark_uploaded() says it has been
  struct Slice {
    size_t from, to;
  };
  int64_t uploaded() const { return dev_n_; }
  Slice pending() const { return {(size_t)dev_n_, hdr_.size()}; }
  void mark_uploaded() { dev_n_ = count(); }
  void reset_upload() { dev_n_ = 0; }

 private:
  std::vector<int64_t> off_;
  std::vector<agz_game_header> hdr_;
  std::vector<uint8_t> scored_;
  std::vector<int64_t> cum_{0}, tcum_{0};
  int64_t positions_ = 0, used_ = 0;
  int64_t first_game_ = 0, first_ply_ = 0;
  bool targets_only_ = false;
  uint64_t change_ = 0;
  int64_t dev_n_ = 0;
};

}  // namespace agz

// agz_wave.h -- what the HIP units that instantiate the search templates share (agz_engine.hip, agz_replay.hip): the
// wave primitives on gfx950, the per-wave scratch, the replay of a move list, and the one view of a packed record.
// HIP only: the host simulator (tests/hostsim) has primitives of its own and does not see this file.
#pragma once
#include <type_traits>

#include "agz_common.h"
#include "agz_layout.h"
#include "agz_search.h"

namespace agz {

// ------------------------------------------------------------------ the wave primitives on gfx950

struct HipWave {
  static constexpr int kLanes = kWave;
  int lane;
  __device__ HipWave() : lane((int)threadIdx.x) {}
  __device__ explicit HipWave(int l) : lane(l) {}      // (a wave of a multi-wave workgroup: kernels that never call sync())
  template <class F>
  __device__ __forceinline__ void for_each(int n, F f) const {
    for (int i = lane; i < n; i += kWave) f(i);
  }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ bool leader() const { return lane == 0; }
  __device__ __forceinline__ int reduce_sum(int v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
  }
  __device__ __forceinline__ int reduce_min(int v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o, kWave); v = t < v ? t : v; }
    return v;
  }
  __device__ __forceinline__ int reduce_max(int v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o, kWave); v = t > v ? t : v; }
    return v;
  }
  __device__ __forceinline__ double reduce_max(double v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(v, o, kWave); v = t > v ? t : v; }
    return v;
  }
  __device__ __forceinline__ float reduce_sum_f(float v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
  }
  __device__ __forceinline__ float reduce_max_f(float v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float t = __shfl_xor(v, o, kWave); v = t > v ? t : v; }
    return v;
  }
  __device__ __forceinline__ bool any(bool v) const { return __any(v) != 0; }
  __device__ __forceinline__ float shfl(float v, int src) const { return __shfl(v, src, kWave); }
  __device__ __forceinline__ int shfl(int v, int src) const { return __shfl(v, src, kWave); }
  __device__ __forceinline__ unsigned long long clock() const { return wall_clock64(); }     // 100 MHz
  __device__ __forceinline__ void count_max(unsigned long long* p, unsigned long long v) const {
    if (lane == 0) atomicMax(p, v);
  }
  // append every get(i) >= 0, i ascending, to a downward stack (base[--sp]); returns the new sp
  template <class F>
  __device__ __forceinline__ int push_desc(int n, F get, int32_t* base, int sp) const {
    for (int b = 0; b < n; b += kWave) {
      const int i = b + lane;
      const int c = i < n ? get(i) : -1;
      const unsigned long long mask = __ballot(c >= 0);
      if (c >= 0) base[sp - 1 - __popcll(mask & ((1ull << lane) - 1ull))] = c;
      sp -= __popcll(mask);
    }
    return sp;
  }
  __device__ __forceinline__ void amin(int32_t* p, int v) const { atomicMin(p, v); }
  __device__ __forceinline__ void amax(int32_t* p, int v) const { atomicMax(p, v); }
  __device__ __forceinline__ void aor(int32_t* p, int v) const { atomicOr(p, v); }
  __device__ __forceinline__ void axor64(uint64_t* p, uint64_t v) const {
    atomicXor((unsigned long long*)p, (unsigned long long)v);
  }
  __device__ __forceinline__ void count(unsigned long long* p, unsigned long long v) const {
    if (lane == 0 && v) atomicAdd(p, v);
  }
  __device__ __forceinline__ unsigned long long fetch_add(unsigned long long* p, unsigned long long v) const {
    unsigned long long r = 0;
    if (lane == 0) r = atomicAdd(p, v);
    const unsigned lo = __shfl((unsigned)(r & 0xffffffffull), 0, kWave);
    const unsigned hi = __shfl((unsigned)(r >> 32), 0, kWave);
    return ((unsigned long long)hi << 32) | lo;
  }
};

#define AGZ_SCRATCH_ARRAYS                                                    \
  __shared__ int8_t s_sb[kPPMax];                                             \
  __shared__ int32_t s_label[kPPMax + kWave];                                 \
  __shared__ int32_t s_minlib[kPPMax];                                        \
  __shared__ int32_t s_maxlib[kPPMax];                                        \
  __shared__ int8_t s_flag[kAPMax];                                           \
  __shared__ double s_dbuf[kAPMax];                                           \
  __shared__ int32_t s_path[kMaxdMax];
#define AGZ_SCRATCH(S)                                                        \
  AGZ_SCRATCH_ARRAYS                                                          \
  __shared__ uint64_t s_key[kAPMax + kSkChunk];                               \
  Scratch S{s_sb, s_label, s_minlib, s_maxlib, s_flag, s_dbuf, s_path, s_key};
// without the superko keys: for a kernel that the host launches only while View::sk_key is null
#define AGZ_SCRATCH_NO_KEYS(S)                                                \
  AGZ_SCRATCH_ARRAYS                                                          \
  Scratch S{s_sb, s_label, s_minlib, s_maxlib, s_flag, s_dbuf, s_path, nullptr};

// replay_position (board.jl:557-578) on the device: rebuild the 17 planes of positions of a game
// from its move list.  One wave walks one game: it replays moves[0 .. nm) from
// the empty board, Black first -- or, with start >= 0, from entry `start` of the start-position table (View::st_*:
// its board, its to_play and its history_len real older boards as the history planes) -- and writes the features of
// the position BEFORE move k for every k >= from to out + (k - from) * 17*P.  (record_features: one block, from 0;
// get_replay_batch, train.jl:4-12: one block per sampled (game, ply), nm = ply+1, from = ply.)
template <class W>
__device__ __forceinline__ void replay_emit(W& w, const View& V, Scratch& S, const int16_t* moves, int nm, int from,
                                            int8_t* hist, float* out, long start = -1) {
  const int P = V.P;
  // hist[0] = current board, hist[k] = k moves ago; avail = number of real older boards
  w.for_each(8 * V.PP, [&](int i) { hist[i] = 0; });
  w.sync();
  int tp = 1, avail = 0;
  if (start >= 0) {
    const agz_position_info f = V.st_info[start];
    tp = f.to_play;
    avail = f.history_len < 7 ? f.history_len : 7;
    w.for_each(P, [&](int p) { hist[p] = V.st_board[start * P + p]; });
    for (int h = 0; h < avail; ++h)
      w.for_each(P, [&](int p) { hist[(h + 1) * V.PP + p] = V.st_hist[(start * 7 + h) * P + p]; });
    w.sync();
  }
  for (int k = 0; k < nm; ++k) {
    if (k >= from) {
      w.for_each(P, [&](int p) {
        float* dst = out + (long)(k - from) * 17 * P;
        for (int s = 0; s < 8; ++s) {
          const int t = s <= avail ? s : avail;
          const int c = hist[t * V.PP + p];
          dst[(2 * s) * P + p] = c == tp ? 1.f : 0.f;
          dst[(2 * s + 1) * P + p] = c == -tp ? 1.f : 0.f;
        }
        dst[16 * P + p] = (float)tp;
      });
      w.sync();
    }
    if (k + 1 == nm) break;      // the last listed move is never needed
    // play move k on hist[0]
    const int a = moves[k];
    w.for_each(P, [&](int p) { S.sb[p] = hist[p]; });
    w.sync();
    int ncap = 0, nko = -1;
    if (a >= 0 && a < P) {
      label_components(w, V, S, true);
      group_liberties(w, V, S);
      apply_move_in_scratch(w, V, S, a, tp, &ncap, &nko);
    }
    for (int s = 7; s >= 1; --s) {
      w.for_each(P, [&](int p) { hist[s * V.PP + p] = hist[(s - 1) * V.PP + p]; });
      w.sync();
    }
    w.for_each(P, [&](int p) { hist[p] = S.sb[p]; });
    w.sync();
    tp = -tp;
    if (avail < 7) avail++;
  }
}

// the table entry a record's game began at, by the index rule of agz_selfplay_set_starts; -1: no table, the empty board
__host__ __device__ inline long record_start(const View& V, uint64_t game_id) {
  return V.st_count > 0 ? (long)((V.arena ? game_id >> 1 : game_id) % (uint64_t)V.st_count) : -1;
}

// ---- the packed record (agz_records_export_packed, agz_replay_*):
//      [agz_game_header 32 B | moves i16[n] | pad 4 | pis f32[n][A] | qs f32[n] | pad 8], records back to back.
// The one place that spells the layout: a view over a record's first byte and its move count (header().num_moves, given
// by the caller: on the host the record usually lies in device memory and its header cannot be read through the view).
template <class Byte>
struct PackedRecordT {
  template <class T>
  using as = std::conditional_t<std::is_const<Byte>::value, const T, T>;
  Byte* base;
  int nm;
  __host__ __device__ static size_t pi_offset(int nm) {
    return (sizeof(agz_game_header) + sizeof(int16_t) * (size_t)nm + 3) & ~(size_t)3;
  }
  __host__ __device__ static size_t bytes(int A, int nm) {
    return (pi_offset(nm) + sizeof(float) * (size_t)nm * A + sizeof(float) * (size_t)nm + 7) & ~(size_t)7;
  }
  __host__ __device__ as<agz_game_header>* header() const { return reinterpret_cast<as<agz_game_header>*>(base); }
  __host__ __device__ as<int16_t>* moves() const { return reinterpret_cast<as<int16_t>*>(base + sizeof(agz_game_header)); }
  __host__ __device__ as<float>* pi(int A, size_t ply = 0) const {       // the pi row of `ply`
    return reinterpret_cast<as<float>*>(base + pi_offset(nm)) + ply * A;
  }
  __host__ __device__ as<float>* qs(int A) const { return pi(A, (size_t)nm); }
  __host__ __device__ size_t unpadded(int A) const { return pi_offset(nm) + sizeof(float) * (size_t)nm * (A + 1); }
};
using PackedRecord = PackedRecordT<const uint8_t>;
using PackedRecordW = PackedRecordT<uint8_t>;

__host__ __device__ inline size_t packed_bytes(int A, int nm) { return PackedRecord::bytes(A, nm); }

// Row b of `out` = row b of `in` under T_sym[b] (inverse = 0) or T_sym[b]^-1 (inverse = 1): k_sym_rows of agz_engine.hip,
// which the symmetric forward and the arena's batches share, on `s`.  B rows of `planes` * N*N values and `tail` more
void launch_sym_rows(const float* in, float* out, const int32_t* sym, int B, int N, int planes, int tail, int inverse,
                     hipStream_t s);

}  // namespace agz

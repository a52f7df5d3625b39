// agz_replay.hip -- the device replay arena (agz_replay.h): its kernels (index, batch, targets, sampler, surprise
// weights and their scan) and the host class that keeps the packed records, their index (agz_replay_index.h) and the
// arrays laid out by the position prefix in step.  Compiled with -ffp-contract=off, as agz_engine.hip is: the value
// targets and the surprise scores are held to the bit against their headers' plain loops.
#include "agz_replay.h"

#include <algorithm>

#include "../../include/agz_surprise.h"
#include "../../include/agz_value_target.h"
#include "agz_wave.h"

namespace agz {

// one wave per source chunk (= one rank's part of the padded all-gather): walk its records and write where
// each one starts: out_off[first[c] + i] = byte offset of record i of chunk c inside `buf`.  nrec[c] >= 0 is
// the record count the sender announced (checked); nrec[c] = -(cap + 1) means "unknown, at most cap".
__global__ __launch_bounds__(kWave) void k_index_records(const uint8_t* buf, const int64_t* chunk_off,
                                                          const int64_t* chunk_bytes, const int64_t* nrec,
                                                          const int64_t* first, int A, int mgl, int64_t* out_off,
                                                          agz_game_header* out_hdr, int64_t* found, int32_t* bad) {
  if (threadIdx.x != 0) return;
  const int c = blockIdx.x;
  int64_t o = chunk_off[c];
  const int64_t end = o + chunk_bytes[c];
  const int64_t want = nrec[c], cap = want < 0 ? -(want + 1) : want;
  int64_t i = 0;
  bool ok = true;
  while (o < end) {
    if (i >= cap || o + (int64_t)sizeof(agz_game_header) > end) { ok = false; break; }
    const agz_game_header h = *PackedRecord{buf + o, 0}.header();
    if (h.num_moves < 0 || h.num_moves > mgl || o + (int64_t)PackedRecord::bytes(A, h.num_moves) > end) { ok = false; break; }
    out_off[first[c] + i] = o;
    out_hdr[first[c] + i] = h;
    o += (int64_t)PackedRecord::bytes(A, h.num_moves);
    ++i;
  }
  if (!ok || o != end || (want >= 0 && i != want)) atomicAdd(bad, 1);
  found[c] = i;
}

// get_replay_batch (train.jl:4-12) straight from the arena: sample b = (record at rec_off[b], ply[b]):
// features of the position before move ply (replay_position, board.jl:557-578), pi of that move, z = result
__global__ __launch_bounds__(kWave) void k_replay_arena_batch(View V, const uint8_t* arena, const int64_t* rec_off,
                                                               const int32_t* ply, int8_t* hist_all, float* feats,
                                                               float* pi_out, float* z_out) {
  AGZ_SCRATCH(S)
  HipWave w;
  const int b = blockIdx.x, A = V.A;
  const uint8_t* r = arena + rec_off[b];
  const agz_game_header h = *PackedRecord{r, 0}.header();
  const PackedRecord rec{r, h.num_moves};
  const float* pi = rec.pi(A, (size_t)ply[b]);
  replay_emit(w, V, S, rec.moves(), ply[b] + 1, ply[b], hist_all + (long)b * 8 * V.PP, feats + (long)b * 17 * V.P,
              record_start(V, h.game_id));
  if (pi_out) w.for_each(A, [&](int i) { pi_out[(long)b * A + i] = pi[i]; });
  if (z_out && w.leader()) z_out[b] = (float)h.result;
}

// agz_replay_set_value_target with alpha > 0: z of sample b = y_ply[b] of its record (include/agz_value_target.h), written
// over the result k_replay_arena_batch left there.  One lane per sample walks the record's qs from its last ply down to
// the sampled one: at most max_game_length dependent f64 steps.
__global__ __launch_bounds__(kWave) void k_replay_value_targets(const uint8_t* arena, const int64_t* rec_off,
                                                                 const int32_t* ply, int B, int A, double alpha,
                                                                 double lambda, float* z_out) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= B) return;
  const uint8_t* r = arena + rec_off[b];
  const agz_game_header h = *PackedRecord{r, 0}.header();
  const float* qs = PackedRecord{r, h.num_moves}.qs(A);
  z_out[b] = agz_value_target(qs, h.num_moves, ply[b], h.result, alpha, lambda);
}

// agz_replay_set_targets_only, the index: one wave per newly filed game scans its pi rows; a ply whose row is not all
// zero is a policy target (a fast search of agz_selfplay_set_playout_cap and an arena record leave zero rows).  The
// game's target plies go, in order, to tply[cum[g] ..] -- its share of an array laid out by the arena's position prefix,
// which has room for every ply -- and their number to count[g].
__global__ __launch_bounds__(kWave) void k_replay_targets(const uint8_t* arena, const int64_t* rec_off,
                                                           const int64_t* cum, int A, int16_t* tply, int32_t* count) {
  HipWave w;
  const int g = blockIdx.x;
  const uint8_t* r = arena + rec_off[g];
  const agz_game_header h = *PackedRecord{r, 0}.header();
  const float* pi = PackedRecord{r, h.num_moves}.pi(A);
  int16_t* out = tply + cum[g];
  int n = 0;
  for (int k = 0; k < h.num_moves; ++k) {
    bool nz = false;
    w.for_each(A, [&](int i) { nz = nz || pi[(size_t)k * A + i] != 0.f; });
    if (w.any(nz)) {
      if (w.leader()) out[n] = (int16_t)k;
      ++n;
    }
  }
  if (w.leader()) count[g] = n;
}

// the commit of a reanalysis run: one wave per result row = (game j, ply k) of the run, j found in the row
// prefix rv_off.  A row whose search finished in full (status AGZ_OK) writes qs[k] = Q, and its pi row over the record's
// unless that one is all zero -- "no policy target" (k_replay_targets) stays that, so the targets-only index, the window
// and the sampler's entry numbering hold.  Every other row leaves the record alone.  counts = {rows committed, pi rows
// overwritten, rows skipped}
__global__ __launch_bounds__(kWave) void k_replay_refresh(uint8_t* arena, const int64_t* rec_off, const int64_t* rv_off,
                                                           int64_t G, int A, const agz_analysis* res, const float* an_pi,
                                                           unsigned long long* counts) {
  HipWave w;
  const int64_t row = blockIdx.x;
  int64_t lo = 0, hi = G;                                         // rv_off[lo] <= row < rv_off[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (rv_off[mid] <= row) lo = mid; else hi = mid;
  }
  const agz_analysis a = res[row];
  if (a.status != AGZ_OK) {
    if (w.leader()) atomicAdd(&counts[2], 1ull);
    return;
  }
  const size_t k = (size_t)(row - rv_off[lo]);
  uint8_t* r = arena + rec_off[lo];
  const agz_game_header h = *PackedRecordW{r, 0}.header();
  const PackedRecordW rec{r, h.num_moves};
  float* pi = rec.pi(A, k);
  float* qs = rec.qs(A);
  bool nz = false;
  w.for_each(A, [&](int i) { nz = nz || pi[i] != 0.f; });
  const bool target = w.any(nz);
  if (target) w.for_each(A, [&](int i) { pi[i] = an_pi[row * A + i]; });
  if (w.leader()) {
    qs[k] = a.Q;
    atomicAdd(&counts[0], 1ull);
    if (target) atomicAdd(&counts[1], 1ull);
  }
}

// agz_replay_sample, the draw: B distinct entries of the window [0, L) by Floyd's algorithm -- for b = 0..B-1 with
// j = L - B + b: t_b = agz_index(agz_draw_u64(seed, call, 0, AGZ_SITE_REPLAY_SAMPLE, j), j + 1); sample b is t_b unless
// t_b is already taken by a sample before it, then j.  All t_b are drawn at once; "t_b is taken" is
//   dup(b)  -- some b' < b drew the same t (the first of them took it, or t was taken before that one), or
//   t_b = j' = L - B + b' for a b' < b that fell back to j' itself (b' collided),
// and b' < b: the second case is a chain through strictly smaller b that each thread follows on its own.  dup is the
// first-drawer test of an LDS hash table (atomicCAS on the key, atomicMin on the drawer).  Each entry e of the window is
// then mapped to (game, ply) by a binary search for the last k with cum[k] <= first + e over the arena's position prefix.
// Targets-only arena (tply != NULL): the entries are target plies, cum is the target prefix, and the entry's index
// inside its game is looked up in the game's target list tply[pcum[k] ..] (k_replay_targets) to give the ply.
constexpr int kSampleMax = 2048, kSampleHash = 4096, kSampleThreads = 1024;
__global__ __launch_bounds__(kSampleThreads) void k_replay_sample(uint64_t seed, uint64_t call, int B, int64_t L,
                                                                  int64_t first, const int64_t* cum, const int64_t* goff,
                                                                  const int64_t* pcum, const int16_t* tply,
                                                                  int64_t ngames, int sym_mode, int64_t* rec_off,
                                                                  int32_t* ply, int32_t* sym, int64_t* game_out,
                                                                  int32_t* ply_out) {
  __shared__ int32_t s_t[kSampleMax];
  __shared__ int32_t s_dup[kSampleMax];
  __shared__ int32_t s_key[kSampleHash];
  __shared__ int32_t s_min[kSampleHash];
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const int64_t j0 = L - B;
  for (int h = tid; h < kSampleHash; h += nt) { s_key[h] = -1; s_min[h] = 0x7fffffff; }
  __syncthreads();
  for (int b = tid; b < B; b += nt) {
    const uint64_t j = (uint64_t)(j0 + b);
    const int32_t t = (int32_t)agz_index(agz_draw_u64(seed, call, 0, AGZ_SITE_REPLAY_SAMPLE, j), (uint32_t)(j + 1));
    s_t[b] = t;
    uint32_t h = ((uint32_t)t * 0x9E3779B1u) >> (32 - 12);       // kSampleHash = 2^12 slots, at most half of them used
    for (;;) {
      const int32_t k = atomicCAS(&s_key[h], -1, t);
      if (k == -1 || k == t) break;
      h = (h + 1) & (kSampleHash - 1);
    }
    atomicMin(&s_min[h], b);
    s_dup[b] = (int32_t)h;                                       // the slot, until every drawer is in
  }
  __syncthreads();
  for (int b = tid; b < B; b += nt) s_dup[b] = s_min[s_dup[b]] < b;
  __syncthreads();
  for (int b = tid; b < B; b += nt) {
    bool taken = false;
    for (int x = b;;) {
      if (s_dup[x]) { taken = true; break; }
      const int64_t tx = s_t[x];
      if (tx >= j0 && tx - j0 < x) x = (int)(tx - j0); else break;
    }
    const int64_t a = first + (taken ? j0 + b : (int64_t)s_t[b]);
    int64_t lo = 0, hi = ngames;                                  // cum[lo] <= a < cum[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (cum[mid] <= a) lo = mid; else hi = mid;
    }
    int32_t p = (int32_t)(a - cum[lo]);
    if (tply) p = (int32_t)tply[pcum[lo] + p];
    rec_off[b] = goff[lo];
    ply[b] = p;
    if (sym)
      sym[b] = sym_mode == AGZ_SYMMETRY_RANDOM
                   ? (int32_t)agz_index(agz_draw_u64(seed, call, 0, AGZ_SITE_REPLAY_SYM, (uint64_t)b), 8u)
                   : sym_mode;
    if (game_out) game_out[b] = lo;
    if (ply_out) ply_out[b] = p;
  }
}

// ---- policy surprise weighting (agz_replay_score / agz_replay_set_surprise, include/agz_surprise.h)

// the scoring pass, behind the forward: one wave per row = (record at rec_off[b], ply[b]).  The row's pi is read from the
// arena, p is row b of the forward's output.  Each lane computes whole terms into LDS; lane 0 adds them in ascending a,
// the order the header's loop adds them in.  A row that is all zero is no target: score 0, flag 0.
constexpr int kSurpriseMaxA = 19 * 19 + 1;
__global__ __launch_bounds__(kWave) void k_replay_surprise(const uint8_t* arena, const int64_t* rec_off,
                                                            const int32_t* ply, const float* p_all, int A, double* kl,
                                                            uint8_t* tgt, unsigned long long* ntargets) {
  __shared__ double s_term[kSurpriseMaxA];
  HipWave w;
  const long b = blockIdx.x;
  const uint8_t* r = arena + rec_off[b];
  const agz_game_header h = *PackedRecord{r, 0}.header();
  const float* pi = PackedRecord{r, h.num_moves}.pi(A, (size_t)ply[b]);
  const float* p = p_all + b * A;
  bool nz = false;
  w.for_each(A, [&](int a) {
    const float x = pi[a];
    nz = nz || x != 0.f;
    s_term[a] = x > 0.f ? agz_surprise_term(x, p[a]) : 0.0;
  });
  const bool target = w.any(nz);
  w.sync();
  if (!w.leader()) return;
  double s = 0.0;
  if (target) {
    for (int a = 0; a < A; ++a)
      if (pi[a] > 0.f) s = s + s_term[a];
    s = s > 0.0 ? s : 0.0;
    atomicAdd(ntargets, 1ull);
  }
  kl[b] = s;
  tgt[b] = target ? 1 : 0;
}

// the weights: one wave per game g0 + blockIdx.x.  Every lane walks the game's plies in order for S and n (the same
// loads in every lane), then the lanes share the plies out for q.  A game that has not been scored, and a ply that is no
// target, weigh 1.  Two masks force q to 0: the plies in front of the window (first_game, first_ply -- counted in target
// plies when the arena is targets-only) and, targets-only (tply != NULL), the plies that are no targets; those are looked
// up in the game's ascending target list tply[cum[g] .. + tcum[g+1] - tcum[g]).  q goes to q_out[cum[g] - shift + ply].
__global__ __launch_bounds__(kWave) void k_replay_weights(const int64_t* cum, int64_t g0, const uint8_t* scored,
                                                           const double* kl, const uint8_t* tgt, double rho,
                                                           int64_t first_game, int64_t first_ply, const int64_t* tcum,
                                                           const int16_t* tply, uint32_t* q_out, int64_t shift) {
  HipWave w;
  const int64_t g = g0 + blockIdx.x;
  const int64_t base = cum[g];
  const int nm = (int)(cum[g + 1] - base);
  uint32_t* q = q_out + (base - shift);
  if (g < first_game) {
    w.for_each(nm, [&](int t) { q[t] = 0u; });
    return;
  }
  const bool sc = scored[g] != 0;
  double S = 0.0;
  int n = 0;
  if (sc)
    for (int t = 0; t < nm; ++t)
      if (tgt[base + t]) { S = S + kl[base + t]; ++n; }
  const int nt = tply ? (int)(tcum[g + 1] - tcum[g]) : 0;
  const int16_t* tl = tply ? tply + base : nullptr;
  const int64_t dead = g == first_game ? first_ply : 0;
  w.for_each(nm, [&](int t) {
    uint32_t v = AGZ_SURPRISE_UNIT;
    if (sc && tgt[base + t]) v = agz_surprise_q(kl[base + t], n, S, rho);
    if (tl) {
      int lo = 0, hi = nt;                                         // the first i with tl[i] >= t
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tl[mid] < t) lo = mid + 1; else hi = mid;
      }
      if (lo >= nt || tl[lo] != t || lo < dead) v = 0u;
    } else if (t < dead) {
      v = 0u;
    }
    q[t] = v;
  });
}

// the inclusive prefix of q (u32 -> u64) over n positions in three launches: k_scan_reduce (one sum per tile of kScanTile
// positions), k_scan_tiles (one workgroup turns the tile sums into their exclusive prefix) and k_scan_add (each tile scans
// its own positions and adds its offset).  No workgroup waits for another: the order is the order of the launches.
constexpr int kScanThreads = 256, kScanItems = 4, kScanTile = kScanThreads * kScanItems, kScanTop = 1024;

// the block-wide inclusive scan of one value per thread (Hillis-Steele in LDS); s has blockDim.x entries
__device__ __forceinline__ uint64_t block_scan_inclusive(uint64_t v, uint64_t* s) {
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  s[tid] = v;
  __syncthreads();
  for (int o = 1; o < nt; o <<= 1) {
    const uint64_t add = tid >= o ? s[tid - o] : 0ull;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  return s[tid];
}

__global__ __launch_bounds__(kScanThreads) void k_scan_reduce(const uint32_t* q, int64_t n, uint64_t* tile_sum) {
  __shared__ uint64_t s[kScanThreads];
  const int64_t at = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint64_t v = 0;
  for (int i = 0; i < kScanItems; ++i)
    if (at + i < n) v += q[at + i];
  const uint64_t incl = block_scan_inclusive(v, s);
  if (threadIdx.x == kScanThreads - 1) tile_sum[blockIdx.x] = incl;
}

__global__ __launch_bounds__(kScanTop) void k_scan_tiles(uint64_t* tile_sum, int64_t ntiles) {
  __shared__ uint64_t s[kScanTop];
  const int64_t per = (ntiles + kScanTop - 1) / kScanTop;          // consecutive tiles per thread
  const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < ntiles ? lo + per : ntiles;
  uint64_t v = 0;
  for (int64_t i = lo; i < hi; ++i) v += tile_sum[i];
  uint64_t run = block_scan_inclusive(v, s) - v;                  // the sum of every tile in front of `lo`
  for (int64_t i = lo; i < hi; ++i) {
    const uint64_t x = tile_sum[i];
    tile_sum[i] = run;
    run += x;
  }
}

__global__ __launch_bounds__(kScanThreads) void k_scan_add(const uint32_t* q, int64_t n, const uint64_t* tile_off,
                                                            uint64_t* out) {
  __shared__ uint64_t s[kScanThreads];
  const int64_t at = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint32_t x[kScanItems];
  uint64_t v = 0;
  for (int i = 0; i < kScanItems; ++i) {
    x[i] = at + i < n ? q[at + i] : 0u;
    v += x[i];
  }
  uint64_t run = tile_off[blockIdx.x] + (block_scan_inclusive(v, s) - v);
  for (int i = 0; i < kScanItems; ++i) {
    run += x[i];
    if (at + i < n) out[at + i] = run;
  }
}

// agz_replay_sample under rho > 0: one lane per sample.  Sample b is the position agz_weighted_pick finds for its draw in
// the prefix qcum of all npos arena positions (with replacement), mapped to (game, ply) by the binary search over the
// position prefix pcum that k_replay_sample makes.  Everything behind the draw is k_replay_sample's.
__global__ __launch_bounds__(kWave) void k_replay_sample_weighted(uint64_t seed, uint64_t call, int B,
                                                                   const uint64_t* qcum, int64_t npos,
                                                                   const int64_t* pcum, const int64_t* goff,
                                                                   int64_t ngames, int sym_mode, int64_t* rec_off,
                                                                   int32_t* ply, int32_t* sym, int64_t* game_out,
                                                                   int32_t* ply_out) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= B) return;
  const int64_t a = agz_weighted_pick(agz_draw_u64(seed, call, 0, AGZ_SITE_REPLAY_WEIGHTED, (uint64_t)b), qcum, npos);
  int64_t lo = 0, hi = ngames;                                    // pcum[lo] <= a < pcum[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (pcum[mid] <= a) lo = mid; else hi = mid;
  }
  const int32_t p = (int32_t)(a - pcum[lo]);
  rec_off[b] = goff[lo];
  ply[b] = p;
  if (sym)
    sym[b] = sym_mode == AGZ_SYMMETRY_RANDOM
                 ? (int32_t)agz_index(agz_draw_u64(seed, call, 0, AGZ_SITE_REPLAY_SYM, (uint64_t)b), 8u)
                 : sym_mode;
  if (game_out) game_out[b] = lo;
  if (ply_out) ply_out[b] = p;
}

// ------------------------------------------------------------------ the host class

void ReplayArena::reserve(size_t bytes) {
  if (bytes <= buf_.n) return;
  regrow(buf_, std::max<size_t>(bytes, std::max<size_t>(2 * buf_.n, (size_t)1 << 20)), 0, (size_t)ix_.used(), stream_);
}

// Append packed records lying in device memory as `chunks` (offset, bytes, expected record count or -1) of
// `dbuf` -- a padded all-gather receive buffer has one chunk per rank.  The variable-length records are
// indexed ON THE DEVICE (one wave walks one chunk); only the index (8 B + 32 B per game) visits the host.
int64_t ReplayArena::ingest_chunks(const uint8_t* dbuf, const std::vector<int64_t>& coff,
                                   const std::vector<int64_t>& cbytes, const std::vector<int64_t>& cnrec) {
  const int nc = (int)coff.size();
  int64_t total_rec = 0, total_bytes = 0;
  std::vector<int64_t> first((size_t)nc), nrec(cnrec);
  for (int c = 0; c < nc; ++c) {
    // an unknown count is bounded by the smallest record (a bare header)
    if (nrec[c] < 0) nrec[c] = -(cbytes[c] / (int64_t)sizeof(agz_game_header)) - 1;
    first[c] = total_rec;
    total_rec += nrec[c] < 0 ? -(nrec[c] + 1) : nrec[c];
    total_bytes += cbytes[c];
  }
  if (total_rec == 0 || total_bytes == 0) return 0;
  ix_.touch();
  // device scratch: [coff | cbytes | nrec | first] int64 x nc, then offsets, found counts, bad flag, headers
  DevBuf<int64_t> d_meta, d_off;
  DevBuf<agz_game_header> d_hdr;
  DevBuf<int32_t> d_flag;
  d_meta.alloc((size_t)5 * nc);
  d_off.alloc((size_t)total_rec);
  d_hdr.alloc((size_t)total_rec);
  d_flag.alloc(1);
  std::vector<int64_t> meta;
  meta.insert(meta.end(), coff.begin(), coff.end());
  meta.insert(meta.end(), cbytes.begin(), cbytes.end());
  meta.insert(meta.end(), nrec.begin(), nrec.end());
  meta.insert(meta.end(), first.begin(), first.end());
  meta.resize((size_t)5 * nc, 0);
  upload(d_meta.p, meta.data(), meta.size(), stream_);
  AGZ_HIP(hipMemsetAsync(d_flag.p, 0, sizeof(int32_t), stream_));
  hipLaunchKernelGGL(k_index_records, dim3(nc), dim3(kWave), 0, stream_, dbuf, (const int64_t*)d_meta.p,
                     (const int64_t*)(d_meta.p + nc), (const int64_t*)(d_meta.p + 2 * nc),
                     (const int64_t*)(d_meta.p + 3 * nc), V_.A, V_.max_game_length, d_off.p, d_hdr.p, d_meta.p + 4 * nc,
                     d_flag.p);
  AGZ_HIP(hipGetLastError());
  std::vector<int64_t> off((size_t)total_rec), found((size_t)nc);
  std::vector<agz_game_header> hdr((size_t)total_rec);
  int32_t bad = 0;
  download(off.data(), d_off.p, off.size(), stream_);
  download(hdr.data(), d_hdr.p, hdr.size(), stream_);
  download(found.data(), d_meta.p + 4 * nc, (size_t)nc, stream_);
  download(&bad, d_flag.p, 1, stream_);
  wait();
  AGZ_REQUIRE(bad == 0, AGZ_BAD_ARGUMENT, "packed records are malformed (a record runs past its chunk or a count does not match)");
  reserve((size_t)(ix_.used() + total_bytes));
  const size_t first_new = (size_t)ix_.count();
  int64_t added = 0;
  for (int c = 0; c < nc; ++c) {
    if (cbytes[c] == 0) continue;
    const int64_t at = ix_.used();          // the chunk's records fill it to the byte (k_index_records checked)
    AGZ_HIP(hipMemcpyAsync(buf_.p + at, dbuf + coff[c], (size_t)cbytes[c], hipMemcpyDeviceToDevice, stream_));
    for (int64_t i = 0; i < found[c]; ++i) {
      const agz_game_header& h = hdr[first[c] + i];
      ix_.append(h, at + off[first[c] + i] - coff[c], (int64_t)PackedRecord::bytes(V_.A, h.num_moves));
    }
    added += found[c];
  }
  if (ix_.targets_only() && added > 0) scan_targets(first_new);
  wait();
  return added;
}

void ReplayArena::header(int64_t k, agz_game_header* out) const {
  AGZ_REQUIRE(k >= 0 && k < ix_.count(), AGZ_BAD_ARGUMENT, "replay game %lld out of range", (long long)k);
  *out = ix_.hdr()[(size_t)k];
}

void ReplayArena::game(int64_t k, int16_t* moves, float* pis, float* qs) {
  agz_game_header h;
  header(k, &h);
  const size_t nm = (size_t)h.num_moves;
  if (nm == 0) return;
  const PackedRecord rec{buf_.p + ix_.off()[(size_t)k], h.num_moves};
  download(moves, rec.moves(), nm, stream_);
  download(pis, rec.pi(V_.A), nm * V_.A, stream_);
  download(qs, rec.qs(V_.A), nm, stream_);
  wait();
}

void ReplayArena::trim(int64_t max_positions) {
  AGZ_REQUIRE(max_positions >= 0, AGZ_BAD_ARGUMENT, "negative window");
  if (const size_t drop = ix_.trim(max_positions)) drop_front(drop);
}

// forget the oldest `drop` games (0 < drop < count): one copy of the rest into a fresh buffer, and of every array that
// lies by the position prefix
void ReplayArena::drop_front(size_t drop) {
  const size_t cut = (size_t)ix_.off()[drop], keep = (size_t)ix_.used() - cut;
  const size_t c0 = (size_t)ix_.cum()[drop], pos = (size_t)ix_.positions() - c0;
  regrow(buf_, std::max(keep, (size_t)1 << 20), cut, keep, stream_);
  if (ix_.targets_only())           // the target lists move up with the prefix
    regrow(d_tply_, std::max(pos, (size_t)1 << 16), c0, pos, stream_);
  if (d_sp_kl_.p) {                 // so do the surprise scores and their target flags, as far as they were ever written
    const size_t have = d_sp_kl_.n > c0 ? std::min(d_sp_kl_.n - c0, pos) : 0, cap = std::max(pos, (size_t)1 << 16);
    regrow(d_sp_kl_, cap, c0, have, stream_);
    regrow(d_sp_tgt_, cap, c0, have, stream_);
  }
  ix_.drop_front(drop);
}

void ReplayArena::set_window(int64_t max_entries) {
  const ReplayIndex::Dead dead = ix_.set_window(max_entries);
  if (dead.drop) drop_front((size_t)dead.games);
}

// The arena counts entries by target plies (agz_replay_set_targets_only).  Only while it is empty: the index of target
// plies is built as games are filed.
void ReplayArena::set_targets_only(bool on) {
  AGZ_REQUIRE(ix_.count() == 0, AGZ_BAD_ARGUMENT, "targets only: the replay arena holds %lld games; clear it first",
              (long long)ix_.count());
  ix_.set_targets_only(on);
}

// The value target of the batch calls (agz_replay_set_value_target).  A host-side pair read at the next batch call: the
// arena and its index do not depend on it, so it may change at any time, and agz_replay_clear leaves it alone.
void ReplayArena::set_value_target(double alpha, double lambda) {
  AGZ_REQUIRE(agz_value_target_params_ok(alpha, lambda), AGZ_BAD_ARGUMENT, "value target: alpha %g, lambda %g: both 0..1",
              alpha, lambda);
  vt_alpha_ = alpha;
  vt_lambda_ = lambda;
}

// games [first_new, count) have just been filed: k_replay_targets writes their target lists, the index extends the
// target prefix by their counts
void ReplayArena::scan_targets(size_t first_new) {
  const size_t m = (size_t)ix_.count() - first_new, npos = (size_t)ix_.positions();
  if (d_tply_.n < npos)
    regrow(d_tply_, std::max<size_t>(2 * npos, (size_t)1 << 16), 0, (size_t)ix_.cum()[first_new], stream_);
  tgt_idx_.ensure(2 * m);           // kept between calls: train() files one game at a time
  tgt_cnt_.ensure(m);
  upload(tgt_idx_.p, ix_.off().data() + first_new, m, stream_);
  upload(tgt_idx_.p + m, ix_.cum().data() + first_new, m, stream_);
  hipLaunchKernelGGL(k_replay_targets, dim3((unsigned)m), dim3(kWave), 0, stream_, (const uint8_t*)buf_.p,
                     (const int64_t*)tgt_idx_.p, (const int64_t*)(tgt_idx_.p + m), V_.A, d_tply_.p, tgt_cnt_.p);
  AGZ_HIP(hipGetLastError());
  std::vector<int32_t> cnt(m);
  download(cnt.data(), tgt_cnt_.p, m, stream_);
  wait();
  ix_.set_targets(first_new, cnt);
}

// get_replay_batch (train.jl:4-12) with the draw on the device: k_replay_sample picks B distinct live entries and maps
// them to (record offset, ply), emit turns them into the batch.  No host copy of the samples; only the arena's index is
// uploaded, and only what changed since the last call.
void ReplayArena::sample(int B, uint64_t call, int sym_mode, float* feats, float* pi, float* z, int64_t* game_out,
                         int32_t* ply_out) {
  const int64_t L = ix_.live();
  AGZ_REQUIRE(B >= 1 && B <= kSampleMax, AGZ_BAD_ARGUMENT, "batch %d: 1..%d samples", B, kSampleMax);
  const bool weighted = sp_rho_ > 0.0;      // agz_replay_set_surprise: drawn by weight, with replacement
  if (weighted)
    AGZ_REQUIRE(L >= 1, AGZ_BAD_ARGUMENT, "batch %d from an empty window", B);
  else
    AGZ_REQUIRE(B <= L, AGZ_BAD_ARGUMENT, "batch %d from a window of %lld entries (sampling without replacement)", B,
                (long long)L);
  AGZ_REQUIRE(L <= 0x7fffffffLL, AGZ_BAD_ARGUMENT, "window of %lld entries: at most 2^31 - 1", (long long)L);
  AGZ_REQUIRE(sym_mode >= AGZ_SYMMETRY_NONE && sym_mode <= AGZ_SYMMETRY_RANDOM, AGZ_BAD_ARGUMENT,
              "sym_mode %d: -1 (none), 0..7 (fixed T_s) or 8 (drawn)", sym_mode);
  AGZ_REQUIRE(feats, AGZ_BAD_ARGUMENT, "feats is NULL");
  const int64_t n = ix_.count();
  const bool tonly = ix_.targets_only();
  index_to_device();
  smp_off_.ensure(kSampleMax);
  smp_ply_.ensure(kSampleMax);
  smp_sym_.ensure(kSampleMax);
  boards_.ensure((size_t)B * 8 * V_.PP);
  const bool with_sym = sym_mode != AGZ_SYMMETRY_NONE;
  if (weighted) {
    weights_to_device();
    AGZ_REQUIRE(sp_total_ > 0, AGZ_BAD_ARGUMENT, "every live entry has weight 0 (rho = %g)", sp_rho_);
    hipLaunchKernelGGL(k_replay_sample_weighted, dim3((unsigned)((B + kWave - 1) / kWave)), dim3(kWave), 0, stream_,
                       (uint64_t)V_.seed, call, B, (const uint64_t*)d_sp_qcum_.p, ix_.positions(),
                       (const int64_t*)d_cum_.p, (const int64_t*)d_off_.p, n, sym_mode, smp_off_.p, smp_ply_.p,
                       with_sym ? smp_sym_.p : nullptr, game_out, ply_out);
  } else {
    hipLaunchKernelGGL(k_replay_sample, dim3(1), dim3(kSampleThreads), 0, stream_, (uint64_t)V_.seed, call, B, L,
                       ix_.window_start(), (const int64_t*)(tonly ? d_tcum_.p : d_cum_.p), (const int64_t*)d_off_.p,
                       (const int64_t*)d_cum_.p, (const int16_t*)(tonly ? d_tply_.p : nullptr), n, sym_mode, smp_off_.p,
                       smp_ply_.p, with_sym ? smp_sym_.p : nullptr, game_out, ply_out);
  }
  AGZ_HIP(hipGetLastError());
  emit(B, smp_off_.p, smp_ply_.p, with_sym ? smp_sym_.p : nullptr, boards_.p, feats, pi, z);
}

// ---- policy surprise weighting (include/agz_surprise.h)

// room in d_sp_kl_ / d_sp_tgt_ for every arena position; what has been written stays where it is
void ReplayArena::scores_reserve() {
  const size_t need = (size_t)ix_.positions();
  if (d_sp_kl_.n >= need && d_sp_kl_.p) return;
  const size_t cap = std::max<size_t>(2 * need, (size_t)1 << 16);
  regrow(d_sp_kl_, cap, 0, d_sp_kl_.n, stream_);
  regrow(d_sp_tgt_, cap, 0, d_sp_tgt_.n, stream_);
}

// the per-game scored flags on the device (a byte per game: all of them, every time)
void ReplayArena::scored_to_device() {
  const size_t n = (size_t)ix_.count();
  if (d_sp_scored_.n < n) d_sp_scored_.alloc(std::max<size_t>(2 * n, 1024));
  upload(d_sp_scored_.p, ix_.scored().data(), n, stream_);
  wait();
}

// agz_replay_score: the games' plies in chunks of at most fwd.cap rows -- k_replay_arena_batch for the features, the
// engine's forward (its buffers are not the ones the games in flight use), k_replay_surprise for one score per row.
// Everything runs on stream_, between steps.
int64_t ReplayArena::score(int64_t first, int64_t count, const ReplayForward& fwd) {
  const int64_t n = ix_.count();
  AGZ_REQUIRE(first >= 0 && count >= 0 && count <= n && first <= n - count, AGZ_BAD_ARGUMENT,
              "score: games %lld .. %lld + %lld: the replay arena holds %lld", (long long)first, (long long)first,
              (long long)count, (long long)n);
  if (count == 0) return 0;
  const int64_t pos0 = ix_.cum()[(size_t)first], rows = ix_.cum()[(size_t)(first + count)] - pos0;
  std::vector<int64_t> off((size_t)rows);
  std::vector<int32_t> ply((size_t)rows);
  for (int64_t k = first, r = 0; k < first + count; ++k)
    for (int32_t t = 0; t < ix_.hdr()[(size_t)k].num_moves; ++t, ++r) {
      off[(size_t)r] = ix_.off()[(size_t)k];
      ply[(size_t)r] = t;
    }
  scores_reserve();
  sp_count_.ensure(1);
  sp_count_.zero(stream_);
  unsigned long long targets = 0;
  if (rows > 0) {
    sp_off_.ensure((size_t)rows);
    sp_ply_.ensure((size_t)rows);
    upload(sp_off_.p, off.data(), (size_t)rows, stream_);
    upload(sp_ply_.p, ply.data(), (size_t)rows, stream_);
    boards_.ensure((size_t)fwd.cap * 8 * V_.PP);
    for (int64_t r0 = 0; r0 < rows; r0 += fwd.cap) {
      const int Bc = (int)std::min<int64_t>(fwd.cap, rows - r0);
      hipLaunchKernelGGL(k_replay_arena_batch, dim3(Bc), dim3(kWave), 0, stream_, V_, (const uint8_t*)buf_.p,
                         (const int64_t*)(sp_off_.p + r0), (const int32_t*)(sp_ply_.p + r0), boards_.p, fwd.whcn,
                         (float*)nullptr, (float*)nullptr);
      const float* p = fwd.run(Bc);
      hipLaunchKernelGGL(k_replay_surprise, dim3(Bc), dim3(kWave), 0, stream_, (const uint8_t*)buf_.p,
                         (const int64_t*)(sp_off_.p + r0), (const int32_t*)(sp_ply_.p + r0), p, V_.A,
                         d_sp_kl_.p + pos0 + r0, d_sp_tgt_.p + pos0 + r0, sp_count_.p);
      AGZ_HIP(hipGetLastError());
      wait();                           // Bc was uploaded from this frame (fwd.run)
      fwd.check();
    }
    download(&targets, sp_count_.p, 1, stream_);
    wait();
  }
  ix_.set_scored(first, count, true);
  ++sp_epoch_;
  return (int64_t)targets;
}

// rho of agz_replay_sample's draw.  A host-side value read at the next sample call: it may change at any time, and
// agz_replay_clear leaves it alone.
void ReplayArena::set_surprise(double rho) {
  AGZ_REQUIRE(agz_surprise_rho_ok(rho), AGZ_BAD_ARGUMENT, "surprise: rho %g: 0..1", rho);
  sp_rho_ = rho;
}

// game k's scores, its q under the rho in force (k_replay_weights on that game alone, without the sampler's masks) and
// its scored flag
void ReplayArena::surprise(int64_t k, double* kl_out, uint32_t* q_out, int32_t* scored_out) {
  AGZ_REQUIRE(k >= 0 && k < ix_.count(), AGZ_BAD_ARGUMENT, "replay game %lld out of range", (long long)k);
  const size_t nm = (size_t)ix_.hdr()[(size_t)k].num_moves;
  const bool sc = ix_.scored()[(size_t)k] != 0;
  const int64_t c0 = ix_.cum()[(size_t)k];
  if (scored_out) *scored_out = sc ? 1 : 0;
  if (nm == 0) return;
  if (kl_out) {
    if (sc) download(kl_out, d_sp_kl_.p + c0, nm, stream_);
    else std::fill(kl_out, kl_out + nm, 0.0);
  }
  if (q_out) {
    index_to_device();
    scored_to_device();
    d_sp_q_.ensure(std::max<size_t>((size_t)ix_.positions(), (size_t)1 << 16));     // (the sampler reads d_sp_qcum_ only)
    hipLaunchKernelGGL(k_replay_weights, dim3(1), dim3(kWave), 0, stream_, (const int64_t*)d_cum_.p, k,
                       (const uint8_t*)d_sp_scored_.p, (const double*)d_sp_kl_.p, (const uint8_t*)d_sp_tgt_.p, sp_rho_,
                       (int64_t)0, (int64_t)0, (const int64_t*)nullptr, (const int16_t*)nullptr, d_sp_q_.p, c0);
    AGZ_HIP(hipGetLastError());
    download(q_out, d_sp_q_.p, nm, stream_);
  }
  wait();
}

// the games' scores are of pi rows that have been replaced (a reanalysis commit): agz_replay_score scores them again
void ReplayArena::forget_scores(int64_t first, int64_t n) {
  ix_.set_scored(first, n, false);
  ++sp_epoch_;
}

// q of every arena position and its inclusive prefix on the device, if the arena, the scores or rho changed since they
// were built: k_replay_weights, then the scan in three launches; the total comes back for the sampler's check
void ReplayArena::weights_to_device() {
  if (sp_built_ && sp_built_change_ == ix_.change() && sp_built_epoch_ == sp_epoch_ && sp_built_rho_ == sp_rho_) return;
  const int64_t n = ix_.count(), npos = ix_.positions();
  const bool tonly = ix_.targets_only();
  index_to_device();
  scored_to_device();
  const int64_t ntiles = (npos + kScanTile - 1) / kScanTile;
  if (d_sp_q_.n < (size_t)npos) d_sp_q_.alloc(std::max<size_t>(2 * (size_t)npos, (size_t)1 << 16));
  if (d_sp_qcum_.n < (size_t)npos) d_sp_qcum_.alloc(std::max<size_t>(2 * (size_t)npos, (size_t)1 << 16));
  if (d_sp_tiles_.n < (size_t)ntiles) d_sp_tiles_.alloc(std::max<size_t>(2 * (size_t)ntiles, 1024));
  hipLaunchKernelGGL(k_replay_weights, dim3((unsigned)n), dim3(kWave), 0, stream_, (const int64_t*)d_cum_.p, (int64_t)0,
                     (const uint8_t*)d_sp_scored_.p, (const double*)d_sp_kl_.p, (const uint8_t*)d_sp_tgt_.p, sp_rho_,
                     ix_.first_game(), ix_.first_ply(), (const int64_t*)(tonly ? d_tcum_.p : nullptr),
                     (const int16_t*)(tonly ? d_tply_.p : nullptr), d_sp_q_.p, (int64_t)0);
  hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)ntiles), dim3(kScanThreads), 0, stream_, (const uint32_t*)d_sp_q_.p,
                     npos, d_sp_tiles_.p);
  hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(kScanTop), 0, stream_, d_sp_tiles_.p, ntiles);
  hipLaunchKernelGGL(k_scan_add, dim3((unsigned)ntiles), dim3(kScanThreads), 0, stream_, (const uint32_t*)d_sp_q_.p, npos,
                     (const uint64_t*)d_sp_tiles_.p, d_sp_qcum_.p);
  AGZ_HIP(hipGetLastError());
  sp_total_ = fetch(d_sp_qcum_.p + (npos - 1), stream_);
  sp_built_ = true;
  sp_built_change_ = ix_.change();
  sp_built_epoch_ = sp_epoch_;
  sp_built_rho_ = sp_rho_;
}

// the arena's index (off, cum and, targets-only, tcum) on the device: only what changed since the last call
void ReplayArena::index_to_device() {
  const size_t n = (size_t)ix_.count();
  const bool tonly = ix_.targets_only();
  if (d_cum_.n < n + 1 || d_off_.n < n || (tonly && d_tcum_.n < n + 1)) {
    const size_t cap = std::max<size_t>(2 * n + 1, 1024);
    d_cum_.alloc(cap);
    d_off_.alloc(cap);
    if (tonly) d_tcum_.alloc(cap);
    ix_.reset_upload();
  }
  const ReplayIndex::Slice s = ix_.pending();
  if (s.from < s.to) {
    upload(d_off_.p + s.from, ix_.off().data() + s.from, s.to - s.from, stream_);
    upload(d_cum_.p + s.from, ix_.cum().data() + s.from, s.to - s.from + 1, stream_);
    if (tonly) upload(d_tcum_.p + s.from, ix_.tcum().data() + s.from, s.to - s.from + 1, stream_);
    wait();      // the host vectors may move with the next ingest
    ix_.mark_uploaded();
  }
}

void ReplayArena::refresh(int64_t first, const int64_t* rv_off, int64_t G, int64_t rows, const agz_analysis* res,
                          const float* an_pi, unsigned long long* counts) {
  if (rows > 0)
    hipLaunchKernelGGL(k_replay_refresh, dim3((unsigned)rows), dim3(kWave), 0, stream_, buf_.p, offsets_device(first),
                       rv_off, G, V_.A, res, an_pi, counts);
  AGZ_HIP(hipGetLastError());
}

// B samples given on the device as (record offset, ply) -> feats [B][17 P], pi [B][A] (or NULL) and z [B] (or NULL) in
// device memory; `boards` is replay scratch of B * 8 * PP.  With `sym` (device, [B]) the samples are written as they are
// into symf_ / symp_ and sample b goes under T_sym[b] into the outputs.  The sampler and agz_replay_batch share that
// pair: both enqueue on stream_ only, so the later call's kernels start after the earlier call's have read it, and a
// regrow goes through hipFree, which waits for the device.  Nothing here waits: agz_replay_sample stays asynchronous.
void ReplayArena::emit(int B, const int64_t* off, const int32_t* ply, const int32_t* sym, int8_t* boards, float* feats,
                       float* pi, float* z) {
  float *f = feats, *p = pi;
  if (sym) {
    symf_.ensure((size_t)B * 17 * V_.P);
    symp_.ensure((size_t)B * V_.A);
    f = symf_.p;
    p = pi ? symp_.p : nullptr;
  }
  hipLaunchKernelGGL(k_replay_arena_batch, dim3(B), dim3(kWave), 0, stream_, V_, (const uint8_t*)buf_.p, off, ply, boards,
                     f, p, z);
  if (sym) {
    launch_sym_rows(f, feats, sym, B, V_.N, 17, 0, 0, stream_);
    if (pi) launch_sym_rows(p, pi, sym, B, V_.N, 1, 1, 0, stream_);
  }
  if (z && vt_alpha_ > 0.0)         // agz_replay_set_value_target: z becomes y (a symmetry does not touch it)
    hipLaunchKernelGGL(k_replay_value_targets, dim3((unsigned)((B + kWave - 1) / kWave)), dim3(kWave), 0, stream_,
                       (const uint8_t*)buf_.p, off, ply, B, V_.A, vt_alpha_, vt_lambda_, z);
  AGZ_HIP(hipGetLastError());
}

}  // namespace agz

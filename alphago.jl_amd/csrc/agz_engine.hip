// agz_engine.hip -- the HIP instantiation of the search templates (one 64-lane wavefront per
// game tree) and the host engine that strings a self-play step together:
//
//   k_pre            lifecycle + per-move phase + select up to 8 leaves     (1 wave / game)
//   k_scan           prefix sum of the leaf counts -> rows of the NN batch
//   k_leaf_features  17 board planes of every leaf -> stem input            (1 wave / leaf)
//   Net::forward     stem + tower (MFMA implicit GEMM) + heads              (agz_nn.hip)
//   k_post           revert virtual loss, expand, back up                   (1 wave / game)
//
// Everything is enqueued on one stream with the batch size left in device memory, so a step
// needs no host synchronisation.  Compiled with -ffp-contract=off: the PUCT arithmetic mixes
// Float32 and Float64 exactly as the reference does.
#include "agz_engine.h"

#include <algorithm>
#include <cstring>
#include <tuple>

#include "../../include/agz_value_target.h"
#include "agz_wave.h"

namespace agz {

__global__ __launch_bounds__(kWave) void k_pre(View V) {
  AGZ_SCRATCH(S)
  HipWave w;
  game_pre(w, V, S, (int)blockIdx.x);
}

// the board updates of the leaves k_pre created (node_create_child, defer): one wave per leaf
__device__ __forceinline__ void expand_block(const View& V, Scratch& S) {
  HipWave w;
  const int half = kMaxPend / 2;                 // a game rarely creates more than parallel_readouts leaves per step
  const int g = (int)blockIdx.x / half, i = (int)blockIdx.x % half;
  game_expand(w, V, S, g, i);
  game_expand(w, V, S, g, i + half);
}
// k_expand holds no key scratch, so with no superko rule its LDS and occupancy are what they were (7 waves per SIMD);
// under a rule (View::sk_key set) the host launches k_expand_keys
__global__ __launch_bounds__(kWave) void k_expand(View V) {
  AGZ_SCRATCH_NO_KEYS(S)
  expand_block(V, S);
}
__global__ __launch_bounds__(kWave) void k_expand_keys(View V) {
  AGZ_SCRATCH(S)
  expand_block(V, S);
}

// (as k_expand: no key scratch while no superko rule is set -- LDS and occupancy as they were -- else k_post_keys)
__global__ __launch_bounds__(kWave) void k_post(View V) {
  AGZ_SCRATCH_NO_KEYS(S)
  HipWave w;
  game_post(w, V, S, (int)blockIdx.x);
}
__global__ __launch_bounds__(kWave) void k_post_keys(View V) {
  AGZ_SCRATCH(S)
  HipWave w;
  game_post(w, V, S, (int)blockIdx.x);
}

// exclusive prefix sum of GameState::nleaves over the games -> leaf_base, total -> batch_count
// arena: two batches, one per network.  Black players' leaves (even slots) get rows [0, n0), White
// players' leaves rows [half, half + n1) with half = games*par/2: each network sees a contiguous
// batch at a FIXED base, so no row offset has to come back to the host.
__global__ __launch_bounds__(256) void k_scan_arena(View V) {
  __shared__ int part[256];
  const int t = threadIdx.x, npairs = V.games / 2;
  const int chunk = (npairs + 255) / 256;
  const int lo = t * chunk, hi = min(npairs, lo + chunk);
  for (int c = 0; c < 2; ++c) {
    int s = 0;
    for (int p = lo; p < hi; ++p) s += V.gs[2 * p + c].nleaves;
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int v = t >= o ? part[t - o] : 0;
      __syncthreads();
      part[t] += v;
      __syncthreads();
    }
    int base = part[t] - s + c * (npairs * V.par);
    for (int p = lo; p < hi; ++p) {
      V.gs[2 * p + c].leaf_base = base;
      base += V.gs[2 * p + c].nleaves;
    }
    if (t == 255) V.batch_count[c] = part[255];
    __syncthreads();
  }
  if (t == 255) atomicAdd(&V.counters[CT_STEPS], 1ull);
}

__global__ __launch_bounds__(256) void k_scan(View V) {
  __shared__ int part[256];
  const int t = threadIdx.x, G = V.games;
  const int chunk = (G + 255) / 256;
  const int lo = t * chunk, hi = min(G, lo + chunk);
  int s = 0;
  for (int g = lo; g < hi; ++g) s += V.gs[g].nleaves;
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int base = part[t] - s;
  for (int g = lo; g < hi; ++g) {
    V.gs[g].leaf_base = base;
    base += V.gs[g].nleaves;
  }
  if (t == 255) {
    *V.batch_count = part[255];
    atomicAdd(&V.counters[CT_STEPS], 1ull);
  }
}

// One workgroup of four waves per leaf slot, each wave a quarter of the leaf's (point, quad) items.  (Neither this, nor
// one wave per leaf, nor four leaves per workgroup changes its 35-39 us per 8192 leaves of 9x9: see leaf_features.)
constexpr int kWavesPerLeaf = 4;
__global__ __launch_bounds__(kWavesPerLeaf * kWave) void k_leaf_features(View V, int g0, int slots, float* x32, float* whcn) {
  const int slot = (int)blockIdx.x;
  if (slot >= slots) return;
  const int g = g0 + slot / V.par, k = slot % V.par;
  if (k >= V.gs[g].nleaves) return;
  HipWave w((int)(threadIdx.x & (kWave - 1)));
  const long row = (long)V.gs[g].leaf_base + k;
  leaf_features(w, V, g, k, x32 ? x32 + row * V.P * 32 : nullptr, whcn ? whcn + row * 17 * V.P : nullptr, (int)(threadIdx.x >> 6),
                kWavesPerLeaf);
}

// The same under the board symmetry each leaf was recorded with (View::leaf_sym): launched instead of k_leaf_features
// while agz_selfplay_set_symmetry is on, so that k_leaf_features itself stays what it is
__global__ __launch_bounds__(kWavesPerLeaf * kWave) void k_leaf_features_sym(View V, int g0, int slots, float* x32, float* whcn) {
  const int slot = (int)blockIdx.x;
  if (slot >= slots) return;
  const int g = g0 + slot / V.par, k = slot % V.par;
  if (k >= V.gs[g].nleaves) return;
  HipWave w((int)(threadIdx.x & (kWave - 1)));
  const long row = (long)V.gs[g].leaf_base + k;
  leaf_features<true>(w, V, g, k, x32 ? x32 + row * V.P * 32 : nullptr, whcn ? whcn + row * 17 * V.P : nullptr,
                      (int)(threadIdx.x >> 6), kWavesPerLeaf);
}

// The network's policy of a leaf evaluated under T_s back to board orientation, in place: pi[p] = pi_net[T_s(p)], pass
// unchanged (the value needs nothing).  One wave per leaf slot, the same slots / rows as k_leaf_features_sym.
__global__ __launch_bounds__(kWave) void k_pi_unpermute(View V, int g0, int slots, float* pi) {
  __shared__ float row[kAPMax];
  const int slot = (int)blockIdx.x;
  if (slot >= slots) return;
  const int g = g0 + slot / V.par, k = slot % V.par;
  if (k >= V.gs[g].nleaves) return;
  const int s = V.leaf_sym[(long)g * V.par + k];
  float* r = pi + ((long)V.gs[g].leaf_base + k) * V.A;
  for (int a = (int)threadIdx.x; a < V.A; a += kWave) row[a] = r[a];
  __syncthreads();
  for (int a = (int)threadIdx.x; a < V.A; a += kWave) r[a] = row[sym_point(s, V.N, a)];
}

// Row b of `out` = row b of `in` under T_sym[b] (inverse = 0) or T_sym[b]^-1 (inverse = 1).  A row is `planes` blocks of
// N*N point values (feature planes in agz_features order, or the board part of a policy row) followed by `tail` values
// that are copied as they are (the pass entry).  Forward: out[plane][T_s(p)] = in[plane][p], written as a gather so the
// stores are consecutive.  Un-permuting a policy the network produced under T_s is the inverse: out[p] = in[T_s(p)].
__global__ __launch_bounds__(256) void k_sym_rows(const float* in, float* out, const int32_t* sym, int N, int planes,
                                                  int tail, int inverse) {
  const int b = (int)blockIdx.x, P = N * N;
  const int body = planes * P, len = body + tail;
  const int s = sym[b];
  const int from = inverse ? s : sym_inverse(s);    // out[q] = in[T_from(q)]
  const float* src = in + (long)b * len;
  float* dst = out + (long)b * len;
  for (int i = (int)threadIdx.x; i < len; i += (int)blockDim.x) {
    int j = i;
    if (i < body) {
      const int plane = i / P;
      j = plane * P + sym_point(from, N, i - plane * P);
    }
    dst[i] = src[j];
  }
}
void launch_sym_rows(const float* in, float* out, const int32_t* sym, int B, int N, int planes, int tail, int inverse,
                     hipStream_t s) {
  hipLaunchKernelGGL(k_sym_rows, dim3(B), dim3(256), 0, s, in, out, sym, N, planes, tail, inverse);
}

// The Vector{Position} a caller-supplied network receives (mcts_play.jl:89): per collected leaf of slot g, its own
// board and the up-to-7 older boards behind the history planes (the same sources k_leaf_features reads), its NodeMeta
// and the move before its last one -- gathered into contiguous rows for ONE copy to the host.
struct LeafPosRow {
  NodeMeta m;
  int32_t node, plen, prev_move, pad;
};
__global__ __launch_bounds__(kWave) void k_leaf_positions(View V, int g, int8_t* boards8, LeafPosRow* rows) {
  const int k = blockIdx.x;
  if (k >= V.gs[g].nleaves) return;
  const long li = (long)g * V.par + k;
  const int P = V.P;
  for (int s = 0; s < 8; ++s) {
    const int src = V.leaf_featsrc[li * 8 + s];
    const int8_t* b = src >= 0 ? V.board + node_index(V, g, src) * V.PP : V.hist + ((long)g * 7 + (-src - 1)) * V.PP;
    for (int p = threadIdx.x; p < P; p += kWave) boards8[((long)k * 8 + s) * P + p] = b[p];
  }
  if (threadIdx.x == 0) {
    LeafPosRow r;
    r.node = V.leaf_node[li];
    r.plen = V.leaf_plen[li];
    r.m = V.meta[node_index(V, g, r.node)];
    r.prev_move = r.m.parent >= 0 ? V.meta[node_index(V, g, r.m.parent)].last_move : -1;
    r.pad = 0;
    rows[k] = r;
  }
}

__global__ __launch_bounds__(kWave) void k_tree_op(View V, TreeArgs T) {
  AGZ_SCRATCH(S)
  HipWave w;
  tree_op(w, V, S, T);
}

// agz_tree_lines: node_lines for one node of single tree g (a kernel of its own: TreeArgs keeps its layout and
// k_tree_op its registers)
__global__ __launch_bounds__(kWave) void k_tree_lines(View V, int g, int node, int K, int D, int min_visits, agz_line* out,
                                                       int16_t* pv, float* pv_N) {
  AGZ_SCRATCH(S)
  HipWave w;
  node_lines(w, V, S, g, node, K, D, min_visits, out, pv, pv_N);
}

// agz_tree_pruned_pi: pruned_pi of one node of single tree g under forced_k = k, whatever the engine's setting; the
// squash is the node's own n <= tau, the scale that of the node's own N
__global__ __launch_bounds__(kWave) void k_tree_pruned_pi(View V, int g, int node, double k, float* out) {
  AGZ_SCRATCH(S)
  HipWave w;
  V.forced_k = k;
  const long ni = node_index(V, g, node);
  pruned_pi(w, V, S, ni, *slotN(V, g, node), V.meta[ni].n <= V.tau, out);
}

// agz_tree_gumbel_pi: gumbel_pi of one node of single tree g under the constants given, whatever the engine's setting
__global__ __launch_bounds__(kWave) void k_tree_gumbel_pi(View V, int g, int node, double c_visit, double c_scale,
                                                           float* out) {
  AGZ_SCRATCH(S)
  HipWave w;
  V.gumbel_cvisit = c_visit;
  V.gumbel_cscale = c_scale;
  gumbel_pi(w, V, S, node_index(V, g, node), out);
}

// agz_tree_explore_rows: root_explore of one node of single tree g on a copy of its prior row, under the engine's
// setting; row [AP] receives the noised row, tempered [A] and alpha [A] what lies between.  The tree is not written.
__global__ __launch_bounds__(kWave) void k_tree_explore_rows(View V, int g, int node, float* row, float* tempered,
                                                              double* alpha) {
  AGZ_SCRATCH(S)
  HipWave w;
  const long ni = node_index(V, g, node);
  w.for_each(V.AP, [&](int a) { row[a] = V.childP[ni * V.AP + a]; });
  w.sync();
  root_explore(w, V, S, g, node, row, tempered, alpha);
}

// agz_tree_child_lcb: child_lcb_rows of one node of single tree g under z, whatever the engine's setting of the rule;
// out [3][A]: mean, sd, lcb
__global__ __launch_bounds__(kWave) void k_tree_child_lcb(View V, int g, int node, double z, double* out) {
  HipWave w;
  child_lcb_rows(w, V, g, node, z, out, out + V.A, out + 2 * V.A);
}

__global__ __launch_bounds__(kWave) void k_go_play(View V, const int8_t* boards, const int8_t* tp, const int32_t* ko,
                                                    const int32_t* moves, int B, int8_t* bo, int32_t* ko_o,
                                                    int32_t* nc, int32_t* st) {
  AGZ_SCRATCH(S)
  HipWave w;
  const int b = blockIdx.x;
  if (b >= B) return;
  go_play_one(w, V, S, boards + (long)b * V.P, tp[b], ko[b], moves[b], bo + (long)b * V.P, ko_o + b, nc + b, st + b);
}

__global__ __launch_bounds__(kWave) void k_go_legal(View V, const int8_t* boards, const int8_t* tp,
                                                     const int32_t* ko, int B, int8_t* out) {
  AGZ_SCRATCH(S)
  HipWave w;
  const int b = blockIdx.x;
  if (b >= B) return;
  go_legal_one(w, V, S, boards + (long)b * V.P, tp[b], ko[b], out + (long)b * V.A);
}

__global__ __launch_bounds__(kWave) void k_go_keys(View V, const int8_t* boards, const int8_t* tp, int B, int rule,
                                                   uint64_t* out) {
  HipWave w;
  const int b = blockIdx.x;
  if (b >= B) return;
  go_key_one(w, V, boards + (long)b * V.P, tp[b], rule, out + b);
}

__global__ __launch_bounds__(kWave) void k_go_legal_seen(View V, const int8_t* boards, const int8_t* tp, const int32_t* ko,
                                                         const uint64_t* seen, const int64_t* off, int B, int rule,
                                                         int8_t* out) {
  AGZ_SCRATCH(S)
  HipWave w;
  const int b = blockIdx.x;
  if (b >= B) return;
  go_legal_seen_one(w, V, S, boards + (long)b * V.P, tp[b], ko[b], seen + off[b], (int)(off[b + 1] - off[b]), rule,
                    out + (long)b * V.A);
}

__global__ __launch_bounds__(kWave) void k_go_score(View V, const int8_t* boards, const float* komi, int B, float* out) {
  AGZ_SCRATCH(S)
  HipWave w;
  const int b = blockIdx.x;
  if (b >= B) return;
  go_score_one(w, V, S, boards + (long)b * V.P, komi[b], out + b);
}

// replay_emit (agz_wave.h) on caller-given move lists: block b replays moves[off[b] .. off[b] + nms[b]) and writes the
// features of the positions from emit_from[b] on to out_all + out_off[b]
__global__ __launch_bounds__(kWave) void k_replay_features(View V, const int16_t* moves, const int32_t* off,
                                                            const int32_t* nms, const int32_t* emit_from,
                                                            const int64_t* out_off,
                                                            int8_t* hist_all /*[blocks][8][PP] scratch in HBM*/,
                                                            float* out_all, const int32_t* start /*[blocks] or NULL*/) {
  AGZ_SCRATCH(S)
  HipWave w;
  const int b = blockIdx.x;
  replay_emit(w, V, S, moves + off[b], nms[b], emit_from[b], hist_all + (long)b * 8 * V.PP, out_all + out_off[b],
              start ? (long)start[b] : -1);
}

// agz_selfplay_set_starts: one wave per candidate entry, ok[s] = its board passes root_board_valid
__global__ __launch_bounds__(kWave) void k_starts_valid(View V, const int8_t* boards, const agz_position_info* info,
                                                         int32_t* ok) {
  AGZ_SCRATCH(S)
  HipWave w;
  const long s = blockIdx.x;
  const bool good = root_board_valid(w, V, S, boards + s * V.P, info[s].ko);
  if (w.leader()) ok[s] = good;
}

// one workgroup per finished record k: copy it from the engine's record ring into dst + off[k], packed (PackedRecord)
__global__ __launch_bounds__(256) void k_pack_records(View V, const int64_t* off, uint8_t* dst, long first) {
  const long k = first + blockIdx.x;
  const agz_game_header h = V.fin_hdr[k];
  const int nm = h.num_moves, mgl = V.max_game_length, A = V.A;
  uint8_t* r = dst + off[blockIdx.x];
  const PackedRecordW rec{r, nm};
  if (threadIdx.x == 0) *rec.header() = h;
  int16_t* mv = rec.moves();
  float* pi = rec.pi(A);
  float* q = rec.qs(A);
  for (int i = threadIdx.x; i < nm; i += 256) {
    mv[i] = V.fin_moves[k * mgl + i];
    q[i] = V.fin_q[k * mgl + i];
  }
  if ((nm & 1) && threadIdx.x == 0) mv[nm] = 0;                       // the 2 pad bytes in front of pis
  for (long i = threadIdx.x; i < (long)nm * A; i += 256) pi[i] = V.fin_pi[k * (long)mgl * A + i];
  const size_t end = rec.unpadded(A);
  if ((end & 7) && threadIdx.x == 0) *reinterpret_cast<uint32_t*>(r + end) = 0u;   // pad to 8
}

// ---- reanalysis (agz_replay_reanalyze_start / _commit): a review run whose games are arena records

// the gather in front of the search: one wave per game j = arena game first + j (rec_off is the arena's offset table from
// `first` on).  Its moves go record to review table in coalesced int16 copies, its start is the table entry every
// kernel that rebuilds a record begins at (record_start; none: the empty board with agz_config.komi), and its draw-stream
// game id is id_base + header.game_id
__global__ __launch_bounds__(kWave) void k_reanalyze_gather(View V, const uint8_t* arena, const int64_t* rec_off,
                                                             const int64_t* rv_off, uint64_t id_base, int16_t* rv_moves,
                                                             int8_t* an_board, int8_t* an_hist,
                                                             agz_position_info* an_info, uint64_t* an_gid) {
  HipWave w;
  const long j = blockIdx.x;
  const int P = V.P;
  const uint8_t* r = arena + rec_off[j];
  const agz_game_header h = *PackedRecord{r, 0}.header();
  const int16_t* mv = PackedRecord{r, h.num_moves}.moves();
  int16_t* out = rv_moves + rv_off[j];
  w.for_each(h.num_moves, [&](int i) { out[i] = mv[i]; });
  const long s = record_start(V, h.game_id);
  w.for_each(P, [&](int p) { an_board[j * P + p] = s >= 0 ? V.st_board[s * P + p] : (int8_t)0; });
  w.for_each(7 * P, [&](int i) { an_hist[j * 7 * P + i] = s >= 0 ? V.st_hist[s * 7 * P + i] : (int8_t)0; });
  if (w.leader()) {
    an_info[j] = s >= 0 ? V.st_info[s] : empty_position_info(V.komi);
    an_gid[j] = id_base + h.game_id;
  }
}

// agz_selfplay_release: every slot parked in G_IDLE may claim its next game at the next k_pre
__global__ void k_release(View V) {
  const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (g < V.games && V.gs[g].phase == G_IDLE) V.released[g] = 1;
}

__global__ void k_debug_draws(uint64_t seed, uint64_t game, uint32_t move, int n, double alpha, double* out) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a < n) out[a] = agz_dirichlet_gamma(seed, game, move, (uint32_t)a, alpha);
}

__global__ void k_debug_math(View V, int op, const double* x, const double* y, int n, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r = 0.0;
  switch (op) {
    case 0: r = agz_log(x[i]); break;
    case 1: r = agz_exp(x[i]); break;
    case 2: r = agz_pow(x[i], 0.98); break;
    case 3: r = (double)sqrtf((float)x[i]); break;
    case 4: r = (double)((float)x[i] / (float)y[i]); break;
    case 5: {
      const float denom = 1.0f + (float)y[i];
      const float q = (float)x[i] / denom;
      const float qs = q * -1.0f;
      const double scale = puct_scale(V, (float)y[i] + 7.0f);
      r = (double)qs + (scale * (double)0.25f) / (double)denom;
    } break;
  }
  out[i] = r;
}

// ------------------------------------------------------------------ host engine

static void validate(const agz_config& c) {
  AGZ_REQUIRE(c.board_size >= 2 && c.board_size <= 19, AGZ_BAD_ARGUMENT, "board_size %d not in 2..19", c.board_size);
  AGZ_REQUIRE(c.tower_height >= 0 && c.tower_height <= 64, AGZ_BAD_ARGUMENT, "tower_height %d", c.tower_height);
  AGZ_REQUIRE(c.games >= 1, AGZ_BAD_ARGUMENT, "games must be >= 1");
  AGZ_REQUIRE(c.num_readouts >= 1, AGZ_BAD_ARGUMENT, "num_readouts must be >= 1");
  AGZ_REQUIRE(c.parallel_readouts >= 1 && c.parallel_readouts <= kMaxPar, AGZ_BAD_ARGUMENT,
              "parallel_readouts %d not in 1..%d", c.parallel_readouts, kMaxPar);
  AGZ_REQUIRE(!c.arena_mode || c.games % 2 == 0, AGZ_BAD_ARGUMENT, "arena_mode needs an even number of slots");
  // the word that is pool_policy now was `stagger_moves` until round 2 (agz_debug_set_stagger since) and a must-be-zero
  // reserved1 until round 4: an old-ABI caller that still puts a move count there must hear about it
  AGZ_REQUIRE(c.reserved0 == 0.f, AGZ_BAD_ARGUMENT, "agz_config.reserved0 must be 0");
  AGZ_REQUIRE(c.pool_policy == AGZ_POOL_MOVE_EARLY || c.pool_policy == AGZ_POOL_STALL, AGZ_BAD_ARGUMENT,
              "agz_config.pool_policy %d: AGZ_POOL_MOVE_EARLY (0) or AGZ_POOL_STALL (1); this word was stagger_moves / "
              "reserved1 in earlier headers (use agz_debug_set_stagger)", c.pool_policy);
  AGZ_REQUIRE(c.max_nodes_per_game >= 0, AGZ_BAD_ARGUMENT, "max_nodes_per_game %d", c.max_nodes_per_game);
}

Engine::Engine(const agz_config& cfg) : cfg_(cfg) {
  validate(cfg);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  AGZ_REQUIRE(e == hipSuccess && ndev > 0, AGZ_HIP_ERROR,
              "no HIP device available (%s): libagz has no CPU fallback", hipGetErrorString(e));
  AGZ_REQUIRE(cfg.device >= 0 && cfg.device < ndev, AGZ_BAD_ARGUMENT, "device %d of %d", cfg.device, ndev);
  AGZ_HIP(hipSetDevice(cfg.device));
  hipDeviceProp_t prop;
  AGZ_HIP(hipGetDeviceProperties(&prop, cfg.device));
  AGZ_REQUIRE(std::string(prop.gcnArchName).rfind("gfx950", 0) == 0, AGZ_HIP_ERROR,
              "device %d is %s; libagz is built for gfx950 (MI355X) only", cfg.device, prop.gcnArchName);
  AGZ_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  replay_.reset(new ReplayArena(stream_, V_));
  fill_dims(V_, cfg);
  V_.defer_expand = 1;      // k_expand follows every k_pre (step, select_external)
  AGZ_REQUIRE(V_.PP <= kPPMax && V_.AP <= kAPMax && V_.maxd <= kMaxdMax, AGZ_BAD_ARGUMENT, "board too large");
  for_each_buffer(V_, [&](auto*& p, size_t n) {
    using T = std::remove_reference_t<decltype(*p)>;
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    void* q = nullptr;
    AGZ_HIP(hipMalloc(&q, bytes));
    AGZ_HIP(hipMemsetAsync(q, 0, bytes, stream_));
    p = (T*)q;
    bufs_.push_back(q);
    state_bytes_ += bytes;
  });
  bcap_ = V_.games * V_.par;
  d_x32_.alloc((size_t)bcap_ * V_.P * 32);
  d_pi_.alloc((size_t)bcap_ * V_.A);
  d_v_.alloc((size_t)bcap_);
  V_.pi = d_pi_.p;
  V_.v = d_v_.p;
  s_iout_.alloc(4);
  net_.reset(new Net(V_.N, cfg.tower_height, stream_));
  if (cfg.arena_mode) net2_.reset(new Net(V_.N, cfg.tower_height, stream_));
  set_all_slots(G_RETIRED);      // every slot idle-retired until start()
}

Engine::~Engine() {
  (void)hipStreamSynchronize(stream_);
  for (auto e : sprof_ev_) (void)hipEventDestroy(e);
  // the trainers point into their networks (host-sync callback) and own device buffers: they go first, then the
  // networks, and the stream they all enqueue on last
  trainer_.reset();
  trainer2_.reset();
  for (void* p : bufs_) (void)hipFree(p);
  net_.reset();
  net2_.reset();
  if (stream_) (void)hipStreamDestroy(stream_);
}

void Engine::sync() {
  wait();
  // an error word a persistent tower launch raised is reported by the first synchronising call behind it, not only by
  // the next persistent forward
  net_->check_async_error();
  if (net2_) net2_->check_async_error();
}

void Engine::net_select(int which) {
  AGZ_REQUIRE(which == 0 || (which == 1 && net2_), AGZ_BAD_ARGUMENT,
              "network %d does not exist (network 1 needs arena_mode)", which);
  net_sel_ = which;
}

void Engine::start(int64_t total_games) {
  V_.analysis = 0;              // back to self-play (the analysis tables stay readable through analyze_results)
  V_.review = 0;
  ra_on_ = false;
  V_.total_games = total_games;
  rec_sent_ = 0;
  abandoned_ = 0;
  stepped_ = false;
  if (hold_rel_.p) hold_rel_.zero(stream_);     // with the hold on, the fresh slots wait for a first release
  AGZ_HIP(hipMemsetAsync(V_.counters, 0, sizeof(unsigned long long) * kCounterSlots, stream_));
  AGZ_HIP(hipMemsetAsync(V_.ar_hdr, 0, sizeof(int32_t) * 5 * (V_.games / 2 + 1), stream_));
  idle_all_slots();
}

// every slot zeroed and in `phase`; returns with the stream idle
void Engine::set_all_slots(int phase) {
  std::vector<GameState> gs(V_.games);
  std::memset(gs.data(), 0, sizeof(GameState) * gs.size());
  for (auto& g : gs) g.phase = phase;
  up(V_.gs, gs.data(), gs.size());
  wait();
}
// every slot idle and zeroed, as a run finds them
void Engine::idle_all_slots() { set_all_slots(G_IDLE); }

void Engine::step(int nsteps) {
  AGZ_REQUIRE(!cfg_.external_network, AGZ_BAD_ARGUMENT,
              "engine was created with external_network=1: use select/incorporate");
  stepped_ = stepped_ || nsteps > 0;
  for (int s = 0; s < nsteps; ++s) {
    // (search-kernel timing, bench.py: seven events per step on the engine's stream; off: no event is recorded)
    hipEvent_t* ev = sprof_on_ && sprof_n_ < kSearchProfMax ? &sprof_ev_[(size_t)7 * sprof_n_] : nullptr;
    if (ev) (void)hipEventRecord(ev[0], stream_);
    hipLaunchKernelGGL(k_pre, dim3(V_.games), dim3(kWave), 0, stream_, V_);
    if (ev) (void)hipEventRecord(ev[1], stream_);
    hipLaunchKernelGGL(V_.sk_key ? k_expand_keys : k_expand, dim3(V_.games * (kMaxPend / 2)), dim3(kWave), 0, stream_, V_);
    if (ev) (void)hipEventRecord(ev[2], stream_);
    hipLaunchKernelGGL(cfg_.arena_mode ? k_scan_arena : k_scan, dim3(1), dim3(256), 0, stream_, V_);
    if (ev) (void)hipEventRecord(ev[3], stream_);
    if (V_.symmetry)
      hipLaunchKernelGGL(k_leaf_features_sym, dim3(bcap_), dim3(kWavesPerLeaf * kWave), 0, stream_, V_, 0, bcap_, d_x32_.p, (float*)nullptr);
    else
      hipLaunchKernelGGL(k_leaf_features, dim3(bcap_), dim3(kWavesPerLeaf * kWave), 0, stream_, V_, 0, bcap_, d_x32_.p, (float*)nullptr);
    if (ev) (void)hipEventRecord(ev[4], stream_);
    if (cfg_.arena_mode) {   // evaluate(): Black's players ask network 0, White's network 1
      const int half = bcap_ / 2;
      net_->forward(d_x32_.p, V_.batch_count, half, d_pi_.p, d_v_.p);
      net2_->forward(d_x32_.p + (size_t)half * V_.P * 32, V_.batch_count + 1, half, d_pi_.p + (size_t)half * V_.A,
                     d_v_.p + half);
    } else {
      net_->forward(d_x32_.p, V_.batch_count, bcap_, d_pi_.p, d_v_.p);
    }
    if (V_.symmetry) hipLaunchKernelGGL(k_pi_unpermute, dim3(bcap_), dim3(kWave), 0, stream_, V_, 0, bcap_, d_pi_.p);
    if (ev) (void)hipEventRecord(ev[5], stream_);
    hipLaunchKernelGGL(V_.sk_key ? k_post_keys : k_post, dim3(V_.games), dim3(kWave), 0, stream_, V_);
    if (ev) {
      (void)hipEventRecord(ev[6], stream_);
      ++sprof_n_;
    }
  }
  AGZ_HIP(hipGetLastError());
}

// ---- batched analysis

void Engine::analyze_start(const int8_t* boards, const agz_position_info* info, const int8_t* history, int64_t B,
                           uint64_t game_id_base) {
  require_selfplay_engine("analysis");
  AGZ_REQUIRE(boards && info && B >= 1, AGZ_BAD_ARGUMENT, "analysis: boards and info of B >= 1 positions");
  check_positions("analysis", "position", info, history, B);
  wait();     // nothing in flight may still read the tables that are replaced here
  upload_positions(boards, info, history, B, B);
  V_.review = 0;
  V_.rv_moves = nullptr;
  V_.rv_off = nullptr;
  begin_analysis_run(B, B, game_id_base);
}

// ---- the search options of self-play: playout cap, forced playouts with target pruning, Gumbel root search
// (agz_selfplay_set_playout_cap / _set_forced_playouts / _set_gumbel).  `what` is the prefix of the error text

void Engine::require_selfplay_engine(const char* what) const {
  AGZ_REQUIRE(!cfg_.arena_mode, AGZ_BAD_ARGUMENT, "%s: an arena_mode engine plays evaluate() games only", what);
}

// a game keeps its options from its first descent to its last move, and its record is rebuilt under them: they change
// only between games (a run that has not stepped yet has claimed none)
void Engine::require_between_games(const char* what) {
  if (V_.analysis || !stepped_) return;
  agz_stats st;
  stats(&st);
  AGZ_REQUIRE(st.live_games == 0, AGZ_BAD_ARGUMENT, "%s: %lld games of the current run are still being played", what,
              (long long)st.live_games);
}

// the range checks a setter shares with its single-tree call (NaN fails each)
static void check_forced_k(const char* what, const char* range, double k) {
  AGZ_REQUIRE(k >= 0.0 && k <= 1024.0, AGZ_BAD_ARGUMENT, "%s: k = %g, not in %s", what, k, range);
}
static void check_gumbel_c(const char* what, double c_visit, double c_scale) {
  AGZ_REQUIRE(c_visit >= 0.0 && c_visit <= 1.0e9, AGZ_BAD_ARGUMENT, "%s: c_visit = %g, not in 0 .. 1e9", what, c_visit);
  AGZ_REQUIRE(c_scale > 0.0 && c_scale <= 1.0e9, AGZ_BAD_ARGUMENT, "%s: c_scale = %g, not in (0, 1e9]", what, c_scale);
}
static void check_lines(int K, int K_min, int D, int min_visits) {
  AGZ_REQUIRE(K >= K_min && K <= 16, AGZ_BAD_ARGUMENT, "lines: K = %d, not in %d..16", K, K_min);
  AGZ_REQUIRE(D >= 1 && D <= 64, AGZ_BAD_ARGUMENT, "lines: D = %d, not in 1..64", D);
  AGZ_REQUIRE(min_visits >= 1, AGZ_BAD_ARGUMENT, "lines: min_visits = %d, not >= 1", min_visits);
}

// what follows a setter's own range checks: single_trees = the option also steers single-tree searches, so it does not
// change inside a select / incorporate pair; write(V_) stores the setting; the counters [first, first + n) of the option
// restart (n = 0: it has none that a setter clears)
template <class Write>
void Engine::set_option(const char* what, bool single_trees, Write write, int first, int n) {
  AGZ_REQUIRE(!single_trees || tree_batch_ == 0, AGZ_BAD_ARGUMENT,
              "%s: not between agz_tree_search_select and agz_tree_search_incorporate", what);
  require_between_games(what);
  wait();
  write(V_);
  if (n == 0) return;
  AGZ_HIP(hipMemsetAsync(V_.counters + first, 0, sizeof(unsigned long long) * n, stream_));
  wait();
}

// counters[first .. first + n): {full, fast} moves, {forced descents, pruned rows}, {begun, halved}, {levels, unvisited},
// {tempered, noised, sampled, off the most visited}
template <class T>
void Engine::read_counters(int first, int n, T* out) {
  unsigned long long c[4];
  down(c, V_.counters + first, (size_t)n);
  wait();
  for (int i = 0; i < n; ++i) out[i] = (T)c[i];
}
static_assert(CT_CAP_FAST == CT_CAP_FULL + 1 && CT_PRUNED_ROWS == CT_FORCED_SEL + 1 && CT_GUMBEL_HALVED == CT_GUMBEL_BEGUN + 1 &&
                  CT_PUCT_UNVISITED == CT_PUCT_LEVELS + 1,
              "the counters of an option are read as one pair");
static_assert(CT_EXP_NOISED == CT_EXP_TEMPERED + 1 && CT_EXP_SAMPLED == CT_EXP_TEMPERED + 2 &&
                  CT_EXP_OFF_MAX == CT_EXP_TEMPERED + 3, "the four counters are cleared and read as one run");
void Engine::playout_cap_counts(int64_t out[2]) { read_counters(CT_CAP_FULL, 2, out); }
void Engine::forced_counts(int64_t out[2]) { read_counters(CT_FORCED_SEL, 2, out); }
void Engine::gumbel_counts(int64_t out[2]) { read_counters(CT_GUMBEL_BEGUN, 2, out); }
void Engine::puct_counts(int64_t out[2]) { read_counters(CT_PUCT_LEVELS, 2, out); }
void Engine::explore_counts(uint64_t out[4]) { read_counters(CT_EXP_TEMPERED, 4, out); }

// one pi row [A] of a single tree's node: `launch` writes it to the device row it is given
template <class Launch>
void Engine::read_tree_pi_row(float* out, Launch launch) {
  AGZ_REQUIRE(out, AGZ_BAD_ARGUMENT, "null pointer");
  s_f32a_.ensure(V_.A);
  launch(s_f32a_.p);
  AGZ_HIP(hipGetLastError());
  down(out, s_f32a_.p, (size_t)V_.A);
  wait();
}

void Engine::set_playout_cap(int fast_readouts, double full_prob) {
  require_selfplay_engine("playout cap");
  AGZ_REQUIRE(fast_readouts >= 0 && fast_readouts <= V_.R, AGZ_BAD_ARGUMENT,
              "playout cap: %d fast readouts, 0 (off) or 1..num_readouts = %d", fast_readouts, V_.R);
  AGZ_REQUIRE(fast_readouts == 0 || (full_prob >= 0.0 && full_prob <= 1.0), AGZ_BAD_ARGUMENT,
              "playout cap: full_prob %g not in [0, 1]", full_prob);
  set_option("playout cap", false, [&](View& V) { view_set_playout_cap(V, fast_readouts, full_prob); }, 0, 0);
}

void Engine::set_forced_playouts(double k, int prune) {
  require_selfplay_engine("forced playouts");
  check_forced_k("forced playouts", "0 (off) .. 1024", k);
  AGZ_REQUIRE(prune == 0 || k > 0.0, AGZ_BAD_ARGUMENT, "forced playouts: pruning needs k > 0");
  AGZ_REQUIRE(!(k > 0.0) || V_.gumbel_m == 0, AGZ_BAD_ARGUMENT, "forced playouts: the Gumbel root search is on (m = %d)", V_.gumbel_m);
  set_option("forced playouts", false, [&](View& V) { view_set_forced_playouts(V, k, prune); }, 0, 0);
}

void Engine::tree_pruned_pi(int g, int node, double k, float* out) {
  check_node(g, node);
  check_forced_k("pruned pi", "0..1024", k);
  read_tree_pi_row(out, [&](float* row) {
    hipLaunchKernelGGL(k_tree_pruned_pi, dim3(1), dim3(kWave), 0, stream_, V_, g, node, k, row);
  });
}

void Engine::set_gumbel(int m, double c_visit, double c_scale) {
  require_selfplay_engine("gumbel");
  AGZ_REQUIRE(m == 0 || (m >= 2 && m <= kGumbelMax), AGZ_BAD_ARGUMENT, "gumbel: m = %d, not 0 (off) or in 2..%d", m,
              kGumbelMax);
  check_gumbel_c("gumbel", c_visit, c_scale);
  AGZ_REQUIRE(m == 0 || !(V_.forced_k > 0.0), AGZ_BAD_ARGUMENT, "gumbel: forced playouts are on (k = %g)", V_.forced_k);
  set_option("gumbel", false, [&](View& V) { view_set_gumbel(V, m, c_visit, c_scale); }, 0, 0);
}

// ---- the PUCT rule options (agz_search_set_puct): every search of every engine, so no require_selfplay_engine

void Engine::set_puct(int fpu_on, double r, double r_root, double c_base) {
  AGZ_REQUIRE(fpu_on == 0 || fpu_on == 1, AGZ_BAD_ARGUMENT, "puct: fpu_on = %d, not 0 or 1", fpu_on);
  AGZ_REQUIRE(r >= 0.0 && r <= 4.0, AGZ_BAD_ARGUMENT, "puct: fpu_reduction = %g, not in 0 .. 4", r);
  AGZ_REQUIRE(r_root >= 0.0 && r_root <= 4.0, AGZ_BAD_ARGUMENT, "puct: fpu_reduction_root = %g, not in 0 .. 4", r_root);
  AGZ_REQUIRE(c_base == 0.0 || (c_base >= 1.0 && c_base <= 1.0e9), AGZ_BAD_ARGUMENT,
              "puct: c_base = %g, not 0 (off) or in 1 .. 1e9", c_base);
  set_option("puct", true, [&](View& V) { view_set_puct(V, fpu_on, r, r_root, c_base); }, CT_PUCT_LEVELS, 2);
}

// ---- root exploration and the move temperature (agz_selfplay_set_root_policy_temperature / _set_root_noise,
// agz_search_set_move_temperature)

// the range checks are explore_*_refusal of agz_state.h, shared with the host simulator
static void check_explore(const char* what, const char* why) {
  AGZ_REQUIRE(!why, AGZ_BAD_ARGUMENT, "%s: %s", what, why ? why : "");
}

// ... and an arena engine is refused after them; every taken setter restarts the four counters
void Engine::set_root_policy_temperature(int on, double early, double late, double halflife) {
  check_explore("root policy temperature", explore_schedule_refusal(V_, on, early, late, halflife, 0.1));
  require_selfplay_engine("root policy temperature");
  set_option("root policy temperature", true,
             [&](View& V) { view_set_root_policy_temperature(V, on, early, late, halflife); }, CT_EXP_TEMPERED, 4);
}

void Engine::set_root_noise(double total_alpha, int shaped) {
  check_explore("root noise", explore_noise_refusal(V_, total_alpha, shaped));
  require_selfplay_engine("root noise");
  set_option("root noise", true, [&](View& V) { view_set_root_noise(V, total_alpha, shaped); }, CT_EXP_TEMPERED, 4);
}

void Engine::set_move_temperature(int on, double early, double late, double halflife) {
  check_explore("move temperature", explore_schedule_refusal(V_, on, early, late, halflife, 0.0));
  require_selfplay_engine("move temperature");
  set_option("move temperature", true, [&](View& V) { view_set_move_temperature(V, on, early, late, halflife); },
             CT_EXP_TEMPERED, 4);
}

// ---- value uncertainty (agz_search_set_value_moments / _set_lcb / _set_puct_variance): every search of
// every engine.  The range checks are *_refusal of agz_state.h, shared with the host simulator; every taken setter
// restarts the four counters

static_assert(CT_UNC_LCB_OFF_MAX == CT_UNC_LCB + 1 && CT_UNC_LEVELS == CT_UNC_LCB + 2 && CT_UNC_RAISED == CT_UNC_LCB + 3,
              "the four counters are cleared and read as one run");
void Engine::uncertainty_counts(uint64_t out[4]) { read_counters(CT_UNC_LCB, 4, out); }

// the middle of a lazy setter: the arrays of one optional group -- `own`, in the order of the group's visitor of
// agz_layout.h, which states their sizes -- allocated and zeroed as temporaries, waited for, then swapped in.  An
// allocation that fails throws here, with `own` and so the option as they were
template <class Visit, class... T>
void Engine::alloc_group(Visit visit, DevBuf<T>&... own) {
  size_t count[sizeof...(T)], k = 0;
  View dims = V_;
  visit(dims, [&](auto*&, size_t n) { count[k++] = n; });
  std::tuple<DevBuf<T>...> fresh;
  std::apply([&](auto&... b) {
    k = 0;
    (b.alloc(count[k++]), ...);
    (b.zero(stream_), ...);
    wait();
    (b.swap(own), ...);
  }, fresh);
}

void Engine::set_value_moments(int on) {
  check_explore("value moments", value_moments_refusal(V_, on));
  // the state checks first (games in flight, a select phase awaiting its incorporate): a call they refuse allocates
  // nothing.  Then the arrays, made the first time the option goes on
  set_option("value moments", true, [](View&) {}, 0, 0);
  if (on && !child_s_.p) alloc_group([](View& V, auto f) { for_each_moment_buffer(V, f); }, child_s_, root_s_);
  set_option("value moments", true, [&](View& V) {
    V.childS = on ? child_s_.p : nullptr;
    V.rootS = on ? root_s_.p : nullptr;
  }, CT_UNC_LCB, 4);
}

// ---- superko (agz_search_set_ko_rule): every search of every engine.  The key arrays are made the first
// time a rule other than simple is taken, behind the state checks, as the moment arrays above
static_assert(CT_SK_MOVES == CT_SK_NODES + 1, "the two counters are cleared and read as one pair");
void Engine::superko_counts(uint64_t out[2]) { read_counters(CT_SK_NODES, 2, out); }

void Engine::set_ko_rule(int rule) {
  AGZ_REQUIRE(agz_ko_rule_valid(rule), AGZ_BAD_ARGUMENT, "ko rule: %d is not 0 (simple), 1 (positional) or 2 (situational)", rule);
  set_option("ko rule", true, [](View&) {}, 0, 0);
  if (rule != AGZ_KO_SIMPLE && !sk_key_.p)
    alloc_group([](View& V, auto f) { for_each_superko_buffer(V, f); }, sk_key_, sk_log_, sk_len_);
  set_option("ko rule", true, [&](View& V) {
    const bool on = rule != AGZ_KO_SIMPLE;
    V.ko_rule = rule;
    V.sk_key = on ? sk_key_.p : nullptr;
    V.sk_log = on ? sk_log_.p : nullptr;
    V.sk_len = on ? sk_len_.p : nullptr;
  }, CT_SK_NODES, 2);
}

void Engine::set_lcb(double z, int min_visits, double min_ratio) {
  check_explore("lcb", lcb_refusal(V_, z, min_visits, min_ratio));
  set_option("lcb", true, [&](View& V) { view_set_lcb(V, z, min_visits, min_ratio); }, CT_UNC_LCB, 4);
}

void Engine::set_puct_variance(double k, double prior, double prior_weight) {
  check_explore("puct variance", puct_variance_refusal(V_, k, prior, prior_weight));
  set_option("puct variance", true, [&](View& V) { view_set_puct_variance(V, k, prior, prior_weight); }, CT_UNC_LCB, 4);
}

void Engine::tree_child_lcb(int g, int node, double z, double* mean, double* sd, double* lcb) {
  check_node(g, node);
  AGZ_REQUIRE(mean && sd && lcb, AGZ_BAD_ARGUMENT, "null pointer");
  AGZ_REQUIRE(V_.childS != nullptr, AGZ_BAD_ARGUMENT, "child lcb: the value moments are off");
  AGZ_REQUIRE(z >= 0.0 && z <= 100.0, AGZ_BAD_ARGUMENT, "child lcb: z = %g, not in 0 .. 100", z);
  const size_t A = (size_t)V_.A;
  s_f64_.ensure(3 * A);
  hipLaunchKernelGGL(k_tree_child_lcb, dim3(1), dim3(kWave), 0, stream_, V_, g, node, z, s_f64_.p);
  AGZ_HIP(hipGetLastError());
  down(mean, s_f64_.p, A);
  down(sd, s_f64_.p + A, A);
  down(lcb, s_f64_.p + 2 * A, A);
  wait();
}

void Engine::analyze_child_S(float* child_S, float* root_S) {
  AGZ_REQUIRE(child_S && root_S, AGZ_BAD_ARGUMENT, "null pointer");
  const int64_t done = analyze_progress(), B = an_count_;
  AGZ_REQUIRE(V_.an_childS != nullptr, AGZ_BAD_ARGUMENT, "analysis: the run began with the value moments off");
  AGZ_REQUIRE(done >= B, AGZ_NOT_READY, "analysis: %lld of %lld rows finished", (long long)done, (long long)B);
  const size_t rows = (size_t)B * V_.A;
  down(child_S, V_.an_childS, rows);
  down(root_S, V_.an_rootS, (size_t)B);
  wait();
}

void Engine::tree_explore_rows(int g, int node, float* tempered, double* alpha, float* noised) {
  check_node(g, node);
  const size_t A = (size_t)V_.A, AP = (size_t)V_.AP;
  s_f32a_.ensure(AP + A);          // [noised row, AP | tempered, A]
  s_f64_.ensure(A);
  hipLaunchKernelGGL(k_tree_explore_rows, dim3(1), dim3(kWave), 0, stream_, V_, g, node, s_f32a_.p, s_f32a_.p + AP,
                     s_f64_.p);
  AGZ_HIP(hipGetLastError());
  if (noised) down(noised, s_f32a_.p, A);
  if (tempered) down(tempered, s_f32a_.p + AP, A);
  if (alpha) down(alpha, s_f64_.p, A);
  wait();
}

void Engine::tree_gumbel_pi(int g, int node, double c_visit, double c_scale, float* out) {
  check_node(g, node);
  check_gumbel_c("gumbel pi", c_visit, c_scale);
  read_tree_pi_row(out, [&](float* row) {
    hipLaunchKernelGGL(k_tree_gumbel_pi, dim3(1), dim3(kWave), 0, stream_, V_, g, node, c_visit, c_scale, row);
  });
}

// ---- start positions of self-play and arena games (agz_selfplay_set_starts)

void Engine::set_starts(const int8_t* boards, const agz_position_info* info, const int8_t* history, int64_t S) {
  AGZ_REQUIRE(S >= 0 && S <= 0x7fffffffLL, AGZ_BAD_ARGUMENT, "starts: S = %lld", (long long)S);
  AGZ_REQUIRE(S == 0 || (boards && info), AGZ_BAD_ARGUMENT, "starts: boards and info of S positions");
  AGZ_REQUIRE(S == 0 || V_.stagger == 0, AGZ_BAD_ARGUMENT,
              "starts: a table and the bench stagger exclude each other (the stagger prefix starts on the empty board)");
  // records are rebuilt through the table: it changes only while nothing is kept that was played under the old one
  const int64_t held = records_count();
  AGZ_REQUIRE(held == 0 && replay_->count() == 0, AGZ_BAD_ARGUMENT,
              "starts: the record ring holds %lld games and the replay arena %lld; clear both first", (long long)held,
              (long long)replay_->count());
  // ... and while no game is on its way into the ring (the table set before a run's first step is that run's)
  require_between_games("starts");
  const int P = V_.P, mgl = V_.max_game_length;
  if (S > 0) {
    check_positions("starts", "entry", info, history, S);
    for (int64_t i = 0; i < S; ++i) {
      AGZ_REQUIRE(!(info[i].last_move == P && info[i].prev_move == P), AGZ_BAD_ARGUMENT,
                  "starts: entry %lld is a finished game (two passes)", (long long)i);
      AGZ_REQUIRE(info[i].n < mgl, AGZ_BAD_ARGUMENT, "starts: entry %lld is a finished game (n %d >= max_game_length %d)",
                  (long long)i, info[i].n, mgl);
    }
  }
  wait();
  if (S == 0) {
    V_.st_count = 0;
    V_.st_board = nullptr;
    V_.st_hist = nullptr;
    V_.st_info = nullptr;
    return;
  }
  // the candidate goes into buffers of its own and is checked there; the table in force is replaced only by a good one
  DevBuf<int8_t> nb, nh;
  DevBuf<agz_position_info> ni;
  DevBuf<int32_t> ok;
  ok.alloc((size_t)S);
  upload_position_table(nb, nh, ni, boards, info, history, S);
  hipLaunchKernelGGL(k_starts_valid, dim3((unsigned)S), dim3(kWave), 0, stream_, V_, (const int8_t*)nb.p,
                     (const agz_position_info*)ni.p, ok.p);
  AGZ_HIP(hipGetLastError());
  std::vector<int32_t> good((size_t)S);
  down(good.data(), ok.p, (size_t)S);
  wait();
  for (int64_t i = 0; i < S; ++i)
    AGZ_REQUIRE(good[(size_t)i], AGZ_BAD_ARGUMENT,
                "starts: entry %lld: bad board (a point outside -1..1, a group without liberty or a stone on the ko point)",
                (long long)i);
  st_board_.swap(nb);
  st_hist_.swap(nh);
  st_info_.swap(ni);
  V_.st_count = (int32_t)S;
  V_.st_board = st_board_.p;
  V_.st_hist = st_hist_.p;
  V_.st_info = st_info_.p;
}

// the scalar fields of caller positions; the boards are checked on the device, per position (root_board_valid)
void Engine::check_positions(const char* mode, const char* item, const agz_position_info* info,
                             const int8_t* history, int64_t B) {
  const int P = V_.P;
  for (int64_t i = 0; i < B; ++i) {
    const agz_position_info& f = info[i];
    AGZ_REQUIRE(f.to_play == 1 || f.to_play == -1, AGZ_BAD_ARGUMENT, "%s: %s %lld: to_play %d", mode, item,
                (long long)i, f.to_play);
    AGZ_REQUIRE(f.history_len >= 0 && f.history_len <= 7, AGZ_BAD_ARGUMENT, "%s: %s %lld: history_len %d", mode, item,
                (long long)i, f.history_len);
    AGZ_REQUIRE(history || f.history_len == 0, AGZ_BAD_ARGUMENT, "%s: %s %lld: history_len %d without history boards",
                mode, item, (long long)i, f.history_len);
    AGZ_REQUIRE(f.n >= 0, AGZ_BAD_ARGUMENT, "%s: %s %lld: n %d", mode, item, (long long)i, f.n);
    AGZ_REQUIRE(f.ko >= -1 && f.ko < P, AGZ_BAD_ARGUMENT, "%s: %s %lld: ko %d", mode, item, (long long)i, f.ko);
    AGZ_REQUIRE(f.last_move >= -1 && f.last_move <= P, AGZ_BAD_ARGUMENT, "%s: %s %lld: last_move %d", mode, item,
                (long long)i, f.last_move);
    AGZ_REQUIRE(f.prev_move >= -1 && f.prev_move <= P, AGZ_BAD_ARGUMENT, "%s: %s %lld: prev_move %d", mode, item,
                (long long)i, f.prev_move);
  }
}

// B positions (boards, info, history or zeros) into a table of three device buffers, grown as needed
void Engine::upload_position_table(DevBuf<int8_t>& board, DevBuf<int8_t>& hist, DevBuf<agz_position_info>& inf,
                                   const int8_t* boards, const agz_position_info* info, const int8_t* history, int64_t B) {
  const size_t nb = (size_t)B * V_.P;
  stage(board, boards, nb);
  hist.ensure(7 * nb);
  if (history) up(hist.p, history, 7 * nb);
  else AGZ_HIP(hipMemsetAsync(hist.p, 0, 7 * nb, stream_));
  stage(inf, info, (size_t)B);
}

// B positions into the an_* tables, result tables of `rows` rows cleared (the stream is idle)
void Engine::upload_positions(const int8_t* boards, const agz_position_info* info, const int8_t* history, int64_t B,
                              int64_t rows) {
  upload_position_table(an_board_, an_hist_, an_info_, boards, info, history, B);
  clear_result_tables(rows);
}

void Engine::clear_result_tables(int64_t rows) {
  const size_t R = (size_t)(rows > 0 ? rows : 1), A = (size_t)V_.A;
  an_res_.ensure(R);
  an_rows_.ensure(3 * R * A);
  AGZ_HIP(hipMemsetAsync(an_res_.p, 0, sizeof(agz_analysis) * R, stream_));
  AGZ_HIP(hipMemsetAsync(an_rows_.p, 0, sizeof(float) * 3 * R * A, stream_));
}

// B claimable items (positions, or games in review mode) filling `rows` result rows: counters cleared, every slot idle
void Engine::begin_analysis_run(int64_t B, int64_t rows, uint64_t game_id_base) {
  const int A = V_.A;
  const size_t R = (size_t)(rows > 0 ? rows : 1);
  AGZ_HIP(hipMemsetAsync(V_.an_ctr, 0, sizeof(unsigned long long) * 2, stream_));
  // every slot idle, as agz_selfplay_start leaves them; the counters and the records ring keep their self-play content
  idle_all_slots();
  an_count_ = rows;
  V_.analysis = 1;
  V_.an_count = B;
  V_.an_id_base = game_id_base;
  V_.an_board = an_board_.p;
  V_.an_hist = an_hist_.p;
  V_.an_info = an_info_.p;
  V_.an_res = an_res_.p;
  V_.an_childN = an_rows_.p;
  V_.an_childW = an_rows_.p + R * A;
  V_.an_prior = an_rows_.p + 2 * R * A;
  // with the moments on, the root's S row and own S beside the three rows (agz_analyze_child_S)
  V_.an_childS = nullptr;
  V_.an_rootS = nullptr;
  if (V_.childS) {
    an_s_.ensure(R * A + R);
    AGZ_HIP(hipMemsetAsync(an_s_.p, 0, sizeof(float) * (R * A + R), stream_));
    V_.an_childS = an_s_.p;
    V_.an_rootS = an_s_.p + R * A;
  }
  V_.an_gid = nullptr;           // agz_replay_reanalyze_start sets the two behind this call
  V_.an_pi = nullptr;
  ra_on_ = false;
  // analysis lines (agz_analyze_set_lines): every slot of the three tables starts unused, which is what a row that is
  // never searched keeps
  V_.an_lines = lines_k_;
  V_.an_pv_depth = lines_k_ ? lines_d_ : 0;
  V_.an_pv_min = lines_k_ ? lines_min_ : 0;
  V_.an_line = nullptr;
  V_.an_pv = nullptr;
  V_.an_pvN = nullptr;
  if (lines_k_ > 0) {
    const size_t nl = R * (size_t)lines_k_, np = nl * (size_t)lines_d_;
    an_pv_.ensure(np);
    an_pvN_.ensure(np);
    agz_line unused;
    unused.move = -1; unused.pv_len = 0; unused.N = 0.f; unused.W = 0.f; unused.prior = 0.f; unused.end_W = 0.f;
    const std::vector<agz_line> fill(nl, unused);
    stage(an_line_, fill.data(), nl);
    AGZ_HIP(hipMemsetAsync(an_pv_.p, 0xff, sizeof(int16_t) * np, stream_));
    AGZ_HIP(hipMemsetAsync(an_pvN_.p, 0, sizeof(float) * np, stream_));
    wait();                      // `fill` dies here
    V_.an_line = an_line_.p;
    V_.an_pv = an_pv_.p;
    V_.an_pvN = an_pvN_.p;
  }
  external_batch_ = external_batch2_ = 0;
}

void Engine::analyze_set_lines(int K, int D, int min_visits) {
  check_lines(K, 0, D, min_visits);
  lines_k_ = K;
  lines_d_ = D;
  lines_min_ = min_visits;
}

void Engine::analyze_lines(agz_line* lines, int16_t* pv, float* pv_N) {
  const int64_t done = analyze_progress(), B = an_count_;
  AGZ_REQUIRE(V_.an_lines > 0, AGZ_BAD_ARGUMENT, "lines: the run was started with lines off (agz_analyze_set_lines)");
  AGZ_REQUIRE(done >= B, AGZ_NOT_READY, "analysis: %lld of %lld rows finished", (long long)done, (long long)B);
  const size_t nl = (size_t)B * V_.an_lines, np = nl * V_.an_pv_depth;
  down(lines, an_line_.p, nl);
  down(pv, an_pv_.p, np);
  down(pv_N, an_pvN_.p, np);
  wait();
}

// the lines of any node of single tree g: one launch, one copy (the three tables lie behind one another in s_lines_)
void Engine::tree_lines(int g, int node, int K, int D, int min_visits, agz_line* lines, int16_t* pv, float* pv_N) {
  check_node(g, node);
  check_lines(K, 1, D, min_visits);
  const size_t kd = (size_t)K * D;
  const size_t off_n = sizeof(agz_line) * K, off_pv = off_n + sizeof(float) * kd, total = off_pv + sizeof(int16_t) * kd;
  s_lines_.ensure(total);
  uint8_t* d = s_lines_.p;
  hipLaunchKernelGGL(k_tree_lines, dim3(1), dim3(kWave), 0, stream_, V_, g, node, K, D, min_visits, (agz_line*)d,
                     (int16_t*)(d + off_pv), (float*)(d + off_n));
  std::vector<uint8_t> h(total);
  down(h.data(), d, total);
  wait();
  if (lines) std::memcpy(lines, h.data(), off_n);
  if (pv_N) std::memcpy(pv_N, h.data() + off_n, sizeof(float) * kd);
  if (pv) std::memcpy(pv, h.data() + off_pv, sizeof(int16_t) * kd);
}

// ---- batched game review

void Engine::review_start(const int16_t* moves, const int64_t* game_offset, const int8_t* boards,
                          const agz_position_info* info, const int8_t* history, int64_t G, uint64_t game_id_base) {
  require_selfplay_engine("review");
  AGZ_REQUIRE(game_offset && G >= 1, AGZ_BAD_ARGUMENT, "review: game_offset of G + 1 entries, G >= 1");
  AGZ_REQUIRE((boards == nullptr) == (info == nullptr), AGZ_BAD_ARGUMENT,
              "review: start boards and info are given together or not at all");
  AGZ_REQUIRE(boards || !history, AGZ_BAD_ARGUMENT, "review: history without start boards");
  const int P = V_.P;
  AGZ_REQUIRE(game_offset[0] == 0, AGZ_BAD_ARGUMENT, "review: game_offset[0] = %lld, not 0", (long long)game_offset[0]);
  for (int64_t j = 0; j < G; ++j)
    AGZ_REQUIRE(game_offset[j + 1] >= game_offset[j], AGZ_BAD_ARGUMENT,
                "review: game %lld: game_offset decreases (%lld -> %lld)", (long long)j, (long long)game_offset[j],
                (long long)game_offset[j + 1]);
  const int64_t total = game_offset[G];
  AGZ_REQUIRE(moves || total == 0, AGZ_BAD_ARGUMENT, "review: %lld moves without a move array", (long long)total);
  for (int64_t j = 0; j < G; ++j)
    for (int64_t t = game_offset[j]; t < game_offset[j + 1]; ++t)
      AGZ_REQUIRE(moves[t] >= 0 && moves[t] <= P, AGZ_BAD_ARGUMENT, "review: game %lld: move %lld is %d, not in 0..%d",
                  (long long)j, (long long)(t - game_offset[j]), (int)moves[t], P);
  std::vector<int8_t> dboards;
  std::vector<agz_position_info> dinfo;
  if (!boards) {       // the empty board with agz_config.komi, Black to play
    dboards.assign((size_t)G * P, 0);
    dinfo.assign((size_t)G, empty_position_info(V_.komi));
    boards = dboards.data();
    info = dinfo.data();
  }
  check_positions("review", "game", info, history, G);
  wait();     // nothing in flight may still read the tables that are replaced here
  upload_positions(boards, info, history, G, total);
  rv_moves_.ensure((size_t)(total > 0 ? total : 1));
  up(rv_moves_.p, moves, (size_t)total);
  stage(rv_off_, game_offset, (size_t)G + 1);
  rv_off_host_.assign(game_offset, game_offset + G + 1);
  V_.review = 1;
  V_.rv_moves = rv_moves_.p;
  V_.rv_off = rv_off_.p;
  begin_analysis_run(G, total, game_id_base);
}

// ---- reanalysis: a review run over arena games [first, first + count), and the commit of its rows into their records

void Engine::replay_reanalyze_start(int64_t first, int64_t count, uint64_t game_id_base) {
  require_selfplay_engine("reanalyze");
  const int64_t n = replay_->count();
  const std::vector<agz_game_header>& hdr = replay_->index().hdr();
  AGZ_REQUIRE(n > 0, AGZ_BAD_ARGUMENT, "reanalyze: the replay arena is empty");
  AGZ_REQUIRE(first >= 0 && count >= 1 && count <= n && first <= n - count, AGZ_BAD_ARGUMENT,
              "reanalyze: games %lld .. %lld + %lld: the replay arena holds %lld", (long long)first, (long long)first,
              (long long)count, (long long)n);
  std::vector<int64_t> off((size_t)count + 1, 0);
  for (int64_t j = 0; j < count; ++j) off[(size_t)j + 1] = off[(size_t)j] + hdr[(size_t)(first + j)].num_moves;
  const int64_t total = off[(size_t)count];
  AGZ_REQUIRE(total <= 0x7fffffffLL, AGZ_BAD_ARGUMENT, "reanalyze: %lld rows in one run: at most 2^31 - 1",
              (long long)total);
  wait();     // nothing in flight may still read the tables that are replaced here
  replay_->index_to_device();
  const size_t G = (size_t)count, P = (size_t)V_.P, A = (size_t)V_.A, R = (size_t)(total > 0 ? total : 1);
  an_board_.ensure(G * P);
  an_hist_.ensure(7 * G * P);
  an_info_.ensure(G);
  an_gid_.ensure(G);
  an_pi_.ensure(R * A);
  AGZ_HIP(hipMemsetAsync(an_pi_.p, 0, sizeof(float) * R * A, stream_));
  clear_result_tables(total);
  rv_moves_.ensure(R);
  stage(rv_off_, off.data(), G + 1);
  hipLaunchKernelGGL(k_reanalyze_gather, dim3((unsigned)G), dim3(kWave), 0, stream_, V_, replay_->buffer(),
                     replay_->offsets_device(first), (const int64_t*)rv_off_.p, game_id_base, rv_moves_.p,
                     an_board_.p, an_hist_.p, an_info_.p, an_gid_.p);
  AGZ_HIP(hipGetLastError());
  rv_off_host_.swap(off);
  V_.review = 1;
  V_.rv_moves = rv_moves_.p;
  V_.rv_off = rv_off_.p;
  begin_analysis_run(count, total, game_id_base);       // (waits: `off` has been read)
  V_.an_gid = an_gid_.p;
  V_.an_pi = an_pi_.p;
  ra_on_ = true;
  ra_committed_ = false;
  ra_first_ = first;
  ra_stamp_ = replay_->index().change();
}

void Engine::replay_reanalyze_commit(int64_t counts_out[3]) {
  AGZ_REQUIRE(ra_on_, AGZ_BAD_ARGUMENT,
              "reanalyze commit: no reanalysis run in force (a later analysis, review or self-play start ends one)");
  AGZ_REQUIRE(!ra_committed_, AGZ_BAD_ARGUMENT, "reanalyze commit: the run has been committed already");
  AGZ_REQUIRE(ra_stamp_ == replay_->index().change(), AGZ_BAD_ARGUMENT,
              "reanalyze commit: the replay arena changed since the run started (ingest, trim, clear, window or targets-only)");
  const int64_t done = analyze_progress(), rows = an_count_;
  AGZ_REQUIRE(done >= rows, AGZ_BAD_ARGUMENT, "reanalyze commit: %lld of %lld rows finished", (long long)done,
              (long long)rows);
  ra_counts_.ensure(3);
  ra_counts_.zero(stream_);
  replay_->refresh(ra_first_, rv_off_.p, (int64_t)V_.an_count, rows, an_res_.p, an_pi_.p, ra_counts_.p);
  unsigned long long c[3];
  down(c, ra_counts_.p, 3);
  wait();
  ra_committed_ = true;
  // the run's games carry new pi rows: their surprise scores are of the old ones (agz_replay_score scores them again)
  replay_->forget_scores(ra_first_, (int64_t)rv_off_host_.size() - 1);
  if (counts_out)
    for (int i = 0; i < 3; ++i) counts_out[i] = (int64_t)c[i];
}

int64_t Engine::analyze_progress() {
  AGZ_REQUIRE(V_.an_res != nullptr, AGZ_BAD_ARGUMENT, "analysis: no agz_analyze_start on this engine");
  const unsigned long long done = fetch(V_.an_ctr + 1);
  net_->check_async_error();
  return (int64_t)done;
}

void Engine::analyze_results(agz_analysis* out, float* child_N, float* child_W, float* prior) {
  const int64_t done = analyze_progress(), B = an_count_;
  AGZ_REQUIRE(done >= B, AGZ_NOT_READY, "analysis: %lld of %lld rows finished", (long long)done, (long long)B);
  const size_t rows = (size_t)B * V_.A;
  down(out, an_res_.p, (size_t)B);
  down(child_N, an_rows_.p, rows);
  down(child_W, an_rows_.p + rows, rows);
  down(prior, an_rows_.p + 2 * rows, rows);
  wait();
}

void Engine::profile_search_enable(bool on) {
  if (on && sprof_ev_.empty()) {
    sprof_ev_.resize((size_t)7 * kSearchProfMax);
    for (auto& e : sprof_ev_) AGZ_HIP(hipEventCreate(&e));
  }
  sprof_on_ = on;
  if (on) sprof_n_ = 0;
}

// ms5: summed milliseconds of k_pre, k_expand, k_scan, k_leaf_features, k_post over the timed steps
void Engine::profile_search_read(double* ms5, int64_t* steps) {
  wait();
  for (int k = 0; k < 5; ++k) ms5[k] = 0.0;
  static const int a[5] = {0, 1, 2, 3, 5}, b[5] = {1, 2, 3, 4, 6};
  for (int i = 0; i < sprof_n_; ++i)
    for (int k = 0; k < 5; ++k) {
      float ms = 0.f;
      AGZ_HIP(hipEventElapsedTime(&ms, sprof_ev_[(size_t)7 * i + a[k]], sprof_ev_[(size_t)7 * i + b[k]]));
      ms5[k] += ms;
    }
  if (steps) *steps = sprof_n_;
}

int Engine::select_external() {
  stepped_ = true;
  hipLaunchKernelGGL(k_pre, dim3(V_.games), dim3(kWave), 0, stream_, V_);
  hipLaunchKernelGGL(V_.sk_key ? k_expand_keys : k_expand, dim3(V_.games * (kMaxPend / 2)), dim3(kWave), 0, stream_, V_);
  hipLaunchKernelGGL(cfg_.arena_mode ? k_scan_arena : k_scan, dim3(1), dim3(256), 0, stream_, V_);
  int32_t n[2] = {0, 0};
  down(n, V_.batch_count, 2);
  wait();
  external_batch_ = n[0];
  external_batch2_ = cfg_.arena_mode ? n[1] : 0;
  return external_batch_ + external_batch2_;
}

void Engine::arena_counts(int32_t* out) const {
  out[0] = external_batch_;
  out[1] = external_batch2_;
}

void Engine::leaf_features_external(float* feats_out) {
  const int B = external_batch_, B2 = external_batch2_;
  if (B + B2 <= 0) return;
  const size_t per = (size_t)17 * V_.P;
  d_whcn_.ensure((size_t)bcap_ * per);
  hipLaunchKernelGGL(k_leaf_features, dim3(bcap_), dim3(kWavesPerLeaf * kWave), 0, stream_, V_, 0, bcap_, (float*)nullptr, d_whcn_.p);
  down(feats_out, d_whcn_.p, (size_t)B * per);
  // arena: the White players' rows follow the Black players' rows in the host buffer
  down(feats_out + (size_t)B * per, d_whcn_.p + (size_t)(bcap_ / 2) * per, (size_t)B2 * per);
  wait();
}

void Engine::incorporate_external(const float* pi, const float* v) {
  const int B = external_batch_, B2 = external_batch2_;
  const size_t A = V_.A, half = (size_t)bcap_ / 2;
  if (B > 0) {
    up(d_pi_.p, pi, (size_t)B * A);
    up(d_v_.p, v, (size_t)B);
  }
  if (B2 > 0) {
    up(d_pi_.p + half * A, pi + (size_t)B * A, (size_t)B2 * A);
    up(d_v_.p + half, v + B, (size_t)B2);
  }
  hipLaunchKernelGGL(V_.sk_key ? k_post_keys : k_post, dim3(V_.games), dim3(kWave), 0, stream_, V_);
  wait();
  external_batch_ = 0;
  external_batch2_ = 0;
}

void Engine::debug_set_stagger(int moves) {
  AGZ_REQUIRE(moves >= 0 && !cfg_.arena_mode, AGZ_BAD_ARGUMENT, "stagger: >= 0 moves, not in arena_mode");
  AGZ_REQUIRE(moves == 0 || V_.st_count == 0, AGZ_BAD_ARGUMENT,
              "stagger: excluded while a table of start positions is set (the stagger prefix starts on the empty board)");
  AGZ_REQUIRE(!stepped_, AGZ_BAD_ARGUMENT, "stagger: set it before the first step of a run (before or right after agz_selfplay_start)");
  V_.stagger = moves;            // the View travels to the kernels by value: effective from the next launch
}

void Engine::debug_live_record(int g, int k, uint64_t* game_id, int32_t* num_moves, int32_t* move, float* pi, float* q) {
  AGZ_REQUIRE(g >= 0 && g < V_.games, AGZ_BAD_ARGUMENT, "slot %d of %d", g, V_.games);
  const GameState G = fetch(V_.gs + g);
  if (game_id) *game_id = G.game_id;
  if (num_moves) *num_moves = G.nqs;
  if (k < 0) return;
  AGZ_REQUIRE(k < G.nqs, AGZ_BAD_ARGUMENT, "slot %d has recorded %d moves", g, G.nqs);
  const long at = (long)g * V_.max_game_length + k;
  int16_t m = 0;
  down(&m, V_.rec_moves + at, 1);
  down(q, V_.rec_q + at, 1);
  down(pi, V_.rec_pi + at * V_.A, (size_t)V_.A);
  wait();
  if (move) *move = m;
}

int Engine::debug_counters(uint64_t* out, int cap) {
  unsigned long long c[CT_COUNT];
  down(c, V_.counters, CT_COUNT);
  wait();
  for (int i = 0; i < CT_COUNT && i < cap; ++i) out[i] = c[i];
  return CT_COUNT;
}

void Engine::stats(agz_stats* out) {
  unsigned long long c[CT_COUNT];
  std::vector<GameState> gs(V_.games);
  down(c, V_.counters, CT_COUNT);
  down(gs.data(), V_.gs, gs.size());
  sync();
  std::memset(out, 0, sizeof(*out));
  out->steps = (int64_t)c[CT_STEPS];
  out->positions = (int64_t)c[CT_POSITIONS];
  out->games_started = (int64_t)c[CT_STARTED];
  out->games_finished = (int64_t)c[CT_FINISHED];
  out->evals = (int64_t)c[CT_EVALS];
  out->duplicate_evals = (int64_t)c[CT_DUP];
  out->terminal_visits = (int64_t)c[CT_TERMINAL];
  out->pool_exhausted = (int64_t)c[CT_POOL_EXHAUSTED];
  out->resigned_games = (int64_t)c[CT_RESIGNED];
  out->root_visits = (int64_t)c[CT_ROOTVISITS];
  out->records_dropped = c[CT_RECORDED] > (unsigned long long)V_.fin_cap ? (int64_t)(c[CT_RECORDED] - V_.fin_cap) : 0;
  out->pool_short_searches = (int64_t)c[CT_POOL_SHORT];
  out->peak_nodes_per_game = (int64_t)c[CT_PEAK_NODES];
  out->node_capacity = V_.cap;
  out->abandoned_games = abandoned_;
  for (const auto& g : gs) {
    out->nodes_in_use += g.nodes_used;
    out->peak_nodes_per_game = std::max<int64_t>(out->peak_nodes_per_game, g.nodes_used);
    out->live_games += (g.phase != G_RETIRED && g.phase != G_IDLE);
    out->stalled_games += (g.stalled != 0 && g.phase == G_SEARCH);
  }
}

// Per slot: AGZ_OK, or AGZ_POOL_EXHAUSTED for a game that is waiting on a full node pool (AGZ_POOL_STALL, or nothing
// to play yet); nodes its tree holds; moves it has played.  The host's side of "recoverable": look, then
// agz_slot_abandon the games it gives up on -- or let AGZ_POOL_MOVE_EARLY (the default) keep them moving.
void Engine::slot_status(int32_t* status, int32_t* nodes, int32_t* moves) {
  std::vector<GameState> gs(V_.games);
  down(gs.data(), V_.gs, gs.size());
  wait();
  for (int g = 0; g < V_.games; ++g) {
    if (status) status[g] = (gs[g].stalled && gs[g].phase == G_SEARCH) ? AGZ_POOL_EXHAUSTED : (gs[g].err == AGZ_POOL_EXHAUSTED ? AGZ_OK : gs[g].err);
    if (nodes) nodes[g] = gs[g].nodes_used;
    if (moves) moves[g] = gs[g].move_count;
  }
}

// Drop the game a slot is playing, without a record: the slot claims the next game id at the next step (or retires
// when the quota of agz_selfplay_start is used up).  Not for arena or single-tree (manual) slots.
void Engine::slot_abandon(int g) {
  AGZ_REQUIRE(g >= 0 && g < V_.games, AGZ_BAD_ARGUMENT, "slot %d of %d", g, V_.games);
  AGZ_REQUIRE(!V_.arena, AGZ_BAD_ARGUMENT, "arena slots come in pairs: not abandonable one by one");
  GameState G = fetch(V_.gs + g);
  std::vector<agz_analysis> rs;      // uploaded below: both live until put() at the end has synchronised
  unsigned long long done = 0;
  AGZ_REQUIRE(G.phase == G_SEARCH || G.phase == G_INIT || G.phase == G_INIT_WAIT, AGZ_BAD_ARGUMENT,
              "slot %d is not playing a self-play game (phase %d)", g, G.phase);
  if (V_.analysis) {
    // the slot's position is given up: its result says so (move -1, the statistics the search reached), and it counts
    // as finished; agz_stats.abandoned_games keeps its self-play meaning
    // (review mode: the rest of the game is given up -- the current ply's row as above, the later rows move -1 and
    // nothing searched, all AGZ_POOL_EXHAUSTED)
    int64_t i = 0;
    down(&i, V_.an_slot + g, 1);
    down(&done, V_.an_ctr + 1, 1);
    wait();
    int64_t row = i, nrows = 1;
    if (V_.review) {
      row = rv_off_host_[i] + G.move_count;
      nrows = rv_off_host_[i + 1] - row;
    }
    rs.resize((size_t)nrows);
    for (auto& r : rs) { r.move = -1; r.status = AGZ_POOL_EXHAUSTED; r.N = 0.f; r.W = 0.f; r.Q = 0.f; r.nodes_used = 0; }
    agz_analysis& r = rs[0];
    r.N = G.rootN; r.W = G.rootW; r.Q = G.rootW / (1.0f + G.rootN);
    r.nodes_used = G.nodes_used;
    done += (unsigned long long)nrows;
    up(V_.an_res + row, rs.data(), (size_t)nrows);
    up(V_.an_ctr + 1, &done, 1);
  }
  G.phase = G_IDLE;
  G.nleaves = 0;
  G.npend = 0;
  G.err = 0;
  G.stalled = 0;
  put(V_.gs + g, G);
  if (!V_.analysis) ++abandoned_;
}

// ---- records

int64_t Engine::records_count() {
  const unsigned long long f = fetch(V_.counters + CT_RECORDED);
  net_->check_async_error();
  if (net2_) net2_->check_async_error();
  return (int64_t)std::min<unsigned long long>(f, (unsigned long long)V_.fin_cap);
}

void Engine::record_header(int64_t k, agz_game_header* out) {
  AGZ_REQUIRE(k >= 0 && k < records_count(), AGZ_BAD_ARGUMENT, "record %lld out of range", (long long)k);
  *out = fetch(V_.fin_hdr + k);
}

void Engine::record_game(int64_t k, int16_t* moves, float* pis, float* qs) {
  agz_game_header h;
  record_header(k, &h);
  const size_t mgl = V_.max_game_length, nm = (size_t)h.num_moves;
  if (nm == 0) return;
  down(moves, V_.fin_moves + k * mgl, nm);
  down(qs, V_.fin_q + k * mgl, nm);
  down(pis, V_.fin_pi + k * mgl * V_.A, nm * V_.A);
  wait();
}

void Engine::record_value_targets(int64_t k, double alpha, double lambda, float* out) {
  AGZ_REQUIRE(agz_value_target_params_ok(alpha, lambda), AGZ_BAD_ARGUMENT, "value target: alpha %g, lambda %g: both 0..1",
              alpha, lambda);
  agz_game_header h;
  record_header(k, &h);
  const size_t nm = (size_t)h.num_moves;
  if (nm == 0) return;
  std::vector<float> qs(nm);
  down(qs.data(), V_.fin_q + k * (size_t)V_.max_game_length, nm);
  wait();
  for (size_t t = 0; t < nm; ++t) out[t] = agz_value_target(qs.data(), h.num_moves, (int32_t)t, h.result, alpha, lambda);
}

// the packed form of records [first, last) (last < 0: records_count()): off[k] = where record first + k begins, one
// entry per record; returns the bytes of all of them.  The headers come over stream_ and are waited for.  (The size
// call used to fetch them with a blocking hipMemcpy on the null stream, which stream_ -- hipStreamNonBlocking -- does not
// order itself against; every caller had come through records_count(), which leaves stream_ idle, so that copy read
// what this one reads.)
size_t Engine::packed_layout(int64_t first, int64_t last, std::vector<int64_t>& off) {
  const int64_t n = (last < 0 ? records_count() : last) - first;
  off.clear();
  if (n <= 0) return 0;
  std::vector<agz_game_header> h((size_t)n);
  down(h.data(), V_.fin_hdr + first, (size_t)n);
  wait();
  size_t total = 0;
  for (auto& x : h) {
    off.push_back((int64_t)total);
    total += packed_bytes(V_.A, x.num_moves);
  }
  return total;
}

// bytes of the packed form of records [first, count)
int64_t Engine::records_packed_size(int64_t first, int64_t last) {
  std::vector<int64_t> off;
  return (int64_t)packed_layout(first, last, off);
}

// pack the finished records [first, count) into `dst` (device memory, >= records_packed_size(first) bytes): one D2H
// of the headers to lay the records out, one kernel to move them.  Returns the number of records packed.
int64_t Engine::pack_records_device(uint8_t* dst, int64_t capacity, int64_t* nbytes, int64_t first, int64_t last) {
  *nbytes = 0;
  std::vector<int64_t> off;
  const size_t total = packed_layout(first, last, off);
  const int64_t n = (int64_t)off.size();
  if (n <= 0) return 0;
  AGZ_REQUIRE((int64_t)total <= capacity, AGZ_BAD_ARGUMENT, "export buffer too small");
  const int64_t* d_off = stage(s_i64a_, off.data(), off.size());
  hipLaunchKernelGGL(k_pack_records, dim3((unsigned)n), dim3(256), 0, stream_, V_, d_off, dst, (long)first);
  AGZ_HIP(hipGetLastError());
  wait();      // `off` is stack-owned
  *nbytes = (int64_t)total;
  return n;
}

void Engine::records_export_packed(void* dst, int64_t capacity, bool is_device) {
  int64_t nb = 0;
  if (is_device) {
    pack_records_device((uint8_t*)dst, capacity, &nb);
    return;
  }
  const int64_t need = records_packed_size();
  AGZ_REQUIRE(need <= capacity, AGZ_BAD_ARGUMENT, "export buffer too small");
  if (need == 0) return;
  s_pack_.ensure((size_t)need);
  pack_records_device(s_pack_.p, need, &nb);
  down((uint8_t*)dst, s_pack_.p, (size_t)nb);
  wait();
}

// ---- device replay arena

int64_t Engine::replay_ingest(const void* packed, int64_t nbytes, bool is_device) {
  AGZ_REQUIRE(nbytes >= 0 && (nbytes == 0 || packed), AGZ_BAD_ARGUMENT, "bad packed buffer");
  AGZ_REQUIRE(nbytes % 8 == 0, AGZ_BAD_ARGUMENT, "packed records are a multiple of 8 bytes");
  if (nbytes == 0) return 0;
  const uint8_t* d = (const uint8_t*)packed;
  if (!is_device) d = stage(s_pack_, d, (size_t)nbytes);
  return replay_->ingest_chunks(d, {0}, {nbytes}, {-1});
}

int64_t Engine::replay_ingest_gathered(const void* buf, bool is_device, size_t nbytes, const std::vector<int64_t>& coff,
                                       const std::vector<int64_t>& cbytes, const std::vector<int64_t>& cnrec) {
  const uint8_t* d = (const uint8_t*)buf;
  if (!is_device) {
    s_pack_.ensure(std::max<size_t>(nbytes, 8));
    up(s_pack_.p, d, nbytes);
    d = s_pack_.p;
  }
  return replay_->ingest_chunks(d, coff, cbytes, cnrec);
}

// files the engine's own finished records that no exchange has filed yet (the watermark rec_sent_ moves; the
// record ring itself is the caller's to clear)
int64_t Engine::replay_ingest_local() {
  const int64_t need = records_packed_size(rec_sent_);
  if (need == 0) return 0;
  s_pack_.ensure((size_t)need);
  int64_t nb = 0;
  const int64_t n = pack_records_device(s_pack_.p, need, &nb, rec_sent_);
  const int64_t added = replay_->ingest_chunks(s_pack_.p, {0}, {nb}, {n});
  rec_sent_ += n;
  return added;
}

// records [first, first + count) of the ring, device to device; the exchange watermark (rec_sent_) does not move
int64_t Engine::replay_ingest_records(int64_t first, int64_t count) {
  const int64_t have = records_count();
  AGZ_REQUIRE(first >= 0 && count >= 0 && first + count <= have, AGZ_BAD_ARGUMENT,
              "records %lld..%lld: the ring holds %lld", (long long)first, (long long)(first + count), (long long)have);
  AGZ_REQUIRE(have <= V_.fin_cap, AGZ_BAD_ARGUMENT, "the record ring has wrapped (record_capacity_games): records lost");
  if (count == 0) return 0;
  const int64_t need = records_packed_size(first, first + count);
  s_pack_.ensure((size_t)need);
  int64_t nb = 0;
  const int64_t n = pack_records_device(s_pack_.p, need, &nb, first, first + count);
  return replay_->ingest_chunks(s_pack_.p, {0}, {nb}, {n});
}

// agz_replay_score: what concerns the engine is checked here, and the arena's scoring loop gets the staged forward of
// the ABI calls on the selected network (its buffers are not the ones the games in flight use) in chunks of at most the
// engine's forward batch.  Scoring never runs without a network: the first check.
int64_t Engine::replay_score(int64_t first, int64_t count) {
  AGZ_REQUIRE(!cfg_.external_network, AGZ_BAD_ARGUMENT,
              "score: engine was created with external_network=1 and has no network to score on");
  AGZ_REQUIRE(!(ra_on_ && !ra_committed_), AGZ_BAD_ARGUMENT, "score: a reanalysis run is open; commit it first");
  d_whcn_.ensure((size_t)bcap_ * 17 * V_.P);
  ReplayForward fwd;
  fwd.cap = bcap_;
  fwd.whcn = d_whcn_.p;
  fwd.run = [this](const int& B) -> const float* {
    launch_whcn_to_x32(d_whcn_.p, B, V_.N, stage_forward(B), stream_);
    forward_x32(B);
    return s_f32b_.p;
  };
  fwd.check = [this] { net().check_async_error(); };
  return replay_->score(first, count, fwd);
}

void Engine::train_step(const float* feats, const float* pi, const float* z, int B, bool is_device, float eta, float rho,
                        float* losses_out) {
  std::unique_ptr<Trainer>& tr = (net_sel_ && net2_) ? trainer2_ : trainer_;
  if (!tr) tr.reset(new Trainer(net(), stream_));
  tr->step(feats, pi, z, B, is_device, eta, rho, losses_out);
}

void Engine::train_reset() {
  std::unique_ptr<Trainer>& tr = (net_sel_ && net2_) ? trainer2_ : trainer_;
  if (tr) tr->reset();
}

// every parameter of the selected network as one flat vector, in the order of the device master (Net::weight_keys)
std::vector<float> Engine::weights_flat() {
  std::vector<std::pair<int, int>> keys;
  Net::weight_keys(net().tower(), keys);
  std::vector<float> w;
  for (auto& lk : keys) {
    const int64_t n = net().param_count(lk.first, lk.second);
    const size_t at = w.size();
    w.resize(at + (size_t)n);
    net().get(lk.first, lk.second, w.data() + at, n);
  }
  return w;
}

void Engine::weights_set_flat(const std::vector<float>& w) {
  std::vector<std::pair<int, int>> keys;
  Net::weight_keys(net().tower(), keys);
  size_t at = 0;
  for (auto& lk : keys) {
    const int64_t n = net().param_count(lk.first, lk.second);
    AGZ_REQUIRE(at + (size_t)n <= w.size(), AGZ_BAD_SHAPE, "flat weight vector too short");
    net().set(lk.first, lk.second, w.data() + at, n);
    at += (size_t)n;
  }
  AGZ_REQUIRE(at == w.size(), AGZ_BAD_SHAPE, "flat weight vector too long");
}

void Engine::replay_batch(const int64_t* game, const int32_t* ply, int B, float* feats, float* pi, float* z,
                          bool out_is_device, const int32_t* sym) {
  AGZ_REQUIRE(B >= 0, AGZ_BAD_ARGUMENT, "negative batch");
  if (B == 0) return;
  AGZ_REQUIRE(game && ply && feats, AGZ_BAD_ARGUMENT, "null pointer");
  if (sym)
    for (int b = 0; b < B; ++b) AGZ_REQUIRE(sym[b] >= 0 && sym[b] < 8, AGZ_BAD_ARGUMENT, "sym[%d] = %d: 0..7", b, sym[b]);
  std::vector<int64_t> off((size_t)B);
  const ReplayIndex& ix = replay_->index();
  for (int b = 0; b < B; ++b) {
    AGZ_REQUIRE(game[b] >= 0 && game[b] < ix.count(), AGZ_BAD_ARGUMENT, "sample %d: game out of range", b);
    AGZ_REQUIRE(ply[b] >= 0 && ply[b] < ix.hdr()[(size_t)game[b]].num_moves, AGZ_BAD_ARGUMENT,
                "sample %d: ply outside the game (searches_pi has one entry per move played)", b);
    off[b] = ix.off()[(size_t)game[b]];
  }
  const size_t n = (size_t)B, per = (size_t)17 * V_.P, A = V_.A;
  s_boards_.ensure(n * 8 * V_.PP);
  float *df = feats, *dp = pi, *dz = z;
  if (!out_is_device) {
    s_f32a_.ensure(per * n);
    s_f32b_.ensure(n * (A + 1));
    df = s_f32a_.p;
    dp = pi ? s_f32b_.p : nullptr;
    dz = z ? s_f32b_.p + n * A : nullptr;
  }
  const int64_t* d_off = stage(s_i64a_, off.data(), n);
  const int32_t* d_ply = stage(s_i32a_, ply, n);
  const int32_t* d_sym = sym ? stage(s_sym_, sym, n) : nullptr;      // agz_replay_batch_sym
  replay_->emit(B, d_off, d_ply, d_sym, s_boards_.p, df, dp, dz);
  if (!out_is_device) {
    down(feats, df, per * n);
    down(pi, dp, n * A);
    down(z, dz, n);
  }
  wait();      // `off` is stack-owned
}

void Engine::records_clear() {
  rec_sent_ = 0;
  AGZ_HIP(hipMemsetAsync(V_.counters + CT_RECORDED, 0, sizeof(unsigned long long), stream_));
  wait();
}

void Engine::record_features(int64_t k, float* out) {
  agz_game_header h;
  record_header(k, &h);
  if (h.num_moves <= 0) return;
  const size_t per = (size_t)17 * V_.P;
  s_f32a_.ensure(per * (size_t)h.num_moves);
  s_boards_.ensure((size_t)8 * V_.PP);
  const int32_t args[4] = {0, h.num_moves, 0, (int32_t)record_start(V_, h.game_id)};
  const int64_t zero = 0;
  int32_t* a = stage(s_i32a_, args, 4);
  int64_t* d_off = stage(s_i64a_, &zero, 1);
  hipLaunchKernelGGL(k_replay_features, dim3(1), dim3(kWave), 0, stream_, V_,
                     (const int16_t*)(V_.fin_moves + k * V_.max_game_length), a, a + 1, a + 2, d_off, s_boards_.p,
                     s_f32a_.p, (const int32_t*)(a + 3));
  down(out, s_f32a_.p, per * (size_t)h.num_moves);
  wait();
}

// get_replay_batch (train.jl:4-12), feature side: B sampled (game, ply) pairs -> [B][17*P].
// moves: the games' action lists back to back; off[b] = where sample b's game starts; ply[b] = which
// position of that game (0 = empty board).
void Engine::replay_batch_features(const int16_t* moves, int64_t nmoves, const int32_t* off, const int32_t* ply,
                                   int B, float* out, bool out_is_device, const int32_t* start) {
  AGZ_REQUIRE(B >= 0 && nmoves >= 0, AGZ_BAD_ARGUMENT, "negative count");
  if (B == 0) return;
  std::vector<int32_t> h32((size_t)4 * B);
  std::vector<int64_t> h64(B);
  const size_t per = (size_t)17 * V_.P;
  for (int b = 0; b < B; ++b) {
    AGZ_REQUIRE(off[b] >= 0 && ply[b] >= 0 && (int64_t)off[b] + ply[b] <= nmoves, AGZ_BAD_ARGUMENT,
                "sample points outside the move list");
    AGZ_REQUIRE(ply[b] <= V_.max_game_length, AGZ_BAD_ARGUMENT, "ply beyond max_game_length");
    h32[b] = off[b];
    h32[B + b] = ply[b] + 1;
    h32[2 * B + b] = ply[b];
    h32[3 * B + b] = start ? start[b] : -1;
    AGZ_REQUIRE(h32[3 * B + b] >= -1 && h32[3 * B + b] < V_.st_count, AGZ_BAD_ARGUMENT,
                "sample %d: start %d, the table holds %d entries (-1 = empty board)", b, h32[3 * B + b], V_.st_count);
    h64[b] = (int64_t)b * (int64_t)per;
  }
  for (int64_t i = 0; i < nmoves; ++i)
    AGZ_REQUIRE(moves[i] >= 0 && moves[i] <= V_.P, AGZ_BAD_ARGUMENT, "move outside 0..N*N");
  s_i16a_.ensure((size_t)std::max<int64_t>(nmoves, 1));
  s_boards_.ensure((size_t)B * 8 * V_.PP);
  float* dst = out;
  if (!out_is_device) {
    s_f32a_.ensure(per * (size_t)B);
    dst = s_f32a_.p;
  }
  up(s_i16a_.p, moves, (size_t)nmoves);
  int32_t* a = stage(s_i32a_, h32.data(), h32.size());      // [off | ply + 1 | ply | start] x B
  int64_t* d_off = stage(s_i64a_, h64.data(), h64.size());
  hipLaunchKernelGGL(k_replay_features, dim3(B), dim3(kWave), 0, stream_, V_, (const int16_t*)s_i16a_.p, a, a + B,
                     a + 2 * B, d_off, s_boards_.p, dst, (const int32_t*)(a + 3 * B));
  AGZ_HIP(hipGetLastError());
  if (!out_is_device) down(out, dst, per * (size_t)B);
  wait();     // the staging vectors above are stack-owned
}

// ---- network entry points

// B caller positions into the staging buffers launch_features_from_deltas reads: s_boards_, s_deltas_, s_i32a_ (the
// delta counts) and s_tp_
void Engine::stage_positions(const int8_t* boards, const int8_t* deltas, const int32_t* ndeltas, const int8_t* to_play,
                             int B) {
  const size_t n = (size_t)B, P = V_.P;
  stage(s_boards_, boards, n * P);
  stage(s_deltas_, deltas, n * 7 * P);
  stage(s_i32a_, ndeltas, n);
  stage(s_tp_, to_play, n);
}

// what a forward of B rows from the ABI needs before its launch: the batch count on the device, room for [pi | v] in
// s_f32b_ and for the x32 rows in s_f32a_.  Returns where the caller writes the x32 rows.  The count is uploaded from
// the caller's `B`, which must live until the caller's next wait() (forward_staged's, fill_synthetic_inputs' own).
float* Engine::stage_forward(const int& B) {
  stage(d_count_, &B, 1);
  s_f32b_.ensure((size_t)B * (V_.A + 1));
  s_f32a_.ensure((size_t)B * V_.P * 32);
  return s_f32a_.p;
}

// the selected network on the rows stage_forward() made room for: pi [B][A] at s_f32b_, v [B] behind it
void Engine::forward_x32(int B) {
  net().forward(s_f32a_.p, d_count_.p, B, s_f32b_.p, s_f32b_.p + (size_t)B * V_.A);
}

// forward_x32 and pi / v back to the host; with d_sym (device, [B]) pi row b goes back to board orientation first
void Engine::forward_staged(int B, const int32_t* d_sym, float* pi_out, float* v_out) {
  const size_t nA = (size_t)B * V_.A;
  const float* pi = s_f32b_.p;
  forward_x32(B);
  if (d_sym) {      // s_symp_: sized by the caller, next to s_symf_
    launch_sym_rows(s_f32b_.p, s_symp_.p, d_sym, B, V_.N, 1, 1, 1, stream_);
    AGZ_HIP(hipGetLastError());
    pi = s_symp_.p;
  }
  down(pi_out, pi, nA);
  down(v_out, s_f32b_.p + nA, (size_t)B);
  wait();
  net().check_async_error();      // a persistent tower launch that gave up: these outputs are garbage, say so now
}

void Engine::features(const int8_t* boards, const int8_t* deltas, const int32_t* ndeltas, const int8_t* to_play,
                      int B, float* out) {
  AGZ_REQUIRE(B >= 0, AGZ_BAD_ARGUMENT, "B < 0");
  if (B == 0) return;
  const size_t n = (size_t)B * 17 * V_.P;
  stage_positions(boards, deltas, ndeltas, to_play, B);
  s_f32a_.ensure(n);
  launch_features_from_deltas(s_boards_.p, s_deltas_.p, s_i32a_.p, s_tp_.p, B, V_.N, nullptr, s_f32a_.p, stream_);
  down(out, s_f32a_.p, n);
  wait();
}

void Engine::net_forward_positions(const int8_t* boards, const int8_t* deltas, const int32_t* ndeltas,
                                   const int8_t* to_play, int B, float* pi_out, float* v_out) {
  AGZ_REQUIRE(B >= 0, AGZ_BAD_ARGUMENT, "B < 0");
  if (B == 0) return;
  stage_positions(boards, deltas, ndeltas, to_play, B);
  float* x32 = stage_forward(B);
  launch_features_from_deltas(s_boards_.p, s_deltas_.p, s_i32a_.p, s_tp_.p, B, V_.N, x32, nullptr, stream_);
  forward_staged(B, nullptr, pi_out, v_out);
}

void Engine::net_forward_features(const float* feats, int B, float* pi_out, float* v_out) {
  AGZ_REQUIRE(B >= 0, AGZ_BAD_ARGUMENT, "B < 0");
  if (B == 0) return;
  const float* whcn = stage(d_whcn_, feats, (size_t)B * 17 * V_.P);
  launch_whcn_to_x32(whcn, B, V_.N, stage_forward(B), stream_);
  forward_staged(B, nullptr, pi_out, v_out);
}

// agz_net_forward_features_sym: row b under T_sym[b] (k_sym_rows), the plain forward, pi back to board orientation
void Engine::net_forward_features_sym(const float* feats, const int32_t* sym, int B, float* pi_out, float* v_out) {
  AGZ_REQUIRE(B >= 0, AGZ_BAD_ARGUMENT, "B < 0");
  if (B == 0) return;
  AGZ_REQUIRE(feats && sym && pi_out && v_out, AGZ_BAD_ARGUMENT, "null pointer");
  for (int b = 0; b < B; ++b) AGZ_REQUIRE(sym[b] >= 0 && sym[b] < 8, AGZ_BAD_ARGUMENT, "sym[%d] = %d: 0..7", b, sym[b]);
  const size_t n = (size_t)B * 17 * V_.P;
  const float* whcn = stage(d_whcn_, feats, n);
  const int32_t* d_sym = stage(s_sym_, sym, (size_t)B);
  s_symf_.ensure(n);
  s_symp_.ensure((size_t)B * V_.A);
  launch_sym_rows(whcn, s_symf_.p, d_sym, B, V_.N, 17, 0, 0, stream_);
  launch_whcn_to_x32(s_symf_.p, B, V_.N, stage_forward(B), stream_);
  forward_staged(B, d_sym, pi_out, v_out);
}

void Engine::set_hold(bool on) {
  AGZ_REQUIRE(!V_.arena, AGZ_BAD_ARGUMENT, "the hold is for self-play slots; arena slots come in pairs");
  if (on && !hold_rel_.p) hold_rel_.alloc((size_t)V_.games);
  if (hold_rel_.p) hold_rel_.zero(stream_);     // pending releases go: a parked slot waits for the next release
  V_.hold = on ? 1 : 0;                         // by value into the kernels: effective from the next step
  V_.released = hold_rel_.p;
  wait();
}

void Engine::release() {
  if (!V_.hold) return;
  hipLaunchKernelGGL(k_release, dim3((V_.games + 255) / 256), dim3(256), 0, stream_, V_);
  AGZ_HIP(hipGetLastError());
}

void Engine::set_symmetry(int mode) {
  AGZ_REQUIRE(mode >= AGZ_SYMMETRY_NONE && mode <= AGZ_SYMMETRY_RANDOM, AGZ_BAD_ARGUMENT,
              "symmetry mode %d: -1 (none), 0..7 (fixed T_s) or 8 (random)", mode);
  AGZ_REQUIRE(!cfg_.external_network, AGZ_BAD_ARGUMENT,
              "symmetry applies to the engine's own network; with external_network=1 the caller evaluates Positions");
  AGZ_REQUIRE(tree_batch_ == 0, AGZ_BAD_ARGUMENT,
              "symmetry: not between agz_tree_search_select and agz_tree_search_incorporate");
  V_.symmetry = mode < 0 ? 0 : mode + 1;    // the View travels to the kernels by value: effective from the next launch
}

// random stone features (not zeros: DVFS makes zero-filled operands look faster than real data)
void Engine::fill_synthetic_inputs(int B) {
  const size_t P = V_.P;
  std::vector<int8_t> boards((size_t)B * P), deltas((size_t)B * 7 * P, 0), tp(B);
  std::vector<int32_t> nd(B, 0);
  uint64_t s = 0x1234567ull;
  for (auto& x : boards) {
    s = agz_mix64(s + 0x9E3779B97F4A7C15ull);
    const int r = (int)(s % 3);
    x = (int8_t)(r == 2 ? -1 : r);
  }
  for (int b = 0; b < B; ++b) tp[b] = (b & 1) ? -1 : 1;
  stage_positions(boards.data(), deltas.data(), nd.data(), tp.data(), B);
  float* x32 = stage_forward(B);
  launch_features_from_deltas(s_boards_.p, s_deltas_.p, s_i32a_.p, s_tp_.p, B, V_.N, x32, nullptr, stream_);
  wait();      // the vectors above are stack-owned
}

// milliseconds per launch over `iters` launches, by two events on stream_
template <class Launch>
float Engine::time_launches(int iters, Launch launch) {
  hipEvent_t e0, e1;
  AGZ_HIP(hipEventCreate(&e0));
  AGZ_HIP(hipEventCreate(&e1));
  AGZ_HIP(hipEventRecord(e0, stream_));
  for (int i = 0; i < iters; ++i) launch();
  AGZ_HIP(hipEventRecord(e1, stream_));
  AGZ_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  AGZ_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return ms / (float)iters;
}

float Engine::time_forward(int B, int iters) {
  AGZ_REQUIRE(B > 0 && iters > 0, AGZ_BAD_ARGUMENT, "B and iters must be positive");
  fill_synthetic_inputs(B);
  forward_x32(B);   // warm-up
  return time_launches(iters, [&] { forward_x32(B); });
}

float Engine::time_conv(int B, int iters) {
  AGZ_REQUIRE(B > 0 && iters > 0, AGZ_BAD_ARGUMENT, "B and iters must be positive");
  fill_synthetic_inputs(B);
  forward_x32(B);   // one forward leaves real (post-ReLU, mixed-sign-weight) activations in the tower buffers
  net_->launch_tower_conv_once(d_count_.p, B);
  return time_launches(iters, [&] { net_->launch_tower_conv_once(d_count_.p, B); });
}

void Engine::debug_draws(uint64_t seed, uint64_t game, uint32_t move, int n, double alpha, double* out) {
  if (n <= 0) return;
  s_f64_.ensure(n);
  hipLaunchKernelGGL(k_debug_draws, dim3(ceil_div(n, 64)), dim3(64), 0, stream_, seed, game, move, n, alpha, s_f64_.p);
  down(out, s_f64_.p, (size_t)n);
  wait();
}

void Engine::debug_math(int op, const double* x, const double* y, int n, double* out) {
  if (n <= 0) return;
  const size_t m = (size_t)n;
  s_f64_.ensure(3 * m);
  double* d = s_f64_.p;      // [x | y | out]
  up(d, x, m);
  if (y) up(d + m, y, m);
  hipLaunchKernelGGL(k_debug_math, dim3(ceil_div(n, 64)), dim3(64), 0, stream_, V_, op, (const double*)d,
                     (const double*)(d + m), n, d + 2 * m);
  down(out, d + 2 * m, m);
  wait();
}

// ---- Go rules

void Engine::go_play(const int8_t* boards, const int8_t* to_play, const int32_t* ko, const int32_t* moves, int B,
                     int8_t* boards_out, int32_t* ko_out, int32_t* ncap_out, int32_t* status_out) {
  if (B <= 0) return;
  const size_t n = (size_t)B, P = V_.P;
  const int8_t *d_boards = stage(s_boards_, boards, n * P), *d_tp = stage(s_tp_, to_play, n);
  const int32_t *d_ko = stage(s_i32a_, ko, n), *d_moves = stage(s_i32b_, moves, n);
  s_boards_out_.ensure(n * P);
  s_i32c_.ensure(3 * n);
  int32_t* o = s_i32c_.p;      // [ko | captures | status]
  hipLaunchKernelGGL(k_go_play, dim3(B), dim3(kWave), 0, stream_, V_, d_boards, d_tp, d_ko, d_moves, B, s_boards_out_.p,
                     o, o + n, o + 2 * n);
  down(boards_out, s_boards_out_.p, n * P);
  down(ko_out, o, n);
  down(ncap_out, o + n, n);
  down(status_out, o + 2 * n, n);
  wait();
}

void Engine::go_legal(const int8_t* boards, const int8_t* to_play, const int32_t* ko, int B, int8_t* out) {
  if (B <= 0) return;
  const size_t n = (size_t)B;
  const int8_t *d_boards = stage(s_boards_, boards, n * V_.P), *d_tp = stage(s_tp_, to_play, n);
  const int32_t* d_ko = stage(s_i32a_, ko, n);
  s_legal_.ensure(n * V_.A);
  hipLaunchKernelGGL(k_go_legal, dim3(B), dim3(kWave), 0, stream_, V_, d_boards, d_tp, d_ko, B, s_legal_.p);
  down(out, s_legal_.p, n * V_.A);
  wait();
}

static void check_ko_rule(const char* what, int rule) {
  AGZ_REQUIRE(agz_ko_rule_valid(rule), AGZ_BAD_ARGUMENT, "%s: rule %d", what, rule);
}

void Engine::go_keys(const int8_t* boards, const int8_t* to_play, int B, int rule, uint64_t* out) {
  check_ko_rule("go keys", rule);
  if (B <= 0) return;
  const size_t n = (size_t)B;
  const int8_t *d_boards = stage(s_boards_, boards, n * V_.P), *d_tp = stage(s_tp_, to_play, n);
  s_u64_.ensure(n);
  hipLaunchKernelGGL(k_go_keys, dim3(B), dim3(kWave), 0, stream_, V_, d_boards, d_tp, B, rule, s_u64_.p);
  down(out, s_u64_.p, n);
  wait();
}

void Engine::go_legal_seen(const int8_t* boards, const int8_t* to_play, const int32_t* ko, const uint64_t* seen_keys,
                           const int64_t* seen_off, int B, int rule, int8_t* out) {
  check_ko_rule("go legal seen", rule);
  if (B <= 0) return;
  const size_t n = (size_t)B;
  AGZ_REQUIRE(seen_off[0] == 0, AGZ_BAD_ARGUMENT, "go legal seen: seen_off[0] = %lld", (long long)seen_off[0]);
  for (size_t b = 0; b < n; ++b)
    AGZ_REQUIRE(seen_off[b + 1] >= seen_off[b] && seen_off[b + 1] - seen_off[b] <= (1 << 30), AGZ_BAD_ARGUMENT,
                "go legal seen: seen_off is not ascending at %lld", (long long)b);
  const size_t total = (size_t)seen_off[n];
  const int8_t *d_boards = stage(s_boards_, boards, n * V_.P), *d_tp = stage(s_tp_, to_play, n);
  const int32_t* d_ko = stage(s_i32a_, ko, n);
  const int64_t* d_off = stage(s_i64a_, seen_off, n + 1);
  s_u64_.ensure(total + 1);
  if (total) up(s_u64_.p, seen_keys, total);
  s_legal_.ensure(n * V_.A);
  hipLaunchKernelGGL(k_go_legal_seen, dim3(B), dim3(kWave), 0, stream_, V_, d_boards, d_tp, d_ko,
                     (const uint64_t*)s_u64_.p, d_off, B, rule, s_legal_.p);
  down(out, s_legal_.p, n * V_.A);
  wait();
}

void Engine::go_score(const int8_t* boards, const float* komi, int B, float* out) {
  if (B <= 0) return;
  const size_t n = (size_t)B;
  const int8_t* d_boards = stage(s_boards_, boards, n * V_.P);
  s_f32a_.ensure(2 * n);
  float* d = s_f32a_.p;      // [komi | score]
  up(d, komi, n);
  hipLaunchKernelGGL(k_go_score, dim3(B), dim3(kWave), 0, stream_, V_, d_boards, (const float*)d, B, d + n);
  down(out, d + n, n);
  wait();
}

// ---- single-tree compat

void Engine::check_game(int g) const {
  AGZ_REQUIRE(g >= 0 && g < V_.games, AGZ_BAD_ARGUMENT, "game slot %d of %d", g, V_.games);
}
void Engine::check_node(int g, int node) const {
  check_game(g);
  AGZ_REQUIRE(node >= 0 && node < V_.cap, AGZ_BAD_ARGUMENT, "node %d of %d", node, V_.cap);
}

int Engine::tree_op(TreeArgs& T, int32_t* r0) {
  check_game(T.g);
  // stage host-side inputs
  if (T.probs) T.probs = stage(s_f32a_, T.probs, (size_t)V_.A);
  if (T.board) T.board = stage(s_boards_, T.board, (size_t)V_.P);
  if (T.history && T.info.history_len > 0) {
    s_deltas_.ensure((size_t)7 * V_.P);
    up(s_deltas_.p, T.history, (size_t)std::min(T.info.history_len, 7) * V_.P);
    T.history = s_deltas_.p;
  }
  double* host_dout = T.dout;
  if (T.dout) {
    s_f64_.ensure(V_.A);
    T.dout = s_f64_.p;
  }
  T.iout = s_iout_.p;
  hipLaunchKernelGGL(k_tree_op, dim3(1), dim3(kWave), 0, stream_, V_, T);
  int32_t iout[4] = {0, 0, 0, 0};
  down(iout, s_iout_.p, 4);
  down(host_dout, s_f64_.p, (size_t)V_.A);
  wait();
  if (r0) *r0 = iout[1];
  return iout[0];
}

// tree_search!(player, parallel_readouts) on slot g, split at the network call so that any
// callable can stand in for the network (MCTSPlayer.network is duck-typed, mcts_play.jl:5,89)
int Engine::tree_search_select(int g, int par, int* nleaves) {
  check_game(g);
  AGZ_REQUIRE(par >= 1 && par <= V_.par, AGZ_BAD_ARGUMENT,
              "parallel_readouts %d exceeds the engine's configured %d", par, V_.par);
  TreeArgs T;
  std::memset(&T, 0, sizeof(T));
  T.op = TOP_SEARCH_SELECT; T.g = g; T.par = par;
  int32_t n = 0;
  const int st = tree_op(T, &n);
  *nleaves = n;
  tree_batch_ = n;
  return st;
}

void Engine::tree_leaf_features(int g, float* feats_out) {
  check_game(g);
  if (tree_batch_ <= 0) return;
  d_whcn_.ensure((size_t)bcap_ * 17 * V_.P);
  hipLaunchKernelGGL(k_leaf_features, dim3(V_.par), dim3(kWavesPerLeaf * kWave), 0, stream_, V_, g, V_.par, (float*)nullptr, d_whcn_.p);
  down(feats_out, d_whcn_.p, (size_t)tree_batch_ * 17 * V_.P);
  wait();
}

// agz_tree_leaf_positions: the leaves of the last tree_search_select as the reference's GoPosition fields
// (board.jl:271-306): board, board_deltas newest first (delta_k = B_k - B_{k+1}: +colour at the played point and where
// an opponent stone vanished, board.jl:479-481,505-506), to_play, n, ko, caps, the last two moves
void Engine::tree_leaf_positions(int g, int32_t* nodes, int8_t* boards, int8_t* deltas, int32_t* ndeltas,
                                 int8_t* to_play, agz_position_info* info) {
  check_game(g);
  const int n = tree_batch_;
  if (n <= 0) return;
  const int P = V_.P;
  s_leafb_.ensure((size_t)V_.par * 8 * P);
  s_leafrows_.ensure((size_t)V_.par * sizeof(LeafPosRow));
  hipLaunchKernelGGL(k_leaf_positions, dim3(n), dim3(kWave), 0, stream_, V_, g, s_leafb_.p, (LeafPosRow*)s_leafrows_.p);
  std::vector<int8_t> b8((size_t)n * 8 * P);
  std::vector<LeafPosRow> rows(n);
  GameState gs;
  down(b8.data(), s_leafb_.p, b8.size());
  down(rows.data(), (const LeafPosRow*)s_leafrows_.p, (size_t)n);
  down(&gs, V_.gs + g, 1);
  wait();
  for (int k = 0; k < n; ++k) {
    const LeafPosRow& r = rows[k];
    const int avail = std::min(7, (r.plen - 1) + gs.hist_len);   // older boards that exist (record_leaf)
    const int8_t* b = b8.data() + (size_t)k * 8 * P;
    if (nodes) nodes[k] = r.node;
    if (boards) std::memcpy(boards + (size_t)k * P, b, P);
    if (deltas) {
      int8_t* d = deltas + (size_t)k * 7 * P;
      std::memset(d, 0, (size_t)7 * P);
      for (int s = 0; s < avail; ++s)
        for (int p = 0; p < P; ++p) d[(size_t)s * P + p] = (int8_t)(b[(size_t)s * P + p] - b[(size_t)(s + 1) * P + p]);
    }
    if (ndeltas) ndeltas[k] = avail;
    if (to_play) to_play[k] = r.m.to_play;
    if (info) {
      agz_position_info& o = info[k];
      o.n = r.m.n; o.to_play = r.m.to_play; o.ko = r.m.ko; o.caps_black = r.m.caps_b; o.caps_white = r.m.caps_w;
      o.last_move = r.m.last_move; o.prev_move = r.prev_move; o.history_len = avail; o.komi = gs.komi;
    }
  }
}

int Engine::tree_search_incorporate(int g, const float* pi, const float* v) {
  check_game(g);
  const int n = tree_batch_;
  if (n > 0) {
    if (pi && v) {
      up(d_pi_.p, pi, (size_t)n * V_.A);
      up(d_v_.p, v, (size_t)n);
    } else {      // the engine's own network, under the symmetry in force (`n` lives until tree_op below has synchronised)
      stage(d_count_, &n, 1);
      hipLaunchKernelGGL(V_.symmetry ? k_leaf_features_sym : k_leaf_features, dim3(V_.par), dim3(kWavesPerLeaf * kWave), 0,
                         stream_, V_, g, V_.par, d_x32_.p, (float*)nullptr);
      net_->forward(d_x32_.p, d_count_.p, std::min(bcap_, V_.par), d_pi_.p, d_v_.p);
      if (V_.symmetry) hipLaunchKernelGGL(k_pi_unpermute, dim3(V_.par), dim3(kWave), 0, stream_, V_, g, V_.par, d_pi_.p);
    }
  }
  TreeArgs T;
  std::memset(&T, 0, sizeof(T));
  T.op = TOP_SEARCH_POST; T.g = g;
  tree_batch_ = 0;
  return tree_op(T, nullptr);
}

void Engine::game_state(int g, GameState* out) {
  check_game(g);
  *out = fetch(V_.gs + g);
}
void Engine::game_patch(int g, const GameState& s) {
  check_game(g);
  put(V_.gs + g, s);
}
void Engine::node_meta(int g, int node, NodeMeta* out) {
  check_node(g, node);
  *out = fetch(V_.meta + node_index(V_, g, node));
}
void Engine::node_meta_set(int g, int node, const NodeMeta& m) {
  check_node(g, node);
  put(V_.meta + node_index(V_, g, node), m);
}
static float* row_base(const View& V, int field) {
  return field == AGZ_F_CHILD_N ? V.childN : field == AGZ_F_CHILD_W ? V.childW : field == AGZ_F_CHILD_S ? V.childS : V.childP;
}
// the float rows a caller reads and writes: N, W, prior, and with the moments on S
static void check_row_field(const View& V, int field) {
  AGZ_REQUIRE((field >= 0 && field <= 2) || field == AGZ_F_CHILD_S, AGZ_BAD_ARGUMENT, "field %d", field);
  AGZ_REQUIRE(field != AGZ_F_CHILD_S || V.childS != nullptr, AGZ_BAD_ARGUMENT, "field %d: the value moments are off", field);
}
void Engine::node_row_get(int g, int node, int field, float* out) {
  check_node(g, node);
  check_row_field(V_, field);
  down(out, row_base(V_, field) + node_index(V_, g, node) * V_.AP, (size_t)V_.A);
  wait();
}
void Engine::node_row_set(int g, int node, int field, const float* in) {
  check_node(g, node);
  check_row_field(V_, field);
  up(row_base(V_, field) + node_index(V_, g, node) * V_.AP, in, (size_t)V_.A);
  wait();
}
void Engine::node_children(int g, int node, int32_t* out) {
  check_node(g, node);
  down(out, V_.child + node_index(V_, g, node) * V_.AP, (size_t)V_.A);
  wait();
}
void Engine::node_board(int g, int node, int8_t* out) {
  check_node(g, node);
  down(out, V_.board + node_index(V_, g, node) * V_.PP, (size_t)V_.P);
  wait();
}
uint64_t Engine::node_key(int g, int node) {
  check_node(g, node);
  if (V_.sk_key) return fetch(V_.sk_key + node_index(V_, g, node));
  std::vector<int8_t> b((size_t)V_.P);
  node_board(g, node, b.data());
  return agz_position_key(b.data(), V_.P, 1, AGZ_KO_SIMPLE);
}
void Engine::node_legal(int g, int node, int8_t* out) {
  check_node(g, node);
  std::vector<uint32_t> words((size_t)V_.LW);
  down(words.data(), V_.legal + node_index(V_, g, node) * V_.LW, (size_t)V_.LW);
  wait();
  for (int a = 0; a < V_.A; ++a) out[a] = (int8_t)((words[a >> 5] >> (a & 31)) & 1u);
}
float Engine::node_stat(int g, int node, int which) {
  NodeMeta m;
  node_meta(g, node, &m);
  const float* src;
  AGZ_REQUIRE(which != 2 || V_.childS != nullptr, AGZ_BAD_ARGUMENT, "node S: the value moments are off");
  if (m.parent < 0) {
    src = which == 2 ? &V_.rootS[g] : which == 0 ? &V_.gs[g].rootN : &V_.gs[g].rootW;
  } else {
    src = (which == 2 ? V_.childS : which == 0 ? V_.childN : V_.childW) + node_index(V_, g, m.parent) * V_.AP + m.fmove;
  }
  return fetch(src);
}
void Engine::node_set_N(int g, int node, float v) {
  NodeMeta m;
  node_meta(g, node, &m);
  float* dst = m.parent < 0 ? &V_.gs[g].rootN : V_.childN + node_index(V_, g, m.parent) * V_.AP + m.fmove;
  put(dst, v);
}

}  // namespace agz

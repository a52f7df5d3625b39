// agz_wino4.hip -- the 3x3 256->256 tower convolution as Winograd F(4x4, 3x3) on the f32 MFMA, for boards of 13x13 and
// larger (BASELINE configs[3]: 19x19, tower 20).
//
// Why a second Winograd kernel: on the exact-f32 matrix pipe the layer is bound by MFMA work (and by the power that work
// costs: HISTORY.md 4f), so the lever is fewer multiplies.  F(3x3,3x3) (agz_wino.hip) tiles a 19x19 board as 7x7 tiles of
// 3 over a 21-wide cover: 49 x 25 = 1225 multiplies per (cin, cout) and board, 3.39 per output point.  F(4x4,3x3) tiles
// it as 5x5 tiles of 4 over a 20-wide cover: 25 x 36 = 900, 2.49 per point -- 27 % less MFMA work, 25 % less V traffic --
// and f32 has four orders of magnitude of head-room on this network (|d pi| ~ 1e-8 against the 1e-4 bar).
//
//   Y = A^T [ (G k G^T) .* (B^T d B) ] A          interpolation points {0, 1, -1, 2, -2, inf}
//   B^T = [ 4  0 -5  0  1  0 ]   A^T = [ 1  1  1  1  1  0 ]   G = [  1/4    0     0   ]
//         [ 0 -4 -4  1  1  0 ]         [ 0  1 -1  2 -2  0 ]       [ -1/6  -1/6  -1/6  ]
//         [ 0  4 -4 -1  1  0 ]         [ 0  1  1  4  4  0 ]       [ -1/6   1/6  -1/6  ]
//         [ 0 -2 -1  2  1  0 ]         [ 0  1 -1  8 -8  1 ]       [ 1/24  1/12   1/6  ]
//         [ 0  2 -1 -2  1  0 ]                                     [ 1/24 -1/12   1/6  ]
//         [ 0  4  0 -5  0  1 ]                                     [  0     0     1   ]
//   (B^T is integral, so the input transform is exact up to its own sums; G is applied on the host in float64.)
//
// The problem this kernel is built around: a workgroup tile of 64 tiles x 64 couts (the one that gives 16 flop per
// LDS-DMA byte, agz_wino.hip) needs 36 planes x 16 accumulator registers = 576 per lane with one wave per SIMD -- more
// than the 512 a lane owns.  So the 36 planes are multiplied in SIX PASSES over the input channels, one per transform
// row i, and each pass is folded into the inverse transform as soon as its K loop ends.  With M[i][j] the plane of
// transform row i and column j,  Y = A^T M A = sum_i A^T[:, i] (x) (A^T M[i][:]):  after pass i the six accumulator
// tuples become t = A^T M[i][:] (four values per element) and Y[i'][:] += A^T[i'][i] t.  Live registers: 96 accumulators
// + the 256 of the 16 running outputs -- nothing of either ever in scratch -- and ONE K-loop body and ONE fold (the row's
// weights are run-time scalars) in 24 KB of code.  Every byte and every MFMA of the one-pass form is kept: a pass moves
// only its own planes of V and U.  (History -- four passes with paired rows, 65 KB of code, tuples in scratch -- and what
// each step measured: HISTORY.md 4g.)
//
// Stage = 24 UNITS; a unit = one plane x 4 input channels = 64 rows x 16 B of V and of U (1 KB each), two MFMAs per wave;
// a stage = 6 planes x 4 channel groups = 48 KB, 16 stages per pass, 96 per layer, triple-buffered in LDS and filled by
// LDS-DMA exactly like agz_wino.hip's, 12 pieces per wave and stage.  The stage sequence is one flat list in HBM
// ([pass][stage][unit]), so the DMA stream runs across pass boundaries.
//
// Accumulators are TRANSPOSED (D = U^T-rows x V-rows: lane = tile row, register = cout): a lane holds, per output point,
// four consecutive couts in a register quad, so the epilogue's image pass moves 16-byte units, and the 64 couts split
// into two halves BY REGISTER INDEX (all four waves work on either half).  That matters because the tile image of 64
// tiles x 16 outputs x 64 couts (256 KB) does not fit the LDS: the epilogue runs twice, on a 128 KB image of 32 couts.
//
// Epilogue per half: residual half-tile -> image by LDS-DMA; BatchNorm affine in registers; image = ReLU(image + value);
// image -> y; the NEXT layer's input transform V = B^T d B (6x6 patches from the image, lane = tile row, 1 KB contiguous
// stores) for every tile whose patch lies in this tile block (whole-board blocks for N = 13..16: 16 tiles per board, 4
// boards per block; five boards per block pair above, where k_wino4_in<FIXUP> does the ends of the one board a pair cuts).
#include "agz_nn.h"
#include "agz_pack.h"
#include "agz_glds.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <type_traits>
#include <vector>

namespace agz {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int W4T = 64;                       // tile rows per workgroup
constexpr int W4C = 64;                       // couts per workgroup
constexpr int W4UNITS = 24;                   // units per stage
constexpr int W4UNIT = W4T * 4;               // floats of a unit image (64 rows x 4 channels): 1 KB
constexpr int W4HALF = W4UNITS * W4UNIT;      // one operand's part of a stage: 6144 floats = 24 KB
constexpr int W4STAGE = 2 * W4HALF;           // 48 KB
constexpr int W4NST = kWino4Stages;           // 96 stages: six passes (transform rows) of 16
constexpr int W4BLOCK = W4NST * W4HALF;       // floats of V per tile block / of U per cout block: 589,824 (2.25 MB)
constexpr int W4CP = 32;                      // couts per epilogue half
constexpr int W4IMG = 16 * W4T * W4CP;        // floats of the half image: 128 KB
static_assert(W4NST == 96 && kC == 256, "pass structure below assumes 64 channel groups");

// where plane (i, j) of 4-channel group c (0..63) lives: pass = transform row i, 16 stages of 4 channel groups x 6 planes
__host__ __device__ __forceinline__ void w4_slot(int i, int j, int c, int& stage, int& unit) {
  stage = i * 16 + (c >> 2);
  unit = (c & 3) * 6 + j;
}
// a unit image row (either operand) is the unit's 4 channels as two pairs, pair h at slot (h + (row >> 4)) & 1: rows r and
// r + 16 start on the same bank and take different slots, so the 32-row ds_read_b64 of the K loop is conflict-free, and a
// producer whose lane is the row writes whole 16-byte rows (agz_wino.hip's V layout; here for U as well)
__host__ __device__ __forceinline__ int w4_off(int row, int h) { return row * 4 + 2 * ((h + (row >> 4)) & 1); }
// U image row r of a cout block -> cout within the block.  The transposed accumulators give lane (l31, hi) of wave wn the
// couts i = (e & 3) + 8 (e >> 2) + 4 hi, e = register; registers 0..7 (i < 16) are epilogue half 0, 8..15 half 1.  Mapping
// i -> (i >> 4) * 32 + wn * 16 + (i & 15) makes each half 32 CONSECUTIVE couts (128-byte runs of y, 8 channel groups of
// the next layer's K loop).
__host__ __device__ __forceinline__ int w4_cout_of_urow(int r) { return (((r & 31) >> 4) << 5) + ((r >> 5) << 4) + (r & 15); }

// Tile geometry, T = ceil(N / 4) tiles per side.  Tiles are numbered board by board (tile = board * T*T + ti * T + tj) and
// a block holds consecutive tiles, so a tile's neighbours (ti + di, tj + dj) are rows row + di T + dj of its block -- if
// they are in its block.  Three packings:
//   * whole boards per 64-row block when they pack with <= 10 % waste (T*T = 16, N = 13..16: 4 boards per block);
//   * T*T = 25 (N = 17..19): FIVE boards in TWO blocks (64 + 61 rows, 3 dead rows in 128: 2.3 %), so that only one of two
//     block boundaries cuts a board -- half the tiles whose patch straddles a boundary, half the fix-up transform;
//   * otherwise dense: block tb starts at tile 64 tb.
__host__ __device__ inline int w4_rows_per_block(int T) {      // whole-board packing: rows that carry tiles; else 64
  const int tt = T * T;
  const int whole = (W4T / tt) * tt;
  return (tt <= W4T && whole * 10 >= W4T * 9) ? whole : W4T;
}
__host__ __device__ inline bool w4_whole_boards(int T) { return w4_rows_per_block(T) % (T * T) == 0 && T * T <= W4T; }
__host__ __device__ __forceinline__ bool w4_paired(int T) { return T * T == 25; }
// first tile of block tb / rows of it that can carry tiles
__host__ __device__ __forceinline__ long w4_block_base(int T, int tb) {
  return w4_paired(T) ? (long)(tb >> 1) * 125 + (tb & 1) * W4T : (long)tb * w4_rows_per_block(T);
}
__host__ __device__ __forceinline__ int w4_block_rows(int T, int tb) {
  return w4_paired(T) ? ((tb & 1) ? 125 - W4T : W4T) : w4_rows_per_block(T);
}
// dense blocks: is the 6x6 input patch of tile (ti, tj) in row `row` made of tiles of the same block?  (its neighbours
// (ti + di, tj + dj) are rows row + di T + dj)
__host__ __device__ __forceinline__ bool w4_tile_fused(int T, int row, int ti, int tj) {
  const int lo = (ti > 0 ? T : 0) + (tj > 0 ? 1 : 0), hi = (ti < T - 1 ? T : 0) + (tj < T - 1 ? 1 : 0);
  return row - lo >= 0 && row + hi < W4T;
}

// ------------------------------------------------------------------ B^T x, six values
// ONE arithmetic for both producers of V (k_wino4_in: scalars; the GEMM epilogue: channel pairs), every multiply-add
// an explicit fma: with dense tile blocks a tile is transformed by one or the other depending on its batch row, and a
// network output must not depend on the batch row (tree parity rests on it).
template <typename V>
__device__ __forceinline__ V w4_fma(float c, V a, V b) {
  if constexpr (std::is_same<V, float>::value) return __builtin_fmaf(c, a, b);
  else return __builtin_elementwise_fma((V){c, c}, a, b);
}
template <typename V>
__device__ __forceinline__ void bt6(V x0, V x1, V x2, V x3, V x4, V x5, V* r) {
  const V a = w4_fma<V>(-4.f, x2, x4), b = w4_fma<V>(-4.f, x1, x3);
  const V c = x4 - x2, d = x3 - x1;
  r[1] = a + b;
  r[2] = a - b;
  r[3] = w4_fma<V>(2.f, d, c);
  r[4] = w4_fma<V>(-2.f, d, c);
  r[0] = w4_fma<V>(4.f, x0, w4_fma<V>(-5.f, x2, x4));
  r[5] = w4_fma<V>(4.f, x1, w4_fma<V>(-5.f, x3, x5));
}

// ------------------------------------------------------------------ input transform (first layer; block ends)
// x[M][256] -> V stage images.  Full form: grid = 2 x tile blocks (32-tile halves); 256 threads = 32 tiles x 8 lanes (a
// lane = one channel pair of one of 4 channel groups): the eight lanes of a tile read one 64-byte run of every patch
// point.  A pass covers 16 channels; the 36 transformed planes go to an LDS copy of this half-block's part of their unit
// images and leave for HBM as whole 512-byte runs, 16 B per lane.
// FIXUP (dense tile blocks only): only the tiles the previous layer's GEMM epilogue could not emit (!w4_tile_fused).
// Those are at most T + 1 <= 8 rows at either end of a block, so the grid is again 2 x tile blocks, but a workgroup
// takes EIGHT rows (0..7 or 56..63) x 32 lanes (16 channel groups): 4 passes of 64 channels instead of 16 of 16 over
// 32 mostly idle tiles (the first form of this kernel: 0.30 ms per layer, a tenth of it); whole 128-byte lines are written.
template <bool FIXUP>
__global__ __launch_bounds__(256) void k_wino4_in(const float* __restrict__ x, float* __restrict__ vimg,
                                                  const int* __restrict__ d_count, int N, int T, int tb0, int tb1) {
  constexpr int TPB = FIXUP ? 8 : 32;            // tile rows per workgroup
  constexpr int LPT = 256 / TPB;                 // lanes per tile: 8 / 32
  constexpr int GP = LPT / 2;                    // channel groups per pass: 4 / 16
  constexpr int CH = TPB * 4;                    // floats per chunk: this workgroup's rows of one unit
  constexpr int IMG = 36 * CH + 8;               // stride between the groups' copies (+8: bank skew of the 8-byte writes)
  __shared__ __attribute__((aligned(16))) float img[GP * IMG];
  const int P = N * N, TT = T * T;
  const long Mt = (long)(*d_count) * TT;
  const int tb = tb0 + (int)(blockIdx.x >> 1), part = blockIdx.x & 1;      // tile blocks [tb0, tb1) of the batch
  if (tb >= tb1) return;
  const int RPB = w4_block_rows(T, tb);
  const long tbase = w4_block_base(T, tb);
  const int row0 = FIXUP ? part * (W4T - TPB) : part * TPB;      // first row of this workgroup
  if (tbase + row0 >= Mt) return;
  const int hs = threadIdx.x % LPT, h = hs & 1, sl = hs >> 1;
  const int tl = threadIdx.x / LPT;
  const int row = row0 + tl;
  const long tile = tbase + row;
  bool live = row < RPB && tile < Mt;
  // (tile numbers fit 32 bits: the launcher checks; a 64-bit division is ~120 instructions)
  const int b = live ? (int)((unsigned)tile / (unsigned)TT) : 0, t = live ? (int)((unsigned)tile % (unsigned)TT) : 0;
  const int ti = t / T, tj = t % T;
  // FIXUP: nothing to do if every tile of these eight rows got its V from the GEMM epilogue (paired packing: a block
  // that starts or ends on a board boundary has nothing to fix at that end).  Otherwise ALL eight rows are transformed
  // and stored -- the rows in place get the same bits again (one arithmetic, bt6) -- so that the stores are whole
  // 128-byte lines: with the rows in place masked out they were 96-byte pieces and L2 fetched every line to merge them.
  if (FIXUP && !__syncthreads_or(live && !w4_tile_fused(T, row, ti, tj))) return;
  // patch point (u, v) = board point (4 ti - 1 + u, 4 tj - 1 + v): one base + a wave-uniform step; off the board (or a
  // lane without a tile) -> -1.  Straight-line selects: the 36 x 4 branches hipcc makes of the obvious form were a third
  // of the fix-up's instructions.
  int off[36];
  {
    const int pi0 = 4 * ti - 1, pj0 = 4 * tj - 1;
    const int base = (b * P + pi0 + N * pj0) * kC;                         // < 2^31 (checked by the launcher)
#pragma unroll
    for (int u = 0; u < 6; ++u) {
      const bool oku = live & ((unsigned)(pi0 + u) < (unsigned)N);
#pragma unroll
      for (int v = 0; v < 6; ++v) {
        const bool ok = oku & ((unsigned)(pj0 + v) < (unsigned)N);
        off[u * 6 + v] = ok ? base + (u + N * v) * kC : -1;
      }
    }
  }
  float* mine = img + sl * IMG + tl * 4 + 2 * ((h + (row >> 4)) & 1);
  float* gdst = vimg + (long)tb * W4BLOCK + row0 * 4;
  constexpr int CPR = 256 / TPB;                                           // chunks copied out per round
  const int cq = threadIdx.x / TPB, cl = threadIdx.x % TPB;
  for (int pass = 0; pass < (kC / 4) / GP; ++pass) {
    const int ch = (pass * GP + sl) * 4 + 2 * h;
    f32x2 d[36];
#pragma unroll
    for (int q = 0; q < 36; ++q) {
      // every lane loads (an off-board point reads x[ch]: in bounds, discarded): 36 loads in flight, no branch per load
      const f32x2 got = *reinterpret_cast<const f32x2*>(x + (off[q] >= 0 ? off[q] : 0) + ch);
      d[q] = off[q] >= 0 ? got : (f32x2){0.f, 0.f};
    }
    f32x2 tx[36];
#pragma unroll
    for (int v = 0; v < 6; ++v) {
      f32x2 r[6];
      bt6<f32x2>(d[0 * 6 + v], d[1 * 6 + v], d[2 * 6 + v], d[3 * 6 + v], d[4 * 6 + v], d[5 * 6 + v], r);
#pragma unroll
      for (int i = 0; i < 6; ++i) tx[i * 6 + v] = r[i];
    }
    if (pass) __syncthreads();                     // the previous pass has left the LDS image
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      f32x2 r[6];
      bt6<f32x2>(tx[i * 6 + 0], tx[i * 6 + 1], tx[i * 6 + 2], tx[i * 6 + 3], tx[i * 6 + 4], tx[i * 6 + 5], r);
#pragma unroll
      for (int j = 0; j < 6; ++j) *reinterpret_cast<f32x2*>(mine + (i * 6 + j) * CH) = r[j];
    }
    __syncthreads();
    static_assert((GP * 36) % CPR == 0, "whole copy-out rounds");
#pragma unroll
    for (int r = 0; r < GP * 36 / CPR; ++r) {
      const int c = r * CPR + cq, s4 = c / 36, pl = c - s4 * 36;          // chunk c = (group s4 of this pass, plane pl)
      const f32x4 v = *reinterpret_cast<const f32x4*>(img + s4 * IMG + pl * CH + cl * 4);
      int stage, unit;
      w4_slot(pl / 6, pl % 6, pass * GP + s4, stage, unit);
      f32x4* gp = reinterpret_cast<f32x4*>(gdst + (long)stage * W4HALF + unit * W4UNIT + cl * 4);
      // FIXUP: 128-byte pieces 1 KB apart -- as plain stores they merge in L2 and leave with the kernel's write-back
      // (0.155 -> 0.12 ms per layer at 2048 boards of 19x19 against the streaming form)
      if (FIXUP) { *gp = v; continue; }
      __builtin_nontemporal_store(v, gp);
    }
  }
}

// ------------------------------------------------------------------ GEMM in six one-row passes + output transform + next input transform

// A^T m for one transform row: six planes -> four values, on register PAIRS (elements 2 q, 2 q + 1 of the accumulator
// tuples).  The running outputs are 128 independent pairs, not sixteen 16-register tuples: tuples need 16 consecutive
// registers each, the file fragments, and hipcc parks whole tuples in scratch -- whose reloads wait, through vmcnt(0),
// for every LDS-DMA piece in flight (the first form of the folds: 0.7 ms per layer, 60 cycles per instruction).
__device__ __forceinline__ void w4_fold_row(const f32x2 m0, const f32x2 m1, const f32x2 m2, const f32x2 m3, const f32x2 m4,
                                            const f32x2 m5, f32x2* t) {
  const f32x2 s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
  t[0] = (m0 + s12) + s34;
  t[1] = d12 + 2.f * d34;
  t[2] = s12 + 4.f * s34;
  t[3] = (d12 + 8.f * d34) + m5;
}


// MODE bit 0: write y (affine, residual, ReLU applied); bit 1: emit the next layer's V stage images; bit 2: add the residual.
// (The timing variants of round 4 -- results WRONG -- and the wall-clock stamps: tools/experiments/agz_wino4_variants.hip,
// which tools/build_timing_lib.sh compiles in place of this file.)
//
// Code size is a design constraint here: the first form of this kernel (each pass's first stage and the two tail stages
// peeled, the epilogue's halves as two copies: 65 KB of code) ran its straight-line sections -- folds, epilogue -- at
// ~35 cycles per instruction, the K-loop bodies (1.7 KB each, resident) at full speed: the instruction cache (64 KB per CU
// pair) does not hold a kernel of that size between a workgroup's visits.  So: every stage of a pass is the same loop
// body (accumulators zeroed in front of a pass, the DMA of the last two stages wraps around to stages 0 and 1 and is
// thrown away), passes C and D are one loop, and the epilogue's second half runs the first half's code after moving the
// upper register quads down.
template <int MODE>
__global__ __launch_bounds__(256, 1) void k_wino4_gemm(
    const float* __restrict__ vimg, const float* __restrict__ uimg, const float* __restrict__ scale,
    const float* __restrict__ shift, const float* __restrict__ res, float* __restrict__ y,
    float* __restrict__ vnext, const int* __restrict__ d_count, int N, int T, int relu, int tb0, int tb1y) {
  __shared__ __attribute__((aligned(256))) float lds[3 * W4STAGE];      // 144 KB: stage buffers, then the half image
  __shared__ int ptab[W4T * 16];            // element offset of output point X = k * 64 + row in y / res, or -1
  __shared__ __attribute__((aligned(256))) float zeros[64];      // what phase 2 reads for a patch point off the board
  constexpr bool RES = (MODE & 4) != 0;
  const int P = N * N, TT = T * T;
  const long Mt = (long)(*d_count) * TT;
  // workgroup -> (tile block, cout block): the four cout blocks of a tile block are four consecutive workgroups of one
  // XCD (block b runs on XCD b % 8), so its V slab comes out of HBM once (agz_wino.hip's placement)
  const int bid = blockIdx.x;
  const int xcd = bid & 7, jb = bid >> 3;
  const int cb = jb & 3;
  // (bit 30 of the last argument: y is wanted only where the fix-up transform reads it -- see the point table)
  const int tb1 = tb1y & 0x3fffffff, ypart = tb1y >> 30;
  const int tb = tb0 + xcd + 8 * (jb >> 2);      // this launch covers tile blocks [tb0, tb1) of the batch
  if (tb >= tb1) return;
  const int RPB = w4_block_rows(T, tb);
  const long tbase = w4_block_base(T, tb);
  if (tbase >= Mt) return;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int l31 = lane & 31, hi = lane >> 5;

  const float* asrc = vimg + (long)tb * W4BLOCK;
  const float* bsrc = uimg + (long)cb * W4BLOCK;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float*)&lds[0];

  // a stage is 48 pieces of 1 KB: 0..23 V units, 24..47 U units; wave w moves pieces 12 w .. 12 w + 11 (waves 0, 1: V;
  // 2, 3: U), wave-uniform base in SGPRs + a 32-bit lane offset
  const float* wsrc = (wave < 2 ? asrc : bsrc - 24 * W4UNIT) + 12 * wave * W4UNIT;
  auto dma = [&](int st, int buf, int j) {
    const int c = 12 * wave + j;
    glds16s(wsrc + (long)st * W4HALF + j * W4UNIT, (unsigned)lane * 16u, lds0 + (unsigned)(buf * W4STAGE + c * W4UNIT) * 4u);
  };
#pragma unroll
  for (int j = 0; j < 12; ++j) dma(0, 0, j);

  if (tid < 64) zeros[tid] = 0.f;
  // ypart (conv1 of a block with paired packing: y is read by the fix-up transform only): the eight rows at the pair's board
  // cut and the T + 1 rows of neighbours on either side -- rows 50.. of the even block, ..13 of the odd one
  const int yrow0 = ypart && !(tb & 1) ? 50 : 0, yrows = (ypart && (tb & 1) ? 14 : RPB) - yrow0;
  for (int idx = tid; idx < W4T * 16; idx += 256) {     // (published by the barrier in front of the first operand reads)
    const int row = idx & (W4T - 1), k = idx >> 6;
    const long tile = tbase + row;
    int off = -1;
    if ((unsigned)(row - yrow0) < (unsigned)yrows && tile < Mt) {
      const unsigned tile32 = (unsigned)tile, b = tile32 / (unsigned)TT, t = tile32 - b * (unsigned)TT;
      const unsigned ti = t / (unsigned)T;
      const int pi = (int)(4 * ti) + (k >> 2), pj = (int)(4 * (t - ti * T)) + (k & 3);
      if (pi < N && pj < N) off = ((int)b * P + pi + N * pj) * kC + cb * W4C;
    }
    ptab[idx] = off;
  }
#pragma unroll
  for (int j = 0; j < 12; ++j) dma(1, 1, j);
  f32x16 acc[6];
  const int arow = wm * 32 + l31, brow = wn * 32 + l31;
  const int aoff = w4_off(arow, hi), boff = W4HALF + w4_off(brow, hi);
#ifndef W4_LA
#define W4_LA 5
#endif
  constexpr int LA = W4_LA, RING = LA + 1;       // 24 % RING == 0: ring slots are compile-time within a stage
  static_assert(W4UNITS % RING == 0, "ring slots must be compile-time within a stage");
  float2 ra[RING], rb[RING];
  auto load = [&](const float* L, int u, float2& a, float2& b) {
    a = *reinterpret_cast<const float2*>(L + aoff + u * W4UNIT);
    b = *reinterpret_cast<const float2*>(L + boff + u * W4UNIT);
  };
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // transposed: srcA = U (its rows become D's rows = registers: couts), srcB = V (D's columns = lanes: tile rows)
  auto mma = [&](int p, const float2& a, const float2& b) {
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(b.x, a.x, acc[p], 0, 0, 0);
    acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(b.y, a.y, acc[p], 0, 0, 0);
  };

  asm volatile("s_waitcnt vmcnt(12)" ::: "memory");      // stage 0 has landed (stage 1's 12 pieces may be in flight)
  __syncthreads();
#pragma unroll
  for (int u = 0; u < RING; ++u) ra[u] = rb[u] = make_float2(1.f, 0.5f);
#pragma unroll
  for (int u = 0; u < LA; ++u) load(lds, u, ra[u], rb[u]);

  // One stage: 24 units = 4 channel groups x the pass's 6 planes (unit u = group * 6 + plane).  Every stage fetches stage
  // st + 2 (the last two wrap around to stages 0 and 1: valid memory, never read) and hands over to stage st + 1 through
  // the barrier in its read stream -- one loop body for the whole kernel.
  int buf = 0;
  auto stage = [&](int st) {
    constexpr int PL = 6;
    const int nbuf = buf == 2 ? 0 : buf + 1;
    const int dbuf = buf == 0 ? 2 : buf - 1;
    const int st2 = st + 2 >= W4NST ? st + 2 - W4NST : st + 2;
    const float* L = lds + buf * W4STAGE;
    const float* Ln = lds + nbuf * W4STAGE;
#pragma unroll
    for (int u = 0; u < W4UNITS; ++u) {
      const int t = u + LA;
      if (t == W4UNITS) {
        // everything this wave owes to stage st + 1 has landed (its 12 pieces of stage st + 2, all issued by now, may be
        // in flight); hipcc adds lgkmcnt(0) in front of the barrier: all reads of stage st are back
        asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        __syncthreads();
      }
      if (t < W4UNITS) load(L, t, ra[t % RING], rb[t % RING]);
      else load(Ln, t - W4UNITS, ra[t % RING], rb[t % RING]);
      // (one unit's reads at a time: left alone, hipcc merges the reads of two units into ds_read2st64_b64, which the LDS
      // serves in 16-lane groups over 32 banks -- 2-way conflicts on this layout, 16 cycles for what two ds_read_b64 do
      // in 4; SQ_LDS_BANK_CONFLICT 0.37 of the LDS cycles, -2.8 % per layer without them, same box)
      __builtin_amdgcn_sched_barrier(0);
      constexpr int D0 = 6;
      if (u >= D0 && u < D0 + 12) {
        __builtin_amdgcn_sched_barrier(0);
        dma(st2, dbuf, u - D0);
        __builtin_amdgcn_sched_barrier(0);
      }
      mma(u % PL, ra[u % RING], rb[u % RING]);
    }
    buf = nbuf;
  };

  // Y[4 i' + j'][q] = elements 2 q, 2 q + 1 (the C/D map's registers) of output point (i', j'); complete after the last pass
  f32x2 Y[16][8];
#pragma unroll
  for (int k = 0; k < 16; ++k)
#pragma unroll
    for (int q = 0; q < 8; ++q) Y[k][q] = (f32x2){0.f, 0.f};
  auto pair_of = [&](int p, int q) { return (f32x2){acc[p][2 * q], acc[p][2 * q + 1]}; };
  // Six passes, one per transform row i: the K loop over that row's six planes, then Y[i'][:] += A^T[i'][i] (A^T M[i][:]).
  // ONE loop body and ONE fold for the whole kernel; the row's weights A^T[0..3][i] are run-time scalars (exact: 0, +-1,
  // +-2, 4, +-8).  96 accumulator registers beside the 256 of Y: nothing of either ever leaves the register file.
#pragma unroll 1
  for (int pass = 0; pass < 6; ++pass) {
#pragma unroll
    for (int p = 0; p < 6; ++p) acc[p] = zero16;
#pragma unroll 1
    for (int st = 0; st < 16; ++st) stage(16 * pass + st);
    //            i =  0   1   2   3   4   5
    // A^T[0][i]      1   1   1   1   1   0
    // A^T[1][i]      0   1  -1   2  -2   0
    // A^T[2][i]      0   1   1   4   4   0
    // A^T[3][i]      0   1  -1   8  -8   1
    const float sgn = (pass & 1) ? 1.f : -1.f, mid = (pass >= 1 && pass <= 4) ? 1.f : 0.f, big = pass >= 3 ? 1.f : 0.f;
    const float w0 = pass == 5 ? 0.f : 1.f;
    const float w1 = mid * sgn * (1.f + big);              // 0 1 -1 2 -2 0
    const float w2 = mid * (1.f + 3.f * big);              // 0 1 1 4 4 0
    const float w3 = pass == 5 ? 1.f : mid * sgn * (1.f + 7.f * big);      // 0 1 -1 8 -8 1
    const f32x2 wv[4] = {{w0, w0}, {w1, w1}, {w2, w2}, {w3, w3}};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      f32x2 t[4];
      w4_fold_row(pair_of(0, q), pair_of(1, q), pair_of(2, q), pair_of(3, q), pair_of(4, q), pair_of(5, q), t);
#pragma unroll
      for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          Y[4 * ii + jj][q] = __builtin_elementwise_fma(wv[ii], t[jj], Y[4 * ii + jj][q]);
          // pin the fold here: hipcc otherwise sinks it towards the epilogue and keeps every pass's accumulators alive
          asm volatile("" : "+v"(Y[4 * ii + jj][q]));
        }
      __builtin_amdgcn_sched_barrier(0);       // a pair at a time: interleaved, their temporaries crowd out the outputs
    }
  }

  // Everything the epilogue derives from the thread id or from its pointer arguments is derived HERE, from opaque copies:
  // left to itself hipcc hoists that arithmetic (and the affine's loads) above the K loops, keeps ~60 registers of it alive
  // through them and parks running outputs in scratch to make room -- and a scratch reload is an s_waitcnt vmcnt(0), which
  // waits for every LDS-DMA piece in flight.
  int tid_e = tid;
  asm volatile("" : "+v"(tid_e));
  const float *scale_e = scale, *shift_e = shift, *res_e = res;
  float *y_e = y, *vnext_e = vnext;
  asm volatile("" : "+s"(scale_e), "+s"(shift_e), "+s"(res_e), "+s"(y_e), "+s"(vnext_e));
  const int lane_e = tid_e & 63;
  const int wave_e = __builtin_amdgcn_readfirstlane(tid_e >> 6);
  const int wm_e = wave_e & 1, wn_e = wave_e >> 1;
  const int l31_e = lane_e & 31, hi_e = lane_e >> 5;
  // ---- epilogue, once per half of the 64 couts (registers 8 hh .. 8 hh + 7 of every tuple = couts 32 hh .. 32 hh + 31).
  // Half image img[X][8 units of 16 B], X = k * 64 + tile row; unit u of row X sits at slot u ^ ((X >> 1) & 7): the 16
  // lanes of a ds_read_b128 group (consecutive rows) then cover 64 banks once, and an LDS-DMA instruction fills eight
  // rows (1 KB), each lane_e choosing the global 16 B that belong in its slot.
  float* img = lds;
  const int trow = wm_e * 32 + l31_e;                       // this lane_e's tile row
  float sc[16], sh[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int i = (e & 3) + 8 * (e >> 2) + 4 * hi_e;
    const int co = cb * W4C + (i >> 4) * 32 + wn_e * 16 + (i & 15);
    sc[e] = scale_e[co];
    sh[e] = shift_e[co];
  }
  const float relu_lo = relu ? 0.f : -3.0e38f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the wrapped-around DMA of the last two stages included)
  __syncthreads();                                       // every wave_e has left the K loop: the stage buffers are dead

#pragma unroll 1
  for (int hh = 0; hh < 2; ++hh) {
    if (RES) {
      // instruction n of wave_e w fills image rows 8 (w + 4 n) .. + 7: lane_e = (row X, slot s) fetches unit s ^ ((X >> 1) & 7)
#pragma unroll 4
      for (int n = 0; n < 32; ++n) {
        const int i = wave_e + 4 * n;
        const int Xp = 8 * i + (lane_e >> 3), u = (lane_e & 7) ^ ((Xp >> 1) & 7);
        const int off = ptab[Xp];
        const unsigned boff = off >= 0 ? 4u * (unsigned)(off + hh * W4CP + 4 * u) : 0u;
        glds16s(res_e, boff, lds0 + (unsigned)(i * 256) * 4u);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the residual half-tile has landed, for every wave_e
      __syncthreads();
    }
    // img = ReLU(img (the residual) + scale_e * value + shift_e): the lane_e's two register quads of this half (registers
    // 0..7: the second half's were moved down) for each of the 16 output points; unit wn_e * 4 + 2 qd + hi_e of row X = k * 64 + trow
    {
      const unsigned rowb = lds0 + 4u * (unsigned)(trow * W4CP);
      const int swz = (trow >> 1) & 7;                   // (X >> 1) & 7 = (trow >> 1) & 7: k * 64 does not reach bits 1..3
      const unsigned a0 = rowb + 16u * (unsigned)((wn_e * 4 + hi_e) ^ swz), a1 = rowb + 16u * (unsigned)((wn_e * 4 + 2 + hi_e) ^ swz);
#pragma unroll
      for (int k0 = 0; k0 < 16; k0 += 4) {
        f32x4 rr[4][2];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const unsigned kb = 4u * (unsigned)((k0 + kk) * W4T * W4CP);
          if (RES) {
            rr[kk][0] = *(const __attribute__((address_space(3))) f32x4*)(size_t)(a0 + kb);
            rr[kk][1] = *(const __attribute__((address_space(3))) f32x4*)(size_t)(a1 + kb);
          } else {
            rr[kk][0] = rr[kk][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
          }
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const unsigned kb = 4u * (unsigned)((k0 + kk) * W4T * W4CP);
#pragma unroll
          for (int qd = 0; qd < 2; ++qd) {
            f32x4 v;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const int e = 4 * qd + c;
              v[c] = fmaxf(__builtin_fmaf(Y[k0 + kk][e >> 1][e & 1], sc[e], sh[e]) + rr[kk][qd][c], relu_lo);
            }
            *(__attribute__((address_space(3))) f32x4*)(size_t)((qd ? a1 : a0) + kb) = v;
          }
        }
      }
    }
    __syncthreads();

    if (MODE & 1) {
      // image -> y_e: 8 consecutive lanes cover the 128 contiguous bytes of one output point's half; thread tid_e handles
      // points X = (tid_e >> 3) + 32 i, always slot tid_e & 7 = unit (tid_e & 7) ^ ((tid_e >> 4) & 7) (32 i does not reach bits 1..3)
      const int cg4 = hh * W4CP + 4 * ((tid_e & 7) ^ ((tid_e >> 4) & 7));
      const f32x4* ip0 = reinterpret_cast<const f32x4*>(img) + tid_e;
      const int* pt0 = ptab + (tid_e >> 3);
#pragma unroll 1
      for (int i0 = 0; i0 < 32; i0 += 8) {
        f32x4 v[8];
        int offs[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          v[j] = ip0[256 * (i0 + j)];
          offs[j] = pt0[32 * (i0 + j)];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (offs[j] >= 0) *reinterpret_cast<f32x4*>(y_e + offs[j] + cg4) = v[j];
      }
    }
    if (MODE & 2) {
      // ---- the next layer's input transform for this half's 32 channels = 8 channel groups (groups cb * 16 + hh * 8 + g
      // of the next layer's 64).  Task = (tile row, group): lane_e = row, wave_e w takes groups w and w + 4.
      const int row = lane_e;
      const long tile = tbase + row;
      const bool live = row < RPB && tile < Mt;
      const int t = live ? (int)(tile % TT) : 0;
      const int ti = t / T, tj = t % T;
      const bool emit = w4_whole_boards(T) || (live && w4_tile_fused(T, row, ti, tj));
      // Patch point (u, v) of tile (ti, tj) is board point (4 ti - 1 + u, 4 tj - 1 + v): output (ku, kv) of the tile du
      // tile rows / dv tiles further on, (du, ku) = (-1, 3), (0, 0..3), (1, 0) for u = 0..5.  A point off the board (or a
      // lane_e that emits nothing) reads a block of zeros instead of being masked out.  adr[q]: LDS byte address of the
      // point's unit for group `wave_e` (+ the lane_e's pair order: rows with bit 4 set store pair 1 first, so they read it
      // first); group wave_e + 4 is the same address with bit 6 flipped (slot ^ 4) -- also inside the 256-byte zeros block.
      unsigned adr[36];
      const unsigned zadr = (unsigned)(size_t)(__attribute__((address_space(3))) float*)&zeros[0];
#pragma unroll
      for (int u = 0; u < 6; ++u)
#pragma unroll
        for (int v = 0; v < 6; ++v) {
          const int du = u == 0 ? -1 : (u == 5 ? 1 : 0), ku = u == 0 ? 3 : (u == 5 ? 0 : u - 1);
          const int dv = v == 0 ? -1 : (v == 5 ? 1 : 0), kv = v == 0 ? 3 : (v == 5 ? 0 : v - 1);
          const int pi = 4 * ti - 1 + u, pj = 4 * tj - 1 + v;
          const bool ok = live && emit && pi >= 0 && pi < N && pj >= 0 && pj < N;
          const int Xq = (ku * 4 + kv) * W4T + row + du * T + dv;
          adr[u * 6 + v] = ok ? lds0 + 4u * (unsigned)(Xq * W4CP + 4 * (wave_e ^ ((Xq >> 1) & 7)) + 2 * ((row >> 4) & 1)) : zadr;
        }
#pragma unroll 1
      for (int it = 0; it < 2; ++it) {
        const int g = wave_e + 4 * it;
        const unsigned xo = (unsigned)it << 6;
        const int c = cb * 16 + hh * 8 + g;               // the next layer's channel group
        float* gbase = vnext_e + (long)tb * W4BLOCK + row * 4;
        // one channel pair at a time (the lane_e's first pair in ITS row's order, then the second: the reads' ^ 8), so that
        // the 36 patch values, their half-transformed form and one pair's results are all that is live beside the outputs
        f32x2 vv[36][2];
#pragma unroll
        for (int hp = 0; hp < 2; ++hp) {
          f32x2 d[36];
#pragma unroll
          for (int q = 0; q < 36; ++q)
            d[q] = *(const __attribute__((address_space(3))) f32x2*)(size_t)((adr[q] ^ xo) ^ (hp ? 8u : 0u));
          f32x2 tx[36];
#pragma unroll
          for (int v = 0; v < 6; ++v) {
            f32x2 r[6];
            bt6<f32x2>(d[0 * 6 + v], d[1 * 6 + v], d[2 * 6 + v], d[3 * 6 + v], d[4 * 6 + v], d[5 * 6 + v], r);
#pragma unroll
            for (int i = 0; i < 6; ++i) tx[i * 6 + v] = r[i];
          }
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            f32x2 r[6];
            bt6<f32x2>(tx[i * 6 + 0], tx[i * 6 + 1], tx[i * 6 + 2], tx[i * 6 + 3], tx[i * 6 + 4], tx[i * 6 + 5], r);
#pragma unroll
            for (int j = 0; j < 6; ++j) vv[i * 6 + j][hp] = r[j];
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        // (plane (i, j) of channel group c: stage 16 i + (c >> 2), unit (c & 3) * 6 + j)
        const int cbase = (c >> 2) * W4HALF + (c & 3) * 6 * W4UNIT;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            const int o = cbase + i * 16 * W4HALF + j * W4UNIT;
            const f32x2 p0 = vv[i * 6 + j][0], p1 = vv[i * 6 + j][1];
            const f32x4 v4 = {p0[0], p0[1], p1[0], p1[1]};      // (already in the row's pair order: see the reads above)
            f32x4* gp = reinterpret_cast<f32x4*>(gbase + o);
            if (emit) __builtin_nontemporal_store(v4, gp);
          }
      }
    }
    if (hh == 0) {
      // the second half runs this same code: its registers (8..15 of every tuple, and of the affine) move down
#pragma unroll
      for (int k = 0; k < 16; ++k)
#pragma unroll
        for (int q = 0; q < 4; ++q) Y[k][q] = Y[k][4 + q];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        sc[e] = sc[8 + e];
        sh[e] = sh[8 + e];
      }
      // every wave has left the image: the second half may overwrite it.  (No vmcnt wait here: the first half's stores
      // read registers, not the image, and drain under the second half's residual DMA, whose own wait is vmcnt(0).)
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------ host side

// Flux [kw,kh,cin,cout] column-major -> U stage images [cout block 4][stage 96][unit 24][row 64][4], U = G k G^T (agz_pack.h).
// One unit = one (cout, cin) pair; every word of an image is written.
struct Wino4Image : ImageDefaults {
  using word = float;
  static constexpr const char* name = "F(4x4,3x3)";
  static constexpr bool tower_only = true;
  __host__ __device__ static size_t words(int) { return (size_t)(kC / W4C) * W4BLOCK; }
  __host__ __device__ static long units(int, int) { return (long)kC * kC; }
  __host__ __device__ static void put(const float* w, int, long unit, int, float* out) {
    const int o = (int)(unit / kC), ci = (int)(unit % kC);
    int r = 0;                                          // the U row that holds this cout: the inverse of w4_cout_of_urow
    for (int q = 0; q < W4C; ++q)
      if (w4_cout_of_urow(q) == o % W4C) r = q;
    const int cb = o / W4C, cg = ci / 4, cl = ci % 4;
    winograd_u<6>(w, kC, o, ci, [&](int i, int j, double u) {
      int stage, unit4;
      w4_slot(i, j, cg, stage, unit4);
      out[(size_t)cb * W4BLOCK + (size_t)stage * W4HALF + (size_t)unit4 * W4UNIT + w4_off(r, cl >> 1) + (cl & 1)] = (float)u;
    });
  }
};
const ImageFamily kWino4Image = image_family<Wino4Image>();

static long wino4_blocks(int bcap, int T) {
  if (w4_paired(T)) {      // five boards per block pair; the last pair's second block exists only if it has a tile
    const long pairs = bcap / 5, rest = (long)(bcap % 5) * 25;
    return 2 * pairs + (rest > W4T ? 2 : rest > 0 ? 1 : 0);
  }
  const long rpb = w4_rows_per_block(T);
  return ((long)bcap * T * T + rpb - 1) / rpb;
}
size_t wino4_v_floats(int bcap, int N) { return (size_t)wino4_blocks(bcap, (N + 3) / 4) * W4BLOCK; }
bool wino4_whole_boards(int N) { return w4_whole_boards((N + 3) / 4); }
bool wino4_paired(int N) { return w4_paired((N + 3) / 4); }
// multiplies per output point: F(4x4,3x3) against F(3x3,3x3); the larger tile pays from 13x13 up
bool wino4_applies(int N) { return N >= 13; }

void wino4_validate(int bcap, int N) { wino_check_32bit(wino4_blocks(bcap, (N + 3) / 4), W4T, bcap, N); }

// part / parts: this launch covers the part-th of `parts` equal ranges of tile blocks (cut at block-pair boundaries, so that
// no board straddles two ranges: a range's layers depend on nothing outside it, and ranges can run on different streams).
// An even block index is a board boundary only with whole-board (N = 13..16) or paired (N = 17..19) packing: dense
// non-paired packing (T >= 6) must run as one range (unreachable while board_size <= 19).
static void wino4_range(int blocks, int part, int parts, int& tb0, int& tb1, int T) {
  wino_block_range(blocks, part, parts, true, tb0, tb1);
  AGZ_REQUIRE(parts == 1 || w4_whole_boards(T) || w4_paired(T), AGZ_BAD_ARGUMENT,
              "F(4x4,3x3): %d layer chains need whole-board or paired tile packing (T = %d packs densely)", parts, T);
}

void launch_wino4_in(const float* x, float* vimg, const int* d_count, int bcap, int N, hipStream_t s, bool fixup, int part, int parts) {
  const int T = (N + 3) / 4;
  int tb0, tb1;
  wino4_range((int)wino4_blocks(bcap, T), part, parts, tb0, tb1, T);
  if (tb1 <= tb0) return;
  wino4_validate(bcap, N);
  if (fixup) {
    AGZ_REQUIRE(!w4_whole_boards(T) && T + 1 <= 8, AGZ_BAD_ARGUMENT, "fix-up transform: dense tile blocks, at most 8 rows at a block's ends");
    hipLaunchKernelGGL((k_wino4_in<true>), dim3(2 * (tb1 - tb0)), dim3(256), 0, s, x, vimg, d_count, N, T, tb0, tb1);
  } else {
    hipLaunchKernelGGL((k_wino4_in<false>), dim3(2 * (tb1 - tb0)), dim3(256), 0, s, x, vimg, d_count, N, T, tb0, tb1);
  }
}

// y == nullptr: the activations are not needed in HBM; vnext == nullptr: no next Winograd layer
void launch_wino4_gemm(const float* vimg, const float* uimg, const float* scale, const float* shift, const float* res,
                       float* y, float* vnext, const int* d_count, int bcap, int N, int relu, hipStream_t s, int part, int parts, bool ypart) {
  const int T = (N + 3) / 4;
  int tb0, tb1;
  wino4_range((int)wino4_blocks(bcap, T), part, parts, tb0, tb1, T);
  if (tb1 <= tb0) return;
  const int blocks = tb1 - tb0;
  const int per_xcd = 4 * ((blocks + 7) / 8);
  const dim3 grid(8 * per_xcd), block(256);
  wino4_validate(bcap, N);
  AGZ_REQUIRE(y || vnext, AGZ_BAD_ARGUMENT, "F(4x4,3x3) GEMM: nothing to write");
  // ypart: y only where the fix-up transform reads it (paired packing, no residual: conv1 of a block) -- bit 30 of the
  // kernel's last argument
  AGZ_REQUIRE(!ypart || (w4_paired(T) && y && !res && tb1 < (1 << 30)), AGZ_BAD_ARGUMENT, "F(4x4,3x3) GEMM: partial y needs paired packing and no residual");
  const int tb1y = tb1 | (ypart ? 1 << 30 : 0);
  dispatch_mode(y, vnext, res, [&](auto mode) {
    hipLaunchKernelGGL((k_wino4_gemm<decltype(mode)::value>), grid, block, 0, s, vimg, uimg, scale, shift, res, y, vnext, d_count, N, T,
                       relu, tb0, tb1y);
  });
}

}  // namespace agz

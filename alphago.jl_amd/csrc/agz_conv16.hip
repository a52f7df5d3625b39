// agz_conv16.hip -- the 3x3 256->256 tower convolution with fp16 operands on
// v_mfma_f32_32x32x16_f16 (f32 accumulate): the "fp16 MFMA path" of BASELINE.json configs[4].
// Opt-in (agz_net_set_precision); the default network is exact f32 (agz_wino.hip).
//
// Implicit GEMM, M = B*N^2 board points, N = 256 couts, K = 9*256 ordered (cin chunk, tap, cin): 144 k-steps of
// 16.  The nine taps come from ONE activation slab per channel chunk: a workgroup owns 224 consecutive rows and
// all 256 output channels, brings the 32-channel slab of its rows plus a halo of N+1 rows on either side into LDS
// once per chunk (LDS-DMA, 64-byte rows, 16-byte pieces swizzled on the source side), and the taps read it at nine
// row offsets; a lane whose neighbour is off the board reads a row of zeros.  Activations are [M][256] half in
// HBM (the f32 stem output is converted once per forward; the last conv writes f32 for the heads; the first
// block's residual is the f32 stem output).
//
// History of the form (all measured at 8192 positions of 9x9, per layer): weights global -> VGPR -> LDS 1.19 ms;
// weights by LDS-DMA, 64 x 128 wave tiles, two workgroups per CU 0.79 ms (round 1; LDS-bound: 0.75 KB of operand
// reads per MFMA plus the DMA writes); the persistent one-wave-per-SIMD form below 0.63-0.66 ms.
// The reduction order of an output is fixed (chunk, tap, k) and does not depend on where its row sits in the
// batch: tree parity with the oracle (which calls this network) stays bit-exact.
//
// What is in this file: THE PRODUCT and nothing else -- k_conv3x3_f16_q<RES> (2 x 2 waves over 256-row x 256-cout tiles) for the
// half-in / half-out layers, k_conv3x3_f16_w2<RES, OUTF> (7 x 2 wave tiles over 224 rows) for the f32-residual and f32-output
// layers, the weight-image and conversion kernels.  No environment variable is read here (tests/test_build_invariants.py).
// The measurement apparatus of rounds 2-5 (timing and measurement variants -- results WRONG --, store policies, pacing, the
// LDS weight ring, register masking, the zero-block form) lives in tools/experiments/agz_conv16_variants.hip, the file this
// one was until round 6; tools/build_timing_lib.sh (ALSO=agz_conv16) compiles it in place of this file, so the tables of
// HISTORY.md 4b / 4h / 12 can still be re-run.
#include "agz_nn.h"
#include "agz_pack.h"

#include <hip/hip_fp16.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace agz {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int HK = 32;             // channels per chunk
constexpr int HCH = kC / HK;       // 8 chunks

// tap reads x[row + da, col + db] with da = tap % 3 - 1, db = tap / 3 - 1 and multiplies Flux's w[a = 1 - da, b = 1 - db]
// (NNlib true convolution: flux_tap, agz_pack.h)

// uniform base in SGPRs + per-lane 32-bit byte offset
__device__ __forceinline__ void glds16hs(const void* gbase_uniform, unsigned lane_byte_off, unsigned lds_byte_addr) {
  unsigned keep;
  lds_byte_addr = __builtin_amdgcn_readfirstlane(lds_byte_addr);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(lane_byte_off), "s"(gbase_uniform), "s"(lds_byte_addr) : "memory");
}


// ---------------------------------------------------------------------------------------------------------
// The kernel: persistent workgroups, one wave per SIMD.
//   * a wave owns 224 rows x 64 couts (7 x 2 accumulator tiles in AGPRs).  Its weight fragments never touch
//     LDS: they are stored in HBM in MFMA operand order, Wf[k-step 144][cout block 8][lane 64][8 halves], so a
//     wave's two fragments of a k-step are one contiguous 2 KB that global_load_dwordx4 brings straight into
//     registers, W2_D k-steps ahead, through a ring of W2_RING register sets.  No wave reads another wave's
//     weights, and LDS carries the activation slab only (two 17 KB buffers, one barrier per channel chunk, placed
//     one k-step before the chunk ends so that no LDS latency is exposed behind it).  A row block's slab fragment
//     of the next k-step is fetched right after the block's two MFMAs, into the same registers.
//   * the accumulators are computed transposed (D = W . X^T: lane = board point, register = cout), so a lane
//     holds four consecutive couts of one row per register quad and the epilogue works on 8-byte groups.
//   * workgroups are persistent (one per CU, tiles blockIdx.x, +gridDim.x, ...): the next tile's first slab and
//     weight fragments are in flight while the epilogue runs; residual pieces are fetched two passes ahead, the
//     first two during the last channel chunk.  The epilogue of a half-in / half-out layer only computes: its
//     results stay in an LDS image (7 passes x 32 rows x 512 bytes, 16-byte pieces swizzled by row; a wave computes
//     into its own 128-byte slice of every row) and leave for HBM two whole rows (1 KB) every fourth k-step of the NEXT
//     tile's loop.  (224 rows, not 256: the image of an eighth pass does not fit beside the slabs.)  The last tile's
//     image is flushed at the end.  Rows past the batch are stored too: the half activation buffers are padded by one tile
//     (Net::reserve).  The f32-residual layer (first block) and the f32-output layer (last) keep a direct
//     epilogue through two small tiles per wave: two layers of twenty.
// What the timing variants and the counters say (tools/c16_x.sh, tools/c16_pmc.sh; 8192 positions of 9x9):
//   cycles per launch (GRBM_GUI_ACTIVE / 8): MFMA floor 747 k; a loop of MFMAs only 841 k (12 tile rounds for 11.6
//   rounds of work, barriers, tile turn-over); + slab operand reads 96 k, + weight loads 50 k, + slab DMA 16 k =
//   995 k for the whole loop; + epilogue 160 k = 1.155 M: MFMA pipe busy 0.65 of the cycles.
//   clock: the same launch runs at 2.2 GHz without its epilogue, 2.1 GHz with the epilogue but without the result
//   stores and 1.77 GHz as it is: 0.65 ms.  The stores cost 4 % in cycles and 23 % in wall time -- the chip is
//   power-limited here (MI355X_MICROARCH.md, DVFS), and every HBM byte is paid in clock.  Everything tried against a
//   supposed "store tail" therefore measured nothing: staggered workgroup starts, a 17-deep weight ring, results
//   trickled through the LDS image instead of stored in a burst, 128-row tiles with two workgroups per CU (0.659 vs
//   0.665 ms), non-temporal stores, whole rows instead of 128-byte segments per store.  (An intermediate form with the weights in LDS -- 128 x 128 wave tiles, 48 KB
//   weight groups by LDS-DMA -- ran its loop in 0.48 ms and 0.38 ms with the DMA compiled out: the DMA writes compete
//   with the operand reads for the LDS port.)  Same lesson from the LDS side: the lanes that read the shared row of
//   zeros make nearly every slab read a 2-way bank conflict (SQ_LDS_BANK_CONFLICT 0.36 of the LDS cycles); giving each
//   lane zeros in the banks of its real address removes them (0.04) -- and the forward got 3 % SLOWER in an A/B on one
//   box (14.15 -> 14.59 ms): fewer cycles, lower clock.  Not kept.
constexpr int W2_RB_PRODUCT = 7;                    // row blocks per tile of the product form (224 rows)
constexpr int W2_KS = HCH * 18;                     // k-steps per tile
constexpr int W2_RR = 2;                            // epilogue passes of residual in flight (f32 residual: 1)

// Wf[k-step 144][cout block 8][lane 64][8 halves]: the A operand of D = W . X^T in register order.  One unit = element
// `idx` of the image, straight from the Flux tensor (agz_pack.h runs put() on the host and on the device).
struct Conv16Image : ImageDefaults {
  using word = uint16_t;
  static constexpr const char* name = "fp16";
  static constexpr bool tower_only = true;
  __host__ __device__ static size_t words(int) { return (size_t)HCH * 9 * kC * HK; }
  __host__ __device__ static long units(int, int) { return (long)words(0); }
  __host__ __device__ static void put(const float* w, int, long idx, int, uint16_t* out) {
    const int k = (int)(idx & 7), lane = (int)((idx >> 3) & 63), cb = (int)((idx >> 9) & 7), ks = (int)((idx >> 12) & 1);
    const int st = (int)(idx >> 13);                                 // chunk * 9 + tap
    const int cc = st / 9, tap = st % 9;
    const int o = cb * 32 + (lane & 31), ci = cc * HK + (ks * 2 + (lane >> 5)) * 8 + k;
    const _Float16 h = (_Float16)flux_tap(w, kC, tap % 3, tap / 3, ci, o);          // round to nearest even, as __float2half_rn
    out[idx] = *reinterpret_cast<const uint16_t*>(&h);
  }
};
const ImageFamily kConv16Image = image_family<Conv16Image>();

template <int I, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < E) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, E>(f);
  }
}

// RES: 0 = no residual, 1 = half, 2 = f32 (first block's skip); OUTF: the output is f32 (last layer), else half.
// The product forms: the f32-residual layer (RES 2) and the three f32-output layers (OUTF) of a tower; 7 row blocks of 32 per
// tile, one workgroup per CU, weight fragments 8 k-steps ahead through a ring of 9 register sets, residual and result across
// wave-private LDS tiles (the direct epilogue).  Everything else this kernel has been -- the half-in / half-out form with its
// trickled result image (rounds 2-4; those layers run k_conv3x3_f16_q since round 5), the weight ring in LDS (WL), register
// masking of off-board fragments (DM), four row blocks with two workgroups per CU, the timing (DBG) and measurement (MEAS)
// variants, store policies and pacing -- is in tools/experiments/agz_conv16_variants.hip, which tools/build_timing_lib.sh
// compiles in place of this file (HISTORY.md 4b, 4h, 12).
template <int RES, bool OUTF>
__global__ __launch_bounds__(256, 1) void k_conv3x3_f16_w2(const _Float16* __restrict__ x, const uint16_t* __restrict__ wf,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         const void* __restrict__ res, void* __restrict__ y,
                                                         const int* __restrict__ d_count, int N, int relu) {
  constexpr bool RESF = RES == 2;
  static_assert(RESF || OUTF, "the half-in / half-out layers are k_conv3x3_f16_q's");
  constexpr int RB = W2_RB_PRODUCT, W2_RB = RB, W2_HM = 32 * RB;
  constexpr int W2_SLABCH = ((W2_HM + 2 * 20) * 4 + 63) / 64, NPJ = (W2_SLABCH + 3) / 4;
  constexpr int W2_SLAB = W2_SLABCH * 512, W2_SLABS = W2_SLAB + 32;
  constexpr int W2_OFF_SC = 2 * W2_SLABS, W2_OFF_OUT = W2_OFF_SC + 1024;
  constexpr int TINB = RES == 0 ? 0 : (RESF ? 32 * 272 : 32 * 144), TOUTB = OUTF ? 32 * 272 : 32 * 144;   // direct epilogue tiles
  constexpr int W2_OUTB = 4 * (TINB + TOUTB);
  constexpr int W2_SMEM = W2_OFF_OUT + W2_OUTB / 2;
  // weight fragments 8 k-steps ahead through a ring of 9 register sets (with 17 / 18 these forms spill 29-44 registers, and
  // a reload, even outside any loop, is a wait behind every weight load in flight)
  constexpr int W2_D = 8, W2_RING = W2_D + 1;
  static_assert(W2_OFF_OUT % 64 == 0 && 18 % W2_RING == 0, "layout");
  static_assert(W2_SMEM * 2 <= 160 * 1024, "LDS");
  // direct epilogue tiles [32 rows][64 couts]: row stride / 16-byte pieces per row / pieces per lane, per element type
  constexpr int RSB = RESF ? 272 : 144, RPR = RESF ? 16 : 8, RNP = RESF ? 8 : 4;
  constexpr int OSB = OUTF ? 272 : 144, OPR = OUTF ? 16 : 8, ONP = OUTF ? 8 : 4;
  constexpr int NRR = RESF ? 1 : W2_RR;               // 8 uint4 of ring either way
  __shared__ __attribute__((aligned(128))) _Float16 smem[W2_SMEM];
  const int P = N * N;
  const int M = (*d_count) * P;                          // < 2^31: 8192 x 361 rows
  const int ntiles = (M + W2_HM - 1) / W2_HM;
  if ((int)blockIdx.x >= ntiles) return;
  const int halo = N + 1, slab = W2_HM + 2 * halo;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const unsigned s0 = (unsigned)(size_t)(__attribute__((address_space(3))) _Float16*)&smem[0];
  const int nslabch = (slab * 4 + 63) / 64;
  char* sm = reinterpret_cast<char*>(smem);
  if (tid < 8) reinterpret_cast<uint4*>(smem + (tid >> 2) * W2_SLABS + W2_SLAB)[tid & 3] = make_uint4(0, 0, 0, 0);
  {
    float* tab = reinterpret_cast<float*>(smem + W2_OFF_SC);
    tab[tid] = scale[tid];
    tab[256 + tid] = shift[tid];
  }
  const float invP = 1.f / (float)P, invN = 1.f / (float)N;
  const unsigned wlane = (unsigned)lane * 16u;

  unsigned aoff[NPJ];                                       // slab piece j of this wave: byte offset of its source row piece
  auto slab_src = [&](int m0) __attribute__((always_inline)) {
    int ln = lane;
    asm volatile("" : "+v"(ln));                          // (keeps hipcc from hoisting the lane terms into spilled registers)
#pragma unroll
    for (int j = 0; j < NPJ; ++j) {                       // the spare slots repeat the last piece
      int c = wave + 4 * j;
      c = c < nslabch ? c : nslabch - 1;
      const int slot = c * 64 + ln, s = slot >> 2, q = (slot & 3) ^ ((s >> 2) & 3);
      int g = m0 - halo + s;
      g = g < 0 ? 0 : (g >= M ? M - 1 : g);               // out-of-range rows are only ever read masked
      aoff[j] = (unsigned)g * (unsigned)(kC * 2) + (unsigned)(q * 16);
    }
  };
  auto dma_a = [&](int cc, int buf, int j) __attribute__((always_inline)) {
    int c = wave + 4 * j;
    c = c < nslabch ? c : nslabch - 1;
    glds16hs(x + cc * HK, aoff[j], s0 + (unsigned)(buf * W2_SLABS + c * 512) * 2u);
  };

  unsigned vm[W2_RB];                                     // per row block: bit `tap` = that neighbour is on the board
  auto tile_masks = [&](int m0) __attribute__((always_inline)) {
    const int p0 = m0 % P;
#pragma unroll
    for (int rbk = 0; rbk < W2_RB; ++rbk) {
      const int lr = rbk * 32 + l31, v = p0 + lr;         // < P + 224: the float quotients below are exact
      const int p = v - (int)(((float)v + 0.5f) * invP) * P;
      const int bj = (int)(((float)p + 0.5f) * invN), bi = p - bj * N;
      const unsigned cm = (bi > 0 ? 1u : 0u) | 2u | (bi < N - 1 ? 4u : 0u);
      unsigned mk = (bj > 0 ? cm : 0u) | (cm << 3) | (bj < N - 1 ? cm << 6 : 0u);
      vm[rbk] = m0 + lr < M ? mk : 0u;
    }
  };

  f32x16 acc[W2_RB][2];
  h8 A[W2_RB], Bf[W2_RING][2];
  int aaddr[W2_RB];
  auto tap_addr = [&](int sbuf, int tapi) __attribute__((always_inline)) {
    const int off = (tapi % 3 - 1) + N * (tapi / 3 - 1);
    const int base = sbuf * (W2_SLABS * 2);
    const int R0 = l31 + halo + off;
    const int a0 = base + (R0 << 6) + ((((R0 >> 2) ^ hi) & 3) << 4);      // row block rbk: + rbk * 2048, same swizzle
#pragma unroll
    for (int rbk = 0; rbk < W2_RB; ++rbk) aaddr[rbk] = ((vm[rbk] >> tapi) & 1u) ? a0 + rbk * 2048 : base + W2_SLAB * 2;
  };
  // (one register set: a row block's fragment of the next k-step is fetched right after the block's two MFMAs)
  auto read_a = [&](int ks, int rbk) __attribute__((always_inline)) {
    A[rbk] = *reinterpret_cast<const h8*>(sm + (aaddr[rbk] ^ (ks << 5)));
  };
  const char* wfw = reinterpret_cast<const char*>(wf) + wave * 2048;
  auto load_b = [&](int slot, const char* wbase, int kk) __attribute__((always_inline)) {   // this wave's two fragments of k-step kk
    const char* p = wbase + (size_t)kk * 8192;
    Bf[slot][0] = *reinterpret_cast<const h8*>(p + wlane);
    Bf[slot][1] = *reinterpret_cast<const h8*>(p + 1024 + wlane);
  };

  int tile = blockIdx.x;
  int m0 = tile * W2_HM;
  slab_src(m0);
#pragma unroll
  for (int j = 0; j < NPJ; ++j) dma_a(0, 0, j);
#pragma unroll
  for (int k = 0; k < W2_D; ++k) load_b(k, wfw, k);
  tile_masks(m0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  tap_addr(0, 0);
  static_for<0, W2_RB>([&](auto ic) __attribute__((always_inline)) { read_a(0, decltype(ic)::value); });
  // Residual pieces of the next NRR epilogue passes (a pass is ~1 us of work, an HBM read under load is more).
  // Scalars, not an array: hipcc moves a by-reference captured array into LDS.
  uint4 rr0, rr1, rr2, rr3, rr4, rr5, rr6, rr7, rr8, rr9, rr10, rr11, rr12, rr13, rr14, rr15;
  auto rr = [&](auto ic) __attribute__((always_inline)) -> uint4& {
    constexpr int i = decltype(ic)::value;
    if constexpr (i == 0) return rr0;
    else if constexpr (i == 1) return rr1;
    else if constexpr (i == 2) return rr2;
    else if constexpr (i == 3) return rr3;
    else if constexpr (i == 4) return rr4;
    else if constexpr (i == 5) return rr5;
    else if constexpr (i == 6) return rr6;
    else if constexpr (i == 7) return rr7;
    else if constexpr (i == 8) return rr8;
    else if constexpr (i == 9) return rr9;
    else if constexpr (i == 10) return rr10;
    else if constexpr (i == 11) return rr11;
    else if constexpr (i == 12) return rr12;
    else if constexpr (i == 13) return rr13;
    else if constexpr (i == 14) return rr14;
    else return rr15;
  };
  auto load_res = [&](auto rc) __attribute__((always_inline)) {      // pass r -> ring slot r % NRR
    constexpr int r = decltype(rc)::value;
    static_for<0, RNP>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      const int pc = lane + 64 * i, row = pc / RPR, c16 = pc % RPR;
      int m = m0 + r * 32 + row;
      m = m < M ? m : M - 1;                              // rows past the batch: any value, never used
      const uint4* rp = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(res) + ((size_t)m * kC + wave * 64) * (RESF ? 4 : 2) + c16 * 16);
      rr(std::integral_constant<int, (r % NRR) * RNP + i>{}) = *rp;
    });
  };

  // one channel chunk: 9 taps x 2 k-steps of 14 MFMAs.  FIRST / LAST chunk of a tile are compile-time.
  auto chunk = [&](int cc, auto firstc, auto lastc) __attribute__((always_inline)) {
    constexpr bool first = decltype(firstc)::value, last = decltype(lastc)::value;
    const int sbuf = cc & 1;
    // (laundered once per chunk: hipcc otherwise hoists every address and every mask test of the 18 k-steps out of the
    // chunk loop and keeps them all live in SGPRs -- which it then spills to VGPR lanes)
    unsigned wboff = 0;
    asm volatile("" : "+s"(wboff));
    const char* wb = wfw + wboff;
#pragma unroll
    for (int rbk = 0; rbk < W2_RB; ++rbk) asm volatile("" : "+v"(vm[rbk]));
    static_for<0, 18>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      constexpr int slot = i % W2_RING;
      constexpr int nks = (i + 1) & 1;
      if (nks == 0) {                                     // the k-step being prefetched opens a new tap
        if (i < 17) tap_addr(sbuf, (i + 1) >> 1);
        else if (!last) tap_addr(sbuf ^ 1, 0);
      }
      int kn = cc * 18 + i + W2_D;
      kn = kn >= W2_KS ? kn - W2_KS : kn;
#pragma unroll
      for (int mi = 0; mi < 2 * W2_RB; ++mi) {
        const int rbk = mi >> 1, cb = mi & 1;
        if (first && i == 0) {
          const f32x16 z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
          acc[rbk][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bf[slot][cb], A[rbk], z, 0, 0, 0);
        } else {
          acc[rbk][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bf[slot][cb], A[rbk], acc[rbk][cb], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (cb == 1 && (i < 17 || !last)) read_a(nks, rbk);
        if (mi == 2) load_b((i + W2_D) % W2_RING, wb, kn);
        // the next chunk's slab (the next tile's first, in the last chunk) goes out in k-steps 0 and 1
        // (after the last tile the spare buffer just receives the first slab once more: no branch in the loop)
        if (i < 2 && mi >= 3 && mi < 6 && i * 3 + mi - 3 < NPJ) dma_a(last ? 0 : cc + 1, sbuf ^ 1, i * 3 + mi - 3);
        if (last && RES != 0 && mi == 2 * RB - 2) {  // the first passes' residual, spread over the last chunk
          if (i == 4) load_res(std::integral_constant<int, 0>{});
          if (i == 10 && NRR > 1) load_res(std::integral_constant<int, 1>{});
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (i == 16) {
        // the slab pieces issued in k-steps 0 and 1 are older than the 2 W2_D weight fragments that may be in flight
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * W2_D) : "memory");
        __syncthreads();
      }
    });
  };

  for (;;) {
    const int next_tile = tile + gridDim.x;
    const bool more = next_tile < ntiles;
    chunk(0, std::true_type{}, std::false_type{});
    for (int cc = 1; cc < HCH - 1; ++cc) chunk(cc, std::false_type{}, std::false_type{});
    if (more) slab_src(next_tile * W2_HM);
    chunk(HCH - 1, std::false_type{}, std::true_type{});

    // ---- epilogue: value = act(scale * acc + shift (+ residual)); acc[rbk][cb][4q + k] is row rbk*32 + l31,
    // cout wave*64 + cb*32 + 8q + 4hi + k
    const float* tab = reinterpret_cast<const float*>(smem + W2_OFF_SC);
    const float lo = relu ? 0.f : -3.0e38f;
    {
      // direct: residual and result cross a wave-private LDS tile each, so that HBM sees 16-byte pieces of whole rows
      char* Tin = sm + W2_OFF_OUT * 2 + wave * TINB;
      char* Tout = sm + W2_OFF_OUT * 2 + 4 * TINB + wave * TOUTB;
      auto pass = [&](auto rc) __attribute__((always_inline)) {
        constexpr int r = decltype(rc)::value;
        if (RES != 0) {
          static_for<0, RNP>([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = decltype(ic)::value;
            const int pc = lane + 64 * i, row = pc / RPR, c16 = pc % RPR;
            *reinterpret_cast<uint4*>(Tin + row * RSB + c16 * 16) = rr(std::integral_constant<int, (r % NRR) * RNP + i>{});
          });
          if constexpr (r + NRR < W2_RB) load_res(std::integral_constant<int, r + NRR>{});
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int n = cb * 32 + 8 * q + 4 * hi;
            const float4 sc = *reinterpret_cast<const float4*>(tab + wave * 64 + n);
            const float4 sh = *reinterpret_cast<const float4*>(tab + 256 + wave * 64 + n);
            float v0 = acc[r][cb][4 * q + 0] * sc.x + sh.x, v1 = acc[r][cb][4 * q + 1] * sc.y + sh.y;
            float v2 = acc[r][cb][4 * q + 2] * sc.z + sh.z, v3 = acc[r][cb][4 * q + 3] * sc.w + sh.w;
            if (RES != 0) {
              if (RESF) {
                const float4 rv = *reinterpret_cast<const float4*>(Tin + l31 * RSB + n * 4);
                v0 += rv.x; v1 += rv.y; v2 += rv.z; v3 += rv.w;
              } else {
                const h4 rv = *reinterpret_cast<const h4*>(Tin + l31 * RSB + n * 2);
                v0 += (float)rv[0]; v1 += (float)rv[1]; v2 += (float)rv[2]; v3 += (float)rv[3];
              }
            }
            v0 = fmaxf(v0, lo); v1 = fmaxf(v1, lo); v2 = fmaxf(v2, lo); v3 = fmaxf(v3, lo);
            if (OUTF) *reinterpret_cast<float4*>(Tout + l31 * OSB + n * 4) = make_float4(v0, v1, v2, v3);
            else *reinterpret_cast<h4*>(Tout + l31 * OSB + n * 2) = h4{(_Float16)v0, (_Float16)v1, (_Float16)v2, (_Float16)v3};
          }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int i = 0; i < ONP; ++i) {
          const int pc = lane + 64 * i, row = pc / OPR, c16 = pc % OPR;
          const int m = m0 + r * 32 + row;
          if (m < M)
            *reinterpret_cast<uint4*>(reinterpret_cast<char*>(y) + ((size_t)m * kC + wave * 64) * (OUTF ? 4 : 2) + c16 * 16) =
                *reinterpret_cast<const uint4*>(Tout + row * OSB + c16 * 16);
        }
        asm volatile("" ::: "memory");
      };
      static_for<0, W2_RB>(pass);
    }
    if (!more) break;
    tile = next_tile;
    m0 = tile * W2_HM;
    tile_masks(m0);
    tap_addr(0, 0);
    static_for<0, W2_RB>([&](auto ic) __attribute__((always_inline)) { read_a(0, decltype(ic)::value); });
  }
}

// ---------------------------------------------------------------------------------------------------------
// Round 5 (the product for half-in / half-out layers): the same convolution with the four waves of a workgroup arranged 2 x 2 over a 256-row x 256-cout tile -- a
// wave owns 128 rows x 128 couts (4 x 4 accumulator tiles = all 256 AGPRs) instead of 224 x 64.  Per k-step a wave then
// reads 4 slab fragments (4 KB) and 4 weight fragments (4 KB) for 16 MFMAs, where the 7 x 2 form reads 7 + 2 for 14: the
// LDS operand reads per row halve (16 KB per k-step and CU for 256 rows against 28 KB for 224), the two waves of a cout half
// ask the TCP for the same weight lines, and a wave issues 8 memory instructions per 16 MFMAs.  Half-in / half-out layers
// only (38 of a tower's 40; the f32-residual and f32-output layers keep k_conv3x3_f16_w2): results leave through
// wave-private 32 x 128 tiles (the result image of a 256-row tile does not fit beside the slabs), weight fragments 8
// k-steps ahead through a ring of 9.  Same reduction order per output (chunk, tap, k) as the 7 x 2 form: bit-identical results.
constexpr int QM = 256;                              // rows per tile
template <int RES>
__global__ __launch_bounds__(256, 1) void k_conv3x3_f16_q(const _Float16* __restrict__ x, const uint16_t* __restrict__ wf,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         const _Float16* __restrict__ res, _Float16* __restrict__ y,
                                                         const int* __restrict__ d_count, int N, int relu) {
  constexpr int SLABCH = ((QM + 2 * 20) * 4 + 63) / 64, NPJ = (SLABCH + 3) / 4;      // 1 KB pieces of a slab (halo <= 20 rows a side)
  constexpr int SLAB = SLABCH * 512, SLABS = SLAB + 32;                              // halves; + one 64-byte row of zeros
  constexpr int OFF_SC = 2 * SLABS, OFF_T = OFF_SC + 1024;
  constexpr int TSB = 264, TB = 32 * TSB;                                            // epilogue tile: 32 rows x 128 halves, row stride 264 B (66 dwords: a lane = row access of 8 bytes is conflict-free)
  constexpr int SMEM = OFF_T + 4 * 2 * TB / 2;
#ifndef AGZ_C16_QD
#define AGZ_C16_QD 5
#endif
  constexpr int D = AGZ_C16_QD, RING = D + 1;
  static_assert(SMEM * 2 <= 160 * 1024 && 18 % RING == 0, "layout");
  __shared__ __attribute__((aligned(256))) _Float16 smem[SMEM];
  const int P = N * N;
  const int M = (*d_count) * P;
  const int ntiles = (M + QM - 1) / QM;
  if ((int)blockIdx.x >= ntiles) return;
  const int halo = N + 1, slab = QM + 2 * halo;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;                 // row half / cout half of this wave
  const int l31 = lane & 31, hi = lane >> 5;
  const unsigned s0 = (unsigned)(size_t)(__attribute__((address_space(3))) _Float16*)&smem[0];
  const int nslabch = (slab * 4 + 63) / 64;
  char* sm = reinterpret_cast<char*>(smem);
  if (tid < 8) reinterpret_cast<uint4*>(smem + (tid >> 2) * SLABS + SLAB)[tid & 3] = make_uint4(0, 0, 0, 0);
  {
    float* tab = reinterpret_cast<float*>(smem + OFF_SC);
    tab[tid] = scale[tid];
    tab[256 + tid] = shift[tid];
  }
  const float invP = 1.f / (float)P, invN = 1.f / (float)N;
  const unsigned wlane = (unsigned)lane * 16u;

  unsigned aoff[NPJ];
  auto slab_src = [&](int m0) __attribute__((always_inline)) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int j = 0; j < NPJ; ++j) {
      int c = wave + 4 * j;
      c = c < nslabch ? c : nslabch - 1;
      const int slot = c * 64 + ln, sr = slot >> 2, q = (slot & 3) ^ ((sr >> 2) & 3);
      int g = m0 - halo + sr;
      g = g < 0 ? 0 : (g >= M ? M - 1 : g);
      aoff[j] = (unsigned)g * (unsigned)(kC * 2) + (unsigned)(q * 16);
    }
  };
  auto dma_a = [&](int cc, int buf, int j) __attribute__((always_inline)) {
    int c = wave + 4 * j;
    c = c < nslabch ? c : nslabch - 1;
    glds16hs(x + cc * HK, aoff[j], s0 + (unsigned)(buf * SLABS + c * 512) * 2u);
  };
  unsigned vm[4];
  auto tile_masks = [&](int m0) __attribute__((always_inline)) {
    const int p0 = m0 % P;
#pragma unroll
    for (int rbk = 0; rbk < 4; ++rbk) {
      const int lr = wr * 128 + rbk * 32 + l31, v = p0 + lr;          // < P + 256: the float quotients below are exact
      const int p = v - (int)(((float)v + 0.5f) * invP) * P;
      const int bj = (int)(((float)p + 0.5f) * invN), bi = p - bj * N;
      const unsigned cm = (bi > 0 ? 1u : 0u) | 2u | (bi < N - 1 ? 4u : 0u);
      const unsigned mk = (bj > 0 ? cm : 0u) | (cm << 3) | (bj < N - 1 ? cm << 6 : 0u);
      vm[rbk] = m0 + lr < M ? mk : 0u;
    }
  };
  f32x16 acc[4][4];
  h8 A[4], Bf[RING][4];
  int aaddr[4];
  auto tap_addr = [&](int sbuf, int tapi) __attribute__((always_inline)) {
    const int off = (tapi % 3 - 1) + N * (tapi / 3 - 1);
    const int base = sbuf * (SLABS * 2);
    const int R0 = wr * 128 + l31 + halo + off;
    const int a0 = base + (R0 << 6) + ((((R0 >> 2) ^ hi) & 3) << 4);
    const int z0 = base + SLAB * 2;
#pragma unroll
    for (int rbk = 0; rbk < 4; ++rbk) aaddr[rbk] = ((vm[rbk] >> tapi) & 1u) ? a0 + rbk * 2048 : z0;
  };
  auto read_a = [&](int ks, int rbk) __attribute__((always_inline)) {
    A[rbk] = *reinterpret_cast<const h8*>(sm + (aaddr[rbk] ^ (ks << 5)));
  };
  const char* wfw = reinterpret_cast<const char*>(wf) + wc * 4096;
  auto load_b = [&](int slot, const char* wbase, int kk) __attribute__((always_inline)) {
    const char* p = wbase + (size_t)kk * 8192 + wlane;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) Bf[slot][cb] = *reinterpret_cast<const h8*>(p + cb * 1024);
  };
  char* Tin = sm + OFF_T * 2 + wave * (2 * TB);
  char* Tout = Tin + TB;
  // residual pieces of one epilogue pass (32 rows x 256 B of this wave's cout half: 8 x 16 B per lane), fetched one pass ahead:
  // pass 0's during the last chunk, pass r + 1's while pass r is computed.  (Scalars: hipcc moves a captured array into LDS.)
  uint4 q0 = {}, q1 = {}, q2 = {}, q3 = {}, q4 = {}, q5 = {}, q6 = {}, q7 = {};
  auto rload_pass = [&](int mr, int ln) __attribute__((always_inline)) {
    auto one = [&](int i) __attribute__((always_inline)) {
      const int pc = ln + 64 * i, row = pc >> 4, c16 = pc & 15;
      int m = mr + row;
      m = m < M ? m : M - 1;
      return *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(res) + ((size_t)m * kC + wc * 128) * 2 + c16 * 16);
    };
    q0 = one(0); q1 = one(1); q2 = one(2); q3 = one(3); q4 = one(4); q5 = one(5); q6 = one(6); q7 = one(7);
  };

  int tile = blockIdx.x;
  int m0 = tile * QM;
  slab_src(m0);
#pragma unroll
  for (int j = 0; j < NPJ; ++j) dma_a(0, 0, j);
#pragma unroll
  for (int k = 0; k < D; ++k) load_b(k, wfw, k);
  tile_masks(m0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  tap_addr(0, 0);
#pragma unroll
  for (int rbk = 0; rbk < 4; ++rbk) read_a(0, rbk);

  for (;;) {
    const int next_tile = tile + gridDim.x;
    const bool more = next_tile < ntiles;

    auto chunk = [&](int cc, auto firstc, auto lastc) __attribute__((always_inline)) {
      constexpr bool first = decltype(firstc)::value, last = decltype(lastc)::value;
      const int sbuf = cc & 1;
      unsigned wboff = 0;
      asm volatile("" : "+s"(wboff));            // (per chunk: keeps hipcc from hoisting 18 k-steps of addresses and mask tests)
      const char* wb = wfw + wboff;
#pragma unroll
      for (int rbk = 0; rbk < 4; ++rbk) asm volatile("" : "+v"(vm[rbk]));
      static_for<0, 18>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        constexpr int slot = i % RING;
        constexpr int nks = (i + 1) & 1;
        if (nks == 0) {
          if (i < 17) tap_addr(sbuf, (i + 1) >> 1);
          else if (!last) tap_addr(sbuf ^ 1, 0);
        }
        int kn = cc * 18 + i + D;
        kn = kn >= W2_KS ? kn - W2_KS : kn;      // (the last chunk's tail fetches the next tile's first fragments: same addresses)
#pragma unroll
        for (int rbk = 0; rbk < 4; ++rbk) {
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) {
            if (first && i == 0) {
              const f32x16 z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
              acc[rbk][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bf[slot][cb], A[rbk], z, 0, 0, 0);
            } else {
              acc[rbk][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bf[slot][cb], A[rbk], acc[rbk][cb], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
          if (i < 17 || !last) read_a(nks, rbk);
          if (rbk == 0) load_b((i + D) % RING, wb, kn);
          if (last && RES != 0 && i == 9 && rbk == 2) rload_pass(m0 + wr * 128, lane);
          // the next chunk's slab (the next tile's first, in the last chunk) goes out in k-steps 0 and 1
          // (after the last tile the spare buffer just receives a slab once more: no branch in the loop)
          if (i < 2 && rbk >= 1 && (i * 3 + rbk - 1) < NPJ) dma_a(last ? 0 : cc + 1, sbuf ^ 1, i * 3 + rbk - 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (i == 16) {
          // the slab pieces issued in k-steps 0 and 1 are older than the 4 D weight fragments that may be in flight
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * D) : "memory");
          __syncthreads();
        }
      });
    };
    chunk(0, std::true_type{}, std::false_type{});
    for (int cc = 1; cc < HCH - 1; ++cc) chunk(cc, std::false_type{}, std::false_type{});
    if (more) slab_src(next_tile * QM);          // the last chunk sends the next tile's first slab and weight fragments ahead
    chunk(HCH - 1, std::false_type{}, std::true_type{});

    // ---- epilogue: value = act(scale * acc + shift (+ residual)); acc[r][cb][4q + k] is row wr*128 + r*32 + l31,
    // cout wc*128 + cb*32 + 8q + 4hi + k.  Residual and result cross a wave-private 32 x 128 tile each.
    const float* tab = reinterpret_cast<const float*>(smem + OFF_SC);
    const float lo = relu ? 0.f : -3.0e38f;
    int eln = lane;
    asm volatile("" : "+v"(eln));              // (opaque: else hipcc computes ~40 epilogue addresses before the K loop and spills them)
    const int el31 = eln & 31, ehi = eln >> 5;
    static_for<0, 4>([&](auto rc) __attribute__((always_inline)) {
      constexpr int r = decltype(rc)::value;
      const int mr = m0 + wr * 128 + r * 32;
      if (RES != 0) {
        auto rput = [&](int i, uint4 v) __attribute__((always_inline)) {        // (row stride 264 B: 8-byte LDS accesses)
          const int pc = eln + 64 * i, row = pc >> 4, c16 = pc & 15;
          *reinterpret_cast<uint2*>(Tin + row * TSB + c16 * 16) = make_uint2(v.x, v.y);
          *reinterpret_cast<uint2*>(Tin + row * TSB + c16 * 16 + 8) = make_uint2(v.z, v.w);
        };
        rput(0, q0); rput(1, q1); rput(2, q2); rput(3, q3); rput(4, q4); rput(5, q5); rput(6, q6); rput(7, q7);
        if constexpr (r + 1 < 4) rload_pass(mr + 32, eln);
      }
      asm volatile("" ::: "memory");
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = cb * 32 + 8 * q + 4 * ehi;
          const float4 sc = *reinterpret_cast<const float4*>(tab + wc * 128 + n);
          const float4 sh = *reinterpret_cast<const float4*>(tab + 256 + wc * 128 + n);
          float v0 = acc[r][cb][4 * q + 0] * sc.x + sh.x, v1 = acc[r][cb][4 * q + 1] * sc.y + sh.y;
          float v2 = acc[r][cb][4 * q + 2] * sc.z + sh.z, v3 = acc[r][cb][4 * q + 3] * sc.w + sh.w;
          if (RES != 0) {
            const h4 rv = *reinterpret_cast<const h4*>(Tin + el31 * TSB + n * 2);
            v0 += (float)rv[0]; v1 += (float)rv[1]; v2 += (float)rv[2]; v3 += (float)rv[3];
          }
          v0 = fmaxf(v0, lo); v1 = fmaxf(v1, lo); v2 = fmaxf(v2, lo); v3 = fmaxf(v3, lo);
          *reinterpret_cast<h4*>(Tout + el31 * TSB + n * 2) = h4{(_Float16)v0, (_Float16)v1, (_Float16)v2, (_Float16)v3};
        }
      asm volatile("" ::: "memory");
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int pc = eln + 64 * i, row = pc >> 4, c16 = pc & 15;
        const int m = mr + row;
        const uint2 o0 = *reinterpret_cast<const uint2*>(Tout + row * TSB + c16 * 16);
        const uint2 o1 = *reinterpret_cast<const uint2*>(Tout + row * TSB + c16 * 16 + 8);
        if (m < M)
          *reinterpret_cast<uint4*>(reinterpret_cast<char*>(y) + ((size_t)m * kC + wc * 128) * 2 + c16 * 16) = make_uint4(o0.x, o0.y, o1.x, o1.y);
      }
      asm volatile("" ::: "memory");
    });
    if (!more) break;
    tile = next_tile;
    m0 = tile * QM;
    tile_masks(m0);
    tap_addr(0, 0);
#pragma unroll
    for (int rbk = 0; rbk < 4; ++rbk) read_a(0, rbk);
  }
}

__global__ __launch_bounds__(256) void k_f32_to_f16(const float* __restrict__ x, _Float16* __restrict__ y,
                                                     const int* __restrict__ d_count, long per_position) {
  const long n = (long)(*d_count) * per_position;        // multiple of 8
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8; i < n; i += (long)gridDim.x * 256 * 8) {
    const float4 u = *reinterpret_cast<const float4*>(x + i), v = *reinterpret_cast<const float4*>(x + i + 4);
    h8 h = {(_Float16)u.x, (_Float16)u.y, (_Float16)u.z, (_Float16)u.w, (_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
    *reinterpret_cast<h8*>(y + i) = h;
  }
}

void launch_f32_to_f16(const float* x, uint16_t* y, const int* d_count, int bcap, int N, hipStream_t s) {
  const long n = (long)bcap * N * N * kC;
  const int grid = (int)std::min<long>((n / 8 + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(k_f32_to_f16, dim3(grid), dim3(256), 0, s, x, (_Float16*)y, d_count, (long)N * N * kC);
}

void launch_conv16_dma(const uint16_t* x, const uint16_t* wi, const float* scale, const float* shift, const void* res,
                       int res_f32, void* y, int out_f32, const int* d_count, int bcap, int N, int relu, hipStream_t s) {
  const long rows = (long)bcap * N * N;
  const _Float16* xh = (const _Float16*)x;
  static int ncu = 0;
  if (!ncu) AGZ_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
  const int rk = !res ? 0 : (res_f32 ? 2 : 1);
  // the half-in / half-out layers (38 of a tower's 40): 2 x 2 waves over a 256-row x 256-cout tile (round 5: -1.8 % per
  // configs[4] step against the 7 x 2 form in a same-box A/B, bit-identical results)
  if (!res_f32 && !out_f32) {
    const int gq = std::min((int)((rows + QM - 1) / QM), ncu);
    if (res) hipLaunchKernelGGL((k_conv3x3_f16_q<1>), dim3(gq), dim3(256), 0, s, xh, wi, scale, shift, (const _Float16*)res, (_Float16*)y, d_count, N, relu);
    else hipLaunchKernelGGL((k_conv3x3_f16_q<0>), dim3(gq), dim3(256), 0, s, xh, wi, scale, shift, (const _Float16*)nullptr, (_Float16*)y, d_count, N, relu);
    return;
  }
  // the f32-residual and f32-output layers (first and last of a tower): 7 x 2 wave tiles over 224 rows, direct epilogue
  const int grid7 = std::min((int)((rows + 32 * W2_RB_PRODUCT - 1) / (32 * W2_RB_PRODUCT)), ncu);
#define AGZ_C16_W2(R, OF) \
  hipLaunchKernelGGL((k_conv3x3_f16_w2<R, OF>), dim3(grid7), dim3(256), 0, s, xh, wi, scale, shift, res, y, d_count, N, relu)
  if (out_f32) {
    if (rk == 0) AGZ_C16_W2(0, true);
    else if (rk == 1) AGZ_C16_W2(1, true);
    else AGZ_C16_W2(2, true);
  } else {
    AGZ_C16_W2(2, false);           // (rk == 2: the half-output layer behind an f32 residual)
  }
#undef AGZ_C16_W2
}

}  // namespace agz

// agz_pack.h -- what every inference weight image shares: the Flux tap with NNlib's flip, U = G k G^T in
// float64, and ONE pack driver (host loop, grid-stride kernel, launcher) over an image trait.  The trait sits next to the
// layout functions of the kernel that reads the image, in that kernel's .hip file, and states
//   word                          the image's element type
//   name                          for messages
//   words(ns)                     elements per layer; ns = K-loop stages = padded input channels / 4 (64 tower, 8 stem)
//   units(cin, ns)                independent pieces of work per layer: (cout, cin) pairs, or elements
//   put(w, cin, unit, ns, out)    one unit of one layer, from the layer's Flux tensor [3][3][cin][256] into its image
//   zeroed                        put() leaves words unwritten: the image is cleared first
//   tower_only, grid_cap          256 -> 256 layers only; the launch's block limit
// The host loop (the test reference of agz_debug_pack_diff) and the kernel (the product: weights never leave the GPU between
// a training step / a broadcast and the next forward) run the same put(), and produce the same bits.
#pragma once
#include <algorithm>
#include <cstring>

#include "agz_nn.h"

namespace agz {

// Flux [kw,kh,cin,cout] column-major.  NNlib's conv is a TRUE convolution: the tap that reads x[i + a - 1, j + b - 1]
// (correlation index (a, b), tap = a + 3 b) carries w[2 - a, 2 - b].
__host__ __device__ inline float flux_tap(const float* w, int cin, int a, int b, int ci, int o) {
  return w[(2 - a) + 3 * ((2 - b) + 3 * (ci + (size_t)cin * o))];
}

// the R x 3 weight transform G of Winograd F((R-2) x (R-2), 3x3): R = 5 (agz_wino.hip, agz_wino5.hip), 6 (agz_wino4.hip)
template <int R> struct WinogradG;
template <> struct WinogradG<5> {
  __host__ __device__ static constexpr double at(int i, int a) {
    constexpr double G[5][3] = {{0.5, 0.0, 0.0}, {0.5, 0.5, 0.5}, {1.0 / 6, -1.0 / 6, 1.0 / 6},
                                {1.0 / 6, 1.0 / 3, 2.0 / 3}, {0.0, 0.0, 1.0}};
    return G[i][a];
  }
};
template <> struct WinogradG<6> {
  __host__ __device__ static constexpr double at(int i, int a) {
    constexpr double G[6][3] = {{0.25, 0.0, 0.0},         {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0.0, 0.0, 1.0}};
    return G[i][a];
  }
};

// emit(i, j, U[i][j]) for the R x R values of U = G k G^T of the (cout o, cin ci) pair, k the correlation kernel, in float64.
// Contraction is switched off HERE: the translation units that call this are built with it allowed.
template <int R, class Emit>
__host__ __device__ inline void winograd_u(const float* w, int cin, int o, int ci, Emit&& emit) {
#pragma clang fp contract(off)
  double k[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) k[a][b] = flux_tap(w, cin, a, b, ci, o);
  for (int i = 0; i < R; ++i)
    for (int j = 0; j < R; ++j) {
      double u = 0.0;
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) u += WinogradG<R>::at(i, a) * k[a][b] * WinogradG<R>::at(j, b);
      emit(i, j, u);
    }
}

struct ImageDefaults {
  static constexpr bool zeroed = false, tower_only = false;
  static constexpr int grid_cap = 65536;
};

// ---- the driver.  Host: one layer.
template <class I>
void pack_host(const ConvHost& c, void* out, int ns) {
  AGZ_REQUIRE(!I::tower_only || (c.cin == kC && c.cout == kC), AGZ_BAD_ARGUMENT, "%s pack: tower layers only (%d -> %d)", I::name,
              c.cin, c.cout);
  auto* o = static_cast<typename I::word*>(out);
  if (I::zeroed) std::memset(o, 0, sizeof(typename I::word) * I::words(ns));
  for (long u = 0, n = I::units(c.cin, ns); u < n; ++u) I::put(c.w.data(), c.cin, u, ns, o);
}
// Device: `layers` consecutive Flux tensors, `wstride` floats apart (Net's master copy), into `layers` images `per` words
// apart.  One thread per (layer, unit).
template <class I>
__global__ __launch_bounds__(256) void k_pack(const float* __restrict__ w, long wstride, int cin, int layers, int ns,
                                              typename I::word* __restrict__ out, long per) {
  const long units = I::units(cin, ns), n = layers * units;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long)gridDim.x * 256) {
    const long l = t / units;
    I::put(w + l * wstride, cin, t - l * units, ns, out + l * per);
  }
}
template <class I>
void pack_device(const float* d_w, long wstride, int cin, int layers, void* d_out, int ns, hipStream_t s) {
  const long per = (long)I::words(ns), n = layers * I::units(cin, ns);
  if (I::zeroed) AGZ_HIP(hipMemsetAsync(d_out, 0, sizeof(typename I::word) * (size_t)per * layers, s));
  hipLaunchKernelGGL(k_pack<I>, dim3((int)std::min<long>((n + 255) / 256, I::grid_cap)), dim3(256), 0, s, d_w, wstride, cin, layers,
                     ns, static_cast<typename I::word*>(d_out), per);
}

template <class I>
size_t image_bytes(int ns) { return sizeof(typename I::word) * I::words(ns); }
// the descriptor agz_nn.h exports for image I.  (Not constexpr: a constant-initialised const object would be emitted for the
// device too, where these host functions do not exist.)
template <class I>
ImageFamily image_family() { return {I::name, image_bytes<I>, pack_host<I>, pack_device<I>}; }

}  // namespace agz

// Device and host helpers shared by the image-quality kernels: the fused evaluation metrics (eval_metrics.hip), the
// training image loss (loss.hip) and the LPIPS input stage (lpips.hip).  One definition each of the evaluation's
// uint8 quantisation, the reference SSIM's constants (utils/metrics.py:93-135), the 32 x 16 tile with its 42 x 26
// halo, the windowed sums, the per-view reduction and the launch plan.  __device__ __forceinline__ leaves: a
// kernel that uses them keeps its own name, __shared__ arrays, barriers and launch shape.
#pragma once
#include "common.h"

namespace sfxi {

// ---- uint8 images of the evaluation loop (train.py:104-113, metrics.py:26-29) ------------------------------------
// torch's float -> uint8 conversion truncates toward zero; out-of-range values saturate instead of wrapping
// (documented divergence: inputs are composited colours and images in [0, 1]).  A caller clamps (fminf(x, 1.f)) and
// masks first, each with its own rounding.
__device__ __forceinline__ int quant_u8(float x) {
  const float y = x * 255.f;
  const int q = (int)y;
  return q < 0 ? 0 : (q > 255 ? 255 : q);
}
// the reference's fp32 division of a uint8 image
__device__ __forceinline__ float unquant_u8(int q) { return (float)q / 255.f; }

// ---- SSIM ---------------------------------------------------------------------------------------------------------
constexpr int WIN = 11, RAD = 5;  // window 11, sigma 1.5 (the caller's taps), conv2d zero padding 5
constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;

// SSIM = A1 A2 / (B1 B2) from the five windowed moments.  The caller divides: the metric with a true division, the
// loss through the reciprocal its derivative maps share.  A1 = 2 mu1 mu2 + C1 is the caller's too: the library is
// built with contraction on, and the two callers' spellings fuse differently -- the metric's 2.0 * mu12 + C1
// compiles to fma(mu12, 2, C1) on the rounded product, the loss's 2.0 * mu1 * mu2 + C1 to fma(2 mu1, mu2, C1) with
// the 2 mu1 its maps share -- so one spelling here would move the other caller's last fp64 bit.
struct SsimTerms {
  double mu12, A2, B1, B2;
};
__device__ __forceinline__ SsimTerms ssim_terms(double mu1, double mu2, double e11, double e22, double e12) {
  const double mu11 = mu1 * mu1, mu22 = mu2 * mu2, mu12 = mu1 * mu2;
  return {mu12, 2.0 * (e12 - mu12) + C2, mu11 + mu22 + C1, (e11 - mu11) + (e22 - mu22) + C2};
}

// ---- tile geometry: 256 threads per 32 x 16 output tile, staged with its halo of RAD pixels ---------------------
constexpr int TILE_X = 32, TILE_Y = 16, THREADS = 256;
constexpr int HALO_X = TILE_X + 2 * RAD, HALO_Y = TILE_Y + 2 * RAD;

// Staging index i in [0, HALO_Y * HALO_X) of the tile at (blockIdx.x, blockIdx.y): the halo slot (yy, xx), its
// image pixel (y, x), whether that lies in the image (outside = the zero padding) and whether the slot is one of
// the tile's own pixels.
struct HaloPx {
  int yy, xx, y, x;
  bool in, own;
};
__device__ __forceinline__ HaloPx halo_px(int i, int H, int W) {
  HaloPx h;
  h.yy = i / HALO_X;
  h.xx = i % HALO_X;
  h.y = blockIdx.y * TILE_Y - RAD + h.yy;
  h.x = blockIdx.x * TILE_X - RAD + h.xx;
  h.in = h.y >= 0 && h.y < H && h.x >= 0 && h.x < W;
  h.own = h.yy >= RAD && h.yy < RAD + TILE_Y && h.xx >= RAD && h.xx < RAD + TILE_X;
  return h;
}

// ---- sums ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One output of a separable pass over K planes: acc[k] = sum_j w[j] * v_j[k], taps in ascending order, fp64.
// `at(j, v)` fills the K plane values under tap j (a row pass reads column x + j, a column pass row ty + j).
template <int K, class At>
__device__ __forceinline__ void window_sum(const double* w, double (&acc)[K], At at) {
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
#pragma unroll
  for (int j = 0; j < WIN; ++j) {
    double v[K];
    at(j, v);
    const double wj = w[j];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = fma(wj, v[k], acc[k]);
  }
}

// Called by the one workgroup of THREADS that owns view blockIdx.x: adds the view's per_view groups of K interleaved
// fp64 partials in one fixed order (a strided sum per thread, then a halving tree), so the same partials give the
// same bits.  Thread 0 returns with the K totals in tot.
template <int K>
__device__ __forceinline__ void view_reduce(long long per_view, const double* __restrict__ partial, double (&tot)[K]) {
  __shared__ double red[K][THREADS];
  const double* p = partial + (long long)blockIdx.x * per_view * K;
#pragma unroll
  for (int k = 0; k < K; ++k) tot[k] = 0.0;
  for (long long i = threadIdx.x; i < per_view; i += THREADS)
#pragma unroll
    for (int k = 0; k < K; ++k) tot[k] += p[i * K + k];
#pragma unroll
  for (int k = 0; k < K; ++k) red[k][threadIdx.x] = tot[k];
  __syncthreads();
  for (int o = THREADS / 2; o >= 1; o >>= 1) {
    if (threadIdx.x < o)
#pragma unroll
      for (int k = 0; k < K; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) tot[k] = red[k][0];
}

// ---- launch plan (host) ---------------------------------------------------------------------------------------------
// V views of H x W with C planes each tiled on their own (the metric tiles all three channels together: C = 1).
struct ImagePlan {
  long long tiles_x, tiles_y, elems, partials;  // partials: tiles of all views and planes
  bool grid_z_fits, grid_y_fits;                // V * C and tiles_y within one grid dimension (65535)
};
// false: a size below 1 (V below 0), or more than 2^40 elements (so every index fits a long long with room)
inline bool image_plan(int V, int H, int W, int C, ImagePlan* p) {
  if (V < 0 || H < 1 || W < 1 || C < 1) return false;
  if ((double)V * H * W * C > (double)(1LL << 40)) return false;
  p->tiles_x = sfx::ceil_div(W, TILE_X);
  p->tiles_y = sfx::ceil_div(H, TILE_Y);
  p->elems = (long long)V * H * W * C;
  p->partials = (long long)V * C * p->tiles_x * p->tiles_y;
  p->grid_z_fits = (long long)V * C <= 65535;
  p->grid_y_fits = p->tiles_y <= 65535;
  return true;
}

}  // namespace sfxi

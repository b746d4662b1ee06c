// Training image loss: l1_weight * mean|p - g| + ssim_weight * (1 - SSIM), per view, and its derivative.
//
// Reference: the L1 term of train.py:275-280 and the SSIM of utils/metrics.py:93-135 (window 11, sigma 1.5, the
// 1-D Gaussian normalised in fp32, conv2d zero padding 5, C1 = 0.01^2, C2 = 0.03^2).  Images are
// [V][H][W][C] fp32, HWC as rendered.
//
// Window: the caller passes the 11 fp32 taps g of the 1-D Gaussian; the 2-D window is their outer product
// g_i * g_j, applied separably (rows, then columns) with the products and sums in fp64.  (The reference rounds each
// g_i * g_j to fp32 once; that is a relative 6e-8 per tap, below the rounding of its own fp32 convolution.)
//
// Layout: one workgroup of 256 threads per 32 x 16 output tile of one channel of one view, grid
// (tiles_x, tiles_y, V * C).
//   pass A  stages the 42 x 26 halo of p and g in LDS (zero outside the image = the padding), forms the five
//           row moments of every halo row (w*p, w*g, w*p^2, w*g^2, w*pg over 11 columns), then the column sums
//           of those, the SSIM map value m and -- when a gradient is wanted -- the three derivative maps
//           dm/dmu1, dm/de11, dm/de12, written as fp32 planes of the workspace.  It also writes the tile's sums of
//           |p - g|, (p - g)^2 and m as one fp64 triple.
//   reduce  one workgroup per view adds that view's triples in a fixed order and writes the four terms.
//   pass B  stages the halo of the three maps, convolves them with the same (self-adjoint) window and writes
//           d_pred = scale * (l1_weight * sign(p - g) - ssim_weight * (w*Dmu + 2p w*D11 + g w*D12)) / (C H W).
// Moments, the map algebra and both convolutions' sums run in fp64: with pred near gt and both near 1 (white
// background) e11 - mu1^2 cancels seven digits and the three terms of the derivative cancel three more, which an
// fp32 sum does not survive; the maps themselves are stored as fp32.  VALU + LDS only, no atomics: every sum
// has one fixed order, so two calls give the same bits.
#include "image_common.h"

namespace {

using namespace sfxi;

// maps != NULL: also write the derivative maps (plane stride `plane` elements) for pass B.  One instantiation, so
// the terms have the same bits with and without a gradient.
__global__ void __launch_bounds__(THREADS) loss_moments_kernel(int H, int W, int C, const float* __restrict__ pred,
                                                                const float* __restrict__ gt,
                                                                const float* __restrict__ taps,
                                                                double* __restrict__ partial,
                                                                float* __restrict__ maps, long long plane) {
  __shared__ float sp[HALO_Y][HALO_X + 1], sg[HALO_Y][HALO_X + 1];
  __shared__ double hm[5][HALO_Y][TILE_X];
  __shared__ double sw[WIN];
  __shared__ double red[THREADS / 64][3];
  const int img = blockIdx.z / C, c = blockIdx.z % C;
  const long long base = (long long)img * H * W * C;
  double l1 = 0.0, l2 = 0.0, sm = 0.0;
  for (int i = threadIdx.x; i < HALO_Y * HALO_X; i += THREADS) {
    const HaloPx h = halo_px(i, H, W);
    float a = 0.f, b = 0.f;
    if (h.in) {
      const long long o = base + ((long long)h.y * W + h.x) * C + c;
      a = pred[o];
      b = gt[o];
      if (h.own) {
        const double d = (double)a - (double)b;
        l1 += fabs(d);
        l2 += d * d;
      }
    }
    sp[h.yy][h.xx] = a;
    sg[h.yy][h.xx] = b;
  }
  if (threadIdx.x < WIN) sw[threadIdx.x] = (double)taps[threadIdx.x];
  __syncthreads();
  for (int i = threadIdx.x; i < HALO_Y * TILE_X; i += THREADS) {  // rows: w*p, w*g, w*p^2, w*g^2, w*pg
    const int yy = i / TILE_X, x = i % TILE_X;
    double r[5];
    window_sum<5>(sw, r, [&](int j, double* v) {
      const double a = sp[yy][x + j], b = sg[yy][x + j];
      v[0] = a, v[1] = b, v[2] = a * a, v[3] = b * b, v[4] = a * b;
    });
#pragma unroll
    for (int k = 0; k < 5; ++k) hm[k][yy][x] = r[k];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TILE_Y * TILE_X; i += THREADS) {  // columns: mu1, mu2, e11, e22, e12
    const int ty = i / TILE_X, tx = i % TILE_X;
    const int y = blockIdx.y * TILE_Y + ty, x = blockIdx.x * TILE_X + tx;
    if (y >= H || x >= W) continue;
    double e[5];
    window_sum<5>(sw, e, [&](int j, double* v) {
#pragma unroll
      for (int k = 0; k < 5; ++k) v[k] = hm[k][ty + j][tx];
    });
    const double mu1 = e[0], mu2 = e[1];
    const SsimTerms t = ssim_terms(mu1, mu2, e[2], e[3], e[4]);
    const double A1 = 2.0 * mu1 * mu2 + C1;
    const double rb = 1.0 / (t.B1 * t.B2);
    const double m = A1 * t.A2 * rb;
    sm += m;
    if (maps) {
      const long long o = base + ((long long)y * W + x) * C + c;
      maps[o] = (float)(2.0 * mu2 * (t.A2 - A1) * rb - 2.0 * mu1 * m / t.B1 + 2.0 * mu1 * m / t.B2);
      maps[plane + o] = (float)(-m / t.B2);
      maps[2 * plane + o] = (float)(2.0 * A1 * rb);
    }
  }
  l1 = wave_sum_f64(l1);
  l2 = wave_sum_f64(l2);
  sm = wave_sum_f64(sm);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = l1;
    red[threadIdx.x >> 6][1] = l2;
    red[threadIdx.x >> 6][2] = sm;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double s = 0.0;
    for (int w = 0; w < THREADS / 64; ++w) s += red[w][threadIdx.x];
    const long long tiles = (long long)gridDim.x * gridDim.y;
    const long long t = (long long)blockIdx.z * tiles + (long long)blockIdx.y * gridDim.x + blockIdx.x;
    partial[t * 3 + threadIdx.x] = s;
  }
}

// terms[v] = mean|p-g|, SSIM mean, mean (p-g)^2, l1_weight * [0] + ssim_weight * (1 - [1])
__global__ void __launch_bounds__(THREADS) loss_reduce_kernel(long long per_view, double denom, float l1_weight,
                                                               float ssim_weight, const double* __restrict__ partial,
                                                               float* __restrict__ terms) {
  double s[3];
  view_reduce<3>(per_view, partial, s);
  if (threadIdx.x == 0) {
    const double l1 = s[0] / denom, mse = s[1] / denom, ssim = s[2] / denom;
    float* t = terms + (long long)blockIdx.x * 4;
    t[0] = (float)l1;
    t[1] = (float)ssim;
    t[2] = (float)mse;
    t[3] = (float)((double)l1_weight * l1 + (double)ssim_weight * (1.0 - ssim));
  }
}

// SSIM: convolve the three maps and combine; otherwise the L1 sign term alone (the maps are not read)
template <bool SSIM>
__global__ void __launch_bounds__(THREADS) loss_grad_kernel(int H, int W, int C, const float* __restrict__ pred,
                                                             const float* __restrict__ gt,
                                                             const float* __restrict__ taps,
                                                             const float* __restrict__ maps, long long plane,
                                                             float l1_weight, float ssim_weight,
                                                             const float* __restrict__ view_scale, double denom,
                                                             float* __restrict__ d_pred) {
  __shared__ float sd[SSIM ? 3 : 1][HALO_Y][HALO_X + 1];
  __shared__ double hd[SSIM ? 3 : 1][HALO_Y][TILE_X];
  __shared__ double sw[WIN];
  const int img = blockIdx.z / C, c = blockIdx.z % C;
  const long long base = (long long)img * H * W * C;
  const double vs = view_scale ? (double)view_scale[img] : 1.0;
  const double cl1 = (double)l1_weight * vs / denom;  // sign's coefficient, rounded to fp32 once at the store
  const double cs = -(double)ssim_weight * vs / denom;
  if (SSIM) {
    for (int i = threadIdx.x; i < HALO_Y * HALO_X; i += THREADS) {
      const HaloPx h = halo_px(i, H, W);
      const long long o = base + ((long long)h.y * W + h.x) * C + c;
#pragma unroll
      for (int k = 0; k < 3; ++k) sd[k][h.yy][h.xx] = h.in ? maps[k * plane + o] : 0.f;
    }
    if (threadIdx.x < WIN) sw[threadIdx.x] = (double)taps[threadIdx.x];
    __syncthreads();
    for (int i = threadIdx.x; i < HALO_Y * TILE_X; i += THREADS) {
      const int yy = i / TILE_X, x = i % TILE_X;
      double r[3];
      window_sum<3>(sw, r, [&](int j, double* v) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = (double)sd[k][yy][x + j];
      });
#pragma unroll
      for (int k = 0; k < 3; ++k) hd[k][yy][x] = r[k];
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < TILE_Y * TILE_X; i += THREADS) {
    const int ty = i / TILE_X, tx = i % TILE_X;
    const int y = blockIdx.y * TILE_Y + ty, x = blockIdx.x * TILE_X + tx;
    if (y >= H || x >= W) continue;
    const long long o = base + ((long long)y * W + x) * C + c;
    const double p = pred[o], g = gt[o];
    const double sgn = p > g ? 1.0 : (p < g ? -1.0 : 0.0);  // sign(0) = 0 (torch's abs backward)
    double out = cl1 * sgn;
    if (SSIM) {
      double s[3];
      window_sum<3>(sw, s, [&](int j, double* v) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = hd[k][ty + j][tx];
      });
      out += cs * (s[0] + 2.0 * p * s[1] + g * s[2]);
    }
    d_pred[o] = (float)out;
  }
}

bool overlaps(const float* a, const float* b, long long n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
  return x < y + bytes && y < x + bytes;
}

}  // namespace

extern "C" {

size_t sfx_image_loss_workspace_bytes(int num_images, int height, int width, int channels) {
  ImagePlan p;
  if (!image_plan(num_images, height, width, channels, &p)) return 0;  // sfx_image_loss refuses these sizes
  return sizeof(double) * 3 * (size_t)p.partials + sizeof(float) * 3 * (size_t)p.elems;
}

int sfx_image_loss(int num_images, int height, int width, int channels, const float* pred, const float* gt,
                   const float* window, float l1_weight, float ssim_weight, const float* view_scale, float* terms,
                   float* d_pred, void* ws, size_t ws_bytes, void* stream) {
  sfx::clear_error();
  ImagePlan p;
  SFX_REQUIRE(image_plan(num_images, height, width, channels, &p),
              "sfx_image_loss: bad sizes (%d images of %d x %d x %d; at most 2^40 elements)", num_images, height, width,
              channels);
  SFX_REQUIRE(l1_weight >= 0.f && ssim_weight >= 0.f, "sfx_image_loss: negative (or NaN) loss weight");
  if (num_images == 0) return SFX_OK;
  SFX_REQUIRE(p.grid_z_fits, "sfx_image_loss: at most 65535 view-channels per call (got %lld)",
              (long long)num_images * channels);
  SFX_REQUIRE(p.grid_y_fits, "sfx_image_loss: height above %d", 65535 * TILE_Y);
  SFX_REQUIRE(pred && gt && window && terms && ws, "sfx_image_loss: null buffer");
  SFX_REQUIRE((uintptr_t)ws % 8 == 0, "sfx_image_loss: workspace must be 8-byte aligned");
  // forward only: the tile sums alone; with d_pred the three derivative maps as well (the query's size)
  const size_t part_bytes = sizeof(double) * 3 * (size_t)p.partials;
  const bool grad_ssim = d_pred != nullptr && ssim_weight > 0.f;
  SFX_REQUIRE(ws_bytes >= part_bytes + (grad_ssim ? sizeof(float) * 3 * (size_t)p.elems : 0),
              "sfx_image_loss: workspace too small");
  SFX_REQUIRE(!d_pred || (!overlaps(d_pred, pred, p.elems) && !overlaps(d_pred, gt, p.elems)),
              "sfx_image_loss: d_pred aliases an input");
  hipStream_t st = sfx::as_stream(stream);
  double* partial = reinterpret_cast<double*>(ws);
  float* maps = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + part_bytes);
  const dim3 grid((unsigned)p.tiles_x, (unsigned)p.tiles_y, (unsigned)(num_images * channels));
  const double denom = (double)channels * height * width;
  loss_moments_kernel<<<grid, THREADS, 0, st>>>(height, width, channels, pred, gt, window, partial,
                                                 grad_ssim ? maps : nullptr, p.elems);
  loss_reduce_kernel<<<num_images, THREADS, 0, st>>>((long long)channels * p.tiles_x * p.tiles_y, denom, l1_weight,
                                                      ssim_weight, partial, terms);
  if (d_pred) {
    if (grad_ssim)
      loss_grad_kernel<true><<<grid, THREADS, 0, st>>>(height, width, channels, pred, gt, window, maps, p.elems,
                                                        l1_weight, ssim_weight, view_scale, denom, d_pred);
    else
      loss_grad_kernel<false><<<grid, THREADS, 0, st>>>(height, width, channels, pred, gt, window, nullptr, 0,
                                                         l1_weight, ssim_weight, view_scale, denom, d_pred);
  }
  return sfx::check_launch("sfx_image_loss");
}

}  // extern "C"

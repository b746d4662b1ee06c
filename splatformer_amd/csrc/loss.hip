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
#include "common.h"

namespace {

constexpr int LT_X = 32, LT_Y = 16, LR = 5, LW = 11;
constexpr int LS_X = LT_X + 2 * LR, LS_Y = LT_Y + 2 * LR;
constexpr int LTHREADS = 256;
constexpr double LC1 = 0.01 * 0.01, LC2 = 0.03 * 0.03;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// maps != NULL: also write the derivative maps (plane stride `plane` elements) for pass B.  One instantiation, so
// the terms have the same bits with and without a gradient.
__global__ void __launch_bounds__(LTHREADS) loss_moments_kernel(int H, int W, int C, const float* __restrict__ pred,
                                                                const float* __restrict__ gt,
                                                                const float* __restrict__ taps,
                                                                double* __restrict__ partial,
                                                                float* __restrict__ maps, long long plane) {
  __shared__ float sp[LS_Y][LS_X + 1], sg[LS_Y][LS_X + 1];
  __shared__ double hm[5][LS_Y][LT_X];
  __shared__ double sw[LW];
  __shared__ double red[LTHREADS / 64][3];
  const int img = blockIdx.z / C, c = blockIdx.z % C;
  const int x0 = blockIdx.x * LT_X - LR, y0 = blockIdx.y * LT_Y - LR;
  const long long base = (long long)img * H * W * C;
  double l1 = 0.0, l2 = 0.0, sm = 0.0;
  for (int i = threadIdx.x; i < LS_Y * LS_X; i += LTHREADS) {
    const int yy = i / LS_X, xx = i % LS_X;
    const int y = y0 + yy, x = x0 + xx;
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    float a = 0.f, b = 0.f;
    if (in) {
      const long long o = base + ((long long)y * W + x) * C + c;
      a = pred[o];
      b = gt[o];
      if (yy >= LR && yy < LR + LT_Y && xx >= LR && xx < LR + LT_X) {  // the tile's own pixels
        const double d = (double)a - (double)b;
        l1 += fabs(d);
        l2 += d * d;
      }
    }
    sp[yy][xx] = a;
    sg[yy][xx] = b;
  }
  if (threadIdx.x < LW) sw[threadIdx.x] = (double)taps[threadIdx.x];
  __syncthreads();
  for (int i = threadIdx.x; i < LS_Y * LT_X; i += LTHREADS) {  // rows: 11 columns
    const int yy = i / LT_X, x = i % LT_X;
    double m1 = 0.0, m2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
#pragma unroll
    for (int j = 0; j < LW; ++j) {
      const double w = sw[j], a = sp[yy][x + j], b = sg[yy][x + j];
      m1 = fma(w, a, m1);
      m2 = fma(w, b, m2);
      s11 = fma(w, a * a, s11);
      s22 = fma(w, b * b, s22);
      s12 = fma(w, a * b, s12);
    }
    hm[0][yy][x] = m1;
    hm[1][yy][x] = m2;
    hm[2][yy][x] = s11;
    hm[3][yy][x] = s22;
    hm[4][yy][x] = s12;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < LT_Y * LT_X; i += LTHREADS) {  // columns: 11 rows
    const int ty = i / LT_X, tx = i % LT_X;
    const int y = blockIdx.y * LT_Y + ty, x = blockIdx.x * LT_X + tx;
    if (y >= H || x >= W) continue;
    double mu1 = 0.0, mu2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
    for (int j = 0; j < LW; ++j) {
      const double w = sw[j];
      mu1 = fma(w, hm[0][ty + j][tx], mu1);
      mu2 = fma(w, hm[1][ty + j][tx], mu2);
      e11 = fma(w, hm[2][ty + j][tx], e11);
      e22 = fma(w, hm[3][ty + j][tx], e22);
      e12 = fma(w, hm[4][ty + j][tx], e12);
    }
    const double A1 = 2.0 * mu1 * mu2 + LC1, A2 = 2.0 * (e12 - mu1 * mu2) + LC2;
    const double B1 = mu1 * mu1 + mu2 * mu2 + LC1, B2 = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + LC2;
    const double rb = 1.0 / (B1 * B2);
    const double m = A1 * A2 * rb;
    sm += m;
    if (maps) {
      const long long o = base + ((long long)y * W + x) * C + c;
      maps[o] = (float)(2.0 * mu2 * (A2 - A1) * rb - 2.0 * mu1 * m / B1 + 2.0 * mu1 * m / B2);
      maps[plane + o] = (float)(-m / B2);
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
    for (int w = 0; w < LTHREADS / 64; ++w) s += red[w][threadIdx.x];
    const long long tiles = (long long)gridDim.x * gridDim.y;
    const long long t = (long long)blockIdx.z * tiles + (long long)blockIdx.y * gridDim.x + blockIdx.x;
    partial[t * 3 + threadIdx.x] = s;
  }
}

// terms[v] = mean|p-g|, SSIM mean, mean (p-g)^2, l1_weight * [0] + ssim_weight * (1 - [1])
__global__ void __launch_bounds__(LTHREADS) loss_reduce_kernel(long long per_view, double denom, float l1_weight,
                                                               float ssim_weight, const double* __restrict__ partial,
                                                               float* __restrict__ terms) {
  __shared__ double red[3][LTHREADS];
  double s[3] = {0.0, 0.0, 0.0};
  const double* p = partial + (long long)blockIdx.x * per_view * 3;
  for (long long i = threadIdx.x; i < per_view; i += LTHREADS) {
    s[0] += p[i * 3 + 0];
    s[1] += p[i * 3 + 1];
    s[2] += p[i * 3 + 2];
  }
  for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int o = LTHREADS / 2; o >= 1; o >>= 1) {
    if (threadIdx.x < o)
      for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double l1 = red[0][0] / denom, mse = red[1][0] / denom, ssim = red[2][0] / denom;
    float* t = terms + (long long)blockIdx.x * 4;
    t[0] = (float)l1;
    t[1] = (float)ssim;
    t[2] = (float)mse;
    t[3] = (float)((double)l1_weight * l1 + (double)ssim_weight * (1.0 - ssim));
  }
}

// SSIM: convolve the three maps and combine; otherwise the L1 sign term alone (the maps are not read)
template <bool SSIM>
__global__ void __launch_bounds__(LTHREADS) loss_grad_kernel(int H, int W, int C, const float* __restrict__ pred,
                                                             const float* __restrict__ gt,
                                                             const float* __restrict__ taps,
                                                             const float* __restrict__ maps, long long plane,
                                                             float l1_weight, float ssim_weight,
                                                             const float* __restrict__ view_scale, double denom,
                                                             float* __restrict__ d_pred) {
  __shared__ float sd[SSIM ? 3 : 1][LS_Y][LS_X + 1];
  __shared__ double hd[SSIM ? 3 : 1][LS_Y][LT_X];
  __shared__ double sw[LW];
  const int img = blockIdx.z / C, c = blockIdx.z % C;
  const long long base = (long long)img * H * W * C;
  const double vs = view_scale ? (double)view_scale[img] : 1.0;
  const double cl1 = (double)l1_weight * vs / denom;  // sign's coefficient, rounded to fp32 once at the store
  const double cs = -(double)ssim_weight * vs / denom;
  if (SSIM) {
    const int x0 = blockIdx.x * LT_X - LR, y0 = blockIdx.y * LT_Y - LR;
    for (int i = threadIdx.x; i < LS_Y * LS_X; i += LTHREADS) {
      const int yy = i / LS_X, xx = i % LS_X;
      const int y = y0 + yy, x = x0 + xx;
      const bool in = y >= 0 && y < H && x >= 0 && x < W;
      const long long o = base + ((long long)y * W + x) * C + c;
#pragma unroll
      for (int k = 0; k < 3; ++k) sd[k][yy][xx] = in ? maps[k * plane + o] : 0.f;
    }
    if (threadIdx.x < LW) sw[threadIdx.x] = (double)taps[threadIdx.x];
    __syncthreads();
    for (int i = threadIdx.x; i < LS_Y * LT_X; i += LTHREADS) {
      const int yy = i / LT_X, x = i % LT_X;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
      for (int j = 0; j < LW; ++j) {
        const double w = sw[j];
        a0 = fma(w, (double)sd[0][yy][x + j], a0);
        a1 = fma(w, (double)sd[1][yy][x + j], a1);
        a2 = fma(w, (double)sd[2][yy][x + j], a2);
      }
      hd[0][yy][x] = a0;
      hd[1][yy][x] = a1;
      hd[2][yy][x] = a2;
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < LT_Y * LT_X; i += LTHREADS) {
    const int ty = i / LT_X, tx = i % LT_X;
    const int y = blockIdx.y * LT_Y + ty, x = blockIdx.x * LT_X + tx;
    if (y >= H || x >= W) continue;
    const long long o = base + ((long long)y * W + x) * C + c;
    const double p = pred[o], g = gt[o];
    const double sgn = p > g ? 1.0 : (p < g ? -1.0 : 0.0);  // sign(0) = 0 (torch's abs backward)
    double out = cl1 * sgn;
    if (SSIM) {
      double c0 = 0.0, c1 = 0.0, c2 = 0.0;
#pragma unroll
      for (int j = 0; j < LW; ++j) {
        const double w = sw[j];
        c0 = fma(w, hd[0][ty + j][tx], c0);
        c1 = fma(w, hd[1][ty + j][tx], c1);
        c2 = fma(w, hd[2][ty + j][tx], c2);
      }
      out += cs * (c0 + 2.0 * p * c1 + g * c2);
    }
    d_pred[o] = (float)out;
  }
}

struct LossPlan {
  long long tiles_x, tiles_y, elems, partials;
};

// false: a non-positive size, or more than 2^40 elements (so every index below fits a long long with room)
bool loss_plan(int V, int H, int W, int C, LossPlan* p) {
  if (V < 0 || H <= 0 || W <= 0 || C <= 0) return false;
  if ((double)V * H * W * C > (double)(1LL << 40)) return false;
  p->tiles_x = sfx::ceil_div(W, LT_X);
  p->tiles_y = sfx::ceil_div(H, LT_Y);
  p->elems = (long long)V * H * W * C;
  p->partials = (long long)V * C * p->tiles_x * p->tiles_y;
  return true;
}

bool overlaps(const float* a, const float* b, long long n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
  return x < y + bytes && y < x + bytes;
}

}  // namespace

extern "C" {

size_t sfx_image_loss_workspace_bytes(int num_images, int height, int width, int channels) {
  LossPlan p;
  if (!loss_plan(num_images, height, width, channels, &p)) return 0;  // sfx_image_loss refuses these sizes
  return sizeof(double) * 3 * (size_t)p.partials + sizeof(float) * 3 * (size_t)p.elems;
}

int sfx_image_loss(int num_images, int height, int width, int channels, const float* pred, const float* gt,
                   const float* window, float l1_weight, float ssim_weight, const float* view_scale, float* terms,
                   float* d_pred, void* ws, size_t ws_bytes, void* stream) {
  sfx::clear_error();
  LossPlan p;
  SFX_REQUIRE(loss_plan(num_images, height, width, channels, &p),
              "sfx_image_loss: bad sizes (%d images of %d x %d x %d; at most 2^40 elements)", num_images, height, width,
              channels);
  SFX_REQUIRE(l1_weight >= 0.f && ssim_weight >= 0.f, "sfx_image_loss: negative (or NaN) loss weight");
  if (num_images == 0) return SFX_OK;
  SFX_REQUIRE((long long)num_images * channels <= 65535,
              "sfx_image_loss: at most 65535 view-channels per call (got %lld)", (long long)num_images * channels);
  SFX_REQUIRE(p.tiles_y <= 65535, "sfx_image_loss: height above %d", 65535 * LT_Y);
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
  loss_moments_kernel<<<grid, LTHREADS, 0, st>>>(height, width, channels, pred, gt, window, partial,
                                                 grad_ssim ? maps : nullptr, p.elems);
  loss_reduce_kernel<<<num_images, LTHREADS, 0, st>>>((long long)channels * p.tiles_x * p.tiles_y, denom, l1_weight,
                                                      ssim_weight, partial, terms);
  if (d_pred) {
    if (grad_ssim)
      loss_grad_kernel<true><<<grid, LTHREADS, 0, st>>>(height, width, channels, pred, gt, window, maps, p.elems,
                                                        l1_weight, ssim_weight, view_scale, denom, d_pred);
    else
      loss_grad_kernel<false><<<grid, LTHREADS, 0, st>>>(height, width, channels, pred, gt, window, nullptr, 0,
                                                         l1_weight, ssim_weight, view_scale, denom, d_pred);
  }
  return sfx::check_launch("sfx_image_loss");
}

}  // extern "C"

// Fused evaluation metrics of one scene's views: uint8 quantisation, the optional object mask of a 'real' scene,
// the exact integer PSNR moments and the SSIM of the quantised images, in one pass over the render and the target.
//
// Reference: train.py:104-113.  With an RGBA target (dataset/GS.py:128-151 appends the mask as a 4th channel) the
// prediction alone is multiplied by the mask, then both images are truncated to uint8; utils/metrics.py:26-29
// divides a batch by 255 when its max exceeds 1, :89-91 is the PSNR and :93-135 the SSIM (window 11, sigma 1.5,
// conv2d zero padding 5, C1 = 0.01^2, C2 = 0.03^2, mean over channels and pixels; no mask weighting).
//
// Per pixel and channel, in the reference's order: p = pred (fminf(p, 1) when clamp_pred), p = p * m with a mask
// (one fp32 multiply), qp = (int)(p * 255.f) (a second fp32 multiply, truncated, saturated to [0, 255]) and
// qg = (int)(g * 255.f): the target is not masked.  The two multiplies stay separate, so the integer moments are
// the ones torch forms on the host, bit for bit.
//
// Layout: one workgroup of 256 threads per 32 x 16 output tile of ALL THREE channels of one view, grid
// (tiles_x, tiles_y, V).
//   stage    every thread quantises whole pixels of the 42 x 26 halo: three consecutive floats of pred, and of an
//            RGBA target one 16-byte load that yields r, g, b and the mask together (a dense mask plane or a
//            3-channel target take scalar loads: the same arithmetic, other addresses).  The quantised values go to
//            LDS as bytes (zero outside the image = the padding): 6.7 KB for both images and three channels.  The
//            tile's own pixels add to the integer moments sum qp^2, sum qg^2, sum qp*qg and the two maxima here, so
//            pred and the target are read from HBM once, plus the halo overlap.
//   rows     per channel: a thread takes 4 adjacent columns of one halo row, reads its 14 bytes of each image as
//            four words, maps them through a 256-entry table of (float)q / 255.f (the reference's fp32 division)
//            and forms the five row moments w*p, w*g, w*p^2, w*g^2, w*pg of the 4 columns in fp64.
//   columns  a thread takes 2 vertically adjacent pixels: 12 rows of the five row moments serve both; the SSIM
//            map value in fp64, in the reference's order of operations with a true division.
// The window is separable (11 + 11 taps, as loss.hip): the caller passes the 11 fp32 taps g, the 2-D window is
// g_i * g_j in fp64 (the reference rounds each product to fp32 once, a relative 6e-8 per tap).  Sums run in fp64
// because e11 - mu1^2 cancels; the inputs are 8-bit, so fp64 leaves no visible rounding.
// The tile's SSIM sum goes to a per-(view, tile) fp64 partial; a second kernel adds a view's partials in a fixed
// order.  No float atomics: the same inputs give the same bits.  The integer moments use 64-bit integer atomics
// (one per quantity and workgroup); integer addition is exact in any order.
#include "image_common.h"

namespace {

using namespace sfxi;

constexpr int EPITCH = 44;  // bytes per staged halo row: 42 used; groups of 4 columns read 16 bytes from 4 * group
constexpr int EGROUPS = TILE_X / 4;
static_assert(4 * (EGROUPS - 1) + 16 <= EPITCH && HALO_X <= EPITCH && EPITCH % 4 == 0, "row pitch");
static_assert(TILE_X * TILE_Y == 2 * THREADS, "two output pixels per thread");

// the reference's order of operations, with a true division
__device__ __forceinline__ double ssim_value(double mu1, double mu2, double e11, double e22, double e12) {
  const SsimTerms t = ssim_terms(mu1, mu2, e11, e22, e12);
  return ((2.0 * t.mu12 + C1) * t.A2) / (t.B1 * t.B2);
}

// RGBA: gt is [V][H][W][4], 16-byte aligned, and its 4th channel is the mask (gs, mask, ms are not read)
template <bool RGBA>
__global__ void __launch_bounds__(THREADS) eval_metrics_kernel(int H, int W, const float* __restrict__ pred,
                                                                const float* __restrict__ gt, int gs,
                                                                const float* __restrict__ mask, int ms,
                                                                int clamp_pred, const float* __restrict__ taps,
                                                                unsigned long long* __restrict__ sums,
                                                                int* __restrict__ maxes,
                                                                double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) unsigned char sp[3][HALO_Y][EPITCH];
  __shared__ __attribute__((aligned(16))) unsigned char sg[3][HALO_Y][EPITCH];
  __shared__ double hm[5][HALO_Y][TILE_X];
  __shared__ double sw[WIN];
  __shared__ float lut[256];
  __shared__ double red[THREADS / 64];
  __shared__ unsigned isum[3];
  __shared__ int imax[2];
  const int tid = threadIdx.x;
  const int img = blockIdx.z;
  const long long img_px = (long long)img * H * W;

  lut[tid] = unquant_u8(tid);
  if (tid < WIN) sw[tid] = (double)taps[tid];
  if (tid < 3) isum[tid] = 0u;
  if (tid < 2) imax[tid] = 0;

  unsigned spp = 0u, sgg = 0u, spg = 0u;
  int mp = 0, mg = 0;
  for (int i = tid; i < HALO_Y * HALO_X; i += THREADS) {
    const HaloPx h = halo_px(i, H, W);
    int qa[3] = {0, 0, 0}, qb[3] = {0, 0, 0};
    if (h.in) {
      const long long px = img_px + (long long)h.y * W + h.x;
      const float* pp = pred + px * 3;
      float p[3] = {pp[0], pp[1], pp[2]};
      float g[3], m = 1.f;
      bool has_mask;
      if (RGBA) {
        const float4 v = *reinterpret_cast<const float4*>(gt + px * 4);
        g[0] = v.x;
        g[1] = v.y;
        g[2] = v.z;
        m = v.w;
        has_mask = true;
      } else {
        const float* gp = gt + px * gs;
        g[0] = gp[0];
        g[1] = gp[1];
        g[2] = gp[2];
        has_mask = mask != nullptr;
        if (has_mask) m = mask[px * ms];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v = p[c];
        if (clamp_pred) v = fminf(v, 1.f);
        if (has_mask) v = v * m;  // its own rounding, before the * 255.f of quant_u8
        qa[c] = quant_u8(v);
        qb[c] = quant_u8(g[c]);
      }
      if (h.own) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          spp += (unsigned)(qa[c] * qa[c]);
          sgg += (unsigned)(qb[c] * qb[c]);
          spg += (unsigned)(qa[c] * qb[c]);
          mp = max(mp, qa[c]);
          mg = max(mg, qb[c]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sp[c][h.yy][h.xx] = (unsigned char)qa[c];
      sg[c][h.yy][h.xx] = (unsigned char)qb[c];
    }
  }
  // a workgroup's sums stay below 512 * 3 * 255^2 < 2^27
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    spp += __shfl_xor(spp, o, 64);
    sgg += __shfl_xor(sgg, o, 64);
    spg += __shfl_xor(spg, o, 64);
    mp = max(mp, __shfl_xor(mp, o, 64));
    mg = max(mg, __shfl_xor(mg, o, 64));
  }
  __syncthreads();  // the staged bytes, the table, the taps, the zeroed counters
  if ((tid & 63) == 0) {
    atomicAdd(&isum[0], spp);
    atomicAdd(&isum[1], sgg);
    atomicAdd(&isum[2], spg);
    atomicMax(&imax[0], mp);
    atomicMax(&imax[1], mg);
  }

  double w[WIN];
#pragma unroll
  for (int j = 0; j < WIN; ++j) w[j] = sw[j];
  const int tx = tid % TILE_X, ty = 2 * (tid / TILE_X);
  const int ox = blockIdx.x * TILE_X + tx, oy = blockIdx.y * TILE_Y + ty;
  double sm = 0.0;
  for (int c = 0; c < 3; ++c) {
    if (tid < HALO_Y * EGROUPS) {  // rows: 4 columns x 11 taps from 14 staged values of each image
      const int yy = tid / EGROUPS, gx = 4 * (tid % EGROUPS);
      const unsigned* ra = reinterpret_cast<const unsigned*>(&sp[c][yy][gx]);  // 4-byte aligned: pitch and gx are
      const unsigned* rb = reinterpret_cast<const unsigned*>(&sg[c][yy][gx]);
      const unsigned wa[4] = {ra[0], ra[1], ra[2], ra[3]}, wb[4] = {rb[0], rb[1], rb[2], rb[3]};
      double acc[4][5];
#pragma unroll
      for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[o][k] = 0.0;
#pragma unroll
      for (int j = 0; j < WIN + 3; ++j) {
        const double a = (double)lut[(wa[j >> 2] >> (8 * (j & 3))) & 255u];
        const double b = (double)lut[(wb[j >> 2] >> (8 * (j & 3))) & 255u];
        const double aa = a * a, bb = b * b, ab = a * b;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          if (j - o >= 0 && j - o < WIN) {  // resolved at compile time: taps in ascending order for every column
            const double wt = w[j - o];
            acc[o][0] = fma(wt, a, acc[o][0]);
            acc[o][1] = fma(wt, b, acc[o][1]);
            acc[o][2] = fma(wt, aa, acc[o][2]);
            acc[o][3] = fma(wt, bb, acc[o][3]);
            acc[o][4] = fma(wt, ab, acc[o][4]);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int o = 0; o < 4; ++o) hm[k][yy][gx + o] = acc[o][k];
    }
    __syncthreads();
    {  // columns: 12 rows of row moments for the pixels (ty, tx) and (ty + 1, tx)
      double c0[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, c1[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < WIN + 1; ++r) {
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const double v = hm[k][ty + r][tx];
          if (r < WIN) c0[k] = fma(w[r], v, c0[k]);
          if (r >= 1) c1[k] = fma(w[r - 1], v, c1[k]);
        }
      }
      if (ox < W && oy < H) sm += ssim_value(c0[0], c0[1], c0[2], c0[3], c0[4]);
      if (ox < W && oy + 1 < H) sm += ssim_value(c1[0], c1[1], c1[2], c1[3], c1[4]);
    }
    __syncthreads();  // hm is rewritten by the next channel; after the last one: the counters are complete
  }
  sm = wave_sum_f64(sm);
  if ((tid & 63) == 0) red[tid >> 6] = sm;
  if (tid < 3) atomicAdd(&sums[(long long)img * 3 + tid], (unsigned long long)isum[tid]);
  if (tid >= 64 && tid < 66) atomicMax(&maxes[(long long)img * 2 + (tid - 64)], imax[tid - 64]);
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < THREADS / 64; ++i) s += red[i];
    const long long tiles = (long long)gridDim.x * gridDim.y;
    partial[(long long)img * tiles + (long long)blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

__global__ void __launch_bounds__(THREADS) eval_ssim_reduce_kernel(long long per_view, double denom,
                                                                    const double* __restrict__ partial,
                                                                    float* __restrict__ out) {
  double s[1];
  view_reduce<1>(per_view, partial, s);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)(s[0] / denom);
}

}  // namespace

extern "C" {

// the plan of a view's pixels: one tile covers all three channels
size_t sfx_eval_metrics_workspace_bytes(int num_images, int height, int width) {
  ImagePlan p;
  if (!image_plan(num_images, height, width, 1, &p)) return 0;  // sfx_eval_metrics_u8 refuses these sizes
  return sizeof(double) * (size_t)p.partials;
}

int sfx_eval_metrics_u8(int num_images, int height, int width, const float* pred, const float* gt,
                        int gt_pixel_stride, const float* mask, int mask_pixel_stride, int clamp_pred,
                        const float* window, unsigned long long* sums, int* maxes, float* ssim, void* ws,
                        size_t ws_bytes, void* stream) {
  sfx::clear_error();
  ImagePlan p;
  SFX_REQUIRE(image_plan(num_images, height, width, 1, &p),
              "sfx_eval_metrics_u8: bad sizes (%d images of %d x %d; at most 2^40 pixels)", num_images, height, width);
  SFX_REQUIRE(gt_pixel_stride == 3 || gt_pixel_stride == 4,
              "sfx_eval_metrics_u8: gt_pixel_stride must be 3 or 4 (got %d)", gt_pixel_stride);
  SFX_REQUIRE(!mask || mask_pixel_stride == 1 || mask_pixel_stride == 4,
              "sfx_eval_metrics_u8: mask_pixel_stride must be 1 or 4 (got %d)", mask_pixel_stride);
  if (num_images == 0) return SFX_OK;
  SFX_REQUIRE(p.grid_z_fits, "sfx_eval_metrics_u8: at most 65535 images per call (got %d)", num_images);
  SFX_REQUIRE(p.grid_y_fits, "sfx_eval_metrics_u8: height above %d", 65535 * TILE_Y);
  SFX_REQUIRE(pred && gt && window && sums && maxes && ssim && ws, "sfx_eval_metrics_u8: null buffer");
  SFX_REQUIRE((uintptr_t)ws % 8 == 0, "sfx_eval_metrics_u8: workspace must be 8-byte aligned");
  SFX_REQUIRE(ws_bytes >= sizeof(double) * (size_t)p.partials, "sfx_eval_metrics_u8: workspace too small");
  hipStream_t st = sfx::as_stream(stream);
  if (hipMemsetAsync(sums, 0, sizeof(unsigned long long) * 3 * num_images, st) != hipSuccess ||
      hipMemsetAsync(maxes, 0, sizeof(int) * 2 * num_images, st) != hipSuccess) {
    sfx::set_error("sfx_eval_metrics_u8: memset failed");
    return SFX_ERR_HIP;
  }
  double* partial = reinterpret_cast<double*>(ws);
  const dim3 grid((unsigned)p.tiles_x, (unsigned)p.tiles_y, (unsigned)num_images);
  // the mask as the 4th channel of an aligned RGBA target: one 16-byte load per pixel
  const bool rgba = gt_pixel_stride == 4 && mask == gt + 3 && mask_pixel_stride == 4 && (uintptr_t)gt % 16 == 0;
  if (rgba)
    eval_metrics_kernel<true><<<grid, THREADS, 0, st>>>(height, width, pred, gt, 4, mask, 4, clamp_pred, window,
                                                         sums, maxes, partial);
  else
    eval_metrics_kernel<false><<<grid, THREADS, 0, st>>>(height, width, pred, gt, gt_pixel_stride, mask,
                                                          mask_pixel_stride, clamp_pred, window, sums, maxes,
                                                          partial);
  eval_ssim_reduce_kernel<<<num_images, THREADS, 0, st>>>(p.tiles_x * p.tiles_y, 3.0 * height * width, partial,
                                                           ssim);
  return sfx::check_launch("sfx_eval_metrics_u8");
}

}  // extern "C"

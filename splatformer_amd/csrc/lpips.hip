// LPIPS(net='vgg') building blocks (reference train.py:269-282, utils/metrics.py:13-17): the frozen VGG16 feature
// stack on NHWC fp32 images and the per-tap distance, forward and data backward.  No weight gradients.
//
//   sfx_lpips_input / _bwd   x in [0,1] (optionally masked and uint8-quantised) -> u = ((2x - 1) - shift) / scale
//   sfx_conv3x3_pack         torch weights [Cout][Cin][3][3] -> MFMA fragments (or, rotated by 180 degrees with in/out
//                            transposed, the weights of the data backward)
//   sfx_conv3x3              y = act(conv3x3(x) + b) [* (mask_src > 0)], zero padding 1, stride 1
//   sfx_maxpool2x2 / _bwd    2x2 / stride 2 max pool, floor semantics; backward adds into dx at the first maximum
//   sfx_tap_normalize        f^ = f / (sqrt(sum_c f^2) + 1e-10)
//   sfx_tap_dist / _bwd      sum_c w_c (f^x - f^y)^2 per pixel, per-image means; d/d fx
//
// Convolution (Cin % 32 == 0 and Cout % 64 == 0): an implicit GEMM, pixels on the A rows, output channels on the
// B columns, in the project's fp32-accurate operand form (gemm_kernel.h: every operand a power-of-two scaled pair
// of fp16 terms h + l, a 32x32x16 block = l*h + h*l + h*h on v_mfma_f32_32x32x16_f16, fp32 accumulation).  A
// workgroup (4 waves) owns an 8 x 16 pixel tile of one image and 128 (or 64) output channels.  Per 32-channel
// chunk of Cin it stages the tile plus its one-pixel halo (10 x 18 pixels) in LDS ONCE, already split, and all 9
// taps read their shifted A fragments from it; halo pixels outside the image are written as zeros, so a row never
// reads across an image edge or into the next image.  The weights are packed once in fragment order and stream
// from L2 straight into registers (every workgroup walks the same (chunk, tap) sequence).
//
// Scales: a GEMM row here is 9 pixels' channel vectors, and neighbouring rows share pixels, so the activation
// scale cannot be per row: it is per IMAGE (max |x| over the image, found by a reduction pass in front of the conv,
// an integer atomicMax of float bits: order independent).  Elements far below the image maximum lose bits of l
// only below 2^-24 of that maximum.  Weight rows (output channels) are scaled by their own maxima.
//
// Every floating-point sum has one fixed order (MFMA chains, in-wave butterflies, one thread's sequential loops):
// two calls give equal bits.  There are no floating-point atomics.
#include "gemm_common.h"
#include "image_common.h"

namespace {

using namespace sfxg;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int TH = 8, TW = 16;                  // pixel tile of the MFMA conv
constexpr int HALO_W = TW + 2, NHALO = (TH + 2) * HALO_W;
constexpr int KC = 32;                          // input channels per staged chunk
constexpr int PXB = 144;                        // LDS bytes per halo pixel: 32 h + 32 l fp16 + 16 pad (pixel p starts
                                                // at bank 4 p mod 32: 8 consecutive pixels' 16-byte reads tile the banks)
constexpr int NSLOT = NHALO * (KC / 4);         // float4 slots of a chunk
constexpr int SLOTS_PER_THREAD = (NSLOT + THREADS - 1) / THREADS;
constexpr long long MAX_BYTES = 1LL << 31;      // operands of 2 GiB or more are refused

__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// ---- image maxima ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) image_absmax_kernel(long long per_image4, const float4* __restrict__ x,
                                                           unsigned* __restrict__ amax) {
  __shared__ float sm[4];
  const int n = blockIdx.y;
  const float4* p = x + (long long)n * per_image4;
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per_image4; i += (long long)gridDim.x * 256) {
    const float4 v = p[i];
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
  }
  m = sfx::wave_max(m);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    atomicMax(amax + n, __builtin_bit_cast(unsigned, m));  // non-negative floats order as their bits
  }
}

// ---- MFMA convolution -----------------------------------------------------------------------------------------
struct ConvArgs {
  int V, H, W, C, N;
  const float* x;
  const char* wp;      // packed fragments
  const float* winv;   // [N] inverse weight-row scales
  const float* bias;   // [N] or null
  const float* mask;   // [V,H,W,N] or null: output *= (mask > 0)
  int relu;
  float* y;
  const float* amax;   // [V] max |x| per image
  int tiles_x, tiles_y;
};

// waves: WM x WN; a wave computes MI 32-pixel blocks x NI 32-channel blocks.  WM * MI = 4 (the 128-pixel tile)
template <int WM, int WN, int MI, int NI>
__global__ void __launch_bounds__(THREADS) conv3x3_mfma_kernel(ConvArgs a) {
  static_assert(WM * WN == 4 && WM * MI * 32 == TH * TW, "tile shape");
  __shared__ __attribute__((aligned(16))) char lds[NHALO * PXB];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r32 = lane & 31, hh = lane >> 5;
  const int wm = wid % WM, wn = wid / WM;
  const int tile = blockIdx.x;
  const int x0 = (tile % a.tiles_x) * TW;
  const int y0 = ((tile / a.tiles_x) % a.tiles_y) * TH;
  const int n = tile / (a.tiles_x * a.tiles_y);
  const int nb0 = ((int)blockIdx.y * WN + wn) * NI;  // first 32-channel block of this wave
  const int KCH = a.C / KC;
  float inv_a;
  const float sc = sfx::pow2_scale(a.amax[n], inv_a);

  // staging slots of this thread: slot j = (halo pixel j / 8, channels 4 (j % 8) ..); -1: padding or no slot
  int goff[SLOTS_PER_THREAD], loff[SLOTS_PER_THREAD];
#pragma unroll
  for (int i = 0; i < SLOTS_PER_THREAD; ++i) {
    const int j = tid + THREADS * i;
    const int px = j >> 3, q = j & 7;
    const int gy = y0 + px / HALO_W - 1, gx = x0 + px % HALO_W - 1;
    loff[i] = j < NSLOT ? px * PXB + q * 8 : -1;
    goff[i] = (j < NSLOT && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
                  ? (((n * a.H + gy) * a.W + gx) * a.C + q * 4) : -1;
  }
  float4 reg[SLOTS_PER_THREAD];
  auto gload = [&](int kc) {
#pragma unroll
    for (int i = 0; i < SLOTS_PER_THREAD; ++i)
      reg[i] = goff[i] >= 0 ? *reinterpret_cast<const float4*>(a.x + goff[i] + kc * KC) : make_float4(0.f, 0.f, 0.f, 0.f);
  };

  floatx16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mi][ni][i] = 0.f;

  // A fragment base of this lane per pixel block: pixel (2 mb + r32 / 16, r32 % 16) of the tile, halo origin (0, 0)
  int abase[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
    abase[mi] = ((2 * (wm * MI + mi) + (r32 >> 4)) * HALO_W + (r32 & 15)) * PXB + hh * 16;

  gload(0);
  for (int kc = 0; kc < KCH; ++kc) {
    __syncthreads();  // the previous chunk's fragment reads are done
#pragma unroll
    for (int i = 0; i < SLOTS_PER_THREAD; ++i)
      if (loff[i] >= 0) {
        uint2 t[2];
        split2h(reg[i], sc, t);
        *reinterpret_cast<uint2*>(lds + loff[i]) = t[0];
        *reinterpret_cast<uint2*>(lds + loff[i] + 64) = t[1];
      }
    __syncthreads();
    if (kc + 1 < KCH) gload(kc + 1);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        f16x8 ah[MI], al[MI], bh[NI], bl[NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const char* p = lds + abase[mi] + ((t / 3) * HALO_W + (t % 3)) * PXB + s * 32;
          ah[mi] = *reinterpret_cast<const f16x8*>(p);
          al[mi] = *reinterpret_cast<const f16x8*>(p + 64);
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          const char* p = a.wp + ((((size_t)((nb0 + ni) * KCH + kc) * 9 + t) * 2 + s) * 2) * 1024 + lane * 16;
          bh[ni] = *reinterpret_cast<const f16x8*>(p);
          bl[ni] = *reinterpret_cast<const f16x8*>(p + 1024);
        }
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) {
            floatx16 c = acc[mi][ni];
            c = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mi], bh[ni], c, 0, 0, 0);  // smallest terms first
            c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mi], bl[ni], c, 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mi], bh[ni], c, 0, 0, 0);
          }
      }
  }

  // epilogue: lane (r32, hh) holds channel 32 nb + r32 of pixels acc_row(i, hh) of each pixel block
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int ch = (nb0 + ni) * 32 + r32;
    const float s = inv_a * a.winv[ch];
    const float b = a.bias ? a.bias[ch] : 0.f;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int r = acc_row(i, hh);
        const int gy = y0 + 2 * (wm * MI + mi) + (r >> 4), gx = x0 + (r & 15);
        if (gy < a.H && gx < a.W) {
          const int idx = ((n * a.H + gy) * a.W + gx) * a.N + ch;
          float v = acc[mi][ni][i] * s + b;
          if (a.relu) v = fmaxf(v, 0.f);
          if (a.mask) v = a.mask[idx] > 0.f ? v : 0.f;
          a.y[idx] = v;
        }
      }
  }
}

// plain-VALU convolution (Cin = 3 forward, Cout = 3 backward): one thread per (pixel, output channel), weights
// [9][C][N] fp32, taps in row-major order, channels ascending
__global__ void __launch_bounds__(256) conv3x3_small_kernel(ConvArgs a, const float* __restrict__ wf, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ch = (int)(idx % a.N);
  const long long p = idx / a.N;
  const int gx = (int)(p % a.W), gy = (int)((p / a.W) % a.H), n = (int)(p / ((long long)a.W * a.H));
  float acc = 0.f;
  for (int t = 0; t < 9; ++t) {
    const int yy = gy + t / 3 - 1, xx = gx + t % 3 - 1;
    if (yy < 0 || yy >= a.H || xx < 0 || xx >= a.W) continue;
    const float* xp = a.x + (((long long)n * a.H + yy) * a.W + xx) * a.C;
    const float* wp = wf + (long long)t * a.C * a.N + ch;
    for (int c = 0; c < a.C; ++c) acc = fmaf(xp[c], wp[(long long)c * a.N], acc);
  }
  float v = acc + (a.bias ? a.bias[ch] : 0.f);
  if (a.relu) v = fmaxf(v, 0.f);
  if (a.mask) v = a.mask[idx] > 0.f ? v : 0.f;
  a.y[idx] = v;
}

// Cin = 3 (the network's first layer), N output channels (a multiple of 64, so a wave holds one pixel group): a
// thread keeps its channel's 27 weights in registers and walks C3_PIX pixels; the pixel's 27 inputs are
// wave-uniform.  Same sum order as conv3x3_small_kernel.
constexpr int C3_PIX = 16;
template <int N>
__global__ void __launch_bounds__(256) conv3x3_c3_kernel(ConvArgs a, const float* __restrict__ wf, long long npix) {
  static_assert(N % 64 == 0 && 256 % N == 0, "one pixel group per wave");
  const int ch = threadIdx.x % N;
  const int pg = __builtin_amdgcn_readfirstlane((int)threadIdx.x / N);
  float w[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) w[k] = wf[k * N + ch];
  const float b = a.bias ? a.bias[ch] : 0.f;
  const long long p0 = ((long long)blockIdx.x * (256 / N) + pg) * C3_PIX;
  for (int i = 0; i < C3_PIX; ++i) {
    const long long p = p0 + i;
    if (p >= npix) break;
    const int gx = (int)(p % a.W), gy = (int)((p / a.W) % a.H), n = (int)(p / ((long long)a.W * a.H));
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int yy = gy + t / 3 - 1, xx = gx + t % 3 - 1;
      if (yy < 0 || yy >= a.H || xx < 0 || xx >= a.W) continue;
      const float* xp = a.x + (((long long)n * a.H + yy) * a.W + xx) * 3;
      acc = fmaf(xp[0], w[3 * t], acc);
      acc = fmaf(xp[1], w[3 * t + 1], acc);
      acc = fmaf(xp[2], w[3 * t + 2], acc);
    }
    float v = acc + b;
    if (a.relu) v = fmaxf(v, 0.f);
    if (a.mask) v = a.mask[p * N + ch] > 0.f ? v : 0.f;
    a.y[p * N + ch] = v;
  }
}

// Cout = 3 (the first layer's data backward), C % 4 == 0: one thread per pixel and all three outputs; the weights
// [9][C][3] are wave-uniform.  Same sum order as conv3x3_small_kernel.
__global__ void __launch_bounds__(256) conv3x3_n3_kernel(ConvArgs a, const float* __restrict__ wf, long long npix) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const int gx = (int)(p % a.W), gy = (int)((p / a.W) % a.H), n = (int)(p / ((long long)a.W * a.H));
  float acc[3] = {0.f, 0.f, 0.f};
  for (int t = 0; t < 9; ++t) {
    const int yy = gy + t / 3 - 1, xx = gx + t % 3 - 1;
    if (yy < 0 || yy >= a.H || xx < 0 || xx >= a.W) continue;
    const float4* xp = reinterpret_cast<const float4*>(a.x + (((long long)n * a.H + yy) * a.W + xx) * a.C);
    const float* w = wf + (long long)t * a.C * 3;
    for (int c4 = 0; c4 < a.C / 4; ++c4) {
      const float4 v = xp[c4];
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int o = 0; o < 3; ++o) acc[o] = fmaf(e[j], w[(4 * c4 + j) * 3 + o], acc[o]);
    }
  }
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    float v = acc[o] + (a.bias ? a.bias[o] : 0.f);
    if (a.relu) v = fmaxf(v, 0.f);
    if (a.mask) v = a.mask[p * 3 + o] > 0.f ? v : 0.f;
    a.y[p * 3 + o] = v;
  }
}

__host__ __device__ inline bool conv_on_mfma(int cin, int cout) { return cin % KC == 0 && cout % 64 == 0; }

// effective weight of output channel n, input channel c, tap t of the packed convolution
__device__ __forceinline__ float weff(const float* w, int C, int N, int flip, int n, int c, int t) {
  return flip ? w[((long long)c * N + n) * 9 + (8 - t)] : w[((long long)n * C + c) * 9 + t];
}

__global__ void conv_pack_rowscale_kernel(int C, int N, int flip, const float* __restrict__ w, float* __restrict__ winv) {
  const int n = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  float m = 0.f;
  for (int k = lane; k < C * 9; k += 64) m = fmaxf(m, fabsf(weff(w, C, N, flip, n, k / 9, k % 9)));
  m = sfx::wave_max(m);
  float inv;
  (void)sfx::pow2_scale(m, inv);
  if (lane == 0) winv[n] = inv;
}

// one thread per packed fp16 pair position: ((((nb * KCH + kc) * 9 + t) * 2 + s) * 64 + lane) * 8 + j
__global__ void conv_pack_frag_kernel(int C, int N, int flip, const float* __restrict__ w,
                                      const float* __restrict__ winv, _Float16* __restrict__ out, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63), s = (int)((idx >> 9) & 1);
  long long r = idx >> 10;
  const int t = (int)(r % 9);
  r /= 9;
  const int KCH = C / KC;
  const int kc = (int)(r % KCH), nb = (int)(r / KCH);
  const int n = nb * 32 + (lane & 31), c = kc * KC + 16 * s + 8 * (lane >> 5) + j;
  const float x = weff(w, C, N, flip, n, c, t) / winv[n];  // winv is a power of two: exact
  const _Float16 h = (_Float16)x;
  const _Float16 l = (_Float16)(x - (float)h);
  const long long o = (((idx >> 10) * 2 + s) * 2) * 512 + lane * 8 + j;
  out[o] = h;
  out[o + 512] = l;
}

__global__ void conv_pack_small_kernel(int C, int N, int flip, const float* __restrict__ w, float* __restrict__ out) {
  const int idx = (int)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 9 * C * N) return;
  const int n = idx % N, c = (idx / N) % C, t = idx / (N * C);
  out[idx] = weff(w, C, N, flip, n, c, t);
}

// ---- pooling ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) maxpool_kernel(int H, int W, int C4, const float4* __restrict__ x,
                                                      float4* __restrict__ y, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int Ho = H / 2, Wo = W / 2;
  const int c = (int)(idx % C4);
  const long long p = idx / C4;
  const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
  const long long n = p / ((long long)Wo * Ho);
  const float4* s = x + ((n * H + 2 * oy) * W + 2 * ox) * C4 + c;
  const float4 a = s[0], b = s[C4], d = s[(long long)W * C4], e = s[(long long)W * C4 + C4];
  y[idx] = make_float4(fmaxf(fmaxf(a.x, b.x), fmaxf(d.x, e.x)), fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, e.y)),
                       fmaxf(fmaxf(a.z, b.z), fmaxf(d.z, e.z)), fmaxf(fmaxf(a.w, b.w), fmaxf(d.w, e.w)));
}

// dx[first maximum of the window] += dy (each input element belongs to at most one window: no atomics)
__global__ void __launch_bounds__(256) maxpool_bwd_kernel(int H, int W, int C, const float* __restrict__ x,
                                                          const float* __restrict__ dy, int relu_mask,
                                                          float* __restrict__ dx, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int Ho = H / 2, Wo = W / 2;
  const int c = (int)(idx % C);
  const long long p = idx / C;
  const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
  const long long n = p / ((long long)Wo * Ho);
  const long long base = ((n * H + 2 * oy) * W + 2 * ox) * C + c;
  const long long o[4] = {base, base + C, base + (long long)W * C, base + (long long)W * C + C};
  int k = 0;
  float m = x[o[0]];
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const float v = x[o[i]];
    if (v > m) {
      m = v;
      k = i;
    }
  }
  if (!relu_mask || m > 0.f) dx[o[k]] += dy[idx];
}

// ---- input stage -----------------------------------------------------------------------------------------------
__device__ __forceinline__ float in_shift(int c) { return c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f); }
__device__ __forceinline__ float in_scale(int c) { return c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f); }

__global__ void __launch_bounds__(256) lpips_input_kernel(long long total, const float* __restrict__ x,
                                                          const float* __restrict__ mask, int quantize,
                                                          float* __restrict__ u) {
#pragma clang fp contract(off)
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % 3);
  float p = x[idx];
  if (mask) p = p * mask[idx / 3];  // its own rounding, before the * 255.f (sfx_eval_metrics_u8)
  if (quantize) p = sfxi::unquant_u8(sfxi::quant_u8(p));
  u[idx] = ((2.f * p - 1.f) - in_shift(c)) / in_scale(c);
}

__global__ void __launch_bounds__(256) lpips_input_bwd_kernel(long long total, const float* __restrict__ du,
                                                              float* __restrict__ dx) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  dx[idx] = du[idx] * (2.f / in_scale((int)(idx % 3)));
}

// ---- tap distance ----------------------------------------------------------------------------------------------
constexpr float TAP_EPS = 1e-10f;

// one wave per pixel
__global__ void __launch_bounds__(256) tap_normalize_kernel(long long P, int C, const float* __restrict__ f,
                                                            float* __restrict__ fh) {
  const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (p >= P) return;
  const float* s = f + p * C;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) q = fmaf(s[c], s[c], q);
  q = sfx::wave_sum(q);
  const float inv = 1.f / (sqrtf(q) + TAP_EPS);
  for (int c = lane; c < C; c += 64) fh[p * C + c] = s[c] * inv;
}

__global__ void __launch_bounds__(256) tap_dist_kernel(long long P, int C, const float* __restrict__ fx,
                                                       const float* __restrict__ fhy, const float* __restrict__ w,
                                                       float* __restrict__ dpix) {
  const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (p >= P) return;
  const float* s = fx + p * C;
  const float* g = fhy + p * C;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) q = fmaf(s[c], s[c], q);
  q = sfx::wave_sum(q);
  const float inv = 1.f / (sqrtf(q) + TAP_EPS);
  float d = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float e = s[c] * inv - g[c];
    d = fmaf(w[c] * e, e, d);
  }
  d = sfx::wave_sum(d);
  if (lane == 0) dpix[p] = d;
}

// out[v] (+)= mean of dpix over image v: strided partial sums in fp64, a fixed LDS tree
__global__ void __launch_bounds__(256) tap_reduce_kernel(long long HW, const float* __restrict__ dpix, int accumulate,
                                                         float* __restrict__ out) {
  __shared__ double sm[256];
  const float* s = dpix + (long long)blockIdx.x * HW;
  double t = 0.0;
  for (long long i = threadIdx.x; i < HW; i += 256) t += (double)s[i];
  sm[threadIdx.x] = t;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float m = (float)(sm[0] / (double)HW);
    out[blockIdx.x] = accumulate ? out[blockIdx.x] + m : m;
  }
}

// d fx of gscale[v] * sum_pixels d: with q_c = 2 w_c (f^_c - y^_c), n = |f|:
//   d/df_k = q_k / (n + eps) - f_k (sum_c q_c f_c) / (n (n + eps)^2)      (second term 0 at n = 0)
__global__ void __launch_bounds__(256) tap_dist_bwd_kernel(long long P, long long HW, int C,
                                                           const float* __restrict__ fx, const float* __restrict__ fhy,
                                                           const float* __restrict__ w, const float* __restrict__ gscale,
                                                           int relu_mask, float* __restrict__ dfx) {
  const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (p >= P) return;
  const float* s = fx + p * C;
  const float* g = fhy + p * C;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) q = fmaf(s[c], s[c], q);
  q = sfx::wave_sum(q);
  const float nrm = sqrtf(q);
  const float inv = 1.f / (nrm + TAP_EPS);
  float dot = 0.f;
  for (int c = lane; c < C; c += 64) dot = fmaf(2.f * w[c] * (s[c] * inv - g[c]), s[c], dot);
  dot = sfx::wave_sum(dot);
  const float gs = gscale[p / HW];
  const float k2 = nrm > 0.f ? dot * inv * inv / nrm : 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = gs * (2.f * w[c] * (s[c] * inv - g[c]) * inv - s[c] * k2);
    dfx[p * C + c] = (!relu_mask || s[c] > 0.f) ? v : 0.f;
  }
}

inline bool fits(long long elems) { return elems > 0 && elems * 4 < MAX_BYTES; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline size_t amax_bytes(int V) { return ((size_t)V * 4 + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int sfx_conv3x3_tile(int* tile_h, int* tile_w) {
  if (tile_h) *tile_h = TH;
  if (tile_w) *tile_w = TW;
  return SFX_OK;
}

size_t sfx_conv3x3_pack_bytes(int cin, int cout) {
  if (cin < 1 || cout < 1 || (long long)cin * cout > (1LL << 24)) return 0;  // sfx_conv3x3_pack refuses these
  return conv_on_mfma(cin, cout) ? (size_t)cin * cout * 36 + (size_t)cout * 4 : (size_t)cin * cout * 36;
}

int sfx_conv3x3_pack(int cin, int cout, const float* w, int transpose_flip, void* packed, void* stream) {
  sfx::clear_error();
  SFX_REQUIRE(cin >= 1 && cout >= 1 && (long long)cin * cout <= (1LL << 24),
              "sfx_conv3x3_pack: bad channel counts (%d -> %d)", cin, cout);
  SFX_REQUIRE(w && packed, "sfx_conv3x3_pack: null buffer");
  SFX_REQUIRE(aligned16(packed), "sfx_conv3x3_pack: packed buffer must be 16-byte aligned");
  hipStream_t st = sfx::as_stream(stream);
  const int flip = transpose_flip ? 1 : 0;
  if (conv_on_mfma(cin, cout)) {
    float* winv = reinterpret_cast<float*>(reinterpret_cast<char*>(packed) + (size_t)cin * cout * 36);
    conv_pack_rowscale_kernel<<<sfx::ceil_div(cout, 4), 256, 0, st>>>(cin, cout, flip, w, winv);
    const long long total = (long long)cin * cout * 9;
    conv_pack_frag_kernel<<<sfx::ceil_div(total, 256), 256, 0, st>>>(cin, cout, flip, w, winv,
                                                                      reinterpret_cast<_Float16*>(packed), total);
  } else {
    conv_pack_small_kernel<<<sfx::ceil_div(9LL * cin * cout, 256), 256, 0, st>>>(cin, cout, flip, w,
                                                                                  reinterpret_cast<float*>(packed));
  }
  return sfx::check_launch("sfx_conv3x3_pack");
}

size_t sfx_conv3x3_workspace_bytes(int num_images) { return num_images < 1 ? 0 : amax_bytes(num_images); }

int sfx_conv3x3(int num_images, int height, int width, int cin, int cout, const float* x, const void* packed,
                const float* bias, const float* mask_src, int relu, float* y, void* ws, size_t ws_bytes,
                void* stream) {
  sfx::clear_error();
  SFX_REQUIRE(num_images >= 1 && height >= 1 && width >= 1 && cin >= 1 && cout >= 1,
              "sfx_conv3x3: bad sizes (%d images of %d x %d, %d -> %d channels)", num_images, height, width, cin, cout);
  const long long px = (long long)num_images * height * width;
  SFX_REQUIRE(fits(px * cin) && fits(px * cout), "sfx_conv3x3: an operand of 2 GiB or more (chunk over images)");
  SFX_REQUIRE(x && packed && y && ws, "sfx_conv3x3: null buffer");
  SFX_REQUIRE(aligned16(x) && aligned16(packed) && aligned16(ws), "sfx_conv3x3: buffers must be 16-byte aligned");
  SFX_REQUIRE(ws_bytes >= amax_bytes(num_images), "sfx_conv3x3: workspace too small");
  SFX_REQUIRE(x != y, "sfx_conv3x3: y aliases x");
  hipStream_t st = sfx::as_stream(stream);
  ConvArgs a;
  a.V = num_images, a.H = height, a.W = width, a.C = cin, a.N = cout;
  a.x = x, a.bias = bias, a.mask = mask_src, a.relu = relu, a.y = y;
  a.wp = reinterpret_cast<const char*>(packed);
  a.winv = reinterpret_cast<const float*>(a.wp + (size_t)cin * cout * 36);
  a.amax = reinterpret_cast<const float*>(ws);
  a.tiles_x = (int)sfx::ceil_div(width, TW), a.tiles_y = (int)sfx::ceil_div(height, TH);
  if (!conv_on_mfma(cin, cout)) {
    const long long total = px * cout;
    const float* wf = reinterpret_cast<const float*>(packed);
    if (cin == 3 && cout == 64)
      conv3x3_c3_kernel<64><<<sfx::ceil_div(px, 4 * C3_PIX), 256, 0, st>>>(a, wf, px);
    else if (cout == 3 && cin % 4 == 0)
      conv3x3_n3_kernel<<<sfx::ceil_div(px, 256), 256, 0, st>>>(a, wf, px);
    else
      conv3x3_small_kernel<<<sfx::ceil_div(total, 256), 256, 0, st>>>(a, wf, total);
    return sfx::check_launch("sfx_conv3x3");
  }
  if (hipMemsetAsync(ws, 0, amax_bytes(num_images), st) != hipSuccess) return sfx::check_launch("sfx_conv3x3");
  const long long per4 = (long long)height * width * cin / 4;
  const unsigned rb = (unsigned)(per4 / 2048 < 1 ? 1 : (per4 / 2048 > 256 ? 256 : per4 / 2048));
  image_absmax_kernel<<<dim3(rb, (unsigned)num_images), 256, 0, st>>>(per4, reinterpret_cast<const float4*>(x),
                                                                       reinterpret_cast<unsigned*>(ws));
  const unsigned tiles = (unsigned)((long long)num_images * a.tiles_x * a.tiles_y);
  if (cout % 128 == 0)
    conv3x3_mfma_kernel<2, 2, 2, 2><<<dim3(tiles, (unsigned)(cout / 128)), THREADS, 0, st>>>(a);
  else
    conv3x3_mfma_kernel<4, 1, 1, 2><<<dim3(tiles, (unsigned)(cout / 64)), THREADS, 0, st>>>(a);
  return sfx::check_launch("sfx_conv3x3");
}

int sfx_maxpool2x2(int num_images, int height, int width, int channels, const float* x, float* y, void* stream) {
  sfx::clear_error();
  SFX_REQUIRE(num_images >= 1 && height >= 2 && width >= 2 && channels >= 4 && channels % 4 == 0,
              "sfx_maxpool2x2: bad sizes (%d images of %d x %d x %d; channels a multiple of 4)", num_images, height,
              width, channels);
  SFX_REQUIRE(fits((long long)num_images * height * width * channels), "sfx_maxpool2x2: an operand of 2 GiB or more");
  SFX_REQUIRE(x && y, "sfx_maxpool2x2: null buffer");
  SFX_REQUIRE(aligned16(x) && aligned16(y), "sfx_maxpool2x2: buffers must be 16-byte aligned");
  const long long total = (long long)num_images * (height / 2) * (width / 2) * (channels / 4);
  maxpool_kernel<<<sfx::ceil_div(total, 256), 256, 0, sfx::as_stream(stream)>>>(
      height, width, channels / 4, reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(y), total);
  return sfx::check_launch("sfx_maxpool2x2");
}

int sfx_maxpool2x2_bwd(int num_images, int height, int width, int channels, const float* x, const float* dy,
                       int relu_mask, float* dx, void* stream) {
  sfx::clear_error();
  SFX_REQUIRE(num_images >= 1 && height >= 2 && width >= 2 && channels >= 1,
              "sfx_maxpool2x2_bwd: bad sizes (%d images of %d x %d x %d)", num_images, height, width, channels);
  SFX_REQUIRE(fits((long long)num_images * height * width * channels),
              "sfx_maxpool2x2_bwd: an operand of 2 GiB or more");
  SFX_REQUIRE(x && dy && dx, "sfx_maxpool2x2_bwd: null buffer");
  SFX_REQUIRE(dx != x && dx != dy, "sfx_maxpool2x2_bwd: dx aliases an input");
  const long long total = (long long)num_images * (height / 2) * (width / 2) * channels;
  maxpool_bwd_kernel<<<sfx::ceil_div(total, 256), 256, 0, sfx::as_stream(stream)>>>(height, width, channels, x, dy,
                                                                                    relu_mask, dx, total);
  return sfx::check_launch("sfx_maxpool2x2_bwd");
}

int sfx_lpips_input(int num_images, int height, int width, const float* x, const float* mask, int quantize_u8,
                    float* u, void* stream) {
  sfx::clear_error();
  SFX_REQUIRE(num_images >= 1, "sfx_lpips_input: bad image count %d", num_images);
  SFX_REQUIRE(height >= 16 && width >= 16, "sfx_lpips_input: images of %d x %d; LPIPS (vgg) needs at least 16 x 16",
              height, width);
  SFX_REQUIRE(fits((long long)num_images * height * width * 3), "sfx_lpips_input: an operand of 2 GiB or more");
  SFX_REQUIRE(x && u, "sfx_lpips_input: null buffer");
  const long long total = (long long)num_images * height * width * 3;
  lpips_input_kernel<<<sfx::ceil_div(total, 256), 256, 0, sfx::as_stream(stream)>>>(total, x, mask, quantize_u8, u);
  return sfx::check_launch("sfx_lpips_input");
}

int sfx_lpips_input_bwd(int num_images, int height, int width, const float* du, float* dx, void* stream) {
  sfx::clear_error();
  SFX_REQUIRE(num_images >= 1 && height >= 1 && width >= 1, "sfx_lpips_input_bwd: bad sizes (%d images of %d x %d)",
              num_images, height, width);
  SFX_REQUIRE(fits((long long)num_images * height * width * 3), "sfx_lpips_input_bwd: an operand of 2 GiB or more");
  SFX_REQUIRE(du && dx, "sfx_lpips_input_bwd: null buffer");
  const long long total = (long long)num_images * height * width * 3;
  lpips_input_bwd_kernel<<<sfx::ceil_div(total, 256), 256, 0, sfx::as_stream(stream)>>>(total, du, dx);
  return sfx::check_launch("sfx_lpips_input_bwd");
}

int sfx_tap_normalize(long long pixels, int channels, const float* f, float* fhat, void* stream) {
  sfx::clear_error();
  SFX_REQUIRE(pixels >= 1 && channels >= 1, "sfx_tap_normalize: bad sizes (%lld pixels of %d channels)", pixels,
              channels);
  SFX_REQUIRE(fits(pixels * channels), "sfx_tap_normalize: an operand of 2 GiB or more");
  SFX_REQUIRE(f && fhat, "sfx_tap_normalize: null buffer");
  tap_normalize_kernel<<<sfx::ceil_div(pixels, 4), 256, 0, sfx::as_stream(stream)>>>(pixels, channels, f, fhat);
  return sfx::check_launch("sfx_tap_normalize");
}

size_t sfx_tap_dist_workspace_bytes(int num_images, long long pixels_per_image) {
  if (num_images < 1 || pixels_per_image < 1) return 0;
  return (size_t)num_images * (size_t)pixels_per_image * 4;
}

int sfx_tap_dist(int num_images, long long pixels_per_image, int channels, const float* fx, const float* fhat_y,
                 const float* w, int accumulate, float* out, void* ws, size_t ws_bytes, void* stream) {
  sfx::clear_error();
  SFX_REQUIRE(num_images >= 1 && pixels_per_image >= 1 && channels >= 1,
              "sfx_tap_dist: bad sizes (%d images of %lld pixels, %d channels)", num_images, pixels_per_image, channels);
  const long long P = (long long)num_images * pixels_per_image;
  SFX_REQUIRE(fits(P * channels), "sfx_tap_dist: an operand of 2 GiB or more");
  SFX_REQUIRE(fx && fhat_y && w && out && ws, "sfx_tap_dist: null buffer");
  SFX_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "sfx_tap_dist: workspace must be 4-byte aligned");
  SFX_REQUIRE(ws_bytes >= (size_t)P * 4, "sfx_tap_dist: workspace too small");
  hipStream_t st = sfx::as_stream(stream);
  float* dpix = reinterpret_cast<float*>(ws);
  tap_dist_kernel<<<sfx::ceil_div(P, 4), 256, 0, st>>>(P, channels, fx, fhat_y, w, dpix);
  tap_reduce_kernel<<<num_images, 256, 0, st>>>(pixels_per_image, dpix, accumulate, out);
  return sfx::check_launch("sfx_tap_dist");
}

int sfx_tap_dist_bwd(int num_images, long long pixels_per_image, int channels, const float* fx, const float* fhat_y,
                     const float* w, const float* image_scale, int relu_mask, float* dfx, void* stream) {
  sfx::clear_error();
  SFX_REQUIRE(num_images >= 1 && pixels_per_image >= 1 && channels >= 1,
              "sfx_tap_dist_bwd: bad sizes (%d images of %lld pixels, %d channels)", num_images, pixels_per_image,
              channels);
  const long long P = (long long)num_images * pixels_per_image;
  SFX_REQUIRE(fits(P * channels), "sfx_tap_dist_bwd: an operand of 2 GiB or more");
  SFX_REQUIRE(fx && fhat_y && w && image_scale && dfx, "sfx_tap_dist_bwd: null buffer");
  SFX_REQUIRE(dfx != fx && dfx != fhat_y, "sfx_tap_dist_bwd: dfx aliases an input");
  tap_dist_bwd_kernel<<<sfx::ceil_div(P, 4), 256, 0, sfx::as_stream(stream)>>>(P, pixels_per_image, channels, fx, fhat_y,
                                                                               w, image_scale, relu_mask, dfx);
  return sfx::check_launch("sfx_tap_dist_bwd");
}

}  // extern "C"

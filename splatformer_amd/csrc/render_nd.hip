// N-channel tile compositor (ABI v16, additive): gsplat's rasterize_gaussians for any channel count -- depth
// maps, alpha-weighted normals, per-Gaussian feature vectors.  The per-pixel arithmetic and control flow are
// rasterize_fwd_kernel's / rasterize_bwd_kernel's (render.hip) with the three colour accumulators replaced by
// CH of them, CH a compile-time tier in {1, 2, 4, 8, 16, 32}; the run-time channel count C <= CH selects the
// smallest tier that holds it, reads only C real channels from global memory and zero-fills the rest.
//
// Layout: one workgroup per tile over (gids_sorted, tile_bins), as the 3-channel kernels -- gsplat's full
// list or a culled one.  The workgroup is bw*bw threads rounded up to whole waves (the extra threads own no
// pixel), so every wave-wide operation below runs with all 64 lanes.  Per batch of blockDim Gaussians the
// geometry (x, y, opacity | conic) is staged in LDS as two float4 and the colour row at a stride of CH + 4
// floats: the inner loop reads one row for all lanes (a broadcast, ds_read_b128), and the staging writes of 8
// consecutive lanes (16 bytes each, rows 4 (CH + 4) bytes apart) fall on 8 different groups of 4 banks instead
// of one, which is where a 32-float stride puts them.  CH = 32: 36 KiB of colours + 9 KiB of geometry.
#include "common.h"

namespace {

constexpr int MAX_BLOCK = 256;

template <int CH>
struct NdLayout {
  static constexpr int STRIDE = CH < 4 ? CH : CH + 4;  // floats per staged colour row
};

// colour row of Gaussian g -> LDS row, channels >= C zero.  vec4: C % 4 == 0 and 16-byte aligned rows.
template <int CH>
__device__ __forceinline__ void stage_colors(const float* __restrict__ colors, int g, int C, int vec4,
                                             float* __restrict__ dst) {
  const float* src = colors + (size_t)g * C;
  if constexpr (CH >= 4) {
    if (vec4) {
#pragma unroll
      for (int k = 0; k < CH / 4; ++k)
        reinterpret_cast<float4*>(dst)[k] =
            (4 * k < C) ? reinterpret_cast<const float4*>(src)[k] : make_float4(0.f, 0.f, 0.f, 0.f);
      return;
    }
  }
#pragma unroll
  for (int c = 0; c < CH; ++c) dst[c] = (c < C) ? src[c] : 0.f;
}

template <int CH>
__device__ __forceinline__ void load_row(const float* __restrict__ row, float (&c)[CH]) {
  if constexpr (CH >= 4) {
#pragma unroll
    for (int k = 0; k < CH / 4; ++k) {
      const float4 v = reinterpret_cast<const float4*>(row)[k];
      c[4 * k] = v.x; c[4 * k + 1] = v.y; c[4 * k + 2] = v.z; c[4 * k + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < CH; ++k) c[k] = row[k];
  }
}

// ---- forward ------------------------------------------------------------------------------------------------
template <int CH>
__global__ void __launch_bounds__(MAX_BLOCK)
rasterize_fwd_nd_kernel(int tiles_x, int bw, int img_h, int img_w, int C, int vec4,
                        const int32_t* __restrict__ gids_sorted, const int* __restrict__ tile_bins,
                        const float* __restrict__ xys, const float* __restrict__ conics,
                        const float* __restrict__ colors, const float* __restrict__ opacity,
                        const float* __restrict__ background, float* __restrict__ final_Ts,
                        int* __restrict__ final_idx, float* __restrict__ out_img, float* __restrict__ out_alpha) {
  constexpr int STRIDE = NdLayout<CH>::STRIDE;
  __shared__ float4 xyo_batch[MAX_BLOCK];    // x, y, opacity, pad
  __shared__ float4 conic_batch[MAX_BLOCK];  // a, b, c, pad
  __shared__ __attribute__((aligned(16))) float col_batch[MAX_BLOCK * STRIDE];

  const int tile_id = blockIdx.y * tiles_x + blockIdx.x;
  const int tr = threadIdx.x, nthreads = blockDim.x;
  const int ty = tr / bw, tx = tr - ty * bw;
  const unsigned pi = blockIdx.y * bw + ty, pj = blockIdx.x * bw + tx;
  const float px = (float)pj + 0.5f, py = (float)pi + 0.5f;
  const bool inside = (tr < bw * bw && pi < (unsigned)img_h && pj < (unsigned)img_w);
  bool done = !inside;

  const int range_x = tile_bins[2 * tile_id], range_y = tile_bins[2 * tile_id + 1];
  const int num_batches = (range_y - range_x + nthreads - 1) / nthreads;

  float T = 1.f;
  int cur_idx = 0;
  float acc[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) acc[c] = 0.f;
  for (int b = 0; b < num_batches; ++b) {
    // resync before overwriting the batch; early exit when the whole tile is done
    if (__syncthreads_count(done) >= nthreads) break;

    const int batch_start = range_x + nthreads * b;
    const int idx = batch_start + tr;
    if (idx < range_y) {
      const int g = gids_sorted[idx];
      xyo_batch[tr] = make_float4(xys[2 * g], xys[2 * g + 1], opacity[g], 0.f);
      conic_batch[tr] = make_float4(conics[3 * g], conics[3 * g + 1], conics[3 * g + 2], 0.f);
      stage_colors<CH>(colors, g, C, vec4, col_batch + tr * STRIDE);
    }
    __syncthreads();
    const int batch_size = min(nthreads, range_y - batch_start);
    for (int t = 0; (t < batch_size) && !done; ++t) {
      const float4 con = conic_batch[t];
      const float4 xyo = xyo_batch[t];
      const float dx = xyo.x - px, dy = xyo.y - py;
      const float sigma = 0.5f * (con.x * dx * dx + con.z * dy * dy) + con.y * dx * dy;
      const float alpha = fminf(0.999f, xyo.z * __expf(-sigma));
      if (sigma < 0.f || alpha < 1.f / 255.f) continue;
      const float next_T = T * (1.f - alpha);
      if (next_T <= 1e-4f) {
        done = true;
        break;
      }
      const float vis = alpha * T;
      float col[CH];
      load_row<CH>(col_batch + t * STRIDE, col);
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[c] = acc[c] + col[c] * vis;
      T = next_T;
      cur_idx = batch_start + t;
    }
  }
  if (inside) {
    const int pix = pi * img_w + pj;
    final_Ts[pix] = T;
    final_idx[pix] = cur_idx;
    float* o = out_img + (size_t)pix * C;
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (c < C) o[c] = acc[c] + T * background[c];
    if (out_alpha) out_alpha[pix] = 1.f - T;
  }
}

// ---- backward -----------------------------------------------------------------------------------------------
// LDS writes of a wave made visible to its other lanes (the LDS serves one wave's accesses in order; the fences
// and the barrier only keep the compiler from moving accesses across this point).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Per Gaussian and wave the colour gradient is g[c] = sum over the 64 lanes of fac(lane) * v_out(lane pixel)[c].
// TRANSPOSE: each lane writes its fac to LDS; lane l owns channel l % CH over the CH pixels of part l / CH of
// the wave (their v_out values sit in its registers for the whole kernel: voT), does CH multiply-adds, and
// log2(64 / CH) shuffles add the parts -- CH + log2(64 / CH) steps instead of CH wave reductions (measured,
// 1.10 vs 2.84 ms at C = 32, 0.73 vs 0.79 ms at C = 4).  Tiers below kTransposeMinCH: one
// wave_sum_dpp per channel.  Both end in one atomic per channel, issued by lane c.
constexpr int kTransposeMinCH = 4;

template <int CH>
__global__ void __launch_bounds__(MAX_BLOCK)
rasterize_bwd_nd_kernel(int tiles_x, int bw, int img_h, int img_w, int C, int vec4,
                        const int32_t* __restrict__ gids_sorted, const int* __restrict__ tile_bins,
                        const float* __restrict__ xys, const float* __restrict__ conics,
                        const float* __restrict__ colors, const float* __restrict__ opacity,
                        const float* __restrict__ background, const float* __restrict__ final_Ts,
                        const int* __restrict__ final_idx, const float* __restrict__ v_out,
                        const float* __restrict__ v_out_alpha, float* __restrict__ v_xy,
                        float* __restrict__ v_xy_abs, float* __restrict__ v_conic, float* __restrict__ v_colors,
                        float* __restrict__ v_opacity) {
  constexpr int STRIDE = NdLayout<CH>::STRIDE;
  constexpr bool TRANSPOSE = CH >= kTransposeMinCH;
  __shared__ int id_batch[MAX_BLOCK];
  __shared__ float4 xyo_batch[MAX_BLOCK];
  __shared__ float4 conic_batch[MAX_BLOCK];
  __shared__ __attribute__((aligned(16))) float col_batch[MAX_BLOCK * STRIDE];
  __shared__ __attribute__((aligned(16))) float fac_lds[TRANSPOSE ? MAX_BLOCK : 1];

  const int tile_id = blockIdx.y * tiles_x + blockIdx.x;
  const int tr = threadIdx.x, nthreads = blockDim.x, block_size = bw * bw;
  const int ty = tr / bw, tx = tr - ty * bw;
  const unsigned pi = blockIdx.y * bw + ty, pj = blockIdx.x * bw + tx;
  const float px = (float)pj + 0.5f, py = (float)pi + 0.5f;
  const bool inside = (tr < block_size && pi < (unsigned)img_h && pj < (unsigned)img_w);
  const int pix = inside ? (int)(pi * img_w + pj) : 0;

  const float T_final = final_Ts[pix];
  float T = T_final;
  const int bin_final = inside ? final_idx[pix] : 0;
  const int range_x = tile_bins[2 * tile_id], range_y = tile_bins[2 * tile_id + 1];
  const int num_batches = (range_y - range_x + nthreads - 1) / nthreads;
  float buf[CH], vo[CH];
  float bgvo = 0.f;  // sum over channels of background[c] * v_out[c]: the pixel's constant in the v_alpha terms
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    buf[c] = 0.f;
    vo[c] = (c < C && inside) ? v_out[(size_t)pix * C + c] : 0.f;
    if (c < C) bgvo += background[c] * vo[c];
  }
  const float voa = (v_out_alpha && inside) ? v_out_alpha[pix] : 0.f;
  const int wave_bin_final = sfx::wave_max_i(bin_final);
  const int lane = tr & 63, wave = tr >> 6;

  // v_out of this lane's channel (lane % CH) at the CH pixels of its part (lane / CH) of the wave
  [[maybe_unused]] float voT[TRANSPOSE ? CH : 1];
  [[maybe_unused]] const int part0 = wave * 64 + (lane / CH) * CH;
  if constexpr (TRANSPOSE) {
    const int rc = lane % CH;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int t2 = part0 + j;
      const int ty2 = t2 / bw, tx2 = t2 - ty2 * bw;
      const unsigned pi2 = blockIdx.y * bw + ty2, pj2 = blockIdx.x * bw + tx2;
      const bool in2 = (t2 < block_size && pi2 < (unsigned)img_h && pj2 < (unsigned)img_w && rc < C);
      voT[j] = in2 ? v_out[(size_t)(pi2 * img_w + pj2) * C + rc] : 0.f;
    }
  }

  for (int b = 0; b < num_batches; ++b) {
    __syncthreads();
    const int batch_end = range_y - 1 - nthreads * b;
    const int batch_size = min(nthreads, batch_end + 1 - range_x);
    const int idx = batch_end - tr;
    if (idx >= range_x) {
      const int g = gids_sorted[idx];
      id_batch[tr] = g;
      xyo_batch[tr] = make_float4(xys[2 * g], xys[2 * g + 1], opacity[g], 0.f);
      conic_batch[tr] = make_float4(conics[3 * g], conics[3 * g + 1], conics[3 * g + 2], 0.f);
      stage_colors<CH>(colors, g, C, vec4, col_batch + tr * STRIDE);
    }
    __syncthreads();
    for (int t = max(0, batch_end - wave_bin_final); t < batch_size; ++t) {
      bool valid = inside && (batch_end - t <= bin_final);
      float alpha = 0.f, opac = 0.f, vis = 0.f, dx = 0.f, dy = 0.f;
      float4 con = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid) {
        con = conic_batch[t];
        const float4 xyo = xyo_batch[t];
        opac = xyo.z;
        dx = xyo.x - px;
        dy = xyo.y - py;
        const float sigma = 0.5f * (con.x * dx * dx + con.z * dy * dy) + con.y * dx * dy;
        vis = __expf(-sigma);
        alpha = fminf(0.99f, opac * vis);
        if (sigma < 0.f || alpha < 1.f / 255.f) valid = false;
      }
      if (!__any(valid)) continue;
      float fac = 0.f, g_c0 = 0.f, g_c1 = 0.f, g_c2 = 0.f;
      float g_xy0 = 0.f, g_xy1 = 0.f, g_ax = 0.f, g_ay = 0.f, g_o = 0.f;
      if (valid) {
        const float ra = 1.f / (1.f - alpha);
        T *= ra;
        fac = alpha * T;
        float col[CH];
        load_row<CH>(col_batch + t * STRIDE, col);
        float v_alpha = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          v_alpha += (col[c] * T - buf[c] * ra) * vo[c];
          buf[c] += col[c] * fac;
        }
        v_alpha += T_final * ra * voa;
        v_alpha += -T_final * ra * bgvo;
        const float v_sigma = -opac * vis * v_alpha;
        g_c0 = 0.5f * v_sigma * dx * dx;
        g_c1 = v_sigma * dx * dy;
        g_c2 = 0.5f * v_sigma * dy * dy;
        g_xy0 = v_sigma * (con.x * dx + con.y * dy);
        g_xy1 = v_sigma * (con.y * dx + con.z * dy);
        g_ax = fabsf(g_xy0);
        g_ay = fabsf(g_xy1);
        g_o = vis * v_alpha;
      }
      float g_col = 0.f;  // lane c < C: the wave's sum for channel c
      if constexpr (TRANSPOSE) {
        fac_lds[tr] = fac;
        wave_lds_sync();
        float f[CH];
        load_row<CH>(fac_lds + part0, f);
        wave_lds_sync();  // the next Gaussian's fac is written only after every lane has read this one's
#pragma unroll
        for (int j = 0; j < CH; ++j) g_col = __builtin_fmaf(f[j], voT[j], g_col);
#pragma unroll
        for (int o = CH; o < 64; o <<= 1) g_col += __shfl_xor(g_col, o, 64);
      } else {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const float s = sfx::wave_sum_dpp(fac * vo[c]);
          if (lane == c) g_col = s;
        }
      }
      g_c0 = sfx::wave_sum_dpp(g_c0);
      g_c1 = sfx::wave_sum_dpp(g_c1);
      g_c2 = sfx::wave_sum_dpp(g_c2);
      g_xy0 = sfx::wave_sum_dpp(g_xy0);
      g_xy1 = sfx::wave_sum_dpp(g_xy1);
      g_o = sfx::wave_sum_dpp(g_o);
      if (v_xy_abs) {
        g_ax = sfx::wave_sum_dpp(g_ax);
        g_ay = sfx::wave_sum_dpp(g_ay);
      }
      const int g = id_batch[t];
      if (lane < C) atomicAdd(v_colors + (size_t)g * C + lane, g_col);
      if (lane == 0) {
        atomicAdd(v_conic + 3 * g + 0, g_c0);
        atomicAdd(v_conic + 3 * g + 1, g_c1);
        atomicAdd(v_conic + 3 * g + 2, g_c2);
        atomicAdd(v_xy + 2 * g + 0, g_xy0);
        atomicAdd(v_xy + 2 * g + 1, g_xy1);
        if (v_xy_abs) {
          atomicAdd(v_xy_abs + 2 * g + 0, g_ax);
          atomicAdd(v_xy_abs + 2 * g + 1, g_ay);
        }
        atomicAdd(v_opacity + g, g_o);
      }
    }
  }
}

// smallest tier that holds `channels` (1 <= channels <= 32)
int nd_tier(int channels) {
  int t = 1;
  while (t < channels) t <<= 1;
  return t;
}

int nd_threads(int block_width) { return (block_width * block_width + 63) / 64 * 64; }

int nd_vec4(int channels, const void* a) { return channels % 4 == 0 && (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

}  // namespace

#define SFX_ND_DISPATCH(tier, KERNEL, ...)                    \
  switch (tier) {                                             \
    case 1: KERNEL<1> __VA_ARGS__; break;                     \
    case 2: KERNEL<2> __VA_ARGS__; break;                     \
    case 4: KERNEL<4> __VA_ARGS__; break;                     \
    case 8: KERNEL<8> __VA_ARGS__; break;                     \
    case 16: KERNEL<16> __VA_ARGS__; break;                   \
    default: KERNEL<32> __VA_ARGS__; break;                   \
  }

extern "C" {

int sfx_rasterize_fwd_nd(int tiles_x, int tiles_y, int block_width, int img_h, int img_w, int channels,
                         const int32_t* gids_sorted, const int* tile_bins, const float* xys, const float* conics,
                         const float* colors, const float* opacity, const float* background, float* final_Ts,
                         int* final_idx, float* out_img, float* out_alpha, void* stream) {
  SFX_REQUIRE(img_h >= 0 && img_w >= 0 && tiles_x >= 0 && tiles_y >= 0, "sfx_rasterize_fwd_nd: negative size");
  SFX_REQUIRE(block_width > 1 && block_width <= 16, "sfx_rasterize_fwd_nd: block_width must be in (1,16]");
  SFX_REQUIRE(channels >= 1 && channels <= 32, "sfx_rasterize_fwd_nd: channels must be in [1,32] (got %d)", channels);
  SFX_REQUIRE(tiles_x == (img_w + block_width - 1) / block_width && tiles_y == (img_h + block_width - 1) / block_width,
              "sfx_rasterize_fwd_nd: tile bounds do not match the image size");
  SFX_REQUIRE(tiles_y <= 65535, "sfx_rasterize_fwd_nd: image too tall for one launch");
  if (tiles_x == 0 || tiles_y == 0) return SFX_OK;
  SFX_REQUIRE(tile_bins && xys && conics && colors && opacity && background && final_Ts && final_idx && out_img,
              "sfx_rasterize_fwd_nd: null buffer");
  const dim3 grid(tiles_x, tiles_y);
  const int threads = nd_threads(block_width), vec4 = nd_vec4(channels, colors);
  hipStream_t st = sfx::as_stream(stream);
  SFX_ND_DISPATCH(nd_tier(channels), rasterize_fwd_nd_kernel,
                  <<<grid, threads, 0, st>>>(tiles_x, block_width, img_h, img_w, channels, vec4, gids_sorted,
                                             tile_bins, xys, conics, colors, opacity, background, final_Ts,
                                             final_idx, out_img, out_alpha));
  return sfx::check_launch("sfx_rasterize_fwd_nd");
}

int sfx_rasterize_bwd_nd(int tiles_x, int tiles_y, int block_width, int img_h, int img_w, int channels,
                         const int32_t* gids_sorted, const int* tile_bins, const float* xys, const float* conics,
                         const float* colors, const float* opacity, const float* background, const float* final_Ts,
                         const int* final_idx, const float* v_out, const float* v_out_alpha, float* v_xy,
                         float* v_xy_abs, float* v_conic, float* v_colors, float* v_opacity, void* stream) {
  SFX_REQUIRE(img_h >= 0 && img_w >= 0 && tiles_x >= 0 && tiles_y >= 0, "sfx_rasterize_bwd_nd: negative size");
  SFX_REQUIRE(block_width > 1 && block_width <= 16, "sfx_rasterize_bwd_nd: block_width must be in (1,16]");
  SFX_REQUIRE(channels >= 1 && channels <= 32, "sfx_rasterize_bwd_nd: channels must be in [1,32] (got %d)", channels);
  SFX_REQUIRE(tiles_x == (img_w + block_width - 1) / block_width && tiles_y == (img_h + block_width - 1) / block_width,
              "sfx_rasterize_bwd_nd: tile bounds do not match the image size");
  SFX_REQUIRE(tiles_y <= 65535, "sfx_rasterize_bwd_nd: image too tall for one launch");
  if (tiles_x == 0 || tiles_y == 0) return SFX_OK;
  SFX_REQUIRE(tile_bins && xys && conics && colors && opacity && background && final_Ts && final_idx && v_out &&
                  v_xy && v_conic && v_colors && v_opacity,
              "sfx_rasterize_bwd_nd: null buffer");
  const dim3 grid(tiles_x, tiles_y);
  const int threads = nd_threads(block_width), vec4 = nd_vec4(channels, colors);
  hipStream_t st = sfx::as_stream(stream);
  SFX_ND_DISPATCH(nd_tier(channels), rasterize_bwd_nd_kernel,
                  <<<grid, threads, 0, st>>>(tiles_x, block_width, img_h, img_w, channels, vec4, gids_sorted,
                                             tile_bins, xys, conics, colors, opacity, background, final_Ts,
                                             final_idx, v_out, v_out_alpha, v_xy, v_xy_abs, v_conic, v_colors,
                                             v_opacity));
  return sfx::check_launch("sfx_rasterize_bwd_nd");
}

}  // extern "C"

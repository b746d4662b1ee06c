// Tile-local front-to-back alpha compositing, forward and backward: gsplat v0.1.11's rasterize_forward /
// rasterize_backward (the version the reference pins: SURVEY.md Appendix A.2; oracle/gsplat_ref.py restates it)
// over (gids_sorted, tile_bins).  One workgroup per tile; per-batch Gaussian records staged in LDS.  The forward
// kernels are built from the steps of raster_common.h and differ in staging and thread mapping only; the backward
// kernels share its prologue, staging and quadrant lists and keep their per-pixel step written out (as helpers it
// cost two of them 5 and 10 %: DESIGN.md section 28):
//   rasterize_fwd_kernel / rasterize_bwd_kernel   four arrays, bw*bw threads, 3 channels
//   rasterize_fwd_packed_kernel                   64-byte records (eval path)
//   rasterize_fwd_quad_kernel / _bwd_quad_kernel  one 8x8 quadrant per wave with per-wave compacted lists
//   rasterize_fwd_nd_kernel / _bwd_nd_kernel<CH>  CH channels (depth maps, normals, feature vectors)
#include "raster_common.h"

namespace {

using namespace sfxr;

// ---- forward, 3 channels ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MAX_BLOCK)
rasterize_fwd_kernel(int tiles_x, int tiles_y, int bw, int img_h, int img_w,
                     const int32_t* __restrict__ gids_sorted, const int* __restrict__ tile_bins,
                     const float* __restrict__ xys, const float* __restrict__ conics,
                     const float* __restrict__ colors, const float* __restrict__ opacity,
                     const float* __restrict__ background, float* __restrict__ final_Ts,
                     int* __restrict__ final_idx, float* __restrict__ out_img, float* __restrict__ out_alpha,
                     int clamp_max1) {
  __shared__ int id_batch[MAX_BLOCK];
  __shared__ float4 xyo_batch[MAX_BLOCK];   // x, y, opacity, pad
  __shared__ float4 conic_batch[MAX_BLOCK]; // a, b, c, pad
  __shared__ float4 rgb_batch[MAX_BLOCK];

  const int tr = threadIdx.x, block_size = bw * bw;
  const TilePix p = tile_pix_rows(tiles_x * tiles_y, tiles_x, bw, block_size, false, img_h, img_w, tile_bins);
  view_advance(img_h, img_w, final_Ts, final_idx, out_img, out_alpha);
  bool done = !p.inside;
  float T = 1.f;
  int cur_idx = 0;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int b = 0; b < p.num_batches; ++b) {
    // resync before overwriting the batch; early exit when the whole tile is done
    if (__syncthreads_count(done) >= block_size) break;
    const int batch_start = p.range_x + block_size * b;
    const int idx = batch_start + tr;
    if (idx < p.range_y)
      stage_arrays(tr, gids_sorted[idx], xys, conics, colors, opacity, id_batch, xyo_batch, conic_batch, rgb_batch);
    __syncthreads();
    const int batch_size = min(block_size, p.range_y - batch_start);
    for (int t = 0; (t < batch_size) && !done; ++t) {
      const float4 con = conic_batch[t];
      const float4 xyo = xyo_batch[t];
      float vis;
      if (!fwd_step(xyo.x, xyo.y, xyo.z, con.x, con.y, con.z, p.px, p.py, T, done, vis)) continue;
      const float4 c = rgb_batch[t];
      fwd_accumulate<3>(acc, {c.x, c.y, c.z}, vis);
      cur_idx = batch_start + t;
    }
  }
  fwd_store<3>(p, img_w, 3, T, cur_idx, acc, background, clamp_max1, final_Ts, final_idx, out_img, out_alpha);
}

__global__ void pack_raster_records_kernel(int n, const float* __restrict__ xys, const float* __restrict__ conics,
                                           const float* __restrict__ colors, const float* __restrict__ opacity,
                                           float4* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  write_record(rec, i, xys + 2 * i, opacity[i], conics + 3 * i, colors + 3 * i);
}

// rasterize_fwd_kernel over packed records: the batch is staged in LDS as the records themselves
__global__ void __launch_bounds__(MAX_BLOCK)
rasterize_fwd_packed_kernel(int tiles_x, int tiles_y, int bw, int img_h, int img_w,
                            const int32_t* __restrict__ gids_sorted, const int* __restrict__ tile_bins,
                            const float4* __restrict__ rec, const float* __restrict__ background,
                            float* __restrict__ final_Ts, int* __restrict__ final_idx, float* __restrict__ out_img,
                            float* __restrict__ out_alpha, int clamp_max1) {
  __shared__ float4 r0_batch[MAX_BLOCK];
  __shared__ float4 r1_batch[MAX_BLOCK];
  __shared__ float r2_batch[MAX_BLOCK];

  const int tr = threadIdx.x, block_size = bw * bw;
  const TilePix p = tile_pix_rows(tiles_x * tiles_y, tiles_x, bw, block_size, false, img_h, img_w, tile_bins);
  view_advance(img_h, img_w, final_Ts, final_idx, out_img, out_alpha);
  bool done = !p.inside;
  float T = 1.f;
  int cur_idx = 0;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int b = 0; b < p.num_batches; ++b) {
    if (__syncthreads_count(done) >= block_size) break;
    const int batch_start = p.range_x + block_size * b;
    const int idx = batch_start + tr;
    if (idx < p.range_y) stage_record(tr, gids_sorted[idx], rec, r0_batch, r1_batch, r2_batch);
    __syncthreads();
    const int batch_size = min(block_size, p.range_y - batch_start);
    for (int t = 0; (t < batch_size) && !done; ++t) {
      const Rec r{r0_batch[t], r1_batch[t]};
      float vis;
      if (!fwd_step(r.x(), r.y(), r.opac(), r.ca(), r.cb(), r.cc(), p.px, p.py, T, done, vis)) continue;
      fwd_accumulate<3>(acc, {r.red(), r.green(), r2_batch[t]}, vis);
      cur_idx = batch_start + t;
    }
  }
  fwd_store<3>(p, img_w, 3, T, cur_idx, acc, background, clamp_max1, final_Ts, final_idx, out_img, out_alpha);
}

// rasterize_fwd_packed_kernel with per-wave Gaussian lists: the 16x16 tile is split into four 8x8 quadrants, one
// per wave; while a batch is staged each lane tests its record against the four quadrants (cull_box_may_hit)
// and every wave compacts the batch to the records that can reach its quadrant.  Each pixel still visits its
// tile's Gaussians in list order and runs the same fwd_step; it only skips records whose alpha is below
// 1/255 at all of its quadrant's pixel centres -- the ones the per-pixel test would `continue` past -- so every
// output is bit-identical to rasterize_fwd_packed_kernel over the same list.  bw must be 16.
__global__ void __launch_bounds__(MAX_BLOCK)
rasterize_fwd_quad_kernel(int tiles_x, int tiles_y, int img_h, int img_w, const int32_t* __restrict__ gids_sorted,
                          const int* __restrict__ tile_bins, const float4* __restrict__ rec,
                          const float* __restrict__ background, float* __restrict__ final_Ts,
                          int* __restrict__ final_idx, float* __restrict__ out_img, float* __restrict__ out_alpha,
                          int clamp_max1) {
  constexpr int BW = 16, BS = BW * BW;
  __shared__ float4 r0_batch[BS];
  __shared__ float4 r1_batch[BS];
  __shared__ float r2_batch[BS];
  __shared__ unsigned char mask_batch[BS];
  __shared__ unsigned char wlist[4][BS];

  const int tr = threadIdx.x, lane = tr & 63, w = tr >> 6;
  const TilePix p = tile_pix_quads(tiles_x * tiles_y, tiles_x, img_h, img_w, tile_bins);
  view_advance(img_h, img_w, final_Ts, final_idx, out_img, out_alpha);
  const int tx0 = blockIdx.x * BW, ty0 = blockIdx.y * BW;
  bool done = !p.inside;
  float T = 1.f;
  int cur_idx = 0;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int b = 0; b < p.num_batches; ++b) {
    if (__syncthreads_count(done) >= BS) break;
    const int batch_start = p.range_x + BS * b;
    const int idx = batch_start + tr;
    unsigned m = 0;
    if (idx < p.range_y) {
      const Rec r = stage_record(tr, gids_sorted[idx], rec, r0_batch, r1_batch, r2_batch);
      m = quad_mask(cull_setup(r.x(), r.y(), r.ca(), r.cb(), r.cc(), r.opac()), tx0, ty0, img_w, img_h);
    }
    mask_batch[tr] = (unsigned char)m;
    __syncthreads();
    // this wave's list: batch positions whose record may reach the quadrant, in batch order
    const int cnt = wave_compact(mask_batch, wlist[w], w, lane, [](int) { return true; });
    __syncthreads();
    for (int j = 0; (j < cnt) && !done; ++j) {
      const int t = wlist[w][j];
      const Rec r{r0_batch[t], r1_batch[t]};
      float vis;
      if (!fwd_step(r.x(), r.y(), r.opac(), r.ca(), r.cb(), r.cc(), p.px, p.py, T, done, vis)) continue;
      fwd_accumulate<3>(acc, {r.red(), r.green(), r2_batch[t]}, vis);
      cur_idx = batch_start + t;
    }
  }
  fwd_store<3>(p, img_w, 3, T, cur_idx, acc, background, clamp_max1, final_Ts, final_idx, out_img, out_alpha);
}

// ---- backward, 3 channels -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(MAX_BLOCK)
rasterize_bwd_kernel(int tiles_x, int tiles_y, int bw, int img_h, int img_w,
                     const int32_t* __restrict__ gids_sorted, const int* __restrict__ tile_bins,
                     const float* __restrict__ xys, const float* __restrict__ conics,
                     const float* __restrict__ colors, const float* __restrict__ opacity,
                     const float* __restrict__ background, const float* __restrict__ final_Ts,
                     const int* __restrict__ final_idx, const float* __restrict__ v_out,
                     const float* __restrict__ v_out_alpha, float* __restrict__ v_xy,
                     float* __restrict__ v_xy_abs, float* __restrict__ v_conic, float* __restrict__ v_rgb,
                     float* __restrict__ v_opacity) {
  __shared__ int id_batch[MAX_BLOCK];
  __shared__ float4 xyo_batch[MAX_BLOCK];
  __shared__ float4 conic_batch[MAX_BLOCK];
  __shared__ float4 rgb_batch[MAX_BLOCK];

  const int tr = threadIdx.x, lane = tr & 63, block_size = bw * bw;
  const TilePix p = tile_pix_rows(0, tiles_x, bw, block_size, false, img_h, img_w, tile_bins);
  const int pix = min((int)(p.pi * img_w + p.pj), img_w * img_h - 1);

  const float T_final = final_Ts[pix];
  float T = T_final;
  float buf0 = 0.f, buf1 = 0.f, buf2 = 0.f;
  const int bin_final = p.inside ? final_idx[pix] : 0;
  const float vo0 = v_out[3 * pix], vo1 = v_out[3 * pix + 1], vo2 = v_out[3 * pix + 2];
  const float voa = v_out_alpha ? v_out_alpha[pix] : 0.f;
  const float bg0 = background[0], bg1 = background[1], bg2 = background[2];
  const int wave_bin_final = sfx::wave_max_i(bin_final);

  for (int b = 0; b < p.num_batches; ++b) {
    __syncthreads();
    const int batch_end = p.range_y - 1 - block_size * b;
    const int batch_size = min(block_size, batch_end + 1 - p.range_x);
    const int idx = batch_end - tr;
    if (idx >= p.range_x)
      stage_arrays(tr, gids_sorted[idx], xys, conics, colors, opacity, id_batch, xyo_batch, conic_batch, rgb_batch);
    __syncthreads();
    for (int t = max(0, batch_end - wave_bin_final); t < batch_size; ++t) {
      bool valid = p.inside && (batch_end - t <= bin_final);
      float alpha = 0.f, opac = 0.f, vis = 0.f, dx = 0.f, dy = 0.f;
      float4 con = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid) {
        con = conic_batch[t];
        const float4 xyo = xyo_batch[t];
        opac = xyo.z;
        dx = xyo.x - p.px;
        dy = xyo.y - p.py;
        const float sigma = 0.5f * (con.x * dx * dx + con.z * dy * dy) + con.y * dx * dy;
        vis = __expf(-sigma);
        alpha = fminf(0.99f, opac * vis);
        if (sigma < 0.f || alpha < 1.f / 255.f) valid = false;
      }
      if (!__any(valid)) continue;
      float g_rgb0 = 0.f, g_rgb1 = 0.f, g_rgb2 = 0.f, g_c0 = 0.f, g_c1 = 0.f, g_c2 = 0.f;
      float g_xy0 = 0.f, g_xy1 = 0.f, g_ax = 0.f, g_ay = 0.f, g_o = 0.f;
      if (valid) {
        const float ra = 1.f / (1.f - alpha);
        T *= ra;
        const float fac = alpha * T;
        g_rgb0 = fac * vo0;
        g_rgb1 = fac * vo1;
        g_rgb2 = fac * vo2;
        const float4 rgb = rgb_batch[t];
        float v_alpha = 0.f;
        v_alpha += (rgb.x * T - buf0 * ra) * vo0;
        v_alpha += (rgb.y * T - buf1 * ra) * vo1;
        v_alpha += (rgb.z * T - buf2 * ra) * vo2;
        v_alpha += T_final * ra * voa;
        v_alpha += -T_final * ra * bg0 * vo0;
        v_alpha += -T_final * ra * bg1 * vo1;
        v_alpha += -T_final * ra * bg2 * vo2;
        buf0 += rgb.x * fac;
        buf1 += rgb.y * fac;
        buf2 += rgb.z * fac;
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
      g_rgb0 = sfx::wave_sum_dpp(g_rgb0);
      g_rgb1 = sfx::wave_sum_dpp(g_rgb1);
      g_rgb2 = sfx::wave_sum_dpp(g_rgb2);
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
      if (lane == 0) {
        const int g = id_batch[t];
        atomicAdd(v_rgb + 3 * g + 0, g_rgb0);
        atomicAdd(v_rgb + 3 * g + 1, g_rgb1);
        atomicAdd(v_rgb + 3 * g + 2, g_rgb2);
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

// rasterize_bwd_kernel over a culled list with rasterize_fwd_quad_kernel's layout: one 8x8 quadrant per wave
// and, per batch, per-wave lists of the records that can reach the quadrant (cull_box_may_hit) and lie at or
// before the wave's last contributing position (final_idx).  Every skipped record has alpha < 1/255 at each
// pixel of the quadrant -- the per-pixel `valid` test would be false for all lanes -- so each pixel sees the same
// contributions in the same back-to-front order; per-Gaussian sums per wave as before (one atomic per wave and
// Gaussian that any lane of the wave touches).  bw = 16.
__global__ void __launch_bounds__(MAX_BLOCK)
rasterize_bwd_quad_kernel(int tiles_x, int tiles_y, int img_h, int img_w, const int32_t* __restrict__ gids_sorted,
                          const int* __restrict__ tile_bins, const float* __restrict__ xys,
                          const float* __restrict__ conics, const float* __restrict__ colors,
                          const float* __restrict__ opacity, const float* __restrict__ background,
                          const float* __restrict__ final_Ts, const int* __restrict__ final_idx,
                          const float* __restrict__ v_out, const float* __restrict__ v_out_alpha,
                          float* __restrict__ v_xy, float* __restrict__ v_xy_abs, float* __restrict__ v_conic,
                          float* __restrict__ v_rgb, float* __restrict__ v_opacity) {
  constexpr int BW = 16, BS = BW * BW;
  __shared__ int id_batch[BS];
  __shared__ float4 xyo_batch[BS];
  __shared__ float4 conic_batch[BS];
  __shared__ float4 rgb_batch[BS];
  __shared__ unsigned char mask_batch[BS];
  __shared__ unsigned char wlist[4][BS];

  // batched views (sfx_rasterize_bwd_views_quad): blockIdx.z = view, as rasterize_fwd_quad_kernel -- tiles numbered
  // per view, per-view image planes; gids_sorted / final_idx index the one multi-view list, the per-Gaussian
  // operands and gradients are per Gaussian-view
  const int tr = threadIdx.x, lane = tr & 63, w = tr >> 6;
  const TilePix p = tile_pix_quads(tiles_x * tiles_y, tiles_x, img_h, img_w, tile_bins);
  view_advance(img_h, img_w, final_Ts, final_idx, v_out, v_out_alpha);
  const int tx0 = blockIdx.x * BW, ty0 = blockIdx.y * BW;
  const int pix = min((int)(p.pi * img_w + p.pj), img_w * img_h - 1);

  const float T_final = final_Ts[pix];
  float T = T_final;
  float buf0 = 0.f, buf1 = 0.f, buf2 = 0.f;
  const int bin_final = p.inside ? final_idx[pix] : 0;
  const float vo0 = v_out[3 * pix], vo1 = v_out[3 * pix + 1], vo2 = v_out[3 * pix + 2];
  const float voa = v_out_alpha ? v_out_alpha[pix] : 0.f;
  const float bg0 = background[0], bg1 = background[1], bg2 = background[2];
  const int wave_bin_final = sfx::wave_max_i(p.inside ? bin_final : -1);
  constexpr int RING = 8;
  __shared__ float ring[4][RING][12][4];
  __shared__ int ring_g[4][RING];
  int nring = 0;  // records parked in this wave's ring (wave-uniform)
  auto flush_ring = [&]() {
    wave_lds_sync();
    const int nv = v_xy_abs ? 11 : 9;
    for (int e = lane; e < nring * nv; e += 64) {
      const int jj = e / nv, c = e - jj * nv;
      const float* q = ring[w][jj][c];
      const float sum = (q[0] + q[1]) + (q[2] + q[3]);
      const int g = ring_g[w][jj];
      float* dst = c < 3 ? v_rgb + 3 * g + c
                 : c < 6 ? v_conic + 3 * g + (c - 3)
                 : c < 8 ? v_xy + 2 * g + (c - 6)
                 : c == 8 ? v_opacity + g
                          : v_xy_abs + 2 * g + (c - 9);
      atomicAdd(dst, sum);
    }
    wave_lds_sync();
    nring = 0;
  };

  for (int b = 0; b < p.num_batches; ++b) {
    __syncthreads();
    const int batch_end = p.range_y - 1 - BS * b;
    const int idx = batch_end - tr;
    unsigned m = 0;
    if (idx >= p.range_x) {
      const Geom s = stage_arrays(tr, gids_sorted[idx], xys, conics, colors, opacity, id_batch, xyo_batch,
                                  conic_batch, rgb_batch);
      // the mask loop written out, not quad_mask: as a function it changes this kernel's registers and occupancy
      const CullG cg = cull_setup(s.xyo.x, s.xyo.y, s.con.x, s.con.y, s.con.z, s.xyo.z);
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const int bx0 = tx0 + (qd & 1) * 8, by0 = ty0 + (qd >> 1) * 8;
        m |= (unsigned)cull_box_may_hit(cg, bx0, min(bx0 + 8, img_w) - 1, by0, min(by0 + 8, img_h) - 1) << qd;
      }
    }
    mask_batch[tr] = (unsigned char)m;
    __syncthreads();
    const int cnt = wave_compact(mask_batch, wlist[w], w, lane,
                                 [&](int t) { return batch_end - t <= wave_bin_final; });
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const int t = wlist[w][j];
      bool valid = p.inside && (batch_end - t <= bin_final);
      float alpha = 0.f, opac = 0.f, vis = 0.f, dx = 0.f, dy = 0.f;
      float4 con = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid) {
        con = conic_batch[t];
        const float4 xyo = xyo_batch[t];
        opac = xyo.z;
        dx = xyo.x - p.px;
        dy = xyo.y - p.py;
        const float sigma = 0.5f * (con.x * dx * dx + con.z * dy * dy) + con.y * dx * dy;
        vis = __expf(-sigma);
        alpha = fminf(0.99f, opac * vis);
        if (sigma < 0.f || alpha < 1.f / 255.f) valid = false;
      }
      if (!__any(valid)) continue;
      float g_rgb0 = 0.f, g_rgb1 = 0.f, g_rgb2 = 0.f, g_c0 = 0.f, g_c1 = 0.f, g_c2 = 0.f;
      float g_xy0 = 0.f, g_xy1 = 0.f, g_ax = 0.f, g_ay = 0.f, g_o = 0.f;
      if (valid) {
        const float ra = 1.f / (1.f - alpha);
        T *= ra;
        const float fac = alpha * T;
        g_rgb0 = fac * vo0;
        g_rgb1 = fac * vo1;
        g_rgb2 = fac * vo2;
        const float4 rgb = rgb_batch[t];
        float v_alpha = 0.f;
        v_alpha += (rgb.x * T - buf0 * ra) * vo0;
        v_alpha += (rgb.y * T - buf1 * ra) * vo1;
        v_alpha += (rgb.z * T - buf2 * ra) * vo2;
        v_alpha += T_final * ra * voa;
        v_alpha += -T_final * ra * bg0 * vo0;
        v_alpha += -T_final * ra * bg1 * vo1;
        v_alpha += -T_final * ra * bg2 * vo2;
        buf0 += rgb.x * fac;
        buf1 += rgb.y * fac;
        buf2 += rgb.z * fac;
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
      // row sums of the 12 slots by a transposing butterfly: lane bit 0 then bit 1 split the slots between the
      // two partners (each keeps half, adds the other's copy of it: 12 -> 6 -> 3 slots per lane), then two
      // rotations sum the row's 4 quads -- 6 + 3 + 6 DPP moves instead of 4 per slot.  Lane (l & 3) of each row
      // then holds slots 6 (l & 1) + 3 ((l >> 1) & 1) + {0, 1, 2}, parked in this wave's LDS ring; the 4 row
      // partials of 8 records are added and sent with one atomic per (record, value) by the wave's lanes in
      // parallel (flush below)
      const float vals[12] = {g_rgb0, g_rgb1, g_rgb2, g_c0, g_c1, g_c2, g_xy0, g_xy1, g_o, g_ax, g_ay, 0.f};
      const bool hi0 = lane & 1, hi1 = lane & 2;
      float h6[6], h3[3];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const float keep = hi0 ? vals[i + 6] : vals[i], send = hi0 ? vals[i] : vals[i + 6];
        h6[i] = keep + sfx::dpp_mov<0xB1>(send);  // quad [1,0,3,2]
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float keep = hi1 ? h6[i + 3] : h6[i], send = hi1 ? h6[i] : h6[i + 3];
        h3[i] = keep + sfx::dpp_mov<0x4E>(send);  // quad [2,3,0,1]
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) h3[i] += sfx::dpp_mov<0x124>(h3[i]);  // row_ror:4
#pragma unroll
      for (int i = 0; i < 3; ++i) h3[i] += sfx::dpp_mov<0x128>(h3[i]);  // row_ror:8
      if ((lane & 15) < 4) {
        const int base = 6 * (lane & 1) + 3 * ((lane >> 1) & 1);
#pragma unroll
        for (int i = 0; i < 3; ++i) ring[w][nring][base + i][lane >> 4] = h3[i];
      }
      if (lane == 0) ring_g[w][nring] = id_batch[t];
      if (++nring == RING) flush_ring();
    }
  }
  flush_ring();
}

// ---- N channels (ABI v16) ---------------------------------------------------------------------------------------
// gsplat's rasterize_gaussians for any channel count -- depth maps, alpha-weighted normals, per-Gaussian feature
// vectors: the three colour accumulators become CH of them, CH a compile-time tier in {1, 2, 4, 8, 16, 32}; the
// run-time channel count C <= CH selects the smallest tier that holds it, reads only C real channels from global
// memory and zero-fills the rest.
//
// Layout: one workgroup per tile over (gids_sorted, tile_bins), as the 3-channel kernels -- gsplat's full
// list or a culled one.  The workgroup is bw*bw threads rounded up to whole waves (the extra threads own no
// pixel), so every wave-wide operation below runs with all 64 lanes.  Per batch of blockDim Gaussians the
// geometry (x, y, opacity | conic) is staged in LDS as two float4 and the colour row at a stride of CH + 4
// floats: the inner loop reads one row for all lanes (a broadcast, ds_read_b128), and the staging writes of 8
// consecutive lanes (16 bytes each, rows 4 (CH + 4) bytes apart) fall on 8 different groups of 4 banks instead
// of one, which is where a 32-float stride puts them.  CH = 32: 36 KiB of colours + 9 KiB of geometry.
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

  const int tr = threadIdx.x, nthreads = blockDim.x;
  const TilePix p = tile_pix_rows(0, tiles_x, bw, nthreads, true, img_h, img_w, tile_bins);
  bool done = !p.inside;
  float T = 1.f;
  int cur_idx = 0;
  float acc[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) acc[c] = 0.f;
  for (int b = 0; b < p.num_batches; ++b) {
    // resync before overwriting the batch; early exit when the whole tile is done
    if (__syncthreads_count(done) >= nthreads) break;
    const int batch_start = p.range_x + nthreads * b;
    const int idx = batch_start + tr;
    if (idx < p.range_y) {
      const int g = gids_sorted[idx];
      stage_geom(tr, g, xys, conics, opacity, xyo_batch, conic_batch);
      stage_colors<CH>(colors, g, C, vec4, col_batch + tr * STRIDE);
    }
    __syncthreads();
    const int batch_size = min(nthreads, p.range_y - batch_start);
    for (int t = 0; (t < batch_size) && !done; ++t) {
      const float4 con = conic_batch[t];
      const float4 xyo = xyo_batch[t];
      float vis;
      if (!fwd_step(xyo.x, xyo.y, xyo.z, con.x, con.y, con.z, p.px, p.py, T, done, vis)) continue;
      float col[CH];
      load_row<CH>(col_batch + t * STRIDE, col);
      fwd_accumulate<CH>(acc, col, vis);
      cur_idx = batch_start + t;
    }
  }
  fwd_store<CH>(p, img_w, C, T, cur_idx, acc, background, 0, final_Ts, final_idx, out_img, out_alpha);
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

  const int tr = threadIdx.x, nthreads = blockDim.x, block_size = bw * bw;
  const TilePix p = tile_pix_rows(0, tiles_x, bw, nthreads, true, img_h, img_w, tile_bins);
  const int pix = p.inside ? (int)(p.pi * img_w + p.pj) : 0;

  const float T_final = final_Ts[pix];
  float T = T_final;
  const int bin_final = p.inside ? final_idx[pix] : 0;
  float buf[CH], vo[CH];
  float bgvo = 0.f;  // sum over channels of background[c] * v_out[c]: the pixel's constant in the v_alpha terms
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    buf[c] = 0.f;
    vo[c] = (c < C && p.inside) ? v_out[(size_t)pix * C + c] : 0.f;
    if (c < C) bgvo += background[c] * vo[c];
  }
  const float voa = (v_out_alpha && p.inside) ? v_out_alpha[pix] : 0.f;
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

  for (int b = 0; b < p.num_batches; ++b) {
    __syncthreads();
    const int batch_end = p.range_y - 1 - nthreads * b;
    const int batch_size = min(nthreads, batch_end + 1 - p.range_x);
    const int idx = batch_end - tr;
    if (idx >= p.range_x) {
      const int g = gids_sorted[idx];
      id_batch[tr] = g;
      stage_geom(tr, g, xys, conics, opacity, xyo_batch, conic_batch);
      stage_colors<CH>(colors, g, C, vec4, col_batch + tr * STRIDE);
    }
    __syncthreads();
    for (int t = max(0, batch_end - wave_bin_final); t < batch_size; ++t) {
      bool valid = p.inside && (batch_end - t <= bin_final);
      float alpha = 0.f, opac = 0.f, vis = 0.f, dx = 0.f, dy = 0.f;
      float4 con = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid) {
        con = conic_batch[t];
        const float4 xyo = xyo_batch[t];
        opac = xyo.z;
        dx = xyo.x - p.px;
        dy = xyo.y - p.py;
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

// ---- host side ------------------------------------------------------------------------------------------------
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

int sfx_rasterize_fwd(int tiles_x, int tiles_y, int block_width, int img_h, int img_w, const int32_t* gids_sorted,
                      const int* tile_bins, const float* xys, const float* conics, const float* colors,
                      const float* opacity, const float* background, float* final_Ts, int* final_idx,
                      float* out_img, float* out_alpha, void* stream) {
  SFX_RASTER_CHECK("sfx_rasterize_fwd", nullptr, tiles_x, tiles_y, block_width, img_h, img_w, false);
  SFX_REQUIRE(tile_bins && xys && conics && colors && opacity && background && final_Ts && final_idx && out_img,
              "sfx_rasterize_fwd: null buffer");
  dim3 grid(tiles_x, tiles_y);
  rasterize_fwd_kernel<<<grid, block_width * block_width, 0, sfx::as_stream(stream)>>>(
      tiles_x, tiles_y, block_width, img_h, img_w, gids_sorted, tile_bins, xys, conics, colors, opacity, background,
      final_Ts, final_idx, out_img, out_alpha, 0);
  return sfx::check_launch("sfx_rasterize_fwd");
}

int sfx_rasterize_bwd(int tiles_x, int tiles_y, int block_width, int img_h, int img_w, const int32_t* gids_sorted,
                      const int* tile_bins, const float* xys, const float* conics, const float* colors,
                      const float* opacity, const float* background, const float* final_Ts, const int* final_idx,
                      const float* v_out, const float* v_out_alpha, float* v_xy, float* v_xy_abs, float* v_conic,
                      float* v_rgb, float* v_opacity, void* stream) {
  SFX_RASTER_CHECK("sfx_rasterize_bwd", nullptr, tiles_x, tiles_y, block_width, img_h, img_w, false);
  SFX_REQUIRE(tile_bins && xys && conics && colors && opacity && background && final_Ts && final_idx && v_out &&
                  v_xy && v_conic && v_rgb && v_opacity,
              "sfx_rasterize_bwd: null buffer");
  dim3 grid(tiles_x, tiles_y);
  rasterize_bwd_kernel<<<grid, block_width * block_width, 0, sfx::as_stream(stream)>>>(
      tiles_x, tiles_y, block_width, img_h, img_w, gids_sorted, tile_bins, xys, conics, colors, opacity, background,
      final_Ts, final_idx, v_out, v_out_alpha, v_xy, v_xy_abs, v_conic, v_rgb, v_opacity);
  return sfx::check_launch("sfx_rasterize_bwd");
}

// ---- batched views (eval path of rasterize_gaussians_to_multiimgs): blockIdx.z = view, one multi-view list -------
int sfx_rasterize_fwd_views(int views, int tiles_x, int tiles_y, int block_width, int img_h, int img_w,
                            const int32_t* gids_sorted, const int* tile_bins, const float* xys, const float* conics,
                            const float* colors, const float* opacity, const float* background, int clamp_max1,
                            float* final_Ts, int* final_idx, float* out_img, float* out_alpha, void* stream) {
  SFX_RASTER_CHECK("sfx_rasterize_fwd_views", &views, tiles_x, tiles_y, block_width, img_h, img_w, false);
  SFX_REQUIRE(tile_bins && xys && conics && colors && opacity && background && final_Ts && final_idx && out_img,
              "sfx_rasterize_fwd_views: null buffer");
  dim3 grid(tiles_x, tiles_y, views);
  rasterize_fwd_kernel<<<grid, block_width * block_width, 0, sfx::as_stream(stream)>>>(
      tiles_x, tiles_y, block_width, img_h, img_w, gids_sorted, tile_bins, xys, conics, colors, opacity, background,
      final_Ts, final_idx, out_img, out_alpha, clamp_max1);
  return sfx::check_launch("sfx_rasterize_fwd_views");
}

int sfx_pack_raster_records(int n, const float* xys, const float* conics, const float* colors, const float* opacity,
                            float* records, void* stream) {
  SFX_REQUIRE(n >= 0, "sfx_pack_raster_records: n < 0");
  if (n == 0) return SFX_OK;
  SFX_REQUIRE(xys && conics && colors && opacity && records, "sfx_pack_raster_records: null buffer");
  SFX_REQUIRE((reinterpret_cast<uintptr_t>(records) & 15) == 0, "sfx_pack_raster_records: records not 16-byte aligned");
  pack_raster_records_kernel<<<sfx::ceil_div(n, 256), 256, 0, sfx::as_stream(stream)>>>(
      n, xys, conics, colors, opacity, reinterpret_cast<float4*>(records));
  return sfx::check_launch("sfx_pack_raster_records");
}

int sfx_rasterize_fwd_views_packed(int views, int tiles_x, int tiles_y, int block_width, int img_h, int img_w,
                                   const int32_t* gids_sorted, const int* tile_bins, const float* records,
                                   const float* background, int clamp_max1, float* final_Ts, int* final_idx,
                                   float* out_img, float* out_alpha, void* stream) {
  SFX_RASTER_CHECK("sfx_rasterize_fwd_views_packed", &views, tiles_x, tiles_y, block_width, img_h, img_w, false);
  SFX_REQUIRE(tile_bins && records && background && final_Ts && final_idx && out_img,
              "sfx_rasterize_fwd_views_packed: null buffer");
  SFX_REQUIRE((reinterpret_cast<uintptr_t>(records) & 15) == 0, "sfx_rasterize_fwd_views_packed: records alignment");
  dim3 grid(tiles_x, tiles_y, views);
  rasterize_fwd_packed_kernel<<<grid, block_width * block_width, 0, sfx::as_stream(stream)>>>(
      tiles_x, tiles_y, block_width, img_h, img_w, gids_sorted, tile_bins, reinterpret_cast<const float4*>(records),
      background, final_Ts, final_idx, out_img, out_alpha, clamp_max1);
  return sfx::check_launch("sfx_rasterize_fwd_views_packed");
}

int sfx_rasterize_fwd_views_quad(int views, int tiles_x, int tiles_y, int block_width, int img_h, int img_w,
                                 const int32_t* gids_sorted, const int* tile_bins, const float* records,
                                 const float* background, int clamp_max1, float* final_Ts, int* final_idx,
                                 float* out_img, float* out_alpha, void* stream) {
  SFX_RASTER_CHECK("sfx_rasterize_fwd_views_quad", &views, tiles_x, tiles_y, block_width, img_h, img_w, true);
  SFX_REQUIRE(tile_bins && records && background && final_Ts && final_idx && out_img,
              "sfx_rasterize_fwd_views_quad: null buffer");
  SFX_REQUIRE((reinterpret_cast<uintptr_t>(records) & 15) == 0, "sfx_rasterize_fwd_views_quad: records alignment");
  dim3 grid(tiles_x, tiles_y, views);
  rasterize_fwd_quad_kernel<<<grid, 256, 0, sfx::as_stream(stream)>>>(
      tiles_x, tiles_y, img_h, img_w, gids_sorted, tile_bins, reinterpret_cast<const float4*>(records), background,
      final_Ts, final_idx, out_img, out_alpha, clamp_max1);
  return sfx::check_launch("sfx_rasterize_fwd_views_quad");
}

int sfx_rasterize_bwd_quad(int tiles_x, int tiles_y, int block_width, int img_h, int img_w, const int32_t* gids_sorted,
                           const int* tile_bins, const float* xys, const float* conics, const float* colors,
                           const float* opacity, const float* background, const float* final_Ts, const int* final_idx,
                           const float* v_out, const float* v_out_alpha, float* v_xy, float* v_xy_abs, float* v_conic,
                           float* v_rgb, float* v_opacity, void* stream) {
  SFX_RASTER_CHECK("sfx_rasterize_bwd_quad", nullptr, tiles_x, tiles_y, block_width, img_h, img_w, true);
  SFX_REQUIRE(tile_bins && xys && conics && colors && opacity && background && final_Ts && final_idx && v_out &&
                  v_xy && v_conic && v_rgb && v_opacity,
              "sfx_rasterize_bwd_quad: null buffer");
  dim3 grid(tiles_x, tiles_y);
  rasterize_bwd_quad_kernel<<<grid, 256, 0, sfx::as_stream(stream)>>>(
      tiles_x, tiles_y, img_h, img_w, gids_sorted, tile_bins, xys, conics, colors, opacity, background, final_Ts,
      final_idx, v_out, v_out_alpha, v_xy, v_xy_abs, v_conic, v_rgb, v_opacity);
  return sfx::check_launch("sfx_rasterize_bwd_quad");
}

// batched views, backward (the training render of rasterize_gaussians_to_multiimgs_batched).  It words the
// view-count message itself, and refuses an empty image (0 x 0 tiles would match) under the tile-bound message.
int sfx_rasterize_bwd_views_quad(int views, int tiles_x, int tiles_y, int block_width, int img_h, int img_w,
                                 const int32_t* gids_sorted, const int* tile_bins, const float* xys,
                                 const float* conics, const float* colors, const float* opacity,
                                 const float* background, const float* final_Ts, const int* final_idx,
                                 const float* v_out, const float* v_out_alpha, float* v_xy, float* v_xy_abs,
                                 float* v_conic, float* v_rgb, float* v_opacity, void* stream) {
  SFX_REQUIRE(views >= 1 && views <= 65535, "sfx_rasterize_bwd_views_quad: views must be in [1,65535]");
  SFX_RASTER_CHECK("sfx_rasterize_bwd_views_quad", nullptr, tiles_x, tiles_y, block_width, img_h, img_w, true);
  SFX_REQUIRE(img_h > 0 && img_w > 0, "sfx_rasterize_bwd_views_quad: tile bounds do not match the image size");
  SFX_REQUIRE(gids_sorted && tile_bins && xys && conics && colors && opacity && background && final_Ts && final_idx &&
                  v_out && v_xy && v_conic && v_rgb && v_opacity,
              "sfx_rasterize_bwd_views_quad: null buffer");
  dim3 grid(tiles_x, tiles_y, views);
  rasterize_bwd_quad_kernel<<<grid, 256, 0, sfx::as_stream(stream)>>>(
      tiles_x, tiles_y, img_h, img_w, gids_sorted, tile_bins, xys, conics, colors, opacity, background, final_Ts,
      final_idx, v_out, v_out_alpha, v_xy, v_xy_abs, v_conic, v_rgb, v_opacity);
  return sfx::check_launch("sfx_rasterize_bwd_views_quad");
}

// ---- N channels ---------------------------------------------------------------------------------------------------
int sfx_rasterize_fwd_nd(int tiles_x, int tiles_y, int block_width, int img_h, int img_w, int channels,
                         const int32_t* gids_sorted, const int* tile_bins, const float* xys, const float* conics,
                         const float* colors, const float* opacity, const float* background, float* final_Ts,
                         int* final_idx, float* out_img, float* out_alpha, void* stream) {
  SFX_REQUIRE(img_h >= 0 && img_w >= 0 && tiles_x >= 0 && tiles_y >= 0, "sfx_rasterize_fwd_nd: negative size");
  SFX_REQUIRE(channels >= 1 && channels <= 32, "sfx_rasterize_fwd_nd: channels must be in [1,32] (got %d)", channels);
  SFX_RASTER_CHECK("sfx_rasterize_fwd_nd", nullptr, tiles_x, tiles_y, block_width, img_h, img_w, false);
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
  SFX_REQUIRE(channels >= 1 && channels <= 32, "sfx_rasterize_bwd_nd: channels must be in [1,32] (got %d)", channels);
  SFX_RASTER_CHECK("sfx_rasterize_bwd_nd", nullptr, tiles_x, tiles_y, block_width, img_h, img_w, false);
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

// Device helpers of the tile rasterizer (rasterize.hip) and of the contribution culling that the intersection
// kernels (render.hip) share with it: tile / pixel geometry, batch staging, the per-pixel forward step of gsplat's
// rasterize_forward, the per-wave quadrant lists.  Leaf functions only:
// the kernels keep their own __shared__ arrays, barriers and loops.
#pragma once

#include "common.h"

namespace sfxr {

constexpr int MAX_BLOCK = 256;

// ---- tile / pixel geometry ------------------------------------------------------------------------------------
// One thread's pixel of one tile, and the tile's slice [range_x, range_y) of the sorted list in batches.
struct TilePix {
  int tile_id;
  unsigned pi, pj;  // pixel row, column
  float px, py;     // pixel centre
  bool inside;      // the thread owns a pixel of the image
  int range_x, range_y, num_batches;
};

__device__ __forceinline__ void tile_pix_finish(TilePix& p, bool owns, int batch, int img_h, int img_w,
                                                const int* __restrict__ tile_bins) {
  p.px = (float)p.pj + 0.5f;
  p.py = (float)p.pi + 0.5f;
  p.inside = (owns && p.pi < (unsigned)img_h && p.pj < (unsigned)img_w);
  p.range_x = tile_bins[2 * p.tile_id];
  p.range_y = tile_bins[2 * p.tile_id + 1];
  p.num_batches = (p.range_y - p.range_x + batch - 1) / batch;
}

// Row-major mapping: flat thread rank -> (ty, tx) of a bw x bw tile.  view_tiles: tiles per view where blockIdx.z
// is the view (tiles are numbered per view), 0 in the single-view kernels.  batch: records staged per batch.
// whole_waves: the workgroup is bw*bw rounded up to whole waves and the extra threads own no pixel.
__device__ __forceinline__ TilePix tile_pix_rows(int view_tiles, int tiles_x, int bw, int batch, bool whole_waves,
                                                 int img_h, int img_w, const int* __restrict__ tile_bins) {
  TilePix p;
  p.tile_id = blockIdx.z * view_tiles + blockIdx.y * tiles_x + blockIdx.x;
  const int tr = threadIdx.x;
  const int ty = tr / bw, tx = tr - ty * bw;
  p.pi = blockIdx.y * bw + ty;
  p.pj = blockIdx.x * bw + tx;
  tile_pix_finish(p, !whole_waves || tr < bw * bw, batch, img_h, img_w, tile_bins);
  return p;
}

// Quadrant mapping of a 16x16 tile: wave w owns the 8x8 quadrant (w & 1, w >> 1), lane -> (lane >> 3, lane & 7).
__device__ __forceinline__ TilePix tile_pix_quads(int view_tiles, int tiles_x, int img_h, int img_w,
                                                  const int* __restrict__ tile_bins) {
  TilePix p;
  p.tile_id = blockIdx.z * view_tiles + blockIdx.y * tiles_x + blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int qx = (w & 1) * 8, qy = (w >> 1) * 8;
  p.pi = blockIdx.y * 16 + qy + (lane >> 3);
  p.pj = blockIdx.x * 16 + qx + (lane & 7);
  tile_pix_finish(p, true, 256, img_h, img_w, tile_bins);
  return p;
}

// Batched views: blockIdx.z = view.  Advances the per-pixel planes (transmittance, index, 3-channel image,
// optional alpha) to this view's.
template <class F, class I>
__device__ __forceinline__ void view_advance(int img_h, int img_w, F& final_Ts, I& final_idx, F& img3, F& alpha) {
  if (blockIdx.z > 0) {
    const long long po = (long long)blockIdx.z * img_h * img_w;
    final_Ts += po; final_idx += po; img3 += 3 * po;
    if (alpha) alpha += po;
  }
}

// ---- staging ----------------------------------------------------------------------------------------------------
struct Geom {
  float4 xyo;  // x, y, opacity, pad
  float4 con;  // conic a, b, c, pad
};

// four-array form: geometry of Gaussian g into slot tr of the batch
__device__ __forceinline__ Geom stage_geom(int tr, int g, const float* __restrict__ xys,
                                           const float* __restrict__ conics, const float* __restrict__ opacity,
                                           float4* xyo_batch, float4* conic_batch) {
  Geom s;
  s.xyo = make_float4(xys[2 * g], xys[2 * g + 1], opacity[g], 0.f);
  s.con = make_float4(conics[3 * g], conics[3 * g + 1], conics[3 * g + 2], 0.f);
  xyo_batch[tr] = s.xyo;
  conic_batch[tr] = s.con;
  return s;
}

// ... with its id and 3-channel colour
__device__ __forceinline__ Geom stage_arrays(int tr, int g, const float* __restrict__ xys,
                                             const float* __restrict__ conics, const float* __restrict__ colors,
                                             const float* __restrict__ opacity, int* id_batch, float4* xyo_batch,
                                             float4* conic_batch, float4* rgb_batch) {
  id_batch[tr] = g;
  const Geom s = stage_geom(tr, g, xys, conics, opacity, xyo_batch, conic_batch);
  rgb_batch[tr] = make_float4(colors[3 * g], colors[3 * g + 1], colors[3 * g + 2], 0.f);
  return s;
}

// Record form (eval path).  One 48-byte record per projected Gaussian, written once per view batch: r0 = (x, y,
// opacity, conic.a), r1 = (conic.b, conic.c, r, g), r2 = (b, 0, 0, 0), at a 64-byte stride (one 64-byte sector per
// record gather; at 48 bytes two of every four records straddle a sector boundary: 1.5 sectors fetched per 36
// bytes used).  The rasterizer's per-batch fetch is one gather of a 16-byte-aligned record instead of four
// gathers from four arrays (xys 8 B, opacity 4 B, conics 12 B, colours 12 B).  Measured: the same kernel time as
// the four-array form (config E 2285 vs 2278 us for 9 1920x1080 views) -- the rasterizer is not bound by its
// gathers.  A wave-uniform skip of Gaussians whose alpha >= 1/255 ellipse misses the wave's 16 x 4 pixels (exact,
// extents in r2) was 25 % slower (2855 us) and is not kept.
__device__ __forceinline__ void write_record(float4* __restrict__ rec, long long i, const float* xy, float opac,
                                             const float* conic, const float* rgb) {
  rec[4 * i + 0] = make_float4(xy[0], xy[1], opac, conic[0]);
  rec[4 * i + 1] = make_float4(conic[1], conic[2], rgb[0], rgb[1]);
  rec[4 * i + 2] = make_float4(rgb[2], 0.f, 0.f, 0.f);
}

struct Rec {
  float4 a, q;  // r0, r1 of the record
  __device__ __forceinline__ float x() const { return a.x; }
  __device__ __forceinline__ float y() const { return a.y; }
  __device__ __forceinline__ float opac() const { return a.z; }
  __device__ __forceinline__ float ca() const { return a.w; }
  __device__ __forceinline__ float cb() const { return q.x; }
  __device__ __forceinline__ float cc() const { return q.y; }
  __device__ __forceinline__ float red() const { return q.z; }
  __device__ __forceinline__ float green() const { return q.w; }
};

// record g into slot tr of the batch; blue (r2.x) is kept apart: it is read only for Gaussians that pass the
// alpha test
__device__ __forceinline__ Rec stage_record(int tr, long long g, const float4* __restrict__ rec, float4* r0_batch,
                                            float4* r1_batch, float* r2_batch) {
  Rec r;
  r.a = rec[4 * g];
  r.q = rec[4 * g + 1];
  r0_batch[tr] = r.a;
  r1_batch[tr] = r.q;
  r2_batch[tr] = reinterpret_cast<const float*>(rec + 4 * g + 2)[0];
  return r;
}

// ---- forward step -------------------------------------------------------------------------------------------------
// One Gaussian (centre, opacity, conic) at one pixel of rasterize_forward: alpha = min(0.999, o exp(-sigma)); skipped
// where sigma < 0 or alpha < 1/255; the pixel is done (nothing added) once T (1 - alpha) <= 1e-4.  Returns whether
// the Gaussian contributes; then vis = alpha T is its weight and T has advanced.  Every fused multiply-add is
// written out (contraction off), so all forward kernels round alike whatever the compiler would pick in each
// inlined copy: the eval path's culled and full lists, and the record and four-array forms, give the same bits.
__device__ __forceinline__ bool fwd_step(float gx, float gy, float opac, float ca, float cb, float cc, float px,
                                         float py, float& T, bool& done, float& vis) {
#pragma clang fp contract(off)
  const float dx = gx - px, dy = gy - py;
  const float sigma = __builtin_fmaf(dy, cb * dx, 0.5f * __builtin_fmaf(dx, ca * dx, dy * (cc * dy)));
  const float alpha = fminf(0.999f, opac * __expf(-sigma));
  if (sigma < 0.f || alpha < 1.f / 255.f) return false;
  const float next_T = T * (1.f - alpha);
  if (next_T <= 1e-4f) {
    done = true;
    return false;
  }
  vis = alpha * T;
  T = next_T;
  return true;
}

template <int CH>
__device__ __forceinline__ void fwd_accumulate(float (&acc)[CH], const float (&col)[CH], float vis) {
#pragma unroll
  for (int c = 0; c < CH; ++c) acc[c] = __builtin_fmaf(vis, col[c], acc[c]);
}

// A pixel's outputs: final T and list position, the first C <= CH channels over the background, alpha.
// clamp_max1: reference utils/gs_utils.py:111 torch.clamp(rgb, max=1), fused for the eval path.
template <int CH>
__device__ __forceinline__ void fwd_store(const TilePix& p, int img_w, int C, float T, int cur_idx,
                                          const float (&acc)[CH], const float* __restrict__ background,
                                          int clamp_max1, float* __restrict__ final_Ts, int* __restrict__ final_idx,
                                          float* __restrict__ out_img, float* __restrict__ out_alpha) {
  if (!p.inside) return;
  const int pix = p.pi * img_w + p.pj;
  final_Ts[pix] = T;
  final_idx[pix] = cur_idx;
  float* o = out_img + (size_t)pix * C;
#pragma unroll
  for (int c = 0; c < CH; ++c)
    if (c < C) {
      const float v = __builtin_fmaf(T, background[c], acc[c]);
      o[c] = clamp_max1 ? fminf(v, 1.f) : v;
    }
  if (out_alpha) out_alpha[pix] = 1.f - T;
}

// ---- wave-level pieces --------------------------------------------------------------------------------------------
// LDS writes of a wave made visible to its other lanes (the LDS serves one wave's accesses in order; the fences
// and the barrier only keep the compiler from moving accesses across this point).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- exact contribution culling (eval path, ABI v9) ---------------------------------------------------------
// gsplat bins a Gaussian into every tile of its 3-sigma square (get_tile_bbox) and the per-pixel loop then skips
// it wherever alpha = min(0.999, o exp(-sigma)) < 1/255.  A (Gaussian, pixel box) pair can be dropped without
// changing any output bit when no pixel centre in the box can pass that test: sigma is a positive-definite
// quadratic in d = (x, y) - pixel, so its minimum over the box of d is 0 (centre inside) or on an edge (a 1-D
// quadratic clamped to the edge).  The minimum is evaluated in fp32 and compared against a limit raised by
// margins far above every rounding involved: the kernel's own fp32 sigma (relative error <= a few ulp *
// (1 + rho) / (1 - rho), rho = |b| / sqrt(ac) <= 0.99 here), this evaluation, __expf / __logf (absolute 1e-4 on
// the log threshold).  Near-degenerate (rho > 0.99), non-PD and non-finite conics or positions are never
// dropped.  Dropped pairs are exactly ones the rasterizer would `continue` past for every pixel of the box, so
// images, alphas and final T are bit-identical; only final_idx (a list position) refers to the shorter list.
struct CullG {
  float gx, gy, a, b, c, ia, ic, lim;  // lim: box minimum of sigma above which the box is dropped
  bool never, always;                  // never: o < 1/255 everywhere; always: never drop (degenerate input)
};

__device__ __forceinline__ CullG cull_setup(float x, float y, float ca, float cb, float cc, float opac) {
  // no contraction here or in cull_box_may_hit: the count and emit kernels must take the same decision for every
  // (Gaussian, tile) (the emit walk fills exactly the slots the count reserved), whatever FMAs the compiler
  // would pick in each inlined copy
#pragma clang fp contract(off)
  CullG g;
  g.gx = x; g.gy = y; g.a = ca; g.b = cb; g.c = cc;
  g.ia = 0.f; g.ic = 0.f; g.lim = 0.f;
  g.always = false; g.never = false;
  const float ac = ca * cc;
  if (!(ca > 0.f) || !(cc > 0.f) || !(cb * cb < 0.9801f * ac) || !isfinite(x) || !isfinite(y) || !isfinite(ac)) {
    g.always = true;  // rho > 0.99, not positive definite, or non-finite
    return g;
  }
  if (!(opac * 255.f >= 0.999f)) {  // o < 1/255 (minus 1e-3): alpha < 1/255 at every pixel; NaN: keep
    if (opac * 255.f < 0.999f) g.never = true; else g.always = true;
    return g;
  }
  const float rho = sqrtf(cb * cb / ac);
  g.ia = 1.f / ca;
  g.ic = 1.f / cc;
  // may contribute iff sigma_min * (1 - 1e-4 / (1 - rho)) <= ln(255 o) + 2e-4
  g.lim = (__logf(opac * 255.f) + 2e-4f) / (1.f - 1e-4f / (1.f - rho));
  return g;
}

// May the Gaussian reach alpha >= 1/255 at a pixel centre of [px0, px1] x [py0, py1] (integer pixel bounds,
// inclusive, already clipped to the image)?
__device__ __forceinline__ bool cull_box_may_hit(const CullG& g, int px0, int px1, int py0, int py1) {
#pragma clang fp contract(off)
  if (g.always) return true;
  if (g.never || px0 > px1 || py0 > py1) return false;
  // d = g - (p + 0.5) over the pixel centres
  const float u0 = g.gx - ((float)px1 + 0.5f), u1 = g.gx - ((float)px0 + 0.5f);
  const float v0 = g.gy - ((float)py1 + 0.5f), v1 = g.gy - ((float)py0 + 0.5f);
  if (u0 <= 0.f && u1 >= 0.f && v0 <= 0.f && v1 >= 0.f) return true;
  float m = 3.0e38f;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float dx = e ? u1 : u0;
    const float dy = fminf(fmaxf(-g.b * dx * g.ic, v0), v1);
    m = fminf(m, 0.5f * (g.a * dx * dx + g.c * dy * dy) + g.b * dx * dy);
    const float ey = e ? v1 : v0;
    const float ex = fminf(fmaxf(-g.b * ey * g.ia, u0), u1);
    m = fminf(m, 0.5f * (g.a * ex * ex + g.c * ey * ey) + g.b * ex * ey);
  }
  return m <= g.lim;
}

// ---- per-wave quadrant lists --------------------------------------------------------------------------------------
// bit qd: may the Gaussian reach the 8x8 quadrant qd (clipped to the image) of the 16x16 tile at (tx0, ty0)?
__device__ __forceinline__ unsigned quad_mask(const CullG& cg, int tx0, int ty0, int img_w, int img_h) {
  unsigned m = 0;
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const int bx0 = tx0 + (qd & 1) * 8, by0 = ty0 + (qd >> 1) * 8;
    m |= (unsigned)cull_box_may_hit(cg, bx0, min(bx0 + 8, img_w) - 1, by0, min(by0 + 8, img_h) - 1) << qd;
  }
  return m;
}

// Wave w's list of a staged batch of 256: the positions t, in batch order, whose mask has bit w and for which
// keep(t) holds.  Returns the list's length.
template <class Keep>
__device__ __forceinline__ int wave_compact(const unsigned char* mask_batch, unsigned char* wlist_w, int w, int lane,
                                            Keep keep) {
  const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  int cnt = 0;
#pragma unroll
  for (int ch = 0; ch < 256 / 64; ++ch) {
    const int t = ch * 64 + lane;
    const bool hit = ((mask_batch[t] >> w) & 1) && keep(t);
    const unsigned long long bal = __ballot(hit);
    if (hit) wlist_w[cnt + __popcll(bal & lt_mask)] = (unsigned char)t;
    cnt += __popcll(bal);
  }
  return cnt;
}

// ---- host side ------------------------------------------------------------------------------------------------
// The argument checks shared by the entry points that take a tile grid: view count (views: null where the entry has
// none or words the message itself), block width (exactly 16 where require_bw16), tile bounds against the image size.
inline int raster_check(const char* name, const int* views, int tiles_x, int tiles_y, int block_width, int img_h,
                        int img_w, bool require_bw16) {
  if (views) SFX_REQUIRE(*views >= 1 && *views <= 65535, "%s: bad view count", name);
  if (require_bw16)
    SFX_REQUIRE(block_width == 16, "%s: block_width must be 16", name);
  else
    SFX_REQUIRE(block_width > 1 && block_width <= 16, "%s: block_width must be in (1,16]", name);
  SFX_REQUIRE(tiles_x == (img_w + block_width - 1) / block_width && tiles_y == (img_h + block_width - 1) / block_width,
              "%s: tile bounds do not match the image size", name);
  return SFX_OK;
}

#define SFX_RASTER_CHECK(...)                                  \
  do {                                                         \
    if (int rc_ = ::sfxr::raster_check(__VA_ARGS__)) return rc_; \
  } while (0)

}  // namespace sfxr

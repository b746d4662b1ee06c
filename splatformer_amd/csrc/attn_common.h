// Device helpers shared by the window-attention kernels (attention.hip, attn_proj.hip): the LDS layouts of the
// split-term operand images, the fragment reads and term products on them, and the steps every kernel runs on a
// block of S^T scores held in registers.  Leaf functions only; the kernels own their shared memory and barriers.
//
// Register layout all of it relies on (v_mfma_f32_32x32x*): a lane owns column l32 = lane & 31 (its query) and,
// per 32-row block, the 16 rows (r & 3) + 8 (r >> 2) + 4 h, h = lane >> 5 -- so a softmax over keys is a register
// reduction plus one exchange with the other half-wave, and registers 8 st .. 8 st + 7 of a block are the 16-deep
// B-operand step st of the next product (element j <-> row 16 st + 8 (j >> 2) + 4 h + (j & 3)).
//
// Term forms (F16): true -- two fp16 terms of a power-of-two-scaled value (sfx::split2h, three term products);
// false -- three bf16 terms (sfx::split3, six term products, no scale).
#pragma once

#include <type_traits>

#include "common.h"

namespace sfxa {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
template <bool F16>
using frag_t = typename std::conditional<F16, f16x8, bf16x8>::type;  // 8 terms of one operand: a 16-deep MFMA step

constexpr int KMAX = 128;  // keys (and queries) per window block
constexpr int VST = 136;   // transposed-image row stride (16-bit elements): 272-byte rows
constexpr int nterms(bool f16) { return f16 ? 2 : 3; }
constexpr int row_bytes(int KD) { return KD == 16 ? 48 : 64; }  // bytes per term row of a row image

// XCD-aware numbering over a 1-D grid padded to a multiple of 8: consecutive blocks go round-robin to the 8
// XCDs, so logical id L = xcd * (grid / 8) + slot puts all heads of a window on one XCD back to back -- the
// 128-byte qkv lines its heads share (d = 16: two heads per line) are fetched from HBM once into that L2.
__device__ __forceinline__ int xcd_logical_id() {
  const int nb = (int)gridDim.x;
  return (int)(blockIdx.x % 8) * (nb / 8) + (int)(blockIdx.x / 8);
}

// ---- row image [terms][128][KD] ------------------------------------------------------------------------------
// KD = 16: 48-byte rows; KD = 32: 64-byte rows, 16-byte chunks XOR-swizzled by row >> 2.  Byte offset of 16-byte
// chunk c of term row r:
template <int KD>
__device__ __forceinline__ int row_off(int r, int c) {
  return KD == 16 ? r * 48 + c * 16 : r * 64 + (((c ^ (r >> 2)) & 3) << 4);
}

// V^T chunk swizzle: the 16-byte chunk c (8 keys) of V^T row dd sits at chunk c ^ vt_swz(dd), 2 x the parity of
// dd's 4-row group.  The staging's transposed dword stores (rows 4 ch .. 4 ch + 3 of 4-8 column chunks per 32
// lanes) were 2- / 3- / 4-way bank conflicts at d = 16 / 24 / 32 (the stride-136 rows put every other chunk group on
// one bank set); swizzled they are 1- / 2- / 2-way (free for ds_write_b32), and the fragment reads stay conflict-
// free (tools/attn_banks.py)
__device__ __forceinline__ int vt_swz(int dd) { return (__builtin_popcount((unsigned)(dd >> 2)) & 1) << 1; }

// 4 elements -> the terms of x * s (bf16 terms take no scale)
template <bool F16>
__device__ __forceinline__ void split(float4 v, float s, uint2 (&t)[nterms(F16)]) {
  if constexpr (F16) sfx::split2h(v, s, t);
  else sfx::split3(v, t);
}

// zero the columns D .. KD - 1 of `term_rows` rows (term-major) that the staging never writes
template <int D, int KD>
__device__ __forceinline__ void zero_row_pad(char* rimg, int term_rows, int tid) {
  if (D < KD)
    for (int rr = tid; rr < term_rows; rr += 256)
      *reinterpret_cast<uint4*>(rimg + row_off<KD>(rr, D / 8)) = make_uint4(0, 0, 0, 0);
}

// float4 column chunk ch of row `row` into the row image, terms of v * s: byte offset within a term's image
template <int KD>
__device__ __forceinline__ int row_off4(int row, int ch) { return row_off<KD>(row, ch >> 1) + ((ch & 1) << 3); }
template <int KD, bool F16>
__device__ __forceinline__ void stage_row(char* rimg, int row, int ch, float4 v, float s) {
  uint2 t[nterms(F16)];
  split<F16>(v, s, t);
  const int o = row_off4<KD>(row, ch);
#pragma unroll
  for (int q = 0; q < nterms(F16); ++q) *reinterpret_cast<uint2*>(rimg + q * KMAX * row_bytes(KD) + o) = t[q];
}

// ---- transposed image [terms][D][136] ------------------------------------------------------------------------
// The rows (keys or queries) of every 16-group are permuted to the B-operand register order, so a lane's 8 rows of
// a 16-deep step are one 16-byte read.  Rows are staged in pairs (row even): rows row, row + 1 land on adjacent
// positions and the four transposed stores are whole dwords.  KD != 0: also into the row image `rimg` of that KD
// (the forward stages V^T only and passes no row image, the backward stages both).
template <int D, bool F16, int KD = 0>
__device__ __forceinline__ void stage_pair(char* rimg, unsigned short* timg, int row, int ch, float4 v0, float4 v1,
                                           float s) {
  constexpr int NT = nterms(F16);
  uint2 t0[NT], t1[NT];
  split<F16>(v0, s, t0);
  split<F16>(v1, s, t1);
  const int kk = row & 15;
  const int pos = (row & ~15) + 8 * ((kk >> 2) & 1) + (((kk >> 3) << 2) | (kk & 3));
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    if constexpr (KD != 0) {
      *reinterpret_cast<uint2*>(rimg + q * KMAX * row_bytes(KD) + row_off4<KD>(row, ch)) = t0[q];
      *reinterpret_cast<uint2*>(rimg + q * KMAX * row_bytes(KD) + row_off4<KD>(row + 1, ch)) = t1[q];
    }
    unsigned* vt = reinterpret_cast<unsigned*>(timg + (q * D + 4 * ch) * VST + (pos ^ (8 * vt_swz(4 * ch))));
    vt[0] = (t0[q].x & 0xffffu) | (t1[q].x << 16);
    vt[VST / 2] = (t0[q].x >> 16) | (t1[q].x & 0xffff0000u);
    vt[VST] = (t0[q].y & 0xffffu) | (t1[q].y << 16);
    vt[3 * VST / 2] = (t0[q].y >> 16) | (t1[q].y & 0xffff0000u);
  }
}

// ---- fragments ------------------------------------------------------------------------------------------------
// A fragment of a row image: 16-byte chunk c of row `row`, every term
template <int KD, bool F16>
__device__ __forceinline__ void row_frag(const char* rimg, int row, int c, frag_t<F16> (&f)[nterms(F16)]) {
#pragma unroll
  for (int q = 0; q < nterms(F16); ++q)
    f[q] = __builtin_bit_cast(frag_t<F16>,
                              *reinterpret_cast<const uint4*>(rimg + q * KMAX * row_bytes(KD) + row_off<KD>(row, c)));
}
// A fragment of a transposed image: lane row dd = l32 (zero past D), 8 keys of 16-step `step` from half h; term q
// and every term
template <int D, bool F16>
__device__ __forceinline__ frag_t<F16> tr_frag1(const unsigned short* timg, int q, int l32, int step, int h) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (l32 < D) v = *reinterpret_cast<const uint4*>(timg + (q * D + l32) * VST + (((2 * step + h) ^ vt_swz(l32)) << 3));
  return __builtin_bit_cast(frag_t<F16>, v);
}
template <int D, bool F16>
__device__ __forceinline__ void tr_frag(const unsigned short* timg, int l32, int step, int h,
                                        frag_t<F16> (&f)[nterms(F16)]) {
#pragma unroll
  for (int q = 0; q < nterms(F16); ++q) f[q] = tr_frag1<D, F16>(timg, q, l32, step, h);
}
// a lane's 8 (or fewer, zero-padded past D) values of the row at `p`, columns d0 .. d0 + 7
template <int D>
__device__ __forceinline__ void load8(const float* p, int d0, bool ok, float4& a, float4& b) {
  a = make_float4(0.f, 0.f, 0.f, 0.f);
  b = a;
  if (ok && d0 < D) {
    a = *reinterpret_cast<const float4*>(p + d0);
    if (d0 + 4 < D) b = *reinterpret_cast<const float4*>(p + d0 + 4);
  }
}
// the terms of 8 scaled values -> B-operand fragments
template <bool F16>
__device__ __forceinline__ void frag(float4 a, float4 b, float s, frag_t<F16> (&f)[nterms(F16)]) {
  uint2 ta[nterms(F16)], tb[nterms(F16)];
  split<F16>(a, s, ta);
  split<F16>(b, s, tb);
#pragma unroll
  for (int t = 0; t < nterms(F16); ++t)
    f[t] = __builtin_bit_cast(frag_t<F16>, make_uint4(ta[t].x, ta[t].y, tb[t].x, tb[t].y));
}
// a lane's query slice of a 16-deep step (B operand of S^T = K Q^T), times qs (scale * log2(e): the softmax
// exponentials are plain exp2; |q * qs| <= |q|, so a bound on |qkv| still holds)
template <bool F16>
__device__ __forceinline__ void q_frag(float4 a, float4 b, float qs, float s, frag_t<F16> (&f)[nterms(F16)]) {
  a.x *= qs; a.y *= qs; a.z *= qs; a.w *= qs;
  b.x *= qs; b.y *= qs; b.z *= qs; b.w *= qs;
  frag<F16>(a, b, s, f);
}

// ---- term products --------------------------------------------------------------------------------------------
// c += a b on one 32x32x16 step: the leading term products, smallest first (fp16x2: l h, h l, h h; bf16x3: t2 t0,
// t1 t1, t0 t2, t1 t0, t0 t1, t0 t0).  ONE (sfx_set_precision(1), the reference's autocast class): fp16 the
// leading product only, bf16 the three leading ones (16-bit significands).
template <bool F16, bool ONE = false>
__device__ __forceinline__ floatx16 mfma_terms(const frag_t<F16> (&a)[nterms(F16)], const frag_t<F16> (&b)[nterms(F16)],
                                               floatx16 c) {
  constexpr int NP = F16 ? 3 : 6;
  constexpr int QA[6] = {F16 ? 1 : 2, F16 ? 0 : 1, 0, 1, 0, 0}, QB[6] = {0, 1, F16 ? 0 : 2, 0, 1, 0};
  constexpr int JS = ONE ? (F16 ? 2 : 3) : 0;  // first term product formed
#pragma unroll
  for (int j = JS; j < NP; ++j) {
    if constexpr (F16) c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[QA[j]], b[QB[j]], c, 0, 0, 0);
    else c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[QA[j]], b[QB[j]], c, 0, 0, 0);
  }
  return c;
}

// ---- steps on NB blocks of S^T[key][query] scores (32 keys each) ----------------------------------------------
template <int NB>
__device__ __forceinline__ void score_zero(floatx16 (&s)[NB]) {
#pragma unroll
  for (int kb = 0; kb < NB; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
}
// the key of register r of block kb in lane half h
constexpr int score_key(int kb, int r, int h) { return kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h; }
// keys >= nk (padding of a short window or of a ragged last block) leave the softmax
template <int NB>
__device__ __forceinline__ void score_mask(floatx16 (&s)[NB], int h, int nk) {
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) {
    floatx16 v = s[kb];  // (a copy: conditional stores through the reference cost the exact flash kernel 25 VGPRs)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (score_key(kb, r, h) >= nk) v[r] = -INFINITY;
    s[kb] = v;
  }
}
// maximum over the blocks' keys: register axis + the other half-wave
template <int NB>
__device__ __forceinline__ float score_max(const floatx16 (&s)[NB]) {
  float mx = -INFINITY;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
  return fmaxf(mx, __shfl_xor(mx, 32, 64));
}
// s <- exp(s - mx), returns the sum over the blocks' keys.  EXP2: scores in log2 units (v_exp_f32), else __expf
template <bool EXP2, int NB>
__device__ __forceinline__ float score_exp(floatx16 (&s)[NB], float mx) {
  float sum = 0.f;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float e;
      if constexpr (EXP2) e = __builtin_amdgcn_exp2f(s[kb][r] - mx);
      else e = __expf(s[kb][r] - mx);
      s[kb][r] = e;
      sum += e;
    }
  return sum + __shfl_xor(sum, 32, 64);
}
// O^T[dd][query] += sum_key V^T[dd][key] P^T[key][query] with P^T straight from the score registers: the
// unnormalised exp values (0, 1] (F16: scaled by 2^14); 1 / sum is applied to O
template <int D, bool F16, bool ONE, int NB>
__device__ __forceinline__ floatx16 pv_terms(const floatx16 (&s)[NB], const unsigned short* Vt, int l32, int h,
                                             floatx16 o) {
#pragma unroll
  for (int kb = 0; kb < NB; ++kb)
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      constexpr int NT = nterms(F16);
      uint2 a[NT], b[NT];
      split<F16>(make_float4(s[kb][8 * st + 0], s[kb][8 * st + 1], s[kb][8 * st + 2], s[kb][8 * st + 3]), 16384.f, a);
      split<F16>(make_float4(s[kb][8 * st + 4], s[kb][8 * st + 5], s[kb][8 * st + 6], s[kb][8 * st + 7]), 16384.f, b);
      frag_t<F16> pf[NT], vf[NT];
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        pf[q] = __builtin_bit_cast(frag_t<F16>, make_uint4(a[q].x, a[q].y, b[q].x, b[q].y));
        vf[q] = tr_frag1<D, F16>(Vt, q, l32, 2 * kb + st, h);
      }
      o = mfma_terms<F16, ONE>(vf, pf, o);
    }
  return o;
}
// this lane's column of an O^T accumulator (rows dd = (r & 3) + 8 (r >> 2) + 4 h) to the D-wide row at dst
template <int D>
__device__ __forceinline__ void store_ot(float* dst, const floatx16& o, int h) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int dd = 8 * g + 4 * h;
    if (dd + 3 < D)
      *reinterpret_cast<float4*>(dst + dd) = make_float4(o[4 * g + 0], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]);
  }
}

}  // namespace sfxa

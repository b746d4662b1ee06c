// Serialized windowed multi-head attention (PTv3 SerializedAttention,
// non-flash path: reference models/pointtransformer_v3.py:121-126 patch 128,
// math restated in-tree at visualize.py:140-179).
//
// For each window of K <= 128 consecutive serialized positions and each head:
//   S = (q * scale) k^T ; P = softmax_keys(S) ; O = P v
// q/k/v rows are gathered straight from the qkv projection [N, 3C] through
// the serialized order (`qkv[order]`, row layout [3][H][d]) and the output row
// is scattered back through the same order (`feat[inverse]`), so neither the
// padded/permuted qkv nor the [N', H, K, K] score tensor is materialised.
//
// Window table: win[w] = (key_start, query_start) in serialized positions.
// Pointcept pads a ragged last window by duplicating the K - n%K points that
// precede it (get_padding_and_inverse); that window therefore attends over
// the last K real points and only its new queries are written -- the table
// encodes exactly that (key_start = n - K, query_start = floor(n/K)*K).
//
// gfx950: one 256-thread workgroup per (window, head), 4 waves x 32 queries.
// S^T = K Q^T on v_mfma_f32_32x32x2_f32 puts each query on a lane column and
// its 128 keys in registers (64 per half-wave), so the softmax is a register
// reduction + one cross-half exchange, and P^T feeds the P.V MFMA directly as
// the B operand (no LDS round trip for P).
#include <cstdlib>

#include "attn_common.h"

#ifndef SFX_ATTN_OCC16
#define SFX_ATTN_OCC16 4  // workgroups per CU the d = 16 split kernel is compiled for
#endif

namespace {

using namespace sfxa;

// ---- exact fp32 kernels (SFX_ATTN_PREC=fp32): shared steps -------------------------------------------------
// LDS rows of KMAX keys / queries: Q and K at stride DP, V at stride DPV, zero beyond D where a lane-indexed column
// read (dd = lane) needs no mask.

// zero the V padding columns D..31 once
template <int D, int DPV>
__device__ __forceinline__ void exact_zero_vpad(float* Vs, int tid) {
  if (D < 32)
    for (int e = tid; e < KMAX * (32 - D) / 4; e += 256) {
      const int row = e / ((32 - D) / 4), c4 = e - row * ((32 - D) / 4);
      *reinterpret_cast<float4*>(&Vs[row * DPV + D + 4 * c4]) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
// gather matrices M0 .. M0 + NM - 1 of (q, k, v) of this head through rows[] (zero rows where rows[] < 0):
// KMAX rows x NM mats x D/4 float4; q is scaled on the way in
template <int D, int M0, int NM, int DP, int DPV>
__device__ __forceinline__ void exact_gather(const float* __restrict__ qkv, const int* rows, long long ld, int C,
                                             int head, float scale, float* Qs, float* Ks, float* Vs, int tid) {
  constexpr int CH = D / 4;
  for (int e = tid; e < KMAX * NM * CH; e += 256) {
    const int row = e / (NM * CH);
    const int rem = e - row * NM * CH;
    const int m = NM == 1 ? 0 : rem / CH, ch = rem - m * CH;  // matrix M0 + m
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int src = rows[row];
    if (src >= 0) v = *reinterpret_cast<const float4*>(qkv + (long long)src * ld + (M0 + m) * C + head * D + 4 * ch);
    if (M0 == 0 && m == 0) {
      v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
      *reinterpret_cast<float4*>(&Qs[row * DP + 4 * ch]) = v;
    } else if (M0 + m == 1) {
      *reinterpret_cast<float4*>(&Ks[row * DP + 4 * ch]) = v;
    } else {
      *reinterpret_cast<float4*>(&Vs[row * DPV + 4 * ch]) = v;
    }
  }
}
// c += a b^T on v_mfma_f32_32x32x2_f32, four k-values of this lane half
__device__ __forceinline__ floatx16 exact_mfma4(float4 a, float4 b, floatx16 c) {
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, c, 0, 0, 0);
}
// this lane's half (HALF = D / 2 k-values per lane half in S = K Q^T) of LDS row `row`
template <int HALF>
__device__ __forceinline__ void exact_load_half(const float* row, int h, float4 (&v)[HALF / 4]) {
#pragma unroll
  for (int c = 0; c < HALF / 4; ++c) v[c] = *reinterpret_cast<const float4*>(row + h * HALF + 4 * c);
}
// S^T[key][query] for this wave's 32 queries, 4 key blocks of 32; qv: this lane's (scaled) query half
template <int HALF, int DP>
__device__ __forceinline__ void exact_scores(const float* Ks, const float4 (&qv)[HALF / 4], int l32, int h,
                                             floatx16 (&s)[4]) {
  score_zero(s);
#pragma unroll
  for (int c = 0; c < HALF / 4; ++c)
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
      s[kb] = exact_mfma4(*reinterpret_cast<const float4*>(&Ks[(kb * 32 + l32) * DP + h * HALF + 4 * c]), qv[c], s[kb]);
}
// o^T[dd][query] += sum_key M[key][dd] b^T[key][query] for key block kb, b from registers; mcol = &M[4 h][l32]
// (the + 4 h of the key is folded into it)
template <int DPV>
__device__ __forceinline__ floatx16 exact_col_mfma(const float* mcol, int kb, const floatx16& b, floatx16 o) {
#pragma unroll
  for (int st = 0; st < 16; ++st)
    o = __builtin_amdgcn_mfma_f32_32x32x2f32(mcol[score_key(kb, st, 0) * DPV], b[st], o, 0, 0, 0);
  return o;
}

template <int D>
__global__ void __launch_bounds__(256, 2)
window_attn_kernel(const float* __restrict__ qkv, const int* __restrict__ order, const int* __restrict__ win,
                   int Kwin, int C, float scale, float* __restrict__ out) {
  constexpr int DP = D + 4;   // Q/K rows: conflict-free ds_read_b128 for D = 16, 24, 32
  constexpr int DPV = 40;     // V rows padded to 32 (+8): the P.V MFMA reads V^T[dd = lane][key] with no
                              // masking for dd >= D, and the two half-waves (keys 4 apart) hit disjoint banks
  __shared__ __attribute__((aligned(16))) float Qs[KMAX * DP];
  __shared__ __attribute__((aligned(16))) float Ks[KMAX * DP];
  __shared__ __attribute__((aligned(16))) float Vs[KMAX * DPV];
  __shared__ int rows[KMAX];

  const int w = blockIdx.x, head = blockIdx.y;
  const int key_start = win[2 * w], query_start = win[2 * w + 1];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const long long ld = 3ll * C;

  if (tid < KMAX) rows[tid] = tid < Kwin ? order[key_start + tid] : -1;
  exact_zero_vpad<D, DPV>(Vs, tid);
  __syncthreads();
  exact_gather<D, 0, 3, DP, DPV>(qkv, rows, ld, C, head, scale, Qs, Ks, Vs, tid);
  __syncthreads();

  constexpr int HALF = D / 2;
  float4 qv[HALF / 4];
  exact_load_half<HALF>(&Qs[(32 * wid + l32) * DP], h, qv);
  floatx16 s[4];
  exact_scores<HALF, DP>(Ks, qv, l32, h, s);
  // softmax over keys; keys >= Kwin only exist in short windows
  if (Kwin < KMAX) score_mask(s, h, Kwin);
  const float mx = score_max(s);
  const float rinv = 1.f / score_exp<false>(s, mx);
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) s[kb][r] *= rinv;

  // O^T[dd][query] = sum_key V[key][dd] P^T[key][query]
  floatx16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  const float* vcol = &Vs[4 * h * DPV + l32];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) o = exact_col_mfma<DPV>(vcol, kb, s[kb], o);

  // scatter: query 32*wid + l32 (lane column)
  const int qi = 32 * wid + l32;
  const int qpos = key_start + qi;
  if (qi < Kwin && qpos >= query_start) store_ot<D>(out + (long long)rows[qi] * C + head * D, o, h);
}


// ---- flash mode: windows of up to 2^20 keys, per-window key count -------------------------------------
// Reference pointtransformer_v3.py:121-123 (patch 1024 when enable_flash) and Pointcept's SerializedAttention
// flash branch: the padded serialized sequence is cut at cu_seqlens, so a batch of n <= K points is ONE window
// of n keys (no padding) and a longer batch has windows of K keys, its ragged last one padded with the points
// that precede it (the same (key_start, query_start) encoding as above).  Table win3[w] = (key_start,
// query_start, key_count).
//
// One 256-thread workgroup per (window, 128-query block, head): the 128 queries stay in registers as S^T
// columns while the window's keys stream through LDS in 128-key blocks with an online softmax (running max and
// sum per query, accumulator rescaled by exp(m_old - m_new)), exact fp32 MFMA (v_mfma_f32_32x32x2_f32) --
// the same S^T = K Q^T / O^T = V^T P^T register dataflow as window_attn_kernel, K/V LDS images reused per
// block.  Query blocks past the window's count or wholly before its query_start exit before any barrier.
template <int D>
__global__ void __launch_bounds__(256, 2)
window_attn_flash_kernel(const float* __restrict__ qkv, const int* __restrict__ order, const int* __restrict__ win3,
                         int qblocks, int C, float scale, float* __restrict__ out) {
  constexpr int DP = D + 4;
  constexpr int DPV = 40;
  constexpr int HALF = D / 2;
  __shared__ __attribute__((aligned(16))) float Qs[KMAX * DP];
  __shared__ __attribute__((aligned(16))) float Ks[KMAX * DP];
  __shared__ __attribute__((aligned(16))) float Vs[KMAX * DPV];
  __shared__ int qrows[KMAX];
  __shared__ int krows[KMAX];

  const int w = blockIdx.x / qblocks, qb = blockIdx.x - w * qblocks, head = blockIdx.y;
  const int key_start = win3[3 * w], query_start = win3[3 * w + 1], count = win3[3 * w + 2];
  const int q0 = qb * KMAX;  // window-relative first query of this block
  if (q0 >= count || key_start + q0 + KMAX <= query_start) return;  // workgroup-uniform, before any barrier
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const long long ld = 3ll * C;

  if (tid < KMAX) qrows[tid] = q0 + tid < count ? order[key_start + q0 + tid] : -1;
  exact_zero_vpad<D, DPV>(Vs, tid);
  __syncthreads();
  exact_gather<D, 0, 1, DP, DPV>(qkv, qrows, ld, C, head, scale, Qs, Ks, Vs, tid);
  __syncthreads();
  float4 qv[HALF / 4];
  exact_load_half<HALF>(&Qs[(32 * wid + l32) * DP], h, qv);

  float m_run = -INFINITY, l_run = 0.f;
  floatx16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  const float* vcol = &Vs[4 * h * DPV + l32];

  for (int k0 = 0; k0 < count; k0 += KMAX) {
    const int nk = min(KMAX, count - k0);
    __syncthreads();  // the previous block's K/V fragment reads are done
    if (tid < KMAX) krows[tid] = tid < nk ? order[key_start + k0 + tid] : -1;
    __syncthreads();
    exact_gather<D, 1, 2, DP, DPV>(qkv, krows, ld, C, head, scale, Qs, Ks, Vs, tid);
    __syncthreads();

    floatx16 s[4];
    exact_scores<HALF, DP>(Ks, qv, l32, h, s);
    if (nk < KMAX) score_mask(s, h, nk);
    const float m_new = fmaxf(m_run, score_max(s));  // finite: every block holds at least one key
    const float corr = __expf(m_run - m_new);
    l_run = l_run * corr + score_exp<false>(s, m_new);
    m_run = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] *= corr;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) o = exact_col_mfma<DPV>(vcol, kb, s[kb], o);
  }

  const float rinv = 1.f / l_run;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] *= rinv;
  const int qi = q0 + 32 * wid + l32;
  if (qi < count && key_start + qi >= query_start)
    store_ot<D>(out + (long long)qrows[32 * wid + l32] * C + head * D, o, h);
}


// ---- flash mode backward (training with enable_flash=True) ----------------------------------------------
// Two launches, fp32 VALU (each lane owns one query or one key; the block's other rows stream through LDS as
// wave-wide broadcasts):
//   query pass: per query i of window w (i >= query_start): m_i, l_i and O_i (online softmax over the window's
//     keys), lse_i = m_i + log l_i, delta_i = dO_i . O_i / l_i, then dQ_i = scale sum_j P_ij (dO_i.v_j - delta_i)
//     k_j (plain store: a point is a query of exactly one window); (lse, delta) saved per (point, head).
//   key pass: per key j of window w: dV_j += sum_i P_ij dO_i, dK_j += scale sum_i P_ij (dO_i.v_j - delta_i) q_i
//     over the window's own queries; float atomics into dqkv (the keys of a ragged last window are also keys of
//     the window before it: two adds onto the zero-filled buffer, order-independent).
constexpr int FB = 128;  // rows per workgroup and per LDS block

template <int D>
__global__ void __launch_bounds__(FB)
flash_bwd_query_kernel(const float* __restrict__ qkv, const int* __restrict__ order, const int* __restrict__ win3,
                       int qblocks, int C, int H, float scale, const float* __restrict__ dout,
                       float* __restrict__ dqkv, float* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) float Ks[FB * D];
  __shared__ __attribute__((aligned(16))) float Vs[FB * D];
  __shared__ int krows[FB];
  const int w = blockIdx.x / qblocks, qb = blockIdx.x - w * qblocks, head = blockIdx.y;
  const int ks = win3[3 * w], qs = win3[3 * w + 1], cnt = win3[3 * w + 2];
  const int q0 = qb * FB;
  if (q0 >= cnt || ks + q0 + FB <= qs) return;  // workgroup-uniform, before any barrier
  const int t = threadIdx.x, qi = q0 + t;
  const bool valid = qi < cnt && ks + qi >= qs;
  const int row = valid ? order[ks + qi] : 0;
  const long long ld = 3ll * C;
  float q[D], g[D], o[D], dq[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    q[c] = valid ? qkv[(long long)row * ld + head * D + c] * scale : 0.f;
    g[c] = valid ? dout[(long long)row * C + head * D + c] : 0.f;
    o[c] = 0.f;
    dq[c] = 0.f;
  }
  auto stage = [&](int k0, int nk) {
    __syncthreads();
    krows[t] = t < nk ? order[ks + k0 + t] : -1;
    __syncthreads();
    for (int e = t; e < FB * D / 4; e += FB) {
      const int r = e / (D / 4), c4 = e - r * (D / 4);
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (krows[r] >= 0) {
        const float* src = qkv + (long long)krows[r] * ld + head * D + 4 * c4;
        kv = *reinterpret_cast<const float4*>(src + C);
        vv = *reinterpret_cast<const float4*>(src + 2 * C);
      }
      *reinterpret_cast<float4*>(&Ks[r * D + 4 * c4]) = kv;
      *reinterpret_cast<float4*>(&Vs[r * D + 4 * c4]) = vv;
    }
    __syncthreads();
  };
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < cnt; k0 += FB) {
    const int nk = min(FB, cnt - k0);
    stage(k0, nk);
    for (int j = 0; j < nk; ++j) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) s = fmaf(q[c], Ks[j * D + c], s);
      const float mn = fmaxf(m, s);
      const float corr = expf(m - mn), p = expf(s - mn);
      l = l * corr + p;
#pragma unroll
      for (int c = 0; c < D; ++c) o[c] = fmaf(p, Vs[j * D + c], o[c] * corr);
      m = mn;
    }
  }
  float delta = 0.f;
#pragma unroll
  for (int c = 0; c < D; ++c) delta = fmaf(g[c], o[c], delta);
  delta /= l;
  const float lse = m + logf(l);
  for (int k0 = 0; k0 < cnt; k0 += FB) {
    const int nk = min(FB, cnt - k0);
    stage(k0, nk);
    for (int j = 0; j < nk; ++j) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        s = fmaf(q[c], Ks[j * D + c], s);
        dp = fmaf(g[c], Vs[j * D + c], dp);
      }
      const float ds = expf(s - lse) * (dp - delta);
#pragma unroll
      for (int c = 0; c < D; ++c) dq[c] = fmaf(ds, Ks[j * D + c], dq[c]);
    }
  }
  if (valid) {
#pragma unroll
    for (int c = 0; c < D; ++c) dqkv[(long long)row * ld + head * D + c] = dq[c] * scale;
    stats[((long long)row * H + head) * 2] = lse;
    stats[((long long)row * H + head) * 2 + 1] = delta;
  }
}

template <int D>
__global__ void __launch_bounds__(FB)
flash_bwd_key_kernel(const float* __restrict__ qkv, const int* __restrict__ order, const int* __restrict__ win3,
                     int kblocks, int C, int H, float scale, const float* __restrict__ dout,
                     float* __restrict__ dqkv, const float* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) float Qs[FB * D];
  __shared__ __attribute__((aligned(16))) float Gs[FB * D];
  __shared__ float Ls[FB], Ds[FB];
  __shared__ int qrows[FB];
  const int w = blockIdx.x / kblocks, kb = blockIdx.x - w * kblocks, head = blockIdx.y;
  const int ks = win3[3 * w], qs = win3[3 * w + 1], cnt = win3[3 * w + 2];
  const int k0 = kb * FB;
  if (k0 >= cnt) return;  // workgroup-uniform
  const int t = threadIdx.x, kj = k0 + t;
  const bool valid = kj < cnt;
  const int row = valid ? order[ks + kj] : 0;
  const long long ld = 3ll * C;
  float k[D], v[D], dk[D], dv[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    k[c] = valid ? qkv[(long long)row * ld + C + head * D + c] : 0.f;
    v[c] = valid ? qkv[(long long)row * ld + 2 * C + head * D + c] : 0.f;
    dk[c] = 0.f;
    dv[c] = 0.f;
  }
  for (int i0 = qs - ks; i0 < cnt; i0 += FB) {  // the window's own queries
    const int ni = min(FB, cnt - i0);
    __syncthreads();
    qrows[t] = t < ni ? order[ks + i0 + t] : -1;
    __syncthreads();
    for (int e = t; e < FB * D / 4; e += FB) {
      const int r = e / (D / 4), c4 = e - r * (D / 4);
      float4 qv = make_float4(0.f, 0.f, 0.f, 0.f), gv = qv;
      if (qrows[r] >= 0) {
        qv = *reinterpret_cast<const float4*>(qkv + (long long)qrows[r] * ld + head * D + 4 * c4);
        qv.x *= scale; qv.y *= scale; qv.z *= scale; qv.w *= scale;
        gv = *reinterpret_cast<const float4*>(dout + (long long)qrows[r] * C + head * D + 4 * c4);
      }
      *reinterpret_cast<float4*>(&Qs[r * D + 4 * c4]) = qv;
      *reinterpret_cast<float4*>(&Gs[r * D + 4 * c4]) = gv;
    }
    Ls[t] = t < ni ? stats[((long long)qrows[t] * H + head) * 2] : INFINITY;
    Ds[t] = t < ni ? stats[((long long)qrows[t] * H + head) * 2 + 1] : 0.f;
    __syncthreads();
    for (int i = 0; i < ni; ++i) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        s = fmaf(Qs[i * D + c], k[c], s);
        dp = fmaf(Gs[i * D + c], v[c], dp);
      }
      const float p = expf(s - Ls[i]);
      const float ds = p * (dp - Ds[i]);
#pragma unroll
      for (int c = 0; c < D; ++c) {
        dv[c] = fmaf(p, Gs[i * D + c], dv[c]);
        dk[c] = fmaf(ds, Qs[i * D + c], dk[c]);
      }
    }
  }
  if (valid) {
    float* dst = dqkv + (long long)row * ld + head * D;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      atomicAdd(dst + C + c, dk[c]);
      atomicAdd(dst + 2 * C + c, dv[c]);
    }
  }
}

// ---- split-bf16 forward (default) ---------------------------------------------------------------------
// The same dataflow on v_mfma_f32_32x32x16_bf16: q, k, v and p enter as three bf16 terms each
// (sfx::split3) and every 32x32x16 block is the six leading term products accumulated in fp32 -- fp32
// accuracy at 6 x 32 MFMA cycles per 16-deep step instead of 8 x 64 on v_mfma_f32_32x32x2_f32.
//   S^T = K Q^T: A = K [key][dd], B = Q^T, KD = 16 (D = 16) or 32 (D = 24, 32; columns >= D zero).
//   O^T = V^T P^T: B = P^T straight from the softmax registers -- registers 8s..8s+7 of key block kb are
//   the 16-key step s (element j <-> key 32kb + 16s + 8(j>>2) + 4h + (j&3)); A = V^T, staged transposed
//   with the keys of every 16-key group permuted to that order so a lane's 8 keys are one 16-byte read.
// LDS: K term image [3][128][KD] (KD = 16: 48-byte rows; KD = 32: 64-byte rows, 16-byte chunks XOR-
// swizzled by row >> 2), V^T [3][D][136] (272-byte rows; lanes dd >= D feed zero fragments); all fragment
// reads are conflict-free.  Q never touches LDS: each lane gathers and splits its own query's 8-wide
// slices.  31-50 KB per workgroup: 3-4 workgroups per CU to hide the row gathers.
//
// F16 (when the caller passes an amax slot bounding |qkv|): fp16x2 terms instead -- q, k, v scaled by a
// power of two that puts the bound in [2^14, 2^15), the unnormalised probabilities (0, 1] by 2^14, two fp16
// terms each (sfx::split2h), three term products per block on v_mfma_f32_32x32x16_f16; S and O are unscaled
// in registers.  Same fp32-level accuracy, half the MFMAs and two-thirds of the LDS images.
// ONE (sfx_set_precision(1), the reference's autocast class): F16 the leading product h*h only, bf16x3 the three
// leading term products (16-bit significands)
//
// The steps window_attn_split_kernel and window_attn_split_flash_kernel share (256 threads; rows[]: the points of
// the 128 keys, -1 past the count); layouts, fragments and term products are attn_common.h's.

// this lane's query slices (B operand of S^T = K Q^T): dd = 16 ks + 8h + j, zero past D; scale * log2(e) folded in
template <int D, bool F16, int NKS>
__device__ __forceinline__ void fwd_query_frags(const float* __restrict__ qkv, int src, long long ld, int head, int h,
                                                float scale, float sq, frag_t<F16> (&qf)[NKS][nterms(F16)]) {
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    float4 a, b;
    load8<D>(qkv + (long long)(src < 0 ? 0 : src) * ld + head * D, 16 * ks + 8 * h, src >= 0, a, b);
    q_frag<F16>(a, b, scale * 1.4426950408889634f, sq, qf[ks]);
  }
}
// gather + split, one matrix at a time (wave-uniform paths): k rows as KMAX x D/4 float4 into the K term image; v as
// key pairs x D/4 float4 so the transposed V^T writes are whole dwords (keys 2m, 2m+1 are adjacent in the permuted
// order)
template <int D, int KD, bool F16>
__device__ __forceinline__ void fwd_stage_kv(const float* __restrict__ qkv, const int* rows, long long ld, int C,
                                             int head, float sq, char* Ks, unsigned short* Vt, int tid) {
  constexpr int CH = D / 4;
  for (int e = tid; e < KMAX * CH; e += 256) {
    const int row = e / CH, ch = e - row * CH;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int src = rows[row];
    if (src >= 0) v = *reinterpret_cast<const float4*>(qkv + (long long)src * ld + C + head * D + 4 * ch);
    stage_row<KD, F16>(Ks, row, ch, v, sq);
  }
  for (int e = tid; e < (KMAX / 2) * CH; e += 256) {
    const int kp = e / CH, ch = e - kp * CH;
    const int row = 2 * kp;
    const int s0 = rows[row], s1 = rows[row + 1];
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    if (s0 >= 0) v0 = *reinterpret_cast<const float4*>(qkv + (long long)s0 * ld + 2 * C + head * D + 4 * ch);
    if (s1 >= 0) v1 = *reinterpret_cast<const float4*>(qkv + (long long)s1 * ld + 2 * C + head * D + 4 * ch);
    stage_pair<D, F16>(nullptr, Vt, row, ch, v0, v1, sq);
  }
}
// S^T[key][query] for this wave's 32 queries, 4 key blocks of 32, unscaled (F16: S was formed from sq-scaled q and k)
template <int KD, bool F16, bool ONE, int NKS>
__device__ __forceinline__ void fwd_scores(const char* Ks, const frag_t<F16> (&qf)[NKS][nterms(F16)], int l32, int h,
                                           float iq, floatx16 (&s)[4]) {
  score_zero(s);
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      frag_t<F16> kf[nterms(F16)];
      row_frag<KD, F16>(Ks, kb * 32 + l32, 2 * ks + h, kf);
      s[kb] = mfma_terms<F16, ONE>(kf, qf[ks], s[kb]);
    }
  }
  if constexpr (F16) {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = s[kb][r] * iq * iq;
  }
}

template <int D, bool F16, bool ONE = false>
__global__ void __launch_bounds__(256, D == 16 ? SFX_ATTN_OCC16 : 3)
window_attn_split_kernel(const float* __restrict__ qkv, const int* __restrict__ order, const int* __restrict__ win,
                         int Kwin, int C, float scale, float* __restrict__ out,
                         const unsigned long long* __restrict__ qkv_amax, unsigned qkv_tag, int nwin) {
  constexpr int NT = nterms(F16);           // terms per operand
  constexpr int KD = D == 16 ? 16 : 32;
  constexpr int NKS = KD / 16;
  constexpr int QK_BYTES = NT * KMAX * row_bytes(KD);
  constexpr int V_BYTES = NT * D * VST * 2;
  // operand scales (F16): qkv by sq, probabilities by 2^14
  float sq = 1.f, iq = 1.f;
  if constexpr (F16) sq = sfx::pow2_scale(sfx::read_amax(qkv_amax, qkv_tag), iq);
  __shared__ __attribute__((aligned(16))) char lds[QK_BYTES + V_BYTES];
  __shared__ int rows[KMAX];
  char* Ks = lds;
  unsigned short* Vt = reinterpret_cast<unsigned short*>(lds + QK_BYTES);

  const int heads = C / D;
  const int L = xcd_logical_id();
  if (L >= nwin * heads) return;
  const int w = L / heads, head = L - w * heads;
  const int key_start = win[2 * w], query_start = win[2 * w + 1];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const long long ld = 3ll * C;

  if (tid < KMAX) rows[tid] = tid < Kwin ? order[key_start + tid] : -1;
  zero_row_pad<D, KD>(Ks, NT * KMAX, tid);
  __syncthreads();
  frag_t<F16> qf[NKS][NT];
  fwd_query_frags<D, F16, NKS>(qkv, rows[32 * wid + l32], ld, head, h, scale, sq, qf);
  fwd_stage_kv<D, KD, F16>(qkv, rows, ld, C, head, sq, Ks, Vt, tid);
  __syncthreads();

  floatx16 s[4];
  fwd_scores<KD, F16, ONE, NKS>(Ks, qf, l32, h, iq, s);
  // softmax over keys; keys >= Kwin only exist in short windows
  if (Kwin < KMAX) score_mask(s, h, Kwin);
  const float mx = score_max(s);
  const float rinv = 1.f / score_exp<true>(s, mx);

  floatx16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  o = pv_terms<D, F16, ONE>(s, Vt, l32, h, o);

  const float oscale = F16 ? rinv * iq * (1.f / 16384.f) : rinv;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] *= oscale;
  // scatter: query 32*wid + l32 (lane column)
  const int qi = 32 * wid + l32;
  const int qpos = key_start + qi;
  if (qi < Kwin && qpos >= query_start) store_ot<D>(out + (long long)rows[qi] * C + head * D, o, h);
}


// Flash mode on split MFMA terms (default for sfx_window_attention_varlen): window_attn_split_kernel's
// dataflow (per-lane query fragments, K / V^T term images, S^T = K Q^T and O^T = V^T P^T on fp16x2 or bf16x3
// terms) with the window's keys streamed in 128-key blocks and an online softmax: the running maximum
// rescales the accumulator by exp2(m_old - m_new), so every block's probabilities stay in (0, 1] (the 2^14
// fp16 scale of P holds).  One workgroup per (window, 128-query block, head), XCD-aware numbering.
template <int D, bool F16>
__global__ void __launch_bounds__(256, D == 16 ? 4 : 3)
window_attn_split_flash_kernel(const float* __restrict__ qkv, const int* __restrict__ order,
                               const int* __restrict__ win3, int qblocks, int C, float scale, float* __restrict__ out,
                               const unsigned long long* __restrict__ qkv_amax, unsigned qkv_tag, int nwin) {
  constexpr int NT = nterms(F16);           // terms per operand
  constexpr int KD = D == 16 ? 16 : 32;
  constexpr int NKS = KD / 16;
  constexpr int QK_BYTES = NT * KMAX * row_bytes(KD);
  constexpr int V_BYTES = NT * D * VST * 2;
  // operand scales (F16): qkv by sq, probabilities by 2^14
  float sq = 1.f, iq = 1.f;
  if constexpr (F16) sq = sfx::pow2_scale(sfx::read_amax(qkv_amax, qkv_tag), iq);
  __shared__ __attribute__((aligned(16))) char lds[QK_BYTES + V_BYTES];
  __shared__ int rows[KMAX];   // keys of the current block
  __shared__ int qrows[KMAX];  // this workgroup's queries
  char* Ks = lds;
  unsigned short* Vt = reinterpret_cast<unsigned short*>(lds + QK_BYTES);

  const int heads = C / D;
  const int L = xcd_logical_id();
  if (L >= nwin * qblocks * heads) return;
  const int wq = L / heads, head = L - wq * heads;
  const int w = wq / qblocks, qb = wq - w * qblocks;
  const int key_start = win3[3 * w], query_start = win3[3 * w + 1], count = win3[3 * w + 2];
  const int q0 = qb * KMAX;
  if (q0 >= count || key_start + q0 + KMAX <= query_start) return;  // workgroup-uniform, before any barrier
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const long long ld = 3ll * C;

  if (tid < KMAX) qrows[tid] = q0 + tid < count ? order[key_start + q0 + tid] : -1;
  zero_row_pad<D, KD>(Ks, NT * KMAX, tid);
  __syncthreads();
  frag_t<F16> qf[NKS][NT];
  fwd_query_frags<D, F16, NKS>(qkv, qrows[32 * wid + l32], ld, head, h, scale, sq, qf);
  float m_run = -INFINITY, l_run = 0.f;
  floatx16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;

  for (int k0 = 0; k0 < count; k0 += KMAX) {
    const int nk = min(KMAX, count - k0);
    __syncthreads();  // the previous block's fragment reads are done
    if (tid < KMAX) rows[tid] = tid < nk ? order[key_start + k0 + tid] : -1;
    __syncthreads();
    // The K-row and V^T staging of fwd_stage_kv, written out: through stage_row / stage_pair (or any smaller helper
    // for the offset or the key-pair permutation) the d = 16 instantiations, compiled at the 128-VGPR limit, spill
    // 12 / 8 B more per lane than the parent and run 4 % / 1 % slower
    constexpr int CH = D / 4;
    for (int e = tid; e < KMAX * CH; e += 256) {
      const int row = e / CH, ch = e - row * CH;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int src = rows[row];
      if (src >= 0) v = *reinterpret_cast<const float4*>(qkv + (long long)src * ld + C + head * D + 4 * ch);
      uint2 t[NT];
      split<F16>(v, sq, t);
      const int o = row_off<KD>(row, ch >> 1) + ((ch & 1) << 3);
#pragma unroll
      for (int q = 0; q < NT; ++q) *reinterpret_cast<uint2*>(Ks + q * KMAX * row_bytes(KD) + o) = t[q];
    }
    for (int e = tid; e < (KMAX / 2) * CH; e += 256) {
      const int kp = e / CH, ch = e - kp * CH;
      const int row = 2 * kp;
      const int s0 = rows[row], s1 = rows[row + 1];
      float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
      if (s0 >= 0) v0 = *reinterpret_cast<const float4*>(qkv + (long long)s0 * ld + 2 * C + head * D + 4 * ch);
      if (s1 >= 0) v1 = *reinterpret_cast<const float4*>(qkv + (long long)s1 * ld + 2 * C + head * D + 4 * ch);
      uint2 t0[NT], t1[NT];
      split<F16>(v0, sq, t0);
      split<F16>(v1, sq, t1);
      const int kk = row & 15;  // even: keys row, row + 1 land on adjacent positions (as stage_pair)
      const int pos = (row & ~15) + 8 * ((kk >> 2) & 1) + (((kk >> 3) << 2) | (kk & 3));
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        unsigned* vt = reinterpret_cast<unsigned*>(Vt + (q * D + 4 * ch) * VST + (pos ^ (8 * vt_swz(4 * ch))));
        vt[0] = (t0[q].x & 0xffffu) | (t1[q].x << 16);
        vt[VST / 2] = (t0[q].x >> 16) | (t1[q].x & 0xffff0000u);
        vt[VST] = (t0[q].y & 0xffffu) | (t1[q].y << 16);
        vt[3 * VST / 2] = (t0[q].y >> 16) | (t1[q].y & 0xffff0000u);
      }
    }
    __syncthreads();

    floatx16 s[4];
    fwd_scores<KD, F16, false, NKS>(Ks, qf, l32, h, iq, s);
    // online softmax over this key block; keys >= nk are padding
    if (nk < KMAX) score_mask(s, h, nk);
    const float mx = fmaxf(score_max(s), m_run);  // finite: every block holds at least one key
    const float corr = __builtin_amdgcn_exp2f(m_run - mx);
    l_run = l_run * corr + score_exp<true>(s, mx);
    m_run = mx;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] *= corr;
    o = pv_terms<D, F16, false>(s, Vt, l32, h, o);
  }  // key blocks

  const float rinv = 1.f / l_run;
  const float oscale = F16 ? rinv * iq * (1.f / 16384.f) : rinv;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] *= oscale;
  // scatter: query q0 + 32*wid + l32 (lane column)
  const int qi = q0 + 32 * wid + l32;
  if (qi < count && key_start + qi >= query_start)
    store_ot<D>(out + (long long)qrows[32 * wid + l32] * C + head * D, o, h);
}



// ---- backward (training, configs C/D) ---------------------------------------------------------------
// Autograd of the non-flash attention math of visualize.py:140-179 for one (window, head):
//   dV = P^T dO ; dP = dO V^T ; dS = P * (dP - rowsum(dO * O)) ; dQ = scale * dS K ; dK = dS^T (scale*Q)
// Phase A (query on the lane column, S^T = K Q^T as in the forward): softmax statistics, O, Delta, dS^T
// and dQ -- every query row belongs to exactly one window, so dQ is a plain store.  Phase B (key on the
// lane column, S = Q K^T recomputed): dV and dK summed over the window's queries; a key can sit in two
// windows (the ragged last window re-uses the K - n%K points before it), so they are accumulated with
// float atomics into dqkv, which the caller zero-fills.  Padding queries (positions < query_start of the
// last window) carry dO = 0 and contribute nothing, exactly as their discarded outputs in the reference.
template <int D>
__global__ void __launch_bounds__(256, 2)
window_attn_bwd_kernel(const float* __restrict__ qkv, const int* __restrict__ order, const int* __restrict__ win,
                       int Kwin, int C, float scale, const float* __restrict__ dout, float* __restrict__ dqkv) {
  // One row stride for all four operands: 36 floats = 32 (+4) columns, zero beyond D.  ds_read_b128 row
  // reads (S, dP) are conflict-free at stride 36 and the MFMA A-operand column reads (V^T, K^T, dO^T, Q^T
  // with dd = lane) need no masking for dd >= D.  4 x 18 KB LDS -> 2 workgroups per CU.
  constexpr int DP = 36;
  constexpr int HALF = D / 2;
  __shared__ __attribute__((aligned(16))) float Qs[KMAX * DP];
  __shared__ __attribute__((aligned(16))) float Ks[KMAX * DP];
  __shared__ __attribute__((aligned(16))) float Vs[KMAX * DP];
  __shared__ __attribute__((aligned(16))) float dOs[KMAX * DP];
  __shared__ float st_max[KMAX], st_rinv[KMAX], st_delta[KMAX];
  __shared__ int rows[KMAX];

  const int w = blockIdx.x, head = blockIdx.y;
  const int key_start = win[2 * w], query_start = win[2 * w + 1];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const long long ld = 3ll * C;

  if (tid < KMAX) rows[tid] = tid < Kwin ? order[key_start + tid] : -1;
  __syncthreads();
  // gather q/k/v/dO rows of this head (zero rows past Kwin, zero dO for padding queries, zero columns >= D)
  constexpr int CH = 8;  // float4 per padded row (32 columns)
  for (int e = tid; e < KMAX * 4 * CH; e += 256) {
    const int row = e / (4 * CH);
    const int rem = e - row * 4 * CH;
    const int mat = rem / CH, ch = rem - mat * CH;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int src = rows[row];
    if (4 * ch < D && src >= 0) {
      if (mat < 3)
        v = *reinterpret_cast<const float4*>(qkv + (long long)src * ld + mat * C + head * D + 4 * ch);
      else if (key_start + row >= query_start)
        v = *reinterpret_cast<const float4*>(dout + (long long)src * C + head * D + 4 * ch);
    }
    float* dst = mat == 0 ? Qs : mat == 1 ? Ks : mat == 2 ? Vs : dOs;
    if (mat == 0) {
      v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
    }
    *reinterpret_cast<float4*>(&dst[row * DP + 4 * ch]) = v;
  }
  __syncthreads();

  // ---------------- phase A: this wave's 32 queries on the lane columns ----------------
  const int qi = 32 * wid + l32;
  floatx16 s[4];
  {
    float4 qv[HALF / 4];
    exact_load_half<HALF>(&Qs[qi * DP], h, qv);
    exact_scores<HALF, DP>(Ks, qv, l32, h, s);
  }
  if (Kwin < KMAX) score_mask(s, h, Kwin);
  const float mx = score_max(s);
  const float rinv = 1.f / score_exp<false>(s, mx);
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) s[kb][r] *= rinv;  // P^T (same normalisation as the forward)
  // O^T[dd][q] (forward recompute) -> Delta_q = sum_dd O[q][dd] dO[q][dd]
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* vcol = &Vs[4 * h * DP + l32];
  const float* kcol = &Ks[4 * h * DP + l32];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) acc = exact_col_mfma<DP>(vcol, kb, s[kb], acc);
  float delta = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) delta += acc[r] * dOs[qi * DP + score_key(0, r, h)];
  delta += __shfl_xor(delta, 32, 64);
  // per key block: dP^T = V dO^T, dS^T = P^T (dP^T - Delta), dQ^T += K^T dS^T
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;  // now dQ^T
  const float* grow = &dOs[qi * DP + h * HALF];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    floatx16 dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
    for (int c = 0; c < HALF / 4; ++c)
      dp = exact_mfma4(*reinterpret_cast<const float4*>(&Vs[(kb * 32 + l32) * DP + h * HALF + 4 * c]),
                       *reinterpret_cast<const float4*>(grow + 4 * c), dp);
#pragma unroll
    for (int st = 0; st < 16; ++st) {
      const float ds = s[kb][st] * (dp[st] - delta);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kcol[score_key(kb, st, 0) * DP], ds, acc, 0, 0, 0);
    }
  }
  const int qpos = key_start + qi;
  if (qi < Kwin && qpos >= query_start) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] *= scale;
    store_ot<D>(dqkv + (long long)rows[qi] * ld + head * D, acc, h);
  }
  if (h == 0) {
    st_max[qi] = mx;
    st_rinv[qi] = rinv;
    st_delta[qi] = delta;
  }
  __syncthreads();

  // ---------------- phase B: this wave's 32 keys on the lane columns ----------------
  const int kk = 32 * wid + l32;
  floatx16 dk, dv;
#pragma unroll
  for (int r = 0; r < 16; ++r) dk[r] = dv[r] = 0.f;
  const bool key_ok = kk < Kwin;
  const float* krow = &Ks[kk * DP + h * HALF];
  const float* vrow = &Vs[kk * DP + h * HALF];
  const float* gcol = &dOs[4 * h * DP + l32];
  const float* qcol = &Qs[4 * h * DP + l32];
#pragma unroll 1
  for (int qb = 0; qb < 4; ++qb) {
    floatx16 sb, pb;
#pragma unroll
    for (int r = 0; r < 16; ++r) sb[r] = pb[r] = 0.f;
    const float* qrow = &Qs[(qb * 32 + l32) * DP + h * HALF];
    const float* grw = &dOs[(qb * 32 + l32) * DP + h * HALF];
#pragma unroll
    for (int c = 0; c < HALF / 4; ++c) {
      const float4 qv = *reinterpret_cast<const float4*>(qrow + 4 * c);
      const float4 gv = *reinterpret_cast<const float4*>(grw + 4 * c);
      const float4 kv = *reinterpret_cast<const float4*>(krow + 4 * c);
      const float4 vv = *reinterpret_cast<const float4*>(vrow + 4 * c);
      sb = exact_mfma4(qv, kv, sb);
      pb = exact_mfma4(gv, vv, pb);
    }
    // sb[r] = S[q][kk], pb[r] = dP[q][kk] for q = qb*32 + (r&3) + 8(r>>2) + 4h
#pragma unroll
    for (int st = 0; st < 16; ++st) {
      const int q = score_key(qb, st, h);
      const float P = key_ok ? __expf(sb[st] - st_max[q]) * st_rinv[q] : 0.f;
      const float dS = P * (pb[st] - st_delta[q]);
      const int qo = score_key(qb, st, 0) * DP;  // + 4h folded into gcol / qcol
      dv = __builtin_amdgcn_mfma_f32_32x32x2f32(gcol[qo], P, dv, 0, 0, 0);
      dk = __builtin_amdgcn_mfma_f32_32x32x2f32(qcol[qo], dS, dk, 0, 0, 0);
    }
  }
  // dK / dV leave through LDS so that each store instruction writes whole row segments (a lane-per-key
  // layout would touch 64 rows per instruction).  Keys in the overlap of the ragged last window with its
  // predecessor receive contributions from both windows and are added atomically; every other key is owned
  // by this window alone and stored plainly.
  __syncthreads();  // all waves done reading Q/K/V/dO
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int dd = score_key(0, r, h);
    Qs[kk * DP + dd] = dk[r];
    Vs[kk * DP + dd] = dv[r];
  }
  __syncthreads();
  const int next_ks = (w + 1 < (int)gridDim.x) ? win[2 * (w + 1)] : 0x7fffffff;
  constexpr int DC = D / 4;
  for (int e = tid; e < Kwin * 2 * DC; e += 256) {
    const int row = e / (2 * DC);
    const int rem = e - row * 2 * DC;
    const int mat = rem / DC, ch = rem - mat * DC;
    const float4 v = *reinterpret_cast<const float4*>(&(mat == 0 ? Qs : Vs)[row * DP + 4 * ch]);
    float* dst = dqkv + (long long)rows[row] * ld + (mat + 1) * C + head * D + 4 * ch;
    const int pos = key_start + row;
    if (pos < query_start || pos >= next_ks) {
      atomicAdd(dst + 0, v.x);
      atomicAdd(dst + 1, v.y);
      atomicAdd(dst + 2, v.z);
      atomicAdd(dst + 3, v.w);
    } else {
      *reinterpret_cast<float4*>(dst) = v;
    }
  }
}

// ---- fp16x2 backward (default) -----------------------------------------------------------------------------
// The same autograd as window_attn_bwd_kernel in two passes over the (window, head) items, on
// v_mfma_f32_32x32x16_f16 with every operand as two fp16 terms (sfx::split2h) of a power-of-two-scaled value and
// three term products per block (the forward's F16 scheme):
//   query pass (lanes = this wave's 32 queries):  S^T = K Q^T -> softmax max and 1/sum ; Delta_q = dO_q . O_q from
//     the forward output (= rowsum(P o dP)) ; per 32-key block dP^T = V dO^T, dS^T = P^T (dP^T - Delta) and
//     dQ^T += K^T dS^T with dS^T straight from registers as the B operand (as P^T in the forward) ; dQ stored plainly
//     (each query belongs to one window) and (max, 1/sum, Delta) written per (query, head) for the key pass;
//   key pass (lanes = this wave's 32 keys): per 32-query block S = Q K^T and dP = dO V^T recomputed, P from the
//     stored statistics, dS = P (dP - Delta) ; dV^T += dO^T P and dK^T += Q^T dS from registers.
// Scales: q, k, v and dO of an item by powers of two putting the item's largest magnitude in [2^14, 2^15); P (<= 1)
// by 2^14; dS by one power of two per (lane column, 32-row block), its block product unscaled before it joins the
// accumulator.  Every MFMA is a 16-deep step of 3 products, against 8 steps of v_mfma_f32_32x32x2_f32 per 16 in the
// exact kernel; recomputing S and dP in the key pass is what keeps both passes' contractions on the register axis.
// LDS per item: row images [2 terms][128][KD] (as the forward's K image) and transposed images [2][D][136] with the
// keys (queries) of each 16-group in the B-operand register order (as the forward's V^T).
__device__ __forceinline__ float amax4(float4 v) {
  return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
}
// workgroup-wide max of 4 values (256 threads, one barrier)
__device__ __forceinline__ float4 bwd_wg_max4(float4 m, float4* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    m.x = fmaxf(m.x, __shfl_xor(m.x, o, 64));
    m.y = fmaxf(m.y, __shfl_xor(m.y, o, 64));
    m.z = fmaxf(m.z, __shfl_xor(m.z, o, 64));
    m.w = fmaxf(m.w, __shfl_xor(m.w, o, 64));
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  float4 r = red[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const float4 t = red[i];
    r = make_float4(fmaxf(r.x, t.x), fmaxf(r.y, t.y), fmaxf(r.z, t.z), fmaxf(r.w, t.w));
  }
  return r;
}

template <int D, bool ONE = false>
__global__ void __launch_bounds__(256, 3)
window_attn_bwd_q_kernel(const float* __restrict__ qkv, const int* __restrict__ order, const int* __restrict__ win,
                         int Kwin, int C, float scale, const float* __restrict__ attn_out,
                         const float* __restrict__ dout, float* __restrict__ dqkv, float4* __restrict__ stats,
                         int nwin) {
  constexpr int KD = D == 16 ? 16 : 32, NKS = KD / 16, QROW = row_bytes(KD);
  constexpr int RB = 2 * KMAX * QROW, TB = 2 * D * VST * 2;
  constexpr int CH = D / 4, NE = (KMAX / 2) * CH, NIT = (NE + 255) / 256;
  __shared__ __attribute__((aligned(16))) char lds[2 * RB + TB];
  __shared__ int rows[KMAX];
  __shared__ float4 red[4];
  char* Kr = lds;
  char* Vr = lds + RB;
  unsigned short* Kt = reinterpret_cast<unsigned short*>(lds + 2 * RB);

  const int heads = C / D;
  const int L = xcd_logical_id();
  if (L >= nwin * heads) return;
  const int w = L / heads, head = L - w * heads;
  const int key_start = win[2 * w], query_start = win[2 * w + 1];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const long long ld = 3ll * C;

  if (tid < KMAX) rows[tid] = tid < Kwin ? order[key_start + tid] : -1;
  if (D < KD)  // zero K / V columns D..KD-1
    for (int rr = tid; rr < 4 * KMAX; rr += 256)
      *reinterpret_cast<uint4*>(lds + (rr >> 8) * RB + ((rr >> 7) & 1) * KMAX * QROW + row_off<KD>(rr & 127, D / 8)) =
          make_uint4(0, 0, 0, 0);
  __syncthreads();
  // dqkv is not zero-filled by the caller: the key pass stores every key's dK / dV plainly except the keys a ragged
  // last window shares with its predecessor (positions key_start .. query_start - 1), which both windows add
  // atomically -- this window zeroes this head's slice of them here, a launch ahead of every key-pass add
  for (int e = tid; e < (query_start - key_start) * 2 * (D / 4); e += 256) {
    const int row = e / (2 * (D / 4)), rem = e - row * 2 * (D / 4);
    const int mat = rem / (D / 4), ch = rem - mat * (D / 4);
    *reinterpret_cast<float4*>(dqkv + (long long)rows[row] * ld + (mat + 1) * C + head * D + 4 * ch) =
        make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // this lane's query: q and dO slices dd = 16 ks + 8h .. +7 (B operands of S^T and dP^T) and Delta = dO . O
  const int qi = 32 * wid + l32;
  const int qsrc = rows[qi];
  const bool qown = qsrc >= 0 && key_start + qi >= query_start;
  float4 qa[NKS][2], ga[NKS][2];
  float delta = 0.f;
  float4 mx4 = make_float4(0.f, 0.f, 0.f, 0.f);  // (q, k, v, dO)
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int d0 = 16 * ks + 8 * h;
    load8<D>(qkv + (long long)(qsrc < 0 ? 0 : qsrc) * ld + head * D, d0, qsrc >= 0, qa[ks][0], qa[ks][1]);
    load8<D>(dout + (long long)(qsrc < 0 ? 0 : qsrc) * C + head * D, d0, qown, ga[ks][0], ga[ks][1]);
    float4 oa, ob;
    load8<D>(attn_out + (long long)(qsrc < 0 ? 0 : qsrc) * C + head * D, d0, qown, oa, ob);
    delta += ga[ks][0].x * oa.x + ga[ks][0].y * oa.y + ga[ks][0].z * oa.z + ga[ks][0].w * oa.w +
             ga[ks][1].x * ob.x + ga[ks][1].y * ob.y + ga[ks][1].z * ob.z + ga[ks][1].w * ob.w;
    mx4.x = fmaxf(mx4.x, fmaxf(amax4(qa[ks][0]), amax4(qa[ks][1])));
    mx4.w = fmaxf(mx4.w, fmaxf(amax4(ga[ks][0]), amax4(ga[ks][1])));
  }
  delta += __shfl_xor(delta, 32, 64);
  // this thread's K / V elements: row pairs x float4 column chunks
  float4 k0[NIT], k1[NIT], v0[NIT], v1[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int e = tid + 256 * it;
    k0[it] = k1[it] = v0[it] = v1[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < NE) {
      const int kp = e / CH, ch = e - kp * CH;
      const int s0 = rows[2 * kp], s1 = rows[2 * kp + 1];
      if (s0 >= 0) {
        k0[it] = *reinterpret_cast<const float4*>(qkv + (long long)s0 * ld + C + head * D + 4 * ch);
        v0[it] = *reinterpret_cast<const float4*>(qkv + (long long)s0 * ld + 2 * C + head * D + 4 * ch);
      }
      if (s1 >= 0) {
        k1[it] = *reinterpret_cast<const float4*>(qkv + (long long)s1 * ld + C + head * D + 4 * ch);
        v1[it] = *reinterpret_cast<const float4*>(qkv + (long long)s1 * ld + 2 * C + head * D + 4 * ch);
      }
    }
    mx4.y = fmaxf(mx4.y, fmaxf(amax4(k0[it]), amax4(k1[it])));
    mx4.z = fmaxf(mx4.z, fmaxf(amax4(v0[it]), amax4(v1[it])));
  }
  mx4 = bwd_wg_max4(mx4, red);
  float iQ, iK, iV, iG;
  const float sQ = sfx::pow2_scale(mx4.x, iQ), sK = sfx::pow2_scale(mx4.y, iK), sV = sfx::pow2_scale(mx4.z, iV),
              sG = sfx::pow2_scale(mx4.w, iG);
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int e = tid + 256 * it;
    if (e < NE) {
      const int kp = e / CH, ch = e - kp * CH;
      stage_pair<D, true, KD>(Kr, Kt, 2 * kp, ch, k0[it], k1[it], sK);
      stage_row<KD, true>(Vr, 2 * kp, ch, v0[it], sV);
      stage_row<KD, true>(Vr, 2 * kp + 1, ch, v1[it], sV);
    }
  }
  f16x8 qf[NKS][2], gf[NKS][2];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    frag<true>(qa[ks][0], qa[ks][1], sQ, qf[ks]);
    frag<true>(ga[ks][0], ga[ks][1], sG, gf[ks]);
  }
  __syncthreads();

  // S^T[key][query] (log2 units, as the forward: scale * log2(e) folded in)
  floatx16 s[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
    for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      f16x8 kf[2];
      row_frag<KD, true>(Kr, kb * 32 + l32, 2 * ks + h, kf);
      s[kb] = mfma_terms<true, ONE>(kf, qf[ks], s[kb]);
    }
  }
  const float cS = scale * 1.4426950408889634f * iQ * iK;
  float mx = -INFINITY;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = score_key(kb, r, h);
      s[kb][r] = key < Kwin ? s[kb][r] * cS : -INFINITY;
      mx = fmaxf(mx, s[kb][r]);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float rinv = 1.f / score_exp<true>(s, mx);
  if (h == 0 && qown) stats[(long long)qsrc * heads + head] = make_float4(mx, rinv, delta, 0.f);

  // per key block: dP^T = V dO^T, dS^T = P^T (dP^T - Delta), dQ^T += K^T dS^T
  const float cP = iV * iG;
  floatx16 dq;
#pragma unroll
  for (int r = 0; r < 16; ++r) dq[r] = 0.f;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    floatx16 dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      f16x8 vf[2];
      row_frag<KD, true>(Vr, kb * 32 + l32, 2 * ks + h, vf);
      dp = mfma_terms<true, ONE>(vf, gf[ks], dp);
    }
    float m = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dp[r] = s[kb][r] * rinv * (dp[r] * cP - delta);  // dS^T
      m = fmaxf(m, fabsf(dp[r]));
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float isd;
    const float sd = sfx::pow2_scale(m, isd);
    floatx16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = 0.f;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      f16x8 bf[2], kt[2];
      frag<true>(make_float4(dp[8 * st + 0], dp[8 * st + 1], dp[8 * st + 2], dp[8 * st + 3]),
               make_float4(dp[8 * st + 4], dp[8 * st + 5], dp[8 * st + 6], dp[8 * st + 7]), sd, bf);
      tr_frag<D, true>(Kt, l32, 2 * kb + st, h, kt);
      t = mfma_terms<true, ONE>(kt, bf, t);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[r] += t[r] * isd;
  }
  if (qown) {
    const float cQ = scale * iK;
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[r] *= cQ;
    store_ot<D>(dqkv + (long long)qsrc * ld + head * D, dq, h);
  }
}

template <int D, bool ONE = false>
__global__ void __launch_bounds__(256, 3)
window_attn_bwd_kv_kernel(const float* __restrict__ qkv, const int* __restrict__ order, const int* __restrict__ win,
                          int Kwin, int C, float scale, const float* __restrict__ dout, float* __restrict__ dqkv,
                          const float4* __restrict__ stats, int nwin) {
  constexpr int KD = D == 16 ? 16 : 32, NKS = KD / 16, QROW = row_bytes(KD);
  constexpr int RB = 2 * KMAX * QROW, TB = 2 * D * VST * 2;
  constexpr int CH = D / 4, NE = (KMAX / 2) * CH, NIT = (NE + 255) / 256;
  constexpr int DP = D + 4;  // fp32 output staging row stride
  static_assert(2 * KMAX * DP * 4 <= 2 * RB + 2 * TB, "output staging must fit the operand images");
  __shared__ __attribute__((aligned(16))) char lds[2 * RB + 2 * TB];
  __shared__ int rows[KMAX];
  __shared__ float4 stat[KMAX];
  __shared__ float4 red[4];
  char* Qr = lds;
  char* Gr = lds + RB;
  unsigned short* Qt = reinterpret_cast<unsigned short*>(lds + 2 * RB);
  unsigned short* Gt = reinterpret_cast<unsigned short*>(lds + 2 * RB + TB);

  const int heads = C / D;
  const int L = xcd_logical_id();
  if (L >= nwin * heads) return;
  const int w = L / heads, head = L - w * heads;
  const int key_start = win[2 * w], query_start = win[2 * w + 1];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const long long ld = 3ll * C;

  if (tid < KMAX) {
    const int src = tid < Kwin ? order[key_start + tid] : -1;
    rows[tid] = src;
    // queries of this window that another window owns (the ragged last window's padding) or past Kwin: P = 0
    // (exp2(s - inf) = 0, 1/sum = 0) and Delta = 0, exactly as their zero dO in the reference
    stat[tid] = (src >= 0 && key_start + tid >= query_start) ? stats[(long long)src * heads + head]
                                                               : make_float4(INFINITY, 0.f, 0.f, 0.f);
  }
  if (D < KD)
    for (int rr = tid; rr < 4 * KMAX; rr += 256)
      *reinterpret_cast<uint4*>(lds + (rr >> 8) * RB + ((rr >> 7) & 1) * KMAX * QROW + row_off<KD>(rr & 127, D / 8)) =
          make_uint4(0, 0, 0, 0);
  __syncthreads();
  // this lane's key: k and v slices (B operands of S and dP)
  const int kk = 32 * wid + l32;
  const int ksrc = rows[kk];
  const bool key_ok = ksrc >= 0;
  float4 ka[NKS][2], va[NKS][2];
  float4 mx4 = make_float4(0.f, 0.f, 0.f, 0.f);  // (q, k, v, dO)
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int d0 = 16 * ks + 8 * h;
    const float* base = qkv + (long long)(key_ok ? ksrc : 0) * ld + head * D;
    load8<D>(base + C, d0, key_ok, ka[ks][0], ka[ks][1]);
    load8<D>(base + 2 * C, d0, key_ok, va[ks][0], va[ks][1]);
    mx4.y = fmaxf(mx4.y, fmaxf(amax4(ka[ks][0]), amax4(ka[ks][1])));
    mx4.z = fmaxf(mx4.z, fmaxf(amax4(va[ks][0]), amax4(va[ks][1])));
  }
  float4 q0[NIT], q1[NIT], g0[NIT], g1[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int e = tid + 256 * it;
    q0[it] = q1[it] = g0[it] = g1[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < NE) {
      const int qp = e / CH, ch = e - qp * CH;
      const int r0 = 2 * qp, s0 = rows[r0], s1 = rows[r0 + 1];
      if (s0 >= 0) {
        q0[it] = *reinterpret_cast<const float4*>(qkv + (long long)s0 * ld + head * D + 4 * ch);
        if (key_start + r0 >= query_start)
          g0[it] = *reinterpret_cast<const float4*>(dout + (long long)s0 * C + head * D + 4 * ch);
      }
      if (s1 >= 0) {
        q1[it] = *reinterpret_cast<const float4*>(qkv + (long long)s1 * ld + head * D + 4 * ch);
        if (key_start + r0 + 1 >= query_start)
          g1[it] = *reinterpret_cast<const float4*>(dout + (long long)s1 * C + head * D + 4 * ch);
      }
    }
    mx4.x = fmaxf(mx4.x, fmaxf(amax4(q0[it]), amax4(q1[it])));
    mx4.w = fmaxf(mx4.w, fmaxf(amax4(g0[it]), amax4(g1[it])));
  }
  mx4 = bwd_wg_max4(mx4, red);
  float iQ, iK, iV, iG;
  const float sQ = sfx::pow2_scale(mx4.x, iQ), sK = sfx::pow2_scale(mx4.y, iK), sV = sfx::pow2_scale(mx4.z, iV),
              sG = sfx::pow2_scale(mx4.w, iG);
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int e = tid + 256 * it;
    if (e < NE) {
      const int qp = e / CH, ch = e - qp * CH;
      stage_pair<D, true, KD>(Qr, Qt, 2 * qp, ch, q0[it], q1[it], sQ);
      stage_pair<D, true, KD>(Gr, Gt, 2 * qp, ch, g0[it], g1[it], sG);
    }
  }
  f16x8 kf[NKS][2], vf[NKS][2];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    frag<true>(ka[ks][0], ka[ks][1], sK, kf[ks]);
    frag<true>(va[ks][0], va[ks][1], sV, vf[ks]);
  }
  __syncthreads();

  const float cS = scale * 1.4426950408889634f * iQ * iK, cP = iG * iV;
  floatx16 dk, dv;
#pragma unroll
  for (int r = 0; r < 16; ++r) dk[r] = dv[r] = 0.f;
#pragma unroll 1
  for (int qb = 0; qb < 4; ++qb) {
    floatx16 sb, pb;
#pragma unroll
    for (int r = 0; r < 16; ++r) sb[r] = pb[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      f16x8 a[2];
      row_frag<KD, true>(Qr, qb * 32 + l32, 2 * ks + h, a);
      sb = mfma_terms<true, ONE>(a, kf[ks], sb);
      row_frag<KD, true>(Gr, qb * 32 + l32, 2 * ks + h, a);
      pb = mfma_terms<true, ONE>(a, vf[ks], pb);
    }
    // rows r: query qb*32 + (r&3) + 8(r>>2) + 4h ; P (<= 1) into sb, dS into pb
    float m = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float4 st = stat[score_key(qb, r, h)];
      const float P = key_ok ? __builtin_amdgcn_exp2f(sb[r] * cS - st.x) * st.y : 0.f;
      sb[r] = P;
      pb[r] = P * (pb[r] * cP - st.z);
      m = fmaxf(m, fabsf(pb[r]));
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float isd;
    const float sd = sfx::pow2_scale(m, isd);
    floatx16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = 0.f;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      f16x8 bp[2], bd[2], at[2];
      frag<true>(make_float4(sb[8 * st + 0], sb[8 * st + 1], sb[8 * st + 2], sb[8 * st + 3]),
               make_float4(sb[8 * st + 4], sb[8 * st + 5], sb[8 * st + 6], sb[8 * st + 7]), 16384.f, bp);
      tr_frag<D, true>(Gt, l32, 2 * qb + st, h, at);
      dv = mfma_terms<true, ONE>(at, bp, dv);
      frag<true>(make_float4(pb[8 * st + 0], pb[8 * st + 1], pb[8 * st + 2], pb[8 * st + 3]),
               make_float4(pb[8 * st + 4], pb[8 * st + 5], pb[8 * st + 6], pb[8 * st + 7]), sd, bd);
      tr_frag<D, true>(Qt, l32, 2 * qb + st, h, at);
      t = mfma_terms<true, ONE>(at, bd, t);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[r] += t[r] * isd;
  }
  // dK / dV leave through LDS (whole row segments per store); keys shared with the neighbouring window (the ragged
  // last window's overlap) are added atomically, every other key is owned by this window and stored plainly
  const float cK = scale * iQ, cV = iG * (1.f / 16384.f);
  __syncthreads();  // all waves done with the operand images
  float* Ok = reinterpret_cast<float*>(lds);
  float* Ov = Ok + KMAX * DP;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int dd = score_key(0, r, h);
    if (dd < D) {
      Ok[kk * DP + dd] = dk[r] * cK;
      Ov[kk * DP + dd] = dv[r] * cV;
    }
  }
  __syncthreads();
  const int next_ks = (w + 1 < nwin) ? win[2 * (w + 1)] : 0x7fffffff;
  for (int e = tid; e < Kwin * 2 * CH; e += 256) {
    const int row = e / (2 * CH);
    const int rem = e - row * 2 * CH;
    const int mat = rem / CH, ch = rem - mat * CH;
    const float4 v = *reinterpret_cast<const float4*>(&(mat == 0 ? Ok : Ov)[row * DP + 4 * ch]);
    float* dst = dqkv + (long long)rows[row] * ld + (mat + 1) * C + head * D + 4 * ch;
    const int pos = key_start + row;
    if (pos < query_start || pos >= next_ks) {
      atomicAdd(dst + 0, v.x);
      atomicAdd(dst + 1, v.y);
      atomicAdd(dst + 2, v.z);
      atomicAdd(dst + 3, v.w);
    } else {
      *reinterpret_cast<float4*>(dst) = v;
    }
  }
}

// SFX_ATTN_PREC=fp32: the exact v_mfma_f32_32x32x2_f32 kernels (read once per process)
bool attn_exact() {
  static int exact = -1;
  if (exact < 0) {
    const char* e = getenv("SFX_ATTN_PREC");
    exact = (e && e[0] == 'f') ? 1 : 0;
  }
  return exact != 0;
}
// f(head_dim as a compile-time constant); the entry points admit 16, 24 and 32 only
template <class F>
void for_head_dim(int head_dim, F&& f) {
  if (head_dim == 16) f(std::integral_constant<int, 16>{});
  else if (head_dim == 24) f(std::integral_constant<int, 24>{});
  else f(std::integral_constant<int, 32>{});
}
constexpr std::true_type kTrue{};
constexpr std::false_type kFalse{};

}  // namespace

extern "C" {

// qkv [N, 3C] (point order), order [N] serialized->point, win [num_windows][2], out [N, C]
int sfx_window_attention(int num_windows, int window, int heads, int head_dim, int channels, const float* qkv,
                         const int* order, const int* win, float scale, float* out,
                         const unsigned long long* qkv_amax, unsigned qkv_tag, void* stream) {
  SFX_REQUIRE(num_windows >= 0, "sfx_window_attention: num_windows < 0");
  SFX_REQUIRE(window >= 1 && window <= KMAX, "sfx_window_attention: window must be in [1, 128]");
  SFX_REQUIRE(heads * head_dim == channels, "sfx_window_attention: heads * head_dim != channels");
  SFX_REQUIRE(head_dim == 16 || head_dim == 24 || head_dim == 32,
              "sfx_window_attention: head_dim %d unsupported (16, 24, 32)", head_dim);
  if (num_windows == 0) return SFX_OK;
  SFX_REQUIRE(qkv && order && win && out, "sfx_window_attention: null buffer");
  dim3 grid(num_windows, heads);
  const long long nblk = ((long long)num_windows * heads + 7) / 8 * 8;
  SFX_REQUIRE(nblk < (1ll << 31), "sfx_window_attention: too many windows");
  hipStream_t st = sfx::as_stream(stream);
  if (attn_exact()) {
    for_head_dim(head_dim, [&](auto d) {
      window_attn_kernel<d()><<<grid, 256, 0, st>>>(qkv, order, win, window, channels, scale, out);
    });
  } else {
    // fp16x2 terms when the caller bounds |qkv| (amax slot), bf16x3 otherwise; reference-precision mode
    // (sfx_set_precision(1)): the leading products only
    const bool one = sfx_get_precision() == 1;
    for_head_dim(head_dim, [&](auto d) {
      auto launch = [&](auto f16, auto o) {
        window_attn_split_kernel<d(), f16(), o()><<<dim3((unsigned)nblk), 256, 0, st>>>(
            qkv, order, win, window, channels, scale, out, qkv_amax, qkv_tag, num_windows);
      };
      if (qkv_amax) { if (one) launch(kTrue, kTrue); else launch(kTrue, kFalse); }
      else { if (one) launch(kFalse, kTrue); else launch(kFalse, kFalse); }
    });
  }
  return sfx::check_launch("sfx_window_attention");
}

// flash mode: win3 [num_windows][3] = (key_start, query_start, key_count), key_count <= max_window
int sfx_window_attention_varlen(int num_windows, int max_window, int heads, int head_dim, int channels,
                                const float* qkv, const int* order, const int* win3, float scale, float* out,
                                const unsigned long long* qkv_amax, unsigned qkv_tag, void* stream) {
  SFX_REQUIRE(num_windows >= 0, "sfx_window_attention_varlen: num_windows < 0");
  SFX_REQUIRE(max_window >= 1 && max_window <= (1 << 20), "sfx_window_attention_varlen: max_window out of [1, 2^20]");
  SFX_REQUIRE(heads * head_dim == channels, "sfx_window_attention_varlen: heads * head_dim != channels");
  SFX_REQUIRE(head_dim == 16 || head_dim == 24 || head_dim == 32,
              "sfx_window_attention_varlen: head_dim %d unsupported (16, 24, 32)", head_dim);
  if (num_windows == 0) return SFX_OK;
  SFX_REQUIRE(qkv && order && win3 && out, "sfx_window_attention_varlen: null buffer");
  const int qblocks = (max_window + KMAX - 1) / KMAX;
  const long long nblk = ((long long)num_windows * qblocks * heads + 7) / 8 * 8;
  SFX_REQUIRE(nblk < (1ll << 31) && heads <= 65535, "sfx_window_attention_varlen: grid too large");
  hipStream_t st = sfx::as_stream(stream);
  if (attn_exact()) {
    dim3 grid((unsigned)(num_windows * qblocks), heads);
    for_head_dim(head_dim, [&](auto d) {
      window_attn_flash_kernel<d()><<<grid, 256, 0, st>>>(qkv, order, win3, qblocks, channels, scale, out);
    });
    return sfx::check_launch("sfx_window_attention_varlen");
  }
  for_head_dim(head_dim, [&](auto d) {
    auto launch = [&](auto f16) {
      window_attn_split_flash_kernel<d(), f16()><<<dim3((unsigned)nblk), 256, 0, st>>>(
          qkv, order, win3, qblocks, channels, scale, out, qkv_amax, qkv_tag, num_windows);
    };
    if (qkv_amax) launch(kTrue);  // fp16x2 terms (the caller bounds |qkv|)
    else launch(kFalse);
  });
  return sfx::check_launch("sfx_window_attention_varlen");
}

// flash-mode backward: dqkv [N, 3C] zero-filled by the caller, stats [N][heads][2] floats of workspace
int sfx_window_attention_varlen_bwd(int num_windows, int max_window, int heads, int head_dim, int channels,
                                    const float* qkv, const int* order, const int* win3, float scale,
                                    const float* dout, float* dqkv, float* stats, void* stream) {
  SFX_REQUIRE(num_windows >= 0, "sfx_window_attention_varlen_bwd: num_windows < 0");
  SFX_REQUIRE(max_window >= 1 && max_window <= (1 << 20),
              "sfx_window_attention_varlen_bwd: max_window out of [1, 2^20]");
  SFX_REQUIRE(heads * head_dim == channels, "sfx_window_attention_varlen_bwd: heads * head_dim != channels");
  SFX_REQUIRE(head_dim == 16 || head_dim == 24 || head_dim == 32,
              "sfx_window_attention_varlen_bwd: head_dim %d unsupported (16, 24, 32)", head_dim);
  if (num_windows == 0) return SFX_OK;
  SFX_REQUIRE(qkv && order && win3 && dout && dqkv && stats, "sfx_window_attention_varlen_bwd: null buffer");
  const int blocks = (max_window + FB - 1) / FB;
  SFX_REQUIRE((long long)num_windows * blocks < (1ll << 31) && heads <= 65535,
              "sfx_window_attention_varlen_bwd: grid too large");
  dim3 grid((unsigned)(num_windows * blocks), heads);
  hipStream_t st = sfx::as_stream(stream);
  for_head_dim(head_dim, [&](auto d) {
    flash_bwd_query_kernel<d()><<<grid, FB, 0, st>>>(qkv, order, win3, blocks, channels, heads, scale, dout, dqkv,
                                                      stats);
    flash_bwd_key_kernel<d()><<<grid, FB, 0, st>>>(qkv, order, win3, blocks, channels, heads, scale, dout, dqkv, stats);
  });
  return sfx::check_launch("sfx_window_attention_varlen_bwd");
}

// dout [N, C] = d(attention output); attn_out [N, C] = the forward's output; dqkv [N, 3C] (every element written;
// the exact kernel needs it zero-filled by the caller); stats: workspace of N * heads float4 (query pass -> key
// pass).  SFX_ATTN_PREC=fp32: the exact single-kernel backward (attn_out and stats unused, dqkv zero-filled)
int sfx_window_attention_bwd(int num_windows, int window, int heads, int head_dim, int channels, const float* qkv,
                             const int* order, const int* win, float scale, const float* attn_out, const float* dout,
                             float* dqkv, float* stats, void* stream) {
  SFX_REQUIRE(num_windows >= 0, "sfx_window_attention_bwd: num_windows < 0");
  SFX_REQUIRE(window >= 1 && window <= KMAX, "sfx_window_attention_bwd: window must be in [1, 128]");
  SFX_REQUIRE(heads * head_dim == channels, "sfx_window_attention_bwd: heads * head_dim != channels");
  SFX_REQUIRE(head_dim == 16 || head_dim == 24 || head_dim == 32,
              "sfx_window_attention_bwd: head_dim %d unsupported (16, 24, 32)", head_dim);
  if (num_windows == 0) return SFX_OK;
  SFX_REQUIRE(qkv && order && win && dout && dqkv, "sfx_window_attention_bwd: null buffer");
  hipStream_t st = sfx::as_stream(stream);
  if (!attn_exact()) {
    SFX_REQUIRE(attn_out && stats, "sfx_window_attention_bwd: null attn_out / stats");
    const long long nblk = ((long long)num_windows * heads + 7) / 8 * 8;
    SFX_REQUIRE(nblk < (1ll << 31), "sfx_window_attention_bwd: too many windows");
    float4* st4 = reinterpret_cast<float4*>(stats);
    const bool one = sfx_get_precision() == 1;  // reference-precision mode: single fp16 products
    for_head_dim(head_dim, [&](auto d) {
      auto launch = [&](auto o) {
        window_attn_bwd_q_kernel<d(), o()><<<dim3((unsigned)nblk), 256, 0, st>>>(
            qkv, order, win, window, channels, scale, attn_out, dout, dqkv, st4, num_windows);
        window_attn_bwd_kv_kernel<d(), o()><<<dim3((unsigned)nblk), 256, 0, st>>>(
            qkv, order, win, window, channels, scale, dout, dqkv, st4, num_windows);
      };
      if (one) launch(kTrue);
      else launch(kFalse);
    });
    return sfx::check_launch("sfx_window_attention_bwd");
  }
  dim3 grid(num_windows, heads);
  for_head_dim(head_dim, [&](auto d) {
    window_attn_bwd_kernel<d()><<<grid, 256, 0, st>>>(qkv, order, win, window, channels, scale, dout, dqkv);
  });
  return sfx::check_launch("sfx_window_attention_bwd");
}

}  // extern "C"

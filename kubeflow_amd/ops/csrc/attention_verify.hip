// attention_verify.hip — multi-token (speculative-verify) GQA attention over
// the KV cache, on the 32x32x16 bf16 MFMA.
//
//   q      [N, T, Hq, 128] bf16   T new tokens per sequence, 1 <= T <= 8,
//                                 g*T <= 32 (g = Hq/Hkv)
//   kcache [SLOTS, SMAX, Hkv, 128] bf16 (same layout for vcache)
//   slots  [N] int32; lens [N] int32 = keys visible to token 0
//   out    [N, T, Hq, 128] bf16
//
// Token t of sequence n sees keys [0, vis), vis = min(max(lens[n],0)+t, SMAX);
// vis == 0 gives a zero row. T = 1 is kf_attn_decode's contract.
//
// Grid (N, Hkv, splits), 4 waves. A kv-head's g*T query rows are stacked into
// ONE 32-column tile (row r = t*g + hg), loaded once as MFMA B fragments and
// kept in registers. Each wave is an independent key stream: within the
// block's [lo, hi) slice wave w owns every fourth 32-key sub-tile, stages its
// K (kf_swz rows) and V (kf_vsub<32> subtiles) into its OWN 16 KiB LDS region,
// prefetches the next sub-tile's rows into registers before computing the
// current one, and keeps its own (m, l, O). Only the owner reads what it
// wrote, so the key loop has no __syncthreads, only the wave-local lgkmcnt
// wait. Per sub-tile: S^T[key,row] = 8 x mfma(K, Q); in-register online
// softmax in the exp2 domain (a lane's accumulator column is one query row);
// P^T re-fragmented with kf_exchange; O^T[d,row] += mfma(V^T, P^T) through
// the ds_read_b64_tr_b16 transpose read. One block barrier, then the four
// partials merge through LDS in wave order 0..3 (wave w owns d-block w).
//
// Lives beside attention_decode.hip rather than in it: this file is built
// without the packed fp32 instructions (build_ext.EXTRA_CFLAGS), a per-file
// flag that must not change the code generated for kf_attn_decode. The
// split partials go through that file's combine kernel unchanged
// (kf_attn_decode_combine_launch).

#include "kf_attn_common.h"

#define AV_D 128
#define AV_SUB 32                       // keys per wave sub-tile
#define AV_WAVES 4
#define AV_STRIDE (AV_SUB * AV_WAVES)   // keys per block round: 128
#define AV_TILEB (AV_SUB * AV_D * 2)    // one K or V sub-tile: 8 KiB
#define AV_ROWB (AV_D * 2)

__global__ __launch_bounds__(256, 2) void kf_attn_verify_kernel(
    unsigned short* __restrict__ out, float* __restrict__ part_o,
    float* __restrict__ part_ml, const unsigned short* __restrict__ q,
    const unsigned short* __restrict__ kcache,
    const unsigned short* __restrict__ vcache,
    const int* __restrict__ slots, const int* __restrict__ lens, int T,
    int smax, int Hq, int Hkv, float scale) {
  // per wave: K sub-tile at +0 (swizzled rows), V at +AV_TILEB (subtiled);
  // after the key loop the same 16 KiB holds the wave's O partial
  __shared__ __attribute__((aligned(16)))
  unsigned char lds[AV_WAVES][2 * AV_TILEB];
  __shared__ float ml_lds[AV_WAVES][2][32];

  const int n = blockIdx.x, hkv = blockIdx.y;
  const int z = blockIdx.z, splits = gridDim.z;
  const int g = Hq / Hkv;
  const int w = threadIdx.x / KF_WAVE;
  const int lane = threadIdx.x & (KF_WAVE - 1);
  const int l31 = lane & 31;
  const int hi = lane >> 5;
  const float scale2 = scale * KF_LOG2E;
  const int nrows = g * T;

  // clamps are memory safety: no content of lens reaches past the slot
  const int len0 = min(max(lens[n], 0), smax);   // smallest vis of the block
  const int vmax = min(len0 + T - 1, smax);      // largest
  const int64_t slot = slots[n];
  const int64_t cbase = (slot * smax * Hkv + hkv) * AV_D;
  const int64_t cstride = (int64_t)Hkv * AV_D;
  // this split's key slice, aligned to one round of the four waves
  const int chunk =
      ((vmax + splits - 1) / splits + AV_STRIDE - 1) / AV_STRIDE * AV_STRIDE;
  const int lo = z * chunk, hi_k = min(vmax, lo + chunk);

  // ---- this lane's query row (accumulator column) ----
  const bool row_ok = l31 < nrows;
  const int tq = row_ok ? l31 / g : 0;
  const int hq = hkv * g + (row_ok ? l31 - tq * g : 0);
  const int64_t orow = ((int64_t)n * T + tq) * Hq + hq;
  const int vis = row_ok ? min(len0 + tq, smax) : 0;

  kf_bf16x8 qfrag[8];
  {
    const kf_short8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      kf_short8 v8 = zero8;
      if (row_ok)
        v8 = *reinterpret_cast<const kf_short8*>(q + orow * AV_D + kk * 16 +
                                                 hi * 8);
      qfrag[kk] = *reinterpret_cast<kf_bf16x8*>(&v8);
    }
  }

  kf_f32x16 oacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) oacc[i] = kf_f32x16{0.f};
  float m_run = -INFINITY, l_run = 0.f;  // m_run in exp2 units

  // staging: lane covers rows (lane>>4) + 4u, 16-byte chunk lane&15 — each
  // 16-lane group reads one whole 256-byte cache row
  unsigned char* const my_k = lds[w];
  unsigned char* const my_v = lds[w] + AV_TILEB;
  const int sr0 = lane >> 4, c8 = lane & 15;
  const unsigned vbase =
      (unsigned)(size_t)my_v + kf_tr_lane_off<AV_SUB>(lane);
  kf_short8 kst[8], vst[8];

  int kb = lo + w * AV_SUB;
  if (kb < hi_k) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      // rows past the slot's end re-read its last row; they are masked
      const int64_t off = cbase +
          (int64_t)min(kb + sr0 + 4 * u, smax - 1) * cstride + c8 * 8;
      kst[u] = *reinterpret_cast<const kf_short8*>(kcache + off);
      vst[u] = *reinterpret_cast<const kf_short8*>(vcache + off);
    }
  }
  for (; kb < hi_k; kb += AV_STRIDE) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = sr0 + 4 * u;
      *reinterpret_cast<kf_short8*>(my_k + kf_swz(r, c8 * 16, AV_ROWB)) =
          kst[u];
      *reinterpret_cast<kf_short8*>(my_v + 2 * kf_vsub<AV_SUB>(r, c8 * 8)) =
          vst[u];
    }
    // next sub-tile's rows fly under this one's compute
    const int nb = kb + AV_STRIDE;
    if (nb < hi_k) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t off = cbase +
            (int64_t)min(nb + sr0 + 4 * u, smax - 1) * cstride + c8 * 8;
        kst[u] = *reinterpret_cast<const kf_short8*>(kcache + off);
        vst[u] = *reinterpret_cast<const kf_short8*>(vcache + off);
      }
    }
    // wave-local write -> read fence (other lanes' rows)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- S^T = mfma(K, Q): K leaves LDS once for all g*T rows ----
    kf_bf16x8 af[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
      af[kk] = *reinterpret_cast<const kf_bf16x8*>(
          my_k + kf_swz(l31, kk * 32 + hi * 16, AV_ROWB));
    kf_f32x16 st = kf_f32x16{0.f};
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[kk], qfrag[kk], st, 0,
                                                   0, 0);
    __builtin_amdgcn_s_setprio(0);

    // ---- online softmax; the compare only where the sub-tile reaches
    // past the block's smallest vis (wave-uniform branch) ----
    float mx = -INFINITY;
    if (kb + AV_SUB > len0) {
      const int key0 = kb + hi * 4;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float sv = st[r] * scale2;
        if (key0 + (r & 3) + 8 * (r >> 2) >= vis) sv = -INFINITY;
        st[r] = sv;
        mx = fmaxf(mx, sv);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float sv = st[r] * scale2;
        st[r] = sv;
        mx = fmaxf(mx, sv);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, KF_WAVE));
    if (!__all(mx <= m_run + KF_DEFER_MAX_THR2)) {
      const float m_new = fmaxf(m_run, mx);
      // a row with no visible key yet keeps m = -inf
      const float alpha = m_new == -INFINITY ? 1.f : kf_exp2(m_run - m_new);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
      l_run *= alpha;
      m_run = m_new;
    }
    const float m_use = m_run == -INFINITY ? 0.f : m_run;
    float lsum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pv = kf_exp2(st[r] - m_use);  // masked -inf -> 0
      st[r] = pv;
      lsum += pv;
    }
    lsum += __shfl_xor(lsum, 32, KF_WAVE);
    l_run += lsum;
    const kf_bf16x8 p0 = kf_exchange(st, 0);
    const kf_bf16x8 p1 = kf_exchange(st, 8);

    // ---- O^T += V^T P^T (ends on lgkmcnt(0): the region is free again) ----
    kf_tr_acc_loop<true, AV_SUB>(oacc, vbase, p0, p1);
  }

  // ---- merge the four key streams: [d-block][quad][lane] float4 ----
  float* const my_o = reinterpret_cast<float*>(lds[w]);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      kf_f32x4 v4 = {oacc[dt][rq * 4], oacc[dt][rq * 4 + 1],
                     oacc[dt][rq * 4 + 2], oacc[dt][rq * 4 + 3]};
      *reinterpret_cast<kf_f32x4*>(my_o + ((dt * 4 + rq) * 64 + lane) * 4) =
          v4;
    }
  if (hi == 0) {
    ml_lds[w][0][l31] = m_run;
    ml_lds[w][1][l31] = l_run;
  }
  __syncthreads();

  // wave w finishes d in [32w, 32w + 32) of every row, sources in order 0..3
  float M = -INFINITY;
#pragma unroll
  for (int s = 0; s < AV_WAVES; ++s) M = fmaxf(M, ml_lds[s][0][l31]);
  float L = 0.f;
  kf_f32x16 res = kf_f32x16{0.f};
#pragma unroll
  for (int s = 0; s < AV_WAVES; ++s) {
    const float ms = ml_lds[s][0][l31];
    const float wz = ms == -INFINITY ? 0.f : kf_exp2(ms - M);
    L += ml_lds[s][1][l31] * wz;
    const float* so = reinterpret_cast<const float*>(lds[s]);
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const kf_f32x4 v4 = *reinterpret_cast<const kf_f32x4*>(
          so + ((w * 4 + rq) * 64 + lane) * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) res[rq * 4 + j] += v4[j] * wz;
    }
  }
  if (!row_ok) return;  // rows >= g*T are padding: never stored

  if (splits == 1) {
    const float inv_l = L > 0.f ? 1.f / L : 0.f;
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      unsigned short q4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        q4[j] = kf_f32_to_bf16(res[rq * 4 + j] * inv_l);
      *reinterpret_cast<kf_short4*>(out + orow * AV_D + w * 32 + 8 * rq +
                                    4 * hi) =
          *reinterpret_cast<kf_short4*>(q4);
    }
  } else {
    // unnormalised (o, m, l) in the combine kernel's layout; its m is in
    // natural-log units with the scale applied
    const int64_t pb = orow * splits + z;
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      kf_f32x4 v4 = {res[rq * 4], res[rq * 4 + 1], res[rq * 4 + 2],
                     res[rq * 4 + 3]};
      *reinterpret_cast<kf_f32x4*>(part_o + pb * AV_D + w * 32 + 8 * rq +
                                   4 * hi) = v4;
    }
    if (w == 0 && hi == 0) {
      part_ml[pb * 2] = M * KF_LN2;  // -inf stays -inf
      part_ml[pb * 2 + 1] = L;
    }
  }
}

// splits > 1 requires part_o [N,T*Hq,splits,128] f32 and part_ml
// [N,T*Hq,splits,2] f32 workspaces.
KF_EXPORT int kf_attn_verify(void* out, void* part_o, void* part_ml,
                             const void* q, const void* kcache,
                             const void* vcache, const int* slots,
                             const int* lens, int64_t N, int64_t T,
                             int64_t smax, int64_t Hq, int64_t Hkv,
                             int64_t D, int64_t splits, float scale,
                             void* stream) {
  if (D != AV_D || Hkv < 1 || Hq % Hkv) return (int)hipErrorInvalidValue;
  if (T < 1 || T > 8 || (Hq / Hkv) * T > 32) return (int)hipErrorInvalidValue;
  if (splits < 1 || smax < 1) return (int)hipErrorInvalidValue;
  if (splits > 1 && (!part_o || !part_ml)) return (int)hipErrorInvalidValue;
  dim3 grid((unsigned)N, (unsigned)Hkv, (unsigned)splits);
  hipLaunchKernelGGL(kf_attn_verify_kernel, grid, dim3(256), 0,
                     (hipStream_t)stream, (unsigned short*)out,
                     (float*)part_o, (float*)part_ml,
                     (const unsigned short*)q, (const unsigned short*)kcache,
                     (const unsigned short*)vcache, slots, lens, (int)T,
                     (int)smax, (int)Hq, (int)Hkv, scale);
  if (splits > 1)
    kf_attn_decode_combine_launch(out, part_o, part_ml, N * T * Hq,
                                  (int)splits, stream);
  return (int)hipGetLastError();
}

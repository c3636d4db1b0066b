// attention_cache64.hip — head-dim-64 GQA attention over the KV cache: decode,
// multi-token verify and ragged prefill through ONE kernel body, on the
// 32x32x16 bf16 MFMA.
//
//   q      [R, Hq, 64] bf16       packed query rows of N sequences
//   kcache [SLOTS, SMAX, Hkv, 64] bf16 (same layout for vcache)
//   slots  [N] int32; starts [N+1] int32 or null; lens [N] int32
//   out    [R, Hq, 64] bf16
//
// kf_attn_prefill's ragged contract: rows [starts[n], starts[n+1]) of q are
// tokens i = 0..C_n-1 of sequence n, whose K/V rows are already in cache slot
// slots[n]; token i sees keys [0, vis), vis = min(max(lens[n],0)+i, SMAX);
// vis == 0 gives a zero row; rows outside every range are never written;
// max_rows (host) bounds every C_n and sizes the grid; the index arrays are
// read on the device only and every index is clamped. Two additions:
// starts == null gives sequence n the rows [n*max_rows, (n+1)*max_rows)
// (decode: max_rows = 1, verify: max_rows = T), and splits > 1 divides each
// block's key range over `splits` blocks that leave (o, m, l) partials for
// kf_attn64_cache_combine.
//
// Grid (ceil(max_rows*g / (32*RW)), Hkv*splits, N), 4 waves. A block owns
// 32*RW tile rows of one (sequence, kv-head, key split); tile row r =
// (token, hg) = (r / g, r % g), so the g q-heads of a kv-head share every
// staged tile. The four waves are RW row groups x KW key streams (RW*KW = 4),
// a template parameter the host picks from max_rows*g:
//   <= 32 rows  <1,4>  four key streams over one 32-row tile (decode, verify)
//   <= 64 rows  <2,2>
//   >  64 rows  <4,1>  four independent row streams (prefill)
// 128-key K tiles (kf_swz rows: a 128-byte row is exactly one swizzle span)
// and V tiles (128 x 64, the first four slabs of kf_vsub<128>) are shared by
// the whole block and double-buffered in LDS: 2 x (16 + 16) KiB = 64 KiB, two
// blocks per CU. A cache row is 8 16-byte chunks, so 256 threads stage 32 rows
// per pass, 4 passes each for K and V. Per tile: the next tile's rows are
// loaded from global into registers, ONE barrier, compute on the current
// buffer, then the registers are written into the other buffer (the hazard
// argument is attention_prefill.hip's). Wave (rg, ks) computes the 32-key
// sub-tiles h with h % KW == ks: S^T[key,row] = 4 x mfma(K, Q) with Q held in
// registers, online softmax in the exp2 domain with defer-max, P^T through
// kf_exchange, O^T[d,row] += mfma(V^T, P^T) through ds_read_b64_tr_b16 into
// two accumulators.
//
// KW > 1: after the key loop the buffer the last tile did NOT use is free
// (its last readers passed the loop's last barrier), so each wave parks its
// (m, l, O) there, one barrier, and the KW partials of a row group merge by
// the online-softmax rule in stream order 0..KW-1; stream ks finishes 8/KW of
// the 8 accumulator quads of every row.
//
// splits > 1: the block's own visible range [0, hi_k) is cut into `splits`
// 128-aligned slices, so long and short sequences divide alike and no tile
// straddles a slice. Each block writes unnormalised fp32 (o, m*ln2, l) per
// row and split — (0, -inf, 0) for an empty slice, so the workspaces may
// arrive with any contents — and kf_attn64_cache_combine merges them in split
// order for exactly the rows some block covered.
//
// Built without the packed fp32 instructions (build_ext.EXTRA_CFLAGS), as
// attention_verify.hip and attention_prefill.hip are.

#include "kf_attn_common.h"

#define AC_D 64
#define AC_KT 128                      // keys per staged tile
#define AC_SUB 32                      // keys per MFMA sub-tile
#define AC_ROWB (AC_D * 2)             // 128 B per cache row
#define AC_TILEB (AC_KT * AC_D * 2)    // one K or V tile: 16 KiB
#define AC_COMB_ROWS 16                // (token, head) rows per combine block

// kf_tr_acc_loop for two d-blocks: acc[dt] += mfma(tr(dt), p) over dt = 0, 1.
// Both d-blocks' transposed fragments are requested up front; the first MFMA
// pair waits for its own four reads only.
template <int ROWS>
__device__ __forceinline__ void ac_tr_acc_loop2(kf_f32x16 (&acc)[2],
                                                unsigned vbase,
                                                const kf_bf16x8& p0,
                                                const kf_bf16x8& p1) {
  kf_short4 t[2][4];
  const unsigned va = vbase + (unsigned)(ROWS * 64);
  KF_TR16(t[0][0], vbase, "0");
  KF_TR16(t[0][1], vbase, "128");
  KF_TR16(t[0][2], vbase, "512");
  KF_TR16(t[0][3], vbase, "640");
  KF_TR16(t[1][0], va, "0");
  KF_TR16(t[1][1], va, "128");
  KF_TR16(t[1][2], va, "512");
  KF_TR16(t[1][3], va, "640");
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    if (dt == 0) {
      asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_sched_barrier(0);
    kf_short8 f0 = __builtin_shufflevector(t[dt][0], t[dt][1], 0, 1, 2, 3, 4,
                                           5, 6, 7);
    kf_short8 f1 = __builtin_shufflevector(t[dt][2], t[dt][3], 0, 1, 2, 3, 4,
                                           5, 6, 7);
    const kf_bf16x8 a0 = *reinterpret_cast<kf_bf16x8*>(&f0);
    const kf_bf16x8 a1 = *reinterpret_cast<kf_bf16x8*>(&f1);
    __builtin_amdgcn_s_setprio(1);
    acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, p0, acc[dt], 0, 0,
                                                      0);
    acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, p1, acc[dt], 0, 0,
                                                      0);
    __builtin_amdgcn_s_setprio(0);
  }
}

// Sequence n's row range [row0, row0 + C), clamped into [0, R) and to
// max_rows. 64-bit so that no difference overflows. Shared by the attention
// kernel and the combine so that both cover exactly the same rows.
__device__ __forceinline__ void ac_row_range(const int* __restrict__ starts,
                                             int n, int R, int max_rows,
                                             int& row0, int& C) {
  int64_t s_lo, s_hi;
  if (starts) {
    s_lo = starts[n];
    s_hi = starts[n + 1];
  } else {
    s_lo = (int64_t)n * max_rows;
    s_hi = s_lo + max_rows;
  }
  row0 = (int)min(max(s_lo, (int64_t)0), (int64_t)R);
  C = (int)min(min(max(s_hi - s_lo, (int64_t)0), (int64_t)max_rows),
               (int64_t)(R - row0));
}

template <int RW, int KW>
__global__ __launch_bounds__(256, 2) void kf_attn64_cache_kernel(
    unsigned short* __restrict__ out, float* __restrict__ part_o,
    float* __restrict__ part_ml, const unsigned short* __restrict__ q,
    const unsigned short* __restrict__ kcache,
    const unsigned short* __restrict__ vcache,
    const int* __restrict__ slots, const int* __restrict__ starts,
    const int* __restrict__ lens, int R, int max_rows, int smax, int n_slots,
    int Hq, int Hkv, int splits, float scale) {
  static_assert(RW * KW == 4, "four waves");
  constexpr int ROWS = AC_SUB * RW;  // tile rows per block
  constexpr int NQ = 8 / KW;         // accumulator quads a wave finishes
  // [buffer][K tile | V tile]; with KW > 1 the free buffer later holds the
  // four waves' O partials (8 KiB each)
  __shared__ __attribute__((aligned(16)))
  unsigned char lds[2][2 * AC_TILEB];
  __shared__ float ml_lds[KW > 1 ? 4 : 1][2][32];

  const int bx = gridDim.x - 1 - blockIdx.x;  // most keys first
  const int hkv = blockIdx.y / splits, z = blockIdx.y % splits;
  const int n = blockIdx.z;
  const int g = Hq / Hkv;

  // clamps are memory safety: no content of starts / lens / slots reaches
  // past q, out, the workspaces or the cache
  int row0, C;
  ac_row_range(starts, n, R, max_rows, row0, C);
  const int tok_blk = bx * ROWS / g;          // g divides 32
  if (tok_blk >= C) return;                   // before any vector load

  const int w = threadIdx.x / KF_WAVE;
  const int rg = w / KW, ks = w % KW;
  const int lane = threadIdx.x & (KF_WAVE - 1);
  const int l31 = lane & 31;
  const int hi = lane >> 5;
  const float scale2 = scale * KF_LOG2E;

  const int len0 = min(max(lens[n], 0), smax);
  const int64_t slot = min(max(slots[n], 0), n_slots - 1);
  const int64_t cbase = (slot * smax * Hkv + hkv) * AC_D;
  const int64_t cstride = (int64_t)Hkv * AC_D;
  // the block's last visible key bounds its key range; this split's slice
  const int tok_last = min(C - 1, (bx * ROWS + ROWS - 1) / g);
  const int hi_k = min(len0 + tok_last, smax);
  const int chunk =
      ((hi_k + splits - 1) / splits + AC_KT - 1) / AC_KT * AC_KT;
  const int lo = min(z * chunk, hi_k);        // chunk * z <= hi_k + 128 * z
  const int hi_s = min(hi_k, lo + chunk);

  // ---- this wave's rows; a lane's accumulator column is one query row ----
  const int tok_w = (bx * ROWS + rg * AC_SUB) / g;     // wave's first token
  const bool wave_live = tok_w < C;
  const int tok_wl = min(C - 1, tok_w + AC_SUB / g - 1);
  const int vis_lo = min(len0 + tok_w, smax);          // wave's smallest vis
  const int vis_hi = wave_live ? min(len0 + tok_wl, smax) : 0;  // largest
  const int tq = tok_w + l31 / g;
  const bool row_ok = tq < C;
  const int hq = hkv * g + l31 % g;
  const int64_t orow = (int64_t)(row0 + (row_ok ? tq : 0)) * Hq + hq;
  const int vis = row_ok ? min(len0 + tq, smax) : 0;

  kf_bf16x8 qfrag[4];
  {
    const kf_short8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      kf_short8 v8 = zero8;
      if (row_ok)
        v8 = *reinterpret_cast<const kf_short8*>(q + orow * AC_D + kk * 16 +
                                                 hi * 8);
      qfrag[kk] = *reinterpret_cast<kf_bf16x8*>(&v8);
    }
  }

  kf_f32x16 oacc[2];
  oacc[0] = kf_f32x16{0.f};
  oacc[1] = kf_f32x16{0.f};
  float m_run = -INFINITY, l_run = 0.f;  // m_run in exp2 units

  // staging: thread covers rows (tid>>3) + 32u, 16-byte chunk tid&7 — each
  // 8-lane group reads one whole 128-byte cache row
  const int sr0 = threadIdx.x >> 3, c8 = threadIdx.x & 7;
  const unsigned tr_off = kf_tr_lane_off<AC_KT>(lane);
  kf_short8 kst[4], vst[4];

  auto load_tile = [&](int kb) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // rows past the slot's end re-read its last row; they are masked
      const int64_t off = cbase +
          (int64_t)min(kb + sr0 + 32 * u, smax - 1) * cstride + c8 * 8;
      kst[u] = *reinterpret_cast<const kf_short8*>(kcache + off);
      vst[u] = *reinterpret_cast<const kf_short8*>(vcache + off);
    }
  };
  auto write_tile = [&](int b) {
    unsigned char* const kt = lds[b];
    unsigned char* const vt = lds[b] + AC_TILEB;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = sr0 + 32 * u;
      *reinterpret_cast<kf_short8*>(kt + kf_swz(r, c8 * 16, AC_ROWB)) = kst[u];
      *reinterpret_cast<kf_short8*>(vt + 2 * kf_vsub<AC_KT>(r, c8 * 8)) =
          vst[u];
    }
  };

  if (lo < hi_s) {
    load_tile(lo);
    write_tile(0);
  }
  int buf = 0;
  for (int kb = lo; kb < hi_s; kb += AC_KT, buf ^= 1) {
    // next tile's rows fly under this one's compute
    const bool more = kb + AC_KT < hi_s;
    if (more) load_tile(kb + AC_KT);
    __syncthreads();

    if (wave_live) {
#pragma unroll
      for (int h = ks; h < AC_KT / AC_SUB; h += KW) {
        const int k0 = kb + h * AC_SUB;
        if (k0 >= vis_hi) break;  // wholly past the wave's last visible key

        // ---- S^T = mfma(K, Q) ----
        const unsigned char* const kt = lds[buf];
        kf_bf16x8 af[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          af[kk] = *reinterpret_cast<const kf_bf16x8*>(
              kt + kf_swz(h * AC_SUB + l31, kk * 32 + hi * 16, AC_ROWB));
        kf_f32x16 st = kf_f32x16{0.f};
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[kk], qfrag[kk], st,
                                                       0, 0, 0);
        __builtin_amdgcn_s_setprio(0);

        // ---- online softmax; the compare only where the sub-tile reaches
        // past the wave's smallest vis (wave-uniform branch) ----
        float mx = -INFINITY;
        if (k0 + AC_SUB > vis_lo) {
          const int key0 = k0 + hi * 4;
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
          const float alpha =
              m_new == -INFINITY ? 1.f : kf_exp2(m_run - m_new);
#pragma unroll
          for (int i = 0; i < 2; ++i)
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

        // ---- O^T += V^T P^T: sub-tile h starts 32 rows = 1 KiB into each
        // slab ----
        const unsigned vbase =
            (unsigned)(size_t)(lds[buf] + AC_TILEB) + h * (AC_SUB * 32) +
            tr_off;
        ac_tr_acc_loop2<AC_KT>(oacc, vbase, p0, p1);
      }
    }
    if (more) write_tile(buf ^ 1);
  }

  // ---- the NQ accumulator quads this wave finishes: quad qd = (dt, rq) is
  // d = 32dt + 8rq + 4hi + (0..3) of the lane's row ----
  float res[NQ][4];
  float M = m_run, L = l_run;
  if constexpr (KW == 1) {
#pragma unroll
    for (int qd = 0; qd < 8; ++qd)
#pragma unroll
      for (int j = 0; j < 4; ++j) res[qd][j] = oacc[qd >> 2][(qd & 3) * 4 + j];
  } else {
    // lds[buf] is the buffer the last tile did not use: park [quad][lane]
    float* const my_o = reinterpret_cast<float*>(lds[buf] + w * (AC_TILEB / 2));
#pragma unroll
    for (int qd = 0; qd < 8; ++qd) {
      kf_f32x4 v4 = {oacc[qd >> 2][(qd & 3) * 4], oacc[qd >> 2][(qd & 3) * 4 + 1],
                     oacc[qd >> 2][(qd & 3) * 4 + 2],
                     oacc[qd >> 2][(qd & 3) * 4 + 3]};
      *reinterpret_cast<kf_f32x4*>(my_o + (qd * 64 + lane) * 4) = v4;
    }
    if (hi == 0) {
      ml_lds[w][0][l31] = m_run;
      ml_lds[w][1][l31] = l_run;
    }
    __syncthreads();

    // stream ks finishes quads [ks*NQ, ks*NQ + NQ), sources in order 0..KW-1
    M = -INFINITY;
#pragma unroll
    for (int s = 0; s < KW; ++s) M = fmaxf(M, ml_lds[rg * KW + s][0][l31]);
    L = 0.f;
#pragma unroll
    for (int i = 0; i < NQ; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) res[i][j] = 0.f;
#pragma unroll
    for (int s = 0; s < KW; ++s) {
      const int sw = rg * KW + s;
      const float ms = ml_lds[sw][0][l31];
      const float wz = ms == -INFINITY ? 0.f : kf_exp2(ms - M);
      L += ml_lds[sw][1][l31] * wz;
      const float* so =
          reinterpret_cast<const float*>(lds[buf] + sw * (AC_TILEB / 2));
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        const kf_f32x4 v4 = *reinterpret_cast<const kf_f32x4*>(
            so + ((ks * NQ + i) * 64 + lane) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) res[i][j] += v4[j] * wz;
      }
    }
  }
  if (!row_ok) return;  // padding rows of the last tile: never stored

  if (splits == 1) {
    const float inv_l = L > 0.f ? 1.f / L : 0.f;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int qd = ks * NQ + i;
      unsigned short q4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) q4[j] = kf_f32_to_bf16(res[i][j] * inv_l);
      *reinterpret_cast<kf_short4*>(out + orow * AC_D + (qd >> 2) * 32 +
                                    8 * (qd & 3) + 4 * hi) =
          *reinterpret_cast<kf_short4*>(q4);
    }
  } else {
    // unnormalised (o, m, l); m in natural-log units with the scale applied
    const int64_t pb = orow * splits + z;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int qd = ks * NQ + i;
      kf_f32x4 v4 = {res[i][0], res[i][1], res[i][2], res[i][3]};
      *reinterpret_cast<kf_f32x4*>(part_o + pb * AC_D + (qd >> 2) * 32 +
                                   8 * (qd & 3) + 4 * hi) = v4;
    }
    if (ks == 0 && hi == 0) {
      part_ml[pb * 2] = M * KF_LN2;  // -inf stays -inf
      part_ml[pb * 2 + 1] = L;
    }
  }
}

// Merge the split partials of every covered row in split order and store
// bf16. Grid (ceil(max_rows*Hq / 16), N): 16 lanes per (token, head) row, a
// lane owns 4 consecutive d. Rows outside [row0, row0 + C) are not touched.
__global__ __launch_bounds__(256) void kf_attn64_cache_combine_kernel(
    unsigned short* __restrict__ out, const float* __restrict__ part_o,
    const float* __restrict__ part_ml, const int* __restrict__ starts, int R,
    int max_rows, int Hq, int splits) {
  const int n = blockIdx.y;
  int row0, C;
  ac_row_range(starts, n, R, max_rows, row0, C);
  const int idx = blockIdx.x * AC_COMB_ROWS + (threadIdx.x >> 4);
  const int tok = idx / Hq, hq = idx % Hq;
  if (tok >= C) return;
  const int d4 = (threadIdx.x & 15) * 4;
  const int64_t row = (int64_t)(row0 + tok) * Hq + hq;
  const float* ml = part_ml + row * splits * 2;
  float M = -INFINITY;
  for (int z = 0; z < splits; ++z) M = fmaxf(M, ml[z * 2]);
  float L = 0.f;
  kf_f32x4 o = {0.f, 0.f, 0.f, 0.f};
  for (int z = 0; z < splits; ++z) {
    const float mz = ml[z * 2];
    if (mz == -INFINITY) continue;
    const float wz = __expf(mz - M);
    L += ml[z * 2 + 1] * wz;
    const kf_f32x4 v4 = *reinterpret_cast<const kf_f32x4*>(
        part_o + (row * splits + z) * AC_D + d4);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] += v4[j] * wz;
  }
  const float inv_l = L > 0.f ? 1.f / L : 0.f;
  unsigned short q4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) q4[j] = kf_f32_to_bf16(o[j] * inv_l);
  *reinterpret_cast<kf_short4*>(out + row * AC_D + d4) =
      *reinterpret_cast<kf_short4*>(q4);
}

template <int RW, int KW>
static void ac_launch(dim3 grid, hipStream_t stream, void* out, void* part_o,
                      void* part_ml, const void* q, const void* kcache,
                      const void* vcache, const int* slots, const int* starts,
                      const int* lens, int R, int max_rows, int smax,
                      int n_slots, int Hq, int Hkv, int splits, float scale) {
  hipLaunchKernelGGL((kf_attn64_cache_kernel<RW, KW>), grid, dim3(256), 0,
                     stream, (unsigned short*)out, (float*)part_o,
                     (float*)part_ml, (const unsigned short*)q,
                     (const unsigned short*)kcache,
                     (const unsigned short*)vcache, slots, starts, lens, R,
                     max_rows, smax, n_slots, Hq, Hkv, splits, scale);
}

// starts == null: sequence n owns rows [n*max_rows, (n+1)*max_rows).
// splits > 1 requires part_o [R*Hq, splits, 64] f32 and part_ml
// [R*Hq, splits, 2] f32 workspaces; their contents on entry do not matter.
KF_EXPORT int kf_attn64_cache(void* out, void* part_o, void* part_ml,
                              const void* q, const void* kcache,
                              const void* vcache, const int* slots,
                              const int* starts, const int* lens, int64_t N,
                              int64_t R, int64_t max_rows, int64_t smax,
                              int64_t n_slots, int64_t Hq, int64_t Hkv,
                              int64_t D, int64_t splits, float scale,
                              void* stream) {
  if (D != AC_D || Hkv < 1 || Hq % Hkv) return (int)hipErrorInvalidValue;
  const int64_t g = Hq / Hkv;
  if (g != 1 && g != 2 && g != 4 && g != 8) return (int)hipErrorInvalidValue;
  if (N < 0 || R < 0 || max_rows < 0 || smax < 1 || n_slots < 1)
    return (int)hipErrorInvalidValue;
  if (splits < 1 || splits > 64) return (int)hipErrorInvalidValue;
  if (splits > 1 && (!part_o || !part_ml)) return (int)hipErrorInvalidValue;
  if (R > INT32_MAX / Hq / splits || N > 65535 || Hkv * splits > 65535 ||
      smax > INT32_MAX / 2)
    return (int)hipErrorInvalidValue;
  if (N == 0 || R == 0 || max_rows == 0) return (int)hipSuccess;
  max_rows = max_rows < R ? max_rows : R;
  const int64_t rows = max_rows * g;
  const int rw = rows <= 32 ? 1 : rows <= 64 ? 2 : 4;
  dim3 grid((unsigned)((rows + 32 * rw - 1) / (32 * rw)),
            (unsigned)(Hkv * splits), (unsigned)N);
  const hipStream_t st = (hipStream_t)stream;
  if (rw == 1)
    ac_launch<1, 4>(grid, st, out, part_o, part_ml, q, kcache, vcache, slots,
                    starts, lens, (int)R, (int)max_rows, (int)smax,
                    (int)n_slots, (int)Hq, (int)Hkv, (int)splits, scale);
  else if (rw == 2)
    ac_launch<2, 2>(grid, st, out, part_o, part_ml, q, kcache, vcache, slots,
                    starts, lens, (int)R, (int)max_rows, (int)smax,
                    (int)n_slots, (int)Hq, (int)Hkv, (int)splits, scale);
  else
    ac_launch<4, 1>(grid, st, out, part_o, part_ml, q, kcache, vcache, slots,
                    starts, lens, (int)R, (int)max_rows, (int)smax,
                    (int)n_slots, (int)Hq, (int)Hkv, (int)splits, scale);
  if (splits > 1) {
    dim3 cgrid((unsigned)((max_rows * Hq + AC_COMB_ROWS - 1) / AC_COMB_ROWS),
               (unsigned)N);
    hipLaunchKernelGGL(kf_attn64_cache_combine_kernel, cgrid, dim3(256), 0, st,
                       (unsigned short*)out, (const float*)part_o,
                       (const float*)part_ml, starts, (int)R, (int)max_rows,
                       (int)Hq, (int)splits);
  }
  return (int)hipGetLastError();
}

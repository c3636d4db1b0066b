// attention_d64.hip — head-dim-64 flash attention, forward + backward (bf16,
// GQA, optional kv_len or per-sequence-length mask) for CDNA4. The BERT-base
// family: 12 heads x 64.
//
// Contract (every entry point):
//   q/o/dq/dout [B,S,Hq,64], k/v/dk/dv [B,S,Hkv,64] bf16 (bshd); lse/delta
//   [B,Hq,S] fp32; Hq % Hkv == 0; S % 128 == 0; causal in {0,1}; kv_len in
//   [1,S]: key/value rows >= kv_len are never attended (kv_len == S: no
//   mask); causal && kv_len != S is rejected. qts/kts are the token-row
//   strides (elements) of q and of k/v, 0 = contiguous — the strided views of
//   a fused QKV projection are read in place. o, dout, dq, dk, dv are
//   contiguous.
//
// Shape of all three MFMA kernels: 256 threads = 4 waves, a block owns 128
// rows (q rows in fwd/dQ, kv rows in dK/dV), a wave 32 of them; the other
// axis streams through LDS in 64-row tiles. A D = 64 bf16 row is exactly
// 128 B, so every LDS tile — row-major [64 rows][64 d] and transposed
// [64 d][64 rows] alike — is 64 x 128 B with the byte ^= (row&7)<<4 swizzle
// spanning one row. Next-tile global loads are issued before the compute of
// the current tile and written to LDS after it (register prefetch).
//
// Math is the swapped form of kf_attn_fwd4: S^T = mfma(K, Q) puts one q row
// in each lane's accumulator column, so the online-softmax max/sum are
// register reductions plus one shfl_xor(32); P^T/dS^T turn into MFMA
// B-fragments in registers (cvt_pk + permlane32_swap: kf_exchange, derived
// in kf_attn_common.h), never through LDS.
// Softmax runs in the exp2 domain. C/D layout of mfma_f32_32x32x16_bf16:
// col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
//
// Backward is the deterministic two-pass scheme of attention_bwd8.hip (no
// atomics): delta pass, dQ pass (block = q rows), one fused dK+dV pass
// (block = kv rows, loops the GQA group's heads x q tiles). At D = 64 the
// accumulators are half the D = 128 size, so the fused pass keeps dK, dV
// and the persistent K and V fragments all in registers — nothing is parked
// in LDS. The headroom is spent on OCCUPANCY, not on more rows per wave:
// small blocks (16-33 KiB LDS, 2-3 waves/SIMD) so several blocks share a CU
// and cover each other's barriers, which matters at BERT's S = 128..512
// where a block only sees 2-8 tiles.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   fwd   152 VGPRs, scratch 0, LDS 16,384 B, 3 waves/SIMD
//   delta  22 VGPRs, scratch 0, LDS      0 B, 8 waves/SIMD
//   dq    177 VGPRs, scratch 0, LDS 24,576 B, 2 waves/SIMD
//   dkv   245 VGPRs, scratch 0, LDS 33,280 B, 2 waves/SIMD
// (4 waves/SIMD on fwd/dq spilled 104 / 224 B per lane.)
// VARLEN instantiations (per-sequence lengths, below):
//   fwd   165 VGPRs, scratch 0, LDS 16,384 B, 3 waves/SIMD
//   dq    189 VGPRs, scratch 0, LDS 24,576 B, 2 waves/SIMD
//   dkv   211 VGPRs, scratch 0, LDS 33,280 B, 2 waves/SIMD
//
// kv_len: tiles wholly past kv_len are neither loaded nor computed (the
// tile loops end at ceil(kv_len/64); dK/dV blocks wholly past it write
// zeros and exit); the per-element mask runs only on 32-row sub-tiles that
// straddle kv_len or the causal diagonal; dK/dV rows >= kv_len are stored
// as exact zeros.
//
// Per-sequence lengths (kf_attn64_fwd_varlen / kf_attn64_bwd_varlen, the
// <true> instantiations of the three MFMA kernels; non-causal only):
// seq_lens is a device int32 [B] and L = clamp(seq_lens[b], 1, S) is read by
// every block (b = blockIdx.z is block-uniform), so no content of seq_lens
// can cause an out-of-range access or an empty softmax row. Rows >= L are
// padding on BOTH axes: k/v rows >= L never enter the math (the kv_len code
// above with kv_len = L), and o, dq, dk, dv rows >= L are stored as exact
// zeros. Skipped, not masked: a fwd/dQ block with qt*128 >= L stores its
// zeros and returns before any K/V load; in the straddling block, waves
// wholly past L run no MFMA and only take part in staging and the barriers;
// the fused dK/dV pass ends its q-tile loop per head at ceil(L/64). Padded q
// rows inside a live 32-row wave or the last dK/dV q tile are killed through
// lse: the forward stores lse = +inf for rows >= L, so P = exp2(s*scale2 -
// lse2) and with it dS are exactly 0 for those rows in dQ and dK/dV, whatever
// finite values q and dout hold there, without a second per-element mask on
// the q axis (the dK/dV kernel has no registers for one). o = 0 there gives
// delta = 0, so the delta pass is shared unchanged.

#include "kf_attn_common.h"

#define A6_D 64
#define A6_BT 128        // rows owned by a block (4 waves x 32)
#define A6_TT 64         // rows per streamed LDS tile
#define A6_THREADS 256
#define A6_ROWB 128      // bytes per LDS row, both orientations
#define A6_TILEB (A6_TT * A6_ROWB)

// These kernels convert with kf_cvt_pk_bf16_builtin (see kf_attn_common.h),
// so the accumulator -> operand exchange is instantiated on it.
__device__ __forceinline__ kf_bf16x8 kf_exchange_builtin(const kf_f32x16& a,
                                                         int base) {
  return kf_exchange<kf_cvt_pk_bf16_builtin>(a, base);
}

// One 64-row x 64-d tile = 512 b128 vectors, 2 per thread.
struct kf_stage64 {
  kf_short8 x[2];
  __device__ __forceinline__ void load(const unsigned short* g, int64_t ts,
                                       int tid) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int vi = tid + A6_THREADS * j;
      x[j] = *reinterpret_cast<const kf_short8*>(g + (vi >> 3) * ts +
                                                 (vi & 7) * 8);
    }
  }
  // row-major [row][d]
  __device__ __forceinline__ void put_rows(unsigned char* lds, int tid) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int vi = tid + A6_THREADS * j;
      *reinterpret_cast<kf_short8*>(
          lds + kf_swz(vi >> 3, (vi & 7) * 16, A6_ROWB)) = x[j];
    }
  }
  // transposed [d][row]: thread (r, c8) scatters its 8 d values down one
  // column. The vector is first rotated by c8 elements in registers (static
  // indices afterwards) so the lanes of a wave that share r hit 8 different
  // swizzle phases instead of one bank group.
  __device__ __forceinline__ void put_cols(unsigned char* lds, int tid) const {
    const int s = tid & 7;  // == c8 for both vectors
    const unsigned sh = (unsigned)(s & 1) * 16u;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = (tid + A6_THREADS * j) >> 3;
      const unsigned int* u = reinterpret_cast<const unsigned int*>(&x[j]);
      const unsigned t0 = (s & 2) ? u[1] : u[0], t1 = (s & 2) ? u[2] : u[1];
      const unsigned t2 = (s & 2) ? u[3] : u[2], t3 = (s & 2) ? u[0] : u[3];
      const unsigned v0 = (s & 4) ? t2 : t0, v1 = (s & 4) ? t3 : t1;
      const unsigned v2 = (s & 4) ? t0 : t2, v3 = (s & 4) ? t1 : t3;
      const unsigned y[4] = {__builtin_amdgcn_alignbit(v1, v0, sh),
                             __builtin_amdgcn_alignbit(v2, v1, sh),
                             __builtin_amdgcn_alignbit(v3, v2, sh),
                             __builtin_amdgcn_alignbit(v0, v3, sh)};
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {  // y element jj == x element (jj+s)&7
        const int dd = s * 8 + ((jj + s) & 7);
        *reinterpret_cast<unsigned short*>(lds + kf_swz(dd, r * 2, A6_ROWB)) =
            (unsigned short)(y[jj >> 1] >> ((jj & 1) * 16));
      }
    }
  }
};

// A-fragment of a 32-row sub-tile: rows sub*32 + (lane&31), k-chunk kk
#define A6_AFRAG(lds, sub, kk)                                  \
  (*reinterpret_cast<const kf_bf16x8*>(                         \
      (lds) + kf_swz((sub) * 32 + l31, (kk) * 32 + hi * 16, A6_ROWB)))

// acc^T[d][n] (4 consecutive d per register quad) -> one bf16 row of 64
__device__ __forceinline__ void kf_store_row64(unsigned short* dst,
                                               const kf_f32x16 (&acc)[2],
                                               int hi, float mul) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      unsigned int u[2] = {
          kf_cvt_pk_bf16_builtin(acc[dt][rq * 4 + 0] * mul,
                                 acc[dt][rq * 4 + 1] * mul),
          kf_cvt_pk_bf16_builtin(acc[dt][rq * 4 + 2] * mul,
                                 acc[dt][rq * 4 + 3] * mul)};
      *reinterpret_cast<kf_short4*>(dst + dt * 32 + 8 * rq + 4 * hi) =
          *reinterpret_cast<kf_short4*>(u);
    }
}

// The length argument of the MFMA kernels: the scalar kv_len, or, in the
// VARLEN instantiations, the device array of per-sequence lengths. Keeping it
// one parameter of a dependent type leaves the scalar instantiations with the
// parameter list and the code they had before VARLEN existed.
template <bool VARLEN> struct kf_len_arg { typedef int type; };
template <> struct kf_len_arg<true> { typedef const int* type; };
__device__ __forceinline__ int kf_len(int kv_len, int64_t, int) {
  return kv_len;
}
// seq_lens[b] clamped into [1, S] as it is read: memory safety, not validation
__device__ __forceinline__ int kf_len(const int* seq_lens, int64_t b, int S) {
  return min(max(seq_lens[b], 1), S);
}

// ---------------------------------------------------------------- forward --
template <bool VARLEN>
__global__ __launch_bounds__(A6_THREADS, 3) void kf_attn64_fwd_kernel(
    unsigned short* __restrict__ o, float* __restrict__ lse,
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, int S, int Hq, int Hkv, int64_t qts,
    int64_t kts, float scale, int causal_arg,
    typename kf_len_arg<VARLEN>::type len_arg) {
  __shared__ __attribute__((aligned(16))) unsigned char k_lds[A6_TILEB];
  __shared__ __attribute__((aligned(16))) unsigned char vt_lds[A6_TILEB];

  const int qt = blockIdx.x, hq = blockIdx.y;
  const int64_t b = blockIdx.z;
  const int hkv = hq / (Hq / Hkv);
  const int tid = threadIdx.x;
  const int w = tid / KF_WAVE;
  const int lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave_qmin = qt * A6_BT + w * 32;
  const int qrow_g = wave_qmin + l31;
  const float scale2 = scale * KF_LOG2E;
  // VARLEN is non-causal; the length bounds the q axis as well as the kv axis
  const int causal = VARLEN ? 0 : causal_arg;
  const int kv_len = kf_len(len_arg, b, S);

  if constexpr (VARLEN) {
    if (qt * A6_BT >= kv_len) {  // block-uniform: all rows padding
      const kf_f32x16 zero[2] = {kf_f32x16{0.f}, kf_f32x16{0.f}};
      kf_store_row64(o + ((b * S + qrow_g) * (int64_t)Hq + hq) * A6_D, zero,
                     hi, 0.f);
      if (hi == 0) lse[(b * Hq + hq) * (int64_t)S + qrow_g] = INFINITY;
      return;
    }
  }
  // waves wholly past the length only help staging (wave-uniform)
  const bool wave_live = !VARLEN || wave_qmin < kv_len;

  // persistent Q B-fragments: B[k=d][n=q], this lane holds q row qrow_g
  kf_bf16x8 qfrag[4];
  {
    const unsigned short* qp = q + (b * S + qrow_g) * qts + (int64_t)hq * A6_D;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      qfrag[kk] = *reinterpret_cast<const kf_bf16x8*>(qp + kk * 16 + hi * 8);
  }

  kf_f32x16 oacc[2] = {kf_f32x16{0.f}, kf_f32x16{0.f}};
  float m_run = -INFINITY, l_run = 0.f;  // m in the scaled log2 domain

  // kv rows this block needs: [0, blk_end); this wave: [0, kv_lim)
  const int blk_end = causal ? qt * A6_BT + A6_BT : kv_len;
  const int kv_lim = causal ? wave_qmin + 32 : kv_len;
  const int n_kt = (blk_end + A6_TT - 1) / A6_TT;
  const unsigned short* kg0 = k + (b * S) * kts + (int64_t)hkv * A6_D;
  const unsigned short* vg0 = v + (b * S) * kts + (int64_t)hkv * A6_D;

  kf_stage64 ks, vs;
  ks.load(kg0, kts, tid);
  vs.load(vg0, kts, tid);
  for (int kt = 0; kt < n_kt; ++kt) {
    ks.put_rows(k_lds, tid);
    vs.put_cols(vt_lds, tid);
    __syncthreads();
    if (kt + 1 < n_kt) {
      ks.load(kg0 + (int64_t)(kt + 1) * A6_TT * kts, kts, tid);
      vs.load(vg0 + (int64_t)(kt + 1) * A6_TT * kts, kts, tid);
    }

#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int kv_lo = kt * A6_TT + mt * 32;
      if (kv_lo >= kv_lim) continue;  // wave-uniform: fully masked sub-tile
      if constexpr (VARLEN)
        if (!wave_live) continue;
      // S^T = mfma(K, Q): rows kv, cols q
      kf_f32x16 st = kf_f32x16{0.f};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A6_AFRAG(k_lds, mt, kk),
                                                     qfrag[kk], st, 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);

      const int kv0 = kv_lo + hi * 4;
      const bool need_mask =
          causal ? (kv_lo + 31 > wave_qmin) : (kv_lo + 32 > kv_len);
      float mx = -INFINITY;
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + (r & 3) + 8 * (r >> 2);
          const bool dead = causal ? (kv > qrow_g) : (kv >= kv_len);
          st[r] = dead ? -INFINITY : st[r] * scale2;
          mx = fmaxf(mx, st[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          st[r] *= scale2;
          mx = fmaxf(mx, st[r]);
        }
      }
      // kv row 0 is live for every q row and sits in the first sub-tile, so
      // m_new is finite from the first update on: no -inf - -inf below
      mx = fmaxf(mx, __shfl_xor(mx, 32, KF_WAVE));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      float lsum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[r] = __builtin_amdgcn_exp2f(st[r] - m_new);
        lsum += st[r];
      }
      lsum += __shfl_xor(lsum, 32, KF_WAVE);
      l_run = l_run * alpha + lsum;
      m_run = m_new;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;

      const kf_bf16x8 pb[2] = {kf_exchange_builtin(st, 0),
                               kf_exchange_builtin(st, 8)};
      // O^T += V^T P^T
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int step = 0; step < 2; ++step)
          oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              A6_AFRAG(vt_lds, dt, mt * 2 + step), pb[step], oacc[dt], 0, 0,
              0);
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();  // all waves done with the tile before it is overwritten
  }

  if constexpr (VARLEN) {
    // padded q row: exact zeros, and lse = +inf makes P = exp2(s - lse)
    // exactly 0 for this row in both backward passes
    const bool pad = qrow_g >= kv_len;
    if (pad) oacc[0] = oacc[1] = kf_f32x16{0.f};
    kf_store_row64(o + ((b * S + qrow_g) * (int64_t)Hq + hq) * A6_D, oacc, hi,
                   pad ? 0.f : 1.f / l_run);
    if (hi == 0)
      lse[(b * Hq + hq) * (int64_t)S + qrow_g] =
          pad ? INFINITY : m_run * KF_LN2 + __logf(l_run);
    return;
  }
  kf_store_row64(o + ((b * S + qrow_g) * (int64_t)Hq + hq) * A6_D, oacc, hi,
                 1.f / l_run);
  if (hi == 0)
    lse[(b * Hq + hq) * (int64_t)S + qrow_g] =
        m_run * KF_LN2 + __logf(l_run);
}

// ------------------------------------------------------------- pass delta --
// delta[b,hq,s] = sum_d o * dout; 8 lanes per 64-wide row.
__global__ __launch_bounds__(A6_THREADS) void kf_attn64_delta_kernel(
    float* __restrict__ delta, const unsigned short* __restrict__ o,
    const unsigned short* __restrict__ dout, int64_t rows, int S, int Hq) {
  const int64_t row = (int64_t)blockIdx.x * (A6_THREADS / 8) + threadIdx.x / 8;
  const int c8 = threadIdx.x & 7;
  float acc = 0.f;
  if (row < rows) {
    const kf_short8 a =
        *reinterpret_cast<const kf_short8*>(o + row * A6_D + c8 * 8);
    const kf_short8 d =
        *reinterpret_cast<const kf_short8*>(dout + row * A6_D + c8 * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      acc += kf_bf16_to_f32((unsigned short)a[j]) *
             kf_bf16_to_f32((unsigned short)d[j]);
  }
#pragma unroll
  for (int off = 4; off > 0; off >>= 1) acc += __shfl_xor(acc, off, KF_WAVE);
  if (row < rows && c8 == 0) {
    const int hq = (int)(row % Hq);
    const int64_t bs = row / Hq;  // b * S + s
    delta[((bs / S) * Hq + hq) * (int64_t)S + bs % S] = acc;
  }
}

// ---------------------------------------------------------------- pass dQ --
//   S^T = mfma(K, Q), dP^T = mfma(V, dO)
//   dS^T = P^T o (dP^T - delta) * scale           (registers)
//   dQ^T += mfma(K^T, exch(dS^T))                 K^T from the transposed tile
template <bool VARLEN>
__global__ __launch_bounds__(A6_THREADS, 2) void kf_attn64_dq_kernel(
    unsigned short* __restrict__ dq, const unsigned short* __restrict__ q,
    const unsigned short* __restrict__ k, const unsigned short* __restrict__ v,
    const unsigned short* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, int S, int Hq, int Hkv, int64_t qts,
    int64_t kts, float scale, int causal_arg,
    typename kf_len_arg<VARLEN>::type len_arg) {
  __shared__ __attribute__((aligned(16))) unsigned char k_lds[A6_TILEB];
  __shared__ __attribute__((aligned(16))) unsigned char v_lds[A6_TILEB];
  __shared__ __attribute__((aligned(16))) unsigned char kt_lds[A6_TILEB];

  const int qt = blockIdx.x, hq = blockIdx.y;
  const int64_t b = blockIdx.z;
  const int hkv = hq / (Hq / Hkv);
  const int tid = threadIdx.x;
  const int w = tid / KF_WAVE;
  const int lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave_qmin = qt * A6_BT + w * 32;
  const int qrow_g = wave_qmin + l31;
  const float scale2 = scale * KF_LOG2E;
  // VARLEN is non-causal; the length bounds the q axis as well as the kv axis
  const int causal = VARLEN ? 0 : causal_arg;
  const int kv_len = kf_len(len_arg, b, S);

  if constexpr (VARLEN) {
    if (qt * A6_BT >= kv_len) {  // block-uniform: all rows padding
      const kf_f32x16 zero[2] = {kf_f32x16{0.f}, kf_f32x16{0.f}};
      kf_store_row64(dq + ((b * S + qrow_g) * (int64_t)Hq + hq) * A6_D, zero,
                     hi, 0.f);
      return;
    }
  }
  const bool wave_live = !VARLEN || wave_qmin < kv_len;  // wave-uniform

  kf_bf16x8 qfrag[4], dofrag[4];
  {
    const unsigned short* qp = q + (b * S + qrow_g) * qts + (int64_t)hq * A6_D;
    const unsigned short* dp =
        dout + ((b * S + qrow_g) * (int64_t)Hq + hq) * A6_D;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      qfrag[kk] = *reinterpret_cast<const kf_bf16x8*>(qp + kk * 16 + hi * 8);
      dofrag[kk] = *reinterpret_cast<const kf_bf16x8*>(dp + kk * 16 + hi * 8);
    }
  }
  const float lse2_q = lse[(b * Hq + hq) * (int64_t)S + qrow_g] * KF_LOG2E;
  const float dlt_q = delta[(b * Hq + hq) * (int64_t)S + qrow_g];

  kf_f32x16 dqacc[2] = {kf_f32x16{0.f}, kf_f32x16{0.f}};

  const int blk_end = causal ? qt * A6_BT + A6_BT : kv_len;
  const int kv_lim = causal ? wave_qmin + 32 : kv_len;
  const int n_kt = (blk_end + A6_TT - 1) / A6_TT;
  const unsigned short* kg0 = k + (b * S) * kts + (int64_t)hkv * A6_D;
  const unsigned short* vg0 = v + (b * S) * kts + (int64_t)hkv * A6_D;

  kf_stage64 ks, vs;
  ks.load(kg0, kts, tid);
  vs.load(vg0, kts, tid);
  for (int kt = 0; kt < n_kt; ++kt) {
    ks.put_rows(k_lds, tid);
    ks.put_cols(kt_lds, tid);
    vs.put_rows(v_lds, tid);
    __syncthreads();
    if (kt + 1 < n_kt) {
      ks.load(kg0 + (int64_t)(kt + 1) * A6_TT * kts, kts, tid);
      vs.load(vg0 + (int64_t)(kt + 1) * A6_TT * kts, kts, tid);
    }

#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int kv_lo = kt * A6_TT + mt * 32;
      if (kv_lo >= kv_lim) continue;  // wave-uniform skip
      if constexpr (VARLEN)
        if (!wave_live) continue;
      kf_f32x16 st = kf_f32x16{0.f}, dpt = kf_f32x16{0.f};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A6_AFRAG(k_lds, mt, kk),
                                                     qfrag[kk], st, 0, 0, 0);
        dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A6_AFRAG(v_lds, mt, kk),
                                                      dofrag[kk], dpt, 0, 0,
                                                      0);
      }
      __builtin_amdgcn_s_setprio(0);

      const int kv0 = kv_lo + hi * 4;
      const bool need_mask =
          causal ? (kv_lo + 31 > wave_qmin) : (kv_lo + 32 > kv_len);
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + (r & 3) + 8 * (r >> 2);
          const bool dead = causal ? (kv > qrow_g) : (kv >= kv_len);
          const float p =
              dead ? 0.f : __builtin_amdgcn_exp2f(st[r] * scale2 - lse2_q);
          st[r] = p * (dpt[r] - dlt_q) * scale;  // dS^T
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = __builtin_amdgcn_exp2f(st[r] * scale2 - lse2_q);
          st[r] = p * (dpt[r] - dlt_q) * scale;
        }
      }
      const kf_bf16x8 pb[2] = {kf_exchange_builtin(st, 0),
                               kf_exchange_builtin(st, 8)};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int step = 0; step < 2; ++step)
          dqacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              A6_AFRAG(kt_lds, dt, mt * 2 + step), pb[step], dqacc[dt], 0, 0,
              0);
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
  }

  // padded q rows: lse = +inf from the forward already made every dS 0; the
  // select keeps the zeros exact whatever dout holds there
  if constexpr (VARLEN)
    if (qrow_g >= kv_len) dqacc[0] = dqacc[1] = kf_f32x16{0.f};
  kf_store_row64(dq + ((b * S + qrow_g) * (int64_t)Hq + hq) * A6_D, dqacc, hi,
                 1.f);
}

// --------------------------------------------------------- fused pass dKV --
// block = (b, hkv, 128 kv rows), wave = 32 kv rows, lane = one kv row; loops
// the GQA group's heads x 64-row q tiles (ascending, so the summation order
// per kv row is fixed):
//   S = mfma(Q, K), dP = mfma(dO, V)       K/V persistent B-fragments
//   dV^T += mfma(dO^T, exch(P))            dO^T, Q^T from transposed tiles
//   dK^T += mfma(Q^T, exch(dS))
template <bool VARLEN>
__global__ __launch_bounds__(A6_THREADS, 2) void kf_attn64_dkv_kernel(
    unsigned short* __restrict__ dk, unsigned short* __restrict__ dv,
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v,
    const unsigned short* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, int S, int Hq, int Hkv, int64_t qts,
    int64_t kts, float scale, int causal_arg,
    typename kf_len_arg<VARLEN>::type len_arg) {
  __shared__ __attribute__((aligned(16))) unsigned char q_lds[A6_TILEB];
  __shared__ __attribute__((aligned(16))) unsigned char do_lds[A6_TILEB];
  __shared__ __attribute__((aligned(16))) unsigned char qt_lds[A6_TILEB];
  __shared__ __attribute__((aligned(16))) unsigned char dot_lds[A6_TILEB];
  __shared__ float lse_s[A6_TT], dlt_s[A6_TT];  // lse pre-multiplied by log2e

  const int kt = blockIdx.x, hkv = blockIdx.y;
  const int64_t b = blockIdx.z;
  const int g = Hq / Hkv;
  const int tid = threadIdx.x;
  const int w = tid / KF_WAVE;
  const int lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave_kv_min = kt * A6_BT + w * 32;
  const int kvrow_g = wave_kv_min + l31;
  const float scale2 = scale * KF_LOG2E;
  // VARLEN is non-causal; the length bounds the q axis as well as the kv axis
  const int causal = VARLEN ? 0 : causal_arg;
  const int kv_len = kf_len(len_arg, b, S);
  unsigned short* dkp = dk + ((b * S + kvrow_g) * (int64_t)Hkv + hkv) * A6_D;
  unsigned short* dvp = dv + ((b * S + kvrow_g) * (int64_t)Hkv + hkv) * A6_D;

  kf_f32x16 dkacc[2] = {kf_f32x16{0.f}, kf_f32x16{0.f}};
  kf_f32x16 dvacc[2] = {kf_f32x16{0.f}, kf_f32x16{0.f}};

  if (kt * A6_BT >= kv_len) {  // block-uniform: tile wholly past kv_len
    kf_store_row64(dkp, dkacc, hi, 0.f);
    kf_store_row64(dvp, dvacc, hi, 0.f);
    return;
  }
  // waves wholly past kv_len only help staging (wave-uniform)
  const bool wave_live = wave_kv_min < kv_len;

  kf_bf16x8 kbf[4], vbf[4];  // persistent B-fragments: B[k=d][n=kv]
  {
    const unsigned short* kp = k + (b * S + kvrow_g) * kts + (int64_t)hkv * A6_D;
    const unsigned short* vp = v + (b * S + kvrow_g) * kts + (int64_t)hkv * A6_D;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      kbf[kk] = *reinterpret_cast<const kf_bf16x8*>(kp + kk * 16 + hi * 8);
      vbf[kk] = *reinterpret_cast<const kf_bf16x8*>(vp + kk * 16 + hi * 8);
    }
  }

  const int qt0 = causal ? (kt * A6_BT) / A6_TT : 0;
  // VARLEN: q tiles wholly past the length are not visited; q rows >= the
  // length inside the last tile carry lse = +inf, so P and dS are exactly 0
  // for them with no mask on the q axis
  const int per_head =
      (VARLEN ? (kv_len + A6_TT - 1) / A6_TT : S / A6_TT) - qt0;
  const int total = g * per_head;

  kf_stage64 qs, ds;
  float rc_ld = 0.f;  // row constant: lse (tid < 64) or delta (tid < 128)
  auto stage_load = [&](int flat) {
    const int hq = hkv * g + flat / per_head;
    const int64_t row0 = b * S + (int64_t)(qt0 + flat % per_head) * A6_TT;
    qs.load(q + row0 * qts + (int64_t)hq * A6_D, qts, tid);
    ds.load(dout + (row0 * Hq + hq) * A6_D, (int64_t)Hq * A6_D, tid);
    if (tid < 2 * A6_TT) {
      const float* rc = tid < A6_TT ? lse : delta;
      rc_ld = rc[(b * Hq + hq) * (int64_t)S + (row0 - b * S) +
                 (tid & (A6_TT - 1))];
    }
  };

  stage_load(0);
  for (int flat = 0; flat < total; ++flat) {
    qs.put_rows(q_lds, tid);
    qs.put_cols(qt_lds, tid);
    ds.put_rows(do_lds, tid);
    ds.put_cols(dot_lds, tid);
    if (tid < A6_TT) lse_s[tid] = rc_ld * KF_LOG2E;
    else if (tid < 2 * A6_TT) dlt_s[tid - A6_TT] = rc_ld;
    __syncthreads();
    if (flat + 1 < total) stage_load(flat + 1);
    const int q_tile0 = (qt0 + flat % per_head) * A6_TT;

    if (wave_live) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const int q_lo = q_tile0 + mt * 32;
        // causal: contributes iff some q >= kv in this wave
        if (causal && q_lo + 31 < wave_kv_min) continue;
        kf_f32x16 sacc = kf_f32x16{0.f}, dpacc = kf_f32x16{0.f};
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              A6_AFRAG(q_lds, mt, kk), kbf[kk], sacc, 0, 0, 0);
          dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              A6_AFRAG(do_lds, mt, kk), vbf[kk], dpacc, 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);

        const int ql0 = mt * 32 + hi * 4;  // q-tile-local
        const bool need_mask = causal ? (q_lo <= wave_kv_min + 31)
                                      : (wave_kv_min + 32 > kv_len);
        if (need_mask) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ql = ql0 + (r & 3) + 8 * (r >> 2);
            const bool dead =
                causal ? (kvrow_g > q_tile0 + ql) : (kvrow_g >= kv_len);
            sacc[r] = dead ? 0.f
                           : __builtin_amdgcn_exp2f(sacc[r] * scale2 -
                                                    lse_s[ql]);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ql = ql0 + (r & 3) + 8 * (r >> 2);
            sacc[r] = __builtin_amdgcn_exp2f(sacc[r] * scale2 - lse_s[ql]);
          }
        }
        const kf_bf16x8 pb[2] = {kf_exchange_builtin(sacc, 0),
                                 kf_exchange_builtin(sacc, 8)};
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = ql0 + (r & 3) + 8 * (r >> 2);
          sacc[r] = sacc[r] * (dpacc[r] - dlt_s[ql]) * scale;  // dS
        }
        const kf_bf16x8 db[2] = {kf_exchange_builtin(sacc, 0),
                                 kf_exchange_builtin(sacc, 8)};
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int step = 0; step < 2; ++step) {
            dvacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                A6_AFRAG(dot_lds, dt, mt * 2 + step), pb[step], dvacc[dt], 0,
                0, 0);
            dkacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                A6_AFRAG(qt_lds, dt, mt * 2 + step), db[step], dkacc[dt], 0,
                0, 0);
          }
        __builtin_amdgcn_s_setprio(0);
      }
    }
    __syncthreads();
  }

  // rows >= kv_len are stored as exact zeros
  if (kvrow_g >= kv_len)
    dkacc[0] = dkacc[1] = dvacc[0] = dvacc[1] = kf_f32x16{0.f};
  kf_store_row64(dkp, dkacc, hi, 1.f);
  kf_store_row64(dvp, dvacc, hi, 1.f);
}

// ----------------------------------------------------------- entry points --
static int kf_attn64_args_bad(int64_t B, int64_t S, int64_t Hq, int64_t Hkv,
                              int causal, int64_t kv_len) {
  if (B < 1 || B > 65535 || S < A6_BT || S % A6_BT || S > (1 << 24) ||
      Hq < 1 || Hq > 65535 || Hkv < 1 || Hq % Hkv)
    return 1;
  if (causal != 0 && causal != 1) return 1;
  if (kv_len < 1 || kv_len > S) return 1;
  if (causal && kv_len != S) return 1;
  return 0;
}

KF_EXPORT int kf_attn64_fwd(void* o, float* lse, const void* q, const void* k,
                            const void* v, int64_t B, int64_t S, int64_t Hq,
                            int64_t Hkv, int64_t qts, int64_t kts, float scale,
                            int causal, int64_t kv_len, void* stream) {
  if (kf_attn64_args_bad(B, S, Hq, Hkv, causal, kv_len))
    return (int)hipErrorInvalidValue;
  if (qts == 0) qts = Hq * A6_D;
  if (kts == 0) kts = Hkv * A6_D;
  dim3 grid((unsigned)(S / A6_BT), (unsigned)Hq, (unsigned)B);
  hipLaunchKernelGGL(kf_attn64_fwd_kernel<false>, grid, dim3(A6_THREADS), 0,
                     (hipStream_t)stream, (unsigned short*)o, lse,
                     (const unsigned short*)q, (const unsigned short*)k,
                     (const unsigned short*)v, (int)S, (int)Hq, (int)Hkv, qts,
                     kts, scale, causal, (int)kv_len);
  return (int)hipGetLastError();
}

// three launches: delta, dQ, fused dK+dV
KF_EXPORT int kf_attn64_bwd(void* dq, void* dk, void* dv, const void* dout,
                            const void* q, const void* k, const void* v,
                            const void* o, const float* lse, float* delta,
                            int64_t B, int64_t S, int64_t Hq, int64_t Hkv,
                            int64_t qts, int64_t kts, float scale, int causal,
                            int64_t kv_len, void* stream) {
  if (kf_attn64_args_bad(B, S, Hq, Hkv, causal, kv_len))
    return (int)hipErrorInvalidValue;
  if (qts == 0) qts = Hq * A6_D;
  if (kts == 0) kts = Hkv * A6_D;
  const int64_t rows = B * S * Hq;
  const int64_t dblocks = (rows + A6_THREADS / 8 - 1) / (A6_THREADS / 8);
  if (dblocks > 0x7fffffff) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kf_attn64_delta_kernel, dim3((unsigned)dblocks),
                     dim3(A6_THREADS), 0, (hipStream_t)stream, delta,
                     (const unsigned short*)o, (const unsigned short*)dout,
                     rows, (int)S, (int)Hq);
  int err = (int)hipGetLastError();
  if (err) return err;
  dim3 gq((unsigned)(S / A6_BT), (unsigned)Hq, (unsigned)B);
  hipLaunchKernelGGL(kf_attn64_dq_kernel<false>, gq, dim3(A6_THREADS), 0,
                     (hipStream_t)stream, (unsigned short*)dq,
                     (const unsigned short*)q, (const unsigned short*)k,
                     (const unsigned short*)v, (const unsigned short*)dout,
                     lse, (const float*)delta, (int)S, (int)Hq, (int)Hkv, qts,
                     kts, scale, causal, (int)kv_len);
  err = (int)hipGetLastError();
  if (err) return err;
  dim3 gkv((unsigned)(S / A6_BT), (unsigned)Hkv, (unsigned)B);
  hipLaunchKernelGGL(kf_attn64_dkv_kernel<false>, gkv, dim3(A6_THREADS), 0,
                     (hipStream_t)stream, (unsigned short*)dk,
                     (unsigned short*)dv, (const unsigned short*)q,
                     (const unsigned short*)k, (const unsigned short*)v,
                     (const unsigned short*)dout, lse, (const float*)delta,
                     (int)S, (int)Hq, (int)Hkv, qts, kts, scale, causal,
                     (int)kv_len);
  return (int)hipGetLastError();
}

// ------------------------------------------ per-sequence lengths (VARLEN) --
// seq_lens: device int32 [B]. Non-causal. Same three backward launches; o and
// lse must come from kf_attn64_fwd_varlen with the same seq_lens.
KF_EXPORT int kf_attn64_fwd_varlen(void* o, float* lse, const void* q,
                                   const void* k, const void* v,
                                   const int32_t* seq_lens, int64_t B,
                                   int64_t S, int64_t Hq, int64_t Hkv,
                                   int64_t qts, int64_t kts, float scale,
                                   void* stream) {
  if (!seq_lens || kf_attn64_args_bad(B, S, Hq, Hkv, 0, S))
    return (int)hipErrorInvalidValue;
  if (qts == 0) qts = Hq * A6_D;
  if (kts == 0) kts = Hkv * A6_D;
  dim3 grid((unsigned)(S / A6_BT), (unsigned)Hq, (unsigned)B);
  hipLaunchKernelGGL(kf_attn64_fwd_kernel<true>, grid, dim3(A6_THREADS), 0,
                     (hipStream_t)stream, (unsigned short*)o, lse,
                     (const unsigned short*)q, (const unsigned short*)k,
                     (const unsigned short*)v, (int)S, (int)Hq, (int)Hkv, qts,
                     kts, scale, 0, (const int*)seq_lens);
  return (int)hipGetLastError();
}

KF_EXPORT int kf_attn64_bwd_varlen(void* dq, void* dk, void* dv,
                                   const void* dout, const void* q,
                                   const void* k, const void* v, const void* o,
                                   const float* lse, float* delta,
                                   const int32_t* seq_lens, int64_t B,
                                   int64_t S, int64_t Hq, int64_t Hkv,
                                   int64_t qts, int64_t kts, float scale,
                                   void* stream) {
  if (!seq_lens || kf_attn64_args_bad(B, S, Hq, Hkv, 0, S))
    return (int)hipErrorInvalidValue;
  if (qts == 0) qts = Hq * A6_D;
  if (kts == 0) kts = Hkv * A6_D;
  const int64_t rows = B * S * Hq;
  const int64_t dblocks = (rows + A6_THREADS / 8 - 1) / (A6_THREADS / 8);
  if (dblocks > 0x7fffffff) return (int)hipErrorInvalidValue;
  // padded rows have o = 0, hence delta = 0: the delta pass is unchanged
  hipLaunchKernelGGL(kf_attn64_delta_kernel, dim3((unsigned)dblocks),
                     dim3(A6_THREADS), 0, (hipStream_t)stream, delta,
                     (const unsigned short*)o, (const unsigned short*)dout,
                     rows, (int)S, (int)Hq);
  int err = (int)hipGetLastError();
  if (err) return err;
  dim3 gq((unsigned)(S / A6_BT), (unsigned)Hq, (unsigned)B);
  hipLaunchKernelGGL(kf_attn64_dq_kernel<true>, gq, dim3(A6_THREADS), 0,
                     (hipStream_t)stream, (unsigned short*)dq,
                     (const unsigned short*)q, (const unsigned short*)k,
                     (const unsigned short*)v, (const unsigned short*)dout,
                     lse, (const float*)delta, (int)S, (int)Hq, (int)Hkv, qts,
                     kts, scale, 0, (const int*)seq_lens);
  err = (int)hipGetLastError();
  if (err) return err;
  dim3 gkv((unsigned)(S / A6_BT), (unsigned)Hkv, (unsigned)B);
  hipLaunchKernelGGL(kf_attn64_dkv_kernel<true>, gkv, dim3(A6_THREADS), 0,
                     (hipStream_t)stream, (unsigned short*)dk,
                     (unsigned short*)dv, (const unsigned short*)q,
                     (const unsigned short*)k, (const unsigned short*)v,
                     (const unsigned short*)dout, lse, (const float*)delta,
                     (int)S, (int)Hq, (int)Hkv, qts, kts, scale, 0,
                     (const int*)seq_lens);
  return (int)hipGetLastError();
}

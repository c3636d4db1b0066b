// attention_bwd8.hip — 8-wave swapped flash-attention backward (bf16, GQA).
//
// Round-2 rework applying the techniques HW-verified on the v4 forward
// (attention_fwd4.hip — ablation + PMC on MI355X):
//  * every transpose-scatter staging path (round 1: 8 scalar ds_writes per
//    staged vector; 30k LDS conflict-cycles/wave in dk8) is replaced by the
//    [d/16-slab][r/4-tile][4][16] SUBTILED layout: staged with plain b128
//    writes and consumed BOTH as row-chunk b128 reads (MFMA A/B row
//    operands) and via ds_read_b64_tr_b16 (hardware transpose, guide T10;
//    lane mapping verified by scripts/probe_tr16.py);
//  * all tiles are DOUBLE-BUFFERED with the async-STAGE split (T14): next
//    tile's global loads issue before compute, LDS writes after, one
//    barrier per tile;
//  * P recomputation runs in the exp2 domain (lse is staged pre-multiplied
//    by log2e; one v_exp_f32 per element);
//  * transpose MFMA feeds use a 1-deep tr_read prefetch with counted
//    lgkmcnt; diagonal sub-blocks only pay the causal mask; fully-masked
//    32-row sub-blocks are skipped per wave.
//
// exch() below is kf_exchange, tr() a KF_TR16 read inside kf_tr_acc_loop; the
// lane-level derivation of both is in kf_attn_common.h.
//
// pass dQ (block = b, hq, 256-row q-tile; wave = 32 q rows):
//   S^T = mfma(K, Q), dP^T = mfma(V, dO)      K/V subtiled in LDS
//   dS^T = P^T ∘ (dP^T − delta) · scale       (registers; P via exp2)
//   dQ^T += mfma(tr(K), exch(dS^T))
//
// pass dKV (block = b, hkv, 256-row kv-tile; wave = 32 kv rows; loops the
// GQA group's heads × 64-row q-tiles):
//   S = mfma(Q, K), dP = mfma(dO, V)          Q/dO subtiled in LDS
//   dV += mfma(exch(P), tr(dO)) ; dK += mfma(exch(dS), tr(Q))
// Default: ONE fused kernel, kf_attn_dkv8f (32 MFMAs per 32x32 sub-block).
// Rounds 1-2 split it into dv8 + dk8 (16 + 24 MFMAs, Q/dO streamed and S,
// exp2 computed twice) because carrying both accumulators spilled 62 VGPRs.
// That attempt already ran at the 256-register budget — launch_bounds'
// second argument is waves per SIMD, and dk8 alone takes 252 — so the fused
// kernel does not get a bigger budget, it needs fewer registers: V
// fragments parked in LDS, one staging register for lse/delta, 32-bit
// staging offsets (255 VGPRs, scratch 0; details at the kernel).
// Measured on MI355X, B7 S4096 Hq32 Hkv8 causal: dv8 + dk8 3.21 ms, dkv8f
// 2.26 ms per call, bit-identical dK/dV; llama3-8b train step 1368.6 ->
// 1334.9 ms (profiles/r03_attn_bwd_fused.md). The split pair stays as the
// bit-exact reference the tests hold dkv8f to (kf_attn_bwd8_dkv[_rope]);
// kf_attn_bwd never launches it.
//
// The dq8, dk8 and dkv8f store epilogues optionally apply the RoPE adjoint
// (cost/sint != nullptr): acc[dt] and acc[dt+2] hold the rotate-half pair
// (d, d+64) in one lane, so the separate kf_rope(backward=1) pass over
// dq/dk is not needed.

#include "kf_attn_common.h"

#define AB_D 128

// row-chunk b128 read address in a subtiled 64-row tile (kf_vsub<64>):
// elements (r, d0..d0+8), d0 % 8 == 0
__device__ __forceinline__ int kf_subrow(int r, int byte_in_row) {
  return 2 * kf_vsub<64>(r, byte_in_row >> 1);
}

// RoPE adjoint on one rotate-half pair (d, d+64) held as fp32 accumulators.
// Rounds to bf16 FIRST, then applies the inverse rotation with the same
// mul + fma forms kf_rope_kernel(backward=1) compiles to, so "rotate in the
// store epilogue" is bit-identical to "store bf16, then kf_rope".
#define KF_ROPE_ADJ_PAIR(x1, x2, c, s)                                \
  {                                                                   \
    const float a_ = kf_bf16_to_f32(kf_f32_to_bf16(x1));              \
    const float b_ = kf_bf16_to_f32(kf_f32_to_bf16(x2));              \
    const float t1_ = b_ * (s), t2_ = a_ * (s);                       \
    (x1) = __builtin_fmaf(a_, (c), t1_);                              \
    (x2) = __builtin_fmaf(b_, (c), -t2_);                             \
  }

// ---------------------------------------------------------------- pass dQ --
#define DQ8_QT 256
#define DQ8_KT 64

__global__ __launch_bounds__(512, 2) void kf_attn_dq8_kernel(
    unsigned short* __restrict__ dq, const unsigned short* __restrict__ q,
    const unsigned short* __restrict__ k, const unsigned short* __restrict__ v,
    const unsigned short* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, int64_t B, int S, int Hq, int Hkv,
    int64_t qts, int64_t kts, int64_t dqts, float scale, int causal,
    const float* __restrict__ cost, const float* __restrict__ sint,
    int64_t pos_offset) {
  __shared__ unsigned char k_lds[2][DQ8_KT * AB_D * 2];  // subtiled
  __shared__ unsigned char v_lds[2][DQ8_KT * AB_D * 2];  // subtiled

  // 1-D LPT grid: longest q-tiles (largest qt) dispatch first
  const int nqt = gridDim.x / (Hq * (int)B);
  const int qt = causal ? (nqt - 1 - blockIdx.x / (Hq * (int)B))
                        : (int)(blockIdx.x / (Hq * (int)B));
  const int rest = blockIdx.x % (Hq * (int)B);
  const int hq = rest % Hq;
  const int64_t b = rest / Hq;
  const int hkv = hq / (Hq / Hkv);
  const int tid = threadIdx.x;
  const int w = tid / KF_WAVE;
  const int lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int qrow_g = qt * DQ8_QT + w * 32 + l31;
  const int wave_qmax = qt * DQ8_QT + w * 32 + 31;
  const float scale2 = scale * KF_LOG2E;

  // persistent B-fragments of Q and dO for this lane's q column
  kf_bf16x8 qfrag[8], dofrag[8];
  {
    const int64_t qb = (b * S + qrow_g) * qts + (int64_t)hq * AB_D;
    const int64_t db = ((b * S + qrow_g) * (int64_t)Hq + hq) * AB_D;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      qfrag[kk] =
          *reinterpret_cast<const kf_bf16x8*>(q + qb + kk * 16 + hi * 8);
      dofrag[kk] =
          *reinterpret_cast<const kf_bf16x8*>(dout + db + kk * 16 + hi * 8);
    }
  }
  const float lse2_q =
      lse[(b * Hq + hq) * (int64_t)S + qrow_g] * KF_LOG2E;
  const float dlt_q = delta[(b * Hq + hq) * (int64_t)S + qrow_g];

  kf_f32x16 dqacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) dqacc[i] = kf_f32x16{0.f};

  const unsigned short* kg0 = k + (b * S) * kts + (int64_t)hkv * AB_D;
  const unsigned short* vg0 = v + (b * S) * kts + (int64_t)hkv * AB_D;
  const int sr0 = tid >> 4, sr1 = (tid + 512) >> 4, c8 = tid & 15;
  const unsigned tr_off = kf_tr_lane_off<64>(lane);

  const int last_kt =
      causal ? (qt * DQ8_QT + DQ8_QT - 1) / DQ8_KT : (S / DQ8_KT - 1);

  // prologue: stage tile 0
  kf_short8 kst0, kst1, vst0, vst1;
  kst0 = *reinterpret_cast<const kf_short8*>(kg0 + sr0 * kts + c8 * 8);
  kst1 = *reinterpret_cast<const kf_short8*>(kg0 + sr1 * kts + c8 * 8);
  vst0 = *reinterpret_cast<const kf_short8*>(vg0 + sr0 * kts + c8 * 8);
  vst1 = *reinterpret_cast<const kf_short8*>(vg0 + sr1 * kts + c8 * 8);
  auto stage_write = [&](int buf) {
    *reinterpret_cast<kf_short8*>(k_lds[buf] + 2 * kf_vsub<64>(sr0, c8 * 8)) =
        kst0;
    *reinterpret_cast<kf_short8*>(k_lds[buf] + 2 * kf_vsub<64>(sr1, c8 * 8)) =
        kst1;
    *reinterpret_cast<kf_short8*>(v_lds[buf] + 2 * kf_vsub<64>(sr0, c8 * 8)) =
        vst0;
    *reinterpret_cast<kf_short8*>(v_lds[buf] + 2 * kf_vsub<64>(sr1, c8 * 8)) =
        vst1;
  };
  stage_write(0);
  __syncthreads();

  for (int kt = 0; kt <= last_kt; ++kt) {
    const int cur = kt & 1;
    const bool have_next = kt < last_kt;
    if (have_next) {
      const unsigned short* kg = kg0 + (int64_t)(kt + 1) * DQ8_KT * kts;
      const unsigned short* vg = vg0 + (int64_t)(kt + 1) * DQ8_KT * kts;
      kst0 = *reinterpret_cast<const kf_short8*>(kg + sr0 * kts + c8 * 8);
      kst1 = *reinterpret_cast<const kf_short8*>(kg + sr1 * kts + c8 * 8);
      vst0 = *reinterpret_cast<const kf_short8*>(vg + sr0 * kts + c8 * 8);
      vst1 = *reinterpret_cast<const kf_short8*>(vg + sr1 * kts + c8 * 8);
    }

#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int kv_lo = kt * DQ8_KT + mt * 32;
      if (causal && kv_lo > wave_qmax) continue;  // wave-uniform skip
      kf_f32x16 st = kf_f32x16{0.f}, dpt = kf_f32x16{0.f};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        kf_bf16x8 ka = *reinterpret_cast<const kf_bf16x8*>(
            k_lds[cur] + kf_subrow(mt * 32 + l31, kk * 32 + hi * 16));
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qfrag[kk], st, 0, 0,
                                                     0);
        kf_bf16x8 va = *reinterpret_cast<const kf_bf16x8*>(
            v_lds[cur] + kf_subrow(mt * 32 + l31, kk * 32 + hi * 16));
        dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, dofrag[kk], dpt, 0,
                                                      0, 0);
      }
      __builtin_amdgcn_s_setprio(0);

      const int kv0 = kv_lo + hi * 4;
      const bool need_mask = causal && kv_lo + 31 > qt * DQ8_QT + w * 32;
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + (r & 3) + 8 * (r >> 2);
          const float p = (kv > qrow_g)
                              ? 0.f
                              : kf_exp2(st[r] * scale2 - lse2_q);
          st[r] = p * (dpt[r] - dlt_q) * scale;  // dS^T
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = kf_exp2(st[r] * scale2 - lse2_q);
          st[r] = p * (dpt[r] - dlt_q) * scale;
        }
      }
      kf_bf16x8 pb0 = kf_exchange(st, 0), pb1 = kf_exchange(st, 8);
      const unsigned vbase =
          (unsigned)(size_t)(k_lds[cur]) + tr_off + (mt << 10);
      kf_tr_acc_loop<true, 64>(dqacc, vbase, pb0, pb1);
    }

    if (have_next) stage_write(cur ^ 1);
    __syncthreads();
  }

  // optional RoPE adjoint (cost != nullptr): acc[dt] / acc[dt+2] hold the
  // rotate-half pair (d, d+64) of this lane's q row
  if (cost) {
    const int64_t cb = (pos_offset + qrow_g) * (AB_D / 2) + 4 * hi;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const kf_float4 c4 =
            *reinterpret_cast<const kf_float4*>(cost + cb + dt * 32 + 8 * rq);
        const kf_float4 s4 =
            *reinterpret_cast<const kf_float4*>(sint + cb + dt * 32 + 8 * rq);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          KF_ROPE_ADJ_PAIR(dqacc[dt][rq * 4 + j], dqacc[dt + 2][rq * 4 + j],
                           c4[j], s4[j]);
      }
  }

  // epilogue: dQ^T regs -> dq (4 consecutive d per quad -> b64 stores)
  const int64_t dqb = (b * S + qrow_g) * dqts + (int64_t)hq * AB_D;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const int d0 = dt * 32 + 8 * rq + 4 * hi;
      unsigned short q4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        q4[j] = kf_f32_to_bf16(dqacc[dt][rq * 4 + j]);
      *reinterpret_cast<kf_short4*>(dq + dqb + d0) =
          *reinterpret_cast<kf_short4*>(q4);
    }
}

// --------------------------------------------------------------- pass dKV --
// Split dV and dK kernels (the test reference; kf_attn_bwd runs the fused
// kf_attn_dkv8f below): carrying both 64-register accumulators in one
// kernel spilled 62 VGPRs at the 2-waves/SIMD budget, and recomputing S in
// a second kernel (+25% MFMA) was far cheaper than scratch traffic.
#define DKV8_KT 256   // kv rows per block (8 waves x 32)
#define DKV8_QT 64    // q rows per LDS tile

__global__ __launch_bounds__(512, 2) void kf_attn_dv8_kernel(
    unsigned short* __restrict__ dv, const unsigned short* __restrict__ q,
    const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ dout, const float* __restrict__ lse,
    int64_t B, int S, int Hq, int Hkv, int64_t qts, int64_t kts,
    int64_t dkts, float scale, int causal) {
  __shared__ unsigned char q_lds[2][DKV8_QT * AB_D * 2];   // subtiled
  __shared__ unsigned char dot_lds[2][DKV8_QT * AB_D * 2]; // subtiled
  __shared__ float lse_s[2][DKV8_QT];                      // pre-mul log2e

  // 1-D grid decoded kt-major: causal work decreases with kt, so the
  // longest blocks (kt=0) dispatch first (LPT order — with only
  // S/256 x Hkv x B blocks the schedule tail otherwise sets the wall)
  const int kt = blockIdx.x / (Hkv * (int)B);
  const int rest = blockIdx.x % (Hkv * (int)B);
  const int hkv = rest % Hkv;
  const int64_t b = rest / Hkv;
  const int g = Hq / Hkv;
  const int tid = threadIdx.x;
  const int w = tid / KF_WAVE;
  const int lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int kvrow_g = kt * DKV8_KT + w * 32 + l31;
  const int wave_kv_min = kt * DKV8_KT + w * 32;
  const float scale2 = scale * KF_LOG2E;

  const unsigned short* kvb_k =
      k + (b * S + kvrow_g) * kts + (int64_t)hkv * AB_D;
  // persistent K B-fragments: loaded ONCE; without the explicit array the
  // compiler rematerialized these 8 global loads inside every sub-block
  // (regression caught by rocprof: dv8 2.97 ms vs round-1 2.16)
  kf_bf16x8 kbf[8];
#pragma unroll
  for (int kk = 0; kk < 8; ++kk)
    kbf[kk] =
        *reinterpret_cast<const kf_bf16x8*>(kvb_k + kk * 16 + hi * 8);

  kf_f32x16 dvacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) dvacc[i] = kf_f32x16{0.f};

  const int qt0 = causal ? (kt * DKV8_KT) / DKV8_QT : 0;
  const int nqt = S / DKV8_QT;
  const int per_head = nqt - qt0;
  const int total = g * per_head;
  const int sr0 = tid >> 4, sr1 = (tid + 512) >> 4, c8 = tid & 15;
  const unsigned tr_off = kf_tr_lane_off<64>(lane);

  // async-STAGE split (T14): loads issue at the top of the iteration, LDS
  // writes land after compute has covered the HBM latency.
  kf_short8 sq0, sq1, sd0, sd1;
  float lse_ld = 0.f;
  auto stage_load = [&](int flat) {
    const int hq = hkv * g + flat / per_head;
    const int qt = qt0 + flat % per_head;
    const unsigned short* qg =
        q + (b * S + qt * DKV8_QT) * qts + (int64_t)hq * AB_D;
    const unsigned short* dog =
        dout + ((b * S + qt * DKV8_QT) * (int64_t)Hq + hq) * AB_D;
    if (tid < DKV8_QT)
      lse_ld = lse[(b * Hq + hq) * (int64_t)S + qt * DKV8_QT + tid];
    sq0 = *reinterpret_cast<const kf_short8*>(qg + sr0 * qts + c8 * 8);
    sq1 = *reinterpret_cast<const kf_short8*>(qg + sr1 * qts + c8 * 8);
    sd0 = *reinterpret_cast<const kf_short8*>(
        dog + sr0 * (int64_t)Hq * AB_D + c8 * 8);
    sd1 = *reinterpret_cast<const kf_short8*>(
        dog + sr1 * (int64_t)Hq * AB_D + c8 * 8);
  };
  auto stage_write = [&](int buf) {
    if (tid < DKV8_QT) lse_s[buf][tid] = lse_ld * KF_LOG2E;
    *reinterpret_cast<kf_short8*>(q_lds[buf] + 2 * kf_vsub<64>(sr0, c8 * 8)) =
        sq0;
    *reinterpret_cast<kf_short8*>(q_lds[buf] + 2 * kf_vsub<64>(sr1, c8 * 8)) =
        sq1;
    *reinterpret_cast<kf_short8*>(dot_lds[buf] + 2 * kf_vsub<64>(sr0, c8 * 8)) =
        sd0;
    *reinterpret_cast<kf_short8*>(dot_lds[buf] + 2 * kf_vsub<64>(sr1, c8 * 8)) =
        sd1;
  };

  stage_load(0);
  stage_write(0);
  __syncthreads();
  for (int flat = 0; flat < total; ++flat) {
    const int cur = flat & 1;
    const bool have_next = flat + 1 < total;
    if (have_next) stage_load(flat + 1);
    const int qt = qt0 + flat % per_head;

#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int q_lo = qt * DKV8_QT + mt * 32;  // global q of sub-block
      // causal: contributes iff some qq >= kv in this wave
      if (causal && q_lo + 31 < wave_kv_min) continue;
      kf_f32x16 sacc = kf_f32x16{0.f};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        kf_bf16x8 qa = *reinterpret_cast<const kf_bf16x8*>(
            q_lds[cur] + kf_subrow(mt * 32 + l31, kk * 32 + hi * 16));
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kbf[kk], sacc, 0,
                                                       0, 0);
      }
      __builtin_amdgcn_s_setprio(0);

      const int q0 = mt * 32 + hi * 4;  // q-tile-local
      const bool need_mask = causal && q_lo <= kt * DKV8_KT + w * 32 + 31;
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = q0 + (r & 3) + 8 * (r >> 2);
          const int qq = qt * DKV8_QT + ql;
          sacc[r] = (kvrow_g > qq)
                        ? 0.f
                        : kf_exp2(sacc[r] * scale2 - lse_s[cur][ql]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = q0 + (r & 3) + 8 * (r >> 2);
          sacc[r] = kf_exp2(sacc[r] * scale2 - lse_s[cur][ql]);
        }
      }
      kf_bf16x8 pa0 = kf_exchange(sacc, 0), pa1 = kf_exchange(sacc, 8);
      const unsigned vbase =
          (unsigned)(size_t)(dot_lds[cur]) + tr_off + (mt << 10);
      kf_tr_acc_loop<false, 64>(dvacc, vbase, pa0, pa1);
    }
    if (have_next) stage_write(cur ^ 1);
    __syncthreads();
  }

  const int kvbase = kt * DKV8_KT + w * 32 + hi * 4;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kvr = kvbase + (r & 3) + 8 * (r >> 2);
    const int64_t base = (b * S + kvr) * dkts + (int64_t)hkv * AB_D;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      dv[base + dt * 32 + l31] = kf_f32_to_bf16(dvacc[dt][r]);
  }
}

__global__ __launch_bounds__(512, 2) void kf_attn_dk8_kernel(
    unsigned short* __restrict__ dk, const unsigned short* __restrict__ q,
    const unsigned short* __restrict__ k, const unsigned short* __restrict__ v,
    const unsigned short* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, int64_t B, int S, int Hq, int Hkv,
    int64_t qts, int64_t kts, int64_t dkts, float scale, int causal,
    const float* __restrict__ cost, const float* __restrict__ sint,
    int64_t pos_offset) {
  __shared__ unsigned char q_lds[2][DKV8_QT * AB_D * 2];   // subtiled
  __shared__ unsigned char do_lds[2][DKV8_QT * AB_D * 2];  // subtiled
  __shared__ float lse_s2[2][DKV8_QT], dlt_s2[2][DKV8_QT];

  const int kt = blockIdx.x / (Hkv * (int)B);  // LPT decode (see dv8)
  const int rest = blockIdx.x % (Hkv * (int)B);
  const int hkv = rest % Hkv;
  const int64_t b = rest / Hkv;
  const int g = Hq / Hkv;
  const int tid = threadIdx.x;
  const int w = tid / KF_WAVE;
  const int lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int kvrow_g = kt * DKV8_KT + w * 32 + l31;
  const int wave_kv_min = kt * DKV8_KT + w * 32;
  const float scale2 = scale * KF_LOG2E;

  const unsigned short* kvb_k =
      k + (b * S + kvrow_g) * kts + (int64_t)hkv * AB_D;
  const unsigned short* kvb_v =
      v + (b * S + kvrow_g) * kts + (int64_t)hkv * AB_D;
  kf_bf16x8 kbf[8], vbf[8];  // persistent B-fragments (see dv8 note)
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) {
    kbf[kk] =
        *reinterpret_cast<const kf_bf16x8*>(kvb_k + kk * 16 + hi * 8);
    vbf[kk] =
        *reinterpret_cast<const kf_bf16x8*>(kvb_v + kk * 16 + hi * 8);
  }

  kf_f32x16 dkacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) dkacc[i] = kf_f32x16{0.f};

  const int qt0 = causal ? (kt * DKV8_KT) / DKV8_QT : 0;
  const int nqt = S / DKV8_QT;
  const int per_head = nqt - qt0;
  const int total = g * per_head;
  const int sr0 = tid >> 4, sr1 = (tid + 512) >> 4, c8 = tid & 15;
  const unsigned tr_off = kf_tr_lane_off<64>(lane);

  kf_short8 sq0, sq1, sd0, sd1;
  float lse_ld = 0.f, dlt_ld = 0.f;
  auto stage_load = [&](int flat) {
    const int hq = hkv * g + flat / per_head;
    const int qt = qt0 + flat % per_head;
    const unsigned short* qg =
        q + (b * S + qt * DKV8_QT) * qts + (int64_t)hq * AB_D;
    const unsigned short* dog =
        dout + ((b * S + qt * DKV8_QT) * (int64_t)Hq + hq) * AB_D;
    if (tid < DKV8_QT)
      lse_ld = lse[(b * Hq + hq) * (int64_t)S + qt * DKV8_QT + tid];
    else if (tid < 2 * DKV8_QT)
      dlt_ld =
          delta[(b * Hq + hq) * (int64_t)S + qt * DKV8_QT + tid - DKV8_QT];
    sq0 = *reinterpret_cast<const kf_short8*>(qg + sr0 * qts + c8 * 8);
    sq1 = *reinterpret_cast<const kf_short8*>(qg + sr1 * qts + c8 * 8);
    sd0 = *reinterpret_cast<const kf_short8*>(
        dog + sr0 * (int64_t)Hq * AB_D + c8 * 8);
    sd1 = *reinterpret_cast<const kf_short8*>(
        dog + sr1 * (int64_t)Hq * AB_D + c8 * 8);
  };
  auto stage_write = [&](int buf) {
    if (tid < DKV8_QT) lse_s2[buf][tid] = lse_ld * KF_LOG2E;
    else if (tid < 2 * DKV8_QT) dlt_s2[buf][tid - DKV8_QT] = dlt_ld;
    *reinterpret_cast<kf_short8*>(q_lds[buf] + 2 * kf_vsub<64>(sr0, c8 * 8)) =
        sq0;
    *reinterpret_cast<kf_short8*>(q_lds[buf] + 2 * kf_vsub<64>(sr1, c8 * 8)) =
        sq1;
    *reinterpret_cast<kf_short8*>(do_lds[buf] + 2 * kf_vsub<64>(sr0, c8 * 8)) =
        sd0;
    *reinterpret_cast<kf_short8*>(do_lds[buf] + 2 * kf_vsub<64>(sr1, c8 * 8)) =
        sd1;
  };

  stage_load(0);
  stage_write(0);
  __syncthreads();
  for (int flat = 0; flat < total; ++flat) {
    const int cur = flat & 1;
    const bool have_next = flat + 1 < total;
    if (have_next) stage_load(flat + 1);
    const int qt = qt0 + flat % per_head;

#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int q_lo = qt * DKV8_QT + mt * 32;
      if (causal && q_lo + 31 < wave_kv_min) continue;
      kf_f32x16 sacc = kf_f32x16{0.f}, dpacc = kf_f32x16{0.f};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        kf_bf16x8 qa = *reinterpret_cast<const kf_bf16x8*>(
            q_lds[cur] + kf_subrow(mt * 32 + l31, kk * 32 + hi * 16));
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kbf[kk], sacc, 0,
                                                       0, 0);
        kf_bf16x8 da = *reinterpret_cast<const kf_bf16x8*>(
            do_lds[cur] + kf_subrow(mt * 32 + l31, kk * 32 + hi * 16));
        dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, vbf[kk], dpacc,
                                                        0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);

      const int q0 = mt * 32 + hi * 4;
      const bool need_mask = causal && q_lo <= kt * DKV8_KT + w * 32 + 31;
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = q0 + (r & 3) + 8 * (r >> 2);
          const int qq = qt * DKV8_QT + ql;
          const float p =
              (kvrow_g > qq)
                  ? 0.f
                  : kf_exp2(sacc[r] * scale2 - lse_s2[cur][ql]);
          sacc[r] = p * (dpacc[r] - dlt_s2[cur][ql]) * scale;  // dS
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = q0 + (r & 3) + 8 * (r >> 2);
          const float p = kf_exp2(sacc[r] * scale2 - lse_s2[cur][ql]);
          sacc[r] = p * (dpacc[r] - dlt_s2[cur][ql]) * scale;
        }
      }
      kf_bf16x8 ds0 = kf_exchange(sacc, 0), ds1 = kf_exchange(sacc, 8);
      const unsigned vbase =
          (unsigned)(size_t)(q_lds[cur]) + tr_off + (mt << 10);
      kf_tr_acc_loop<false, 64>(dkacc, vbase, ds0, ds1);
    }
    if (have_next) stage_write(cur ^ 1);
    __syncthreads();
  }

  const int kvbase = kt * DKV8_KT + w * 32 + hi * 4;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kvr = kvbase + (r & 3) + 8 * (r >> 2);
    const int64_t base = (b * S + kvr) * dkts + (int64_t)hkv * AB_D;
    if (cost) {  // RoPE adjoint: (acc[dt], acc[dt+2]) is the pair (d, d+64)
      const int64_t cb = (pos_offset + kvr) * (AB_D / 2) + l31;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        KF_ROPE_ADJ_PAIR(dkacc[dt][r], dkacc[dt + 2][r], cost[cb + dt * 32],
                         sint[cb + dt * 32]);
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      dk[base + dt * 32 + l31] = kf_f32_to_bf16(dkacc[dt][r]);
  }
}

// --------------------------------------------------------- fused pass dKV --
// One pass producing dK and dV: S and P are computed once per sub-block and
// Q/dO are streamed once, so a 32x32 sub-block costs 32 MFMAs (8 S + 8 dP +
// 8 P^T dO + 8 dS^T Q) where the dv8 + dk8 pair spends 40.
//
// Shape: the split kernels' — 512 threads, 8 waves x 32 kv rows, one block
// per CU, 2 waves/SIMD and therefore 256 registers per lane
// (__launch_bounds__'s second argument counts waves per SIMD: dk8 already
// uses 252 of them, it never ran at a 128-register budget). dkacc 64 +
// dvacc 64 + K and V fragments 64 + sacc/dpacc 32 + staging 16 + tr
// temporaries 16 is ~260 before addresses and spilled, so:
//  * the V B-fragments are parked in LDS (64 KiB, each lane re-reads only
//    the 8 chunks it wrote itself, one extra ds_read_b128 per dP MFMA);
//  * lse and delta share one staging register (a two-variable version went
//    through a stack slot);
//  * the per-lane staging offsets are 32-bit on a wave-uniform base.
// With a 4-wave, 128-kv-row block the compiler took 373 registers, i.e. one
// 4-wave block per CU: rejected before any run.
// Per kv row the work and the summation order are exactly those of dv8/dk8
// (same MFMA shape, q sub-blocks ascending within head order, d contracted
// in the same 8 steps), so dK and dV are bit-identical to the split kernels.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   255 VGPRs, 0 AGPRs, scratch 0, 2 waves/SIMD, LDS 132,096 B/block.
#define DKVF_WAVES 8
#define DKVF_THREADS (DKVF_WAVES * KF_WAVE)
#define DKVF_KT (DKVF_WAVES * 32)  // kv rows per block
#define DKVF_NST (DKV8_QT * 16 / DKVF_THREADS)  // staged b128 per thread
#define DKVF_SLAB (DKV8_QT * 16 * 2)  // bytes per 16-wide d-slab of a tile

__global__ __launch_bounds__(DKVF_THREADS, 2) void kf_attn_dkv8f_kernel(
    unsigned short* __restrict__ dk, unsigned short* __restrict__ dv,
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v,
    const unsigned short* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, int64_t B, int S, int Hq, int Hkv,
    int64_t qts, int64_t kts, int64_t dkts, float scale, int causal,
    const float* __restrict__ cost, const float* __restrict__ sint,
    int64_t pos_offset) {
  __shared__ unsigned char q_lds[2][DKV8_QT * AB_D * 2];   // subtiled
  __shared__ unsigned char do_lds[2][DKV8_QT * AB_D * 2];  // subtiled
  __shared__ float lse_s3[2][DKV8_QT], dlt_s3[2][DKV8_QT];
  // V B-fragments parked in LDS: every lane writes its own 8 chunks once and
  // reads back only those (no barrier needed), subtiled like q_lds so the
  // b128 reads bank exactly like the Q/dO row-chunk reads
  __shared__ unsigned char v_lds[DKVF_WAVES / 2][DKV8_QT * AB_D * 2];

  const int kt = blockIdx.x / (Hkv * (int)B);  // LPT decode (see dv8)
  const int rest = blockIdx.x % (Hkv * (int)B);
  const int hkv = rest % Hkv;
  const int64_t b = rest / Hkv;
  const int g = Hq / Hkv;
  const int tid = threadIdx.x;
  const int w = tid / KF_WAVE;
  const int lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int kvrow_g = kt * DKVF_KT + w * 32 + l31;
  const int wave_kv_min = kt * DKVF_KT + w * 32;
  const float scale2 = scale * KF_LOG2E;

  const unsigned short* kvb_k =
      k + (b * S + kvrow_g) * kts + (int64_t)hkv * AB_D;
  const unsigned short* kvb_v =
      v + (b * S + kvrow_g) * kts + (int64_t)hkv * AB_D;
  kf_bf16x8 kbf[8];  // persistent K B-fragments (see dv8 note)
  // chunk kk of the lane's row lives in d-slab kk: kf_subrow(r, kk * 32 +
  // hi * 16) == kf_subrow(r, hi * 16) + kk * DKVF_SLAB (64 rows x 16 d x 2 B)
  unsigned char* vfrag =
      v_lds[w >> 1] + kf_subrow((w & 1) * 32 + l31, hi * 16);
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) {
    kbf[kk] =
        *reinterpret_cast<const kf_bf16x8*>(kvb_k + kk * 16 + hi * 8);
    *reinterpret_cast<kf_bf16x8*>(vfrag + kk * DKVF_SLAB) =
        *reinterpret_cast<const kf_bf16x8*>(kvb_v + kk * 16 + hi * 8);
  }

  kf_f32x16 dkacc[4], dvacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dkacc[i] = kf_f32x16{0.f};
    dvacc[i] = kf_f32x16{0.f};
  }

  const int qt0 = causal ? (kt * DKVF_KT) / DKV8_QT : 0;
  const int nqt = S / DKV8_QT;
  const int per_head = nqt - qt0;
  const int total = g * per_head;
  const int c8 = tid & 15;
  const unsigned tr_off = kf_tr_lane_off<64>(lane);
  // per-lane staging offsets kept 32-bit (uniform 64-bit base + lane offset)
  constexpr int kRowsPerPass = DKVF_THREADS / 16;
  const unsigned qoff = (unsigned)((tid >> 4) * (int)qts + c8 * 8);
  const unsigned dooff = (unsigned)((tid >> 4) * Hq * AB_D + c8 * 8);

  kf_short8 sq[DKVF_NST], sd[DKVF_NST];
  float rc_ld = 0.f;  // row constant: lse (tid < 64) or delta (tid < 128)
  auto stage_load = [&](int flat) {
    const int hq = hkv * g + flat / per_head;
    const int qt = qt0 + flat % per_head;
    const unsigned short* qg =
        q + (b * S + qt * DKV8_QT) * qts + (int64_t)hq * AB_D;
    const unsigned short* dog =
        dout + ((b * S + qt * DKV8_QT) * (int64_t)Hq + hq) * AB_D;
    if (tid < 2 * DKV8_QT) {
      const float* rc = tid < DKV8_QT ? lse : delta;
      rc_ld = rc[(b * Hq + hq) * (int64_t)S + qt * DKV8_QT +
                 (tid & (DKV8_QT - 1))];
    }
#pragma unroll
    for (int j = 0; j < DKVF_NST; ++j) {
      sq[j] = *reinterpret_cast<const kf_short8*>(
          qg + j * kRowsPerPass * qts + qoff);
      sd[j] = *reinterpret_cast<const kf_short8*>(
          dog + j * kRowsPerPass * (int64_t)Hq * AB_D + dooff);
    }
  };
  auto stage_write = [&](int buf) {
    if (tid < DKV8_QT) lse_s3[buf][tid] = rc_ld * KF_LOG2E;
    else if (tid < 2 * DKV8_QT) dlt_s3[buf][tid - DKV8_QT] = rc_ld;
#pragma unroll
    for (int j = 0; j < DKVF_NST; ++j) {
      const int sr = (tid + j * DKVF_THREADS) >> 4;
      *reinterpret_cast<kf_short8*>(q_lds[buf] + 2 * kf_vsub<64>(sr, c8 * 8)) =
          sq[j];
      *reinterpret_cast<kf_short8*>(do_lds[buf] + 2 * kf_vsub<64>(sr, c8 * 8)) =
          sd[j];
    }
  };

  stage_load(0);
  stage_write(0);
  __syncthreads();
  for (int flat = 0; flat < total; ++flat) {
    const int cur = flat & 1;
    const bool have_next = flat + 1 < total;
    if (have_next) stage_load(flat + 1);
    const int qt = qt0 + flat % per_head;

#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int q_lo = qt * DKV8_QT + mt * 32;
      if (causal && q_lo + 31 < wave_kv_min) continue;
      kf_f32x16 sacc = kf_f32x16{0.f}, dpacc = kf_f32x16{0.f};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        kf_bf16x8 qa = *reinterpret_cast<const kf_bf16x8*>(
            q_lds[cur] + kf_subrow(mt * 32 + l31, kk * 32 + hi * 16));
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kbf[kk], sacc, 0,
                                                       0, 0);
        kf_bf16x8 da = *reinterpret_cast<const kf_bf16x8*>(
            do_lds[cur] + kf_subrow(mt * 32 + l31, kk * 32 + hi * 16));
        kf_bf16x8 vb =
            *reinterpret_cast<const kf_bf16x8*>(vfrag + kk * DKVF_SLAB);
        dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, vb, dpacc, 0, 0,
                                                        0);
      }
      __builtin_amdgcn_s_setprio(0);

      // P once (exactly dv8's expression), then dS from it (dk8's)
      const int q0 = mt * 32 + hi * 4;
      const bool need_mask = causal && q_lo <= kt * DKVF_KT + w * 32 + 31;
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = q0 + (r & 3) + 8 * (r >> 2);
          const int qq = qt * DKV8_QT + ql;
          sacc[r] = (kvrow_g > qq)
                        ? 0.f
                        : kf_exp2(sacc[r] * scale2 - lse_s3[cur][ql]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = q0 + (r & 3) + 8 * (r >> 2);
          sacc[r] = kf_exp2(sacc[r] * scale2 - lse_s3[cur][ql]);
        }
      }
      kf_bf16x8 pa0 = kf_exchange(sacc, 0), pa1 = kf_exchange(sacc, 8);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ql = q0 + (r & 3) + 8 * (r >> 2);
        sacc[r] = sacc[r] * (dpacc[r] - dlt_s3[cur][ql]) * scale;  // dS
      }
      kf_bf16x8 ds0 = kf_exchange(sacc, 0), ds1 = kf_exchange(sacc, 8);

      const unsigned vbase_do =
          (unsigned)(size_t)(do_lds[cur]) + tr_off + (mt << 10);
      kf_tr_acc_loop<false, 64>(dvacc, vbase_do, pa0, pa1);
      const unsigned vbase_q =
          (unsigned)(size_t)(q_lds[cur]) + tr_off + (mt << 10);
      kf_tr_acc_loop<false, 64>(dkacc, vbase_q, ds0, ds1);
    }
    if (have_next) stage_write(cur ^ 1);
    __syncthreads();
  }

  const int kvbase = kt * DKVF_KT + w * 32 + hi * 4;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kvr = kvbase + (r & 3) + 8 * (r >> 2);
    const int64_t base = (b * S + kvr) * dkts + (int64_t)hkv * AB_D;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      dv[base + dt * 32 + l31] = kf_f32_to_bf16(dvacc[dt][r]);
    if (cost) {  // RoPE adjoint on dK only (see dk8)
      const int64_t cb = (pos_offset + kvr) * (AB_D / 2) + l31;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        KF_ROPE_ADJ_PAIR(dkacc[dt][r], dkacc[dt + 2][r], cost[cb + dt * 32],
                         sint[cb + dt * 32]);
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      dk[base + dt * 32 + l31] = kf_f32_to_bf16(dkacc[dt][r]);
  }
}

// ----------------------------------------------------------- entry points --
// The *_rope variants take cos/sin tables [pos, D/2] fp32 and a position
// offset; nullptr tables mean no rotation. dk and dv must not alias.
KF_EXPORT int kf_attn_bwd8_dq_rope(void* dq, const void* q, const void* k,
                                   const void* v, const void* dout,
                                   const float* lse, const float* delta,
                                   int64_t B, int64_t S, int64_t Hq,
                                   int64_t Hkv, int64_t qts, int64_t kts,
                                   int64_t dqts, float scale, int causal,
                                   const float* cost, const float* sint,
                                   int64_t pos_offset, void* stream) {
  dim3 gq((unsigned)((S / DQ8_QT) * Hq * B), 1, 1);
  hipLaunchKernelGGL(kf_attn_dq8_kernel, gq, dim3(512), 0,
                     (hipStream_t)stream, (unsigned short*)dq,
                     (const unsigned short*)q, (const unsigned short*)k,
                     (const unsigned short*)v, (const unsigned short*)dout,
                     lse, delta, B, (int)S, (int)Hq, (int)Hkv, qts, kts, dqts,
                     scale, causal, cost, sint, pos_offset);
  return (int)hipGetLastError();
}

KF_EXPORT int kf_attn_bwd8_dq(void* dq, const void* q, const void* k,
                              const void* v, const void* dout,
                              const float* lse, const float* delta, int64_t B,
                              int64_t S, int64_t Hq, int64_t Hkv, int64_t qts,
                              int64_t kts, int64_t dqts, float scale,
                              int causal, void* stream) {
  return kf_attn_bwd8_dq_rope(dq, q, k, v, dout, lse, delta, B, S, Hq, Hkv,
                              qts, kts, dqts, scale, causal, nullptr, nullptr,
                              0, stream);
}

// split pair: dv8 then dk8
KF_EXPORT int kf_attn_bwd8_dkv_rope(void* dk, void* dv, const void* q,
                                    const void* k, const void* v,
                                    const void* dout, const float* lse,
                                    const float* delta, int64_t B, int64_t S,
                                    int64_t Hq, int64_t Hkv, int64_t qts,
                                    int64_t kts, int64_t dkts, float scale,
                                    int causal, const float* cost,
                                    const float* sint, int64_t pos_offset,
                                    void* stream) {
  dim3 gkv((unsigned)((S / DKV8_KT) * Hkv * B), 1, 1);
  hipLaunchKernelGGL(kf_attn_dv8_kernel, gkv, dim3(512), 0,
                     (hipStream_t)stream, (unsigned short*)dv,
                     (const unsigned short*)q, (const unsigned short*)k,
                     (const unsigned short*)dout, lse, B, (int)S, (int)Hq,
                     (int)Hkv, qts, kts, dkts, scale, causal);
  int err = (int)hipGetLastError();
  if (err) return err;
  hipLaunchKernelGGL(kf_attn_dk8_kernel, gkv, dim3(512), 0,
                     (hipStream_t)stream, (unsigned short*)dk,
                     (const unsigned short*)q, (const unsigned short*)k,
                     (const unsigned short*)v, (const unsigned short*)dout,
                     lse, delta, B, (int)S, (int)Hq, (int)Hkv, qts, kts,
                     dkts, scale, causal, cost, sint, pos_offset);
  return (int)hipGetLastError();
}

KF_EXPORT int kf_attn_bwd8_dkv(void* dk, void* dv, const void* q,
                               const void* k, const void* v, const void* dout,
                               const float* lse, const float* delta,
                               int64_t B, int64_t S, int64_t Hq, int64_t Hkv,
                               int64_t qts, int64_t kts, int64_t dkts,
                               float scale, int causal, void* stream) {
  return kf_attn_bwd8_dkv_rope(dk, dv, q, k, v, dout, lse, delta, B, S, Hq,
                               Hkv, qts, kts, dkts, scale, causal, nullptr,
                               nullptr, 0, stream);
}

// fused dK+dV pass (S % 128 == 0)
KF_EXPORT int kf_attn_bwd8_dkv_fused_rope(
    void* dk, void* dv, const void* q, const void* k, const void* v,
    const void* dout, const float* lse, const float* delta, int64_t B,
    int64_t S, int64_t Hq, int64_t Hkv, int64_t qts, int64_t kts,
    int64_t dkts, float scale, int causal, const float* cost,
    const float* sint, int64_t pos_offset, void* stream) {
  if (S % DKVF_KT || Hq % Hkv) return (int)hipErrorInvalidValue;
  dim3 gkv((unsigned)((S / DKVF_KT) * Hkv * B), 1, 1);
  hipLaunchKernelGGL(kf_attn_dkv8f_kernel, gkv, dim3(DKVF_THREADS), 0,
                     (hipStream_t)stream, (unsigned short*)dk,
                     (unsigned short*)dv, (const unsigned short*)q,
                     (const unsigned short*)k, (const unsigned short*)v,
                     (const unsigned short*)dout, lse, delta, B, (int)S,
                     (int)Hq, (int)Hkv, qts, kts, dkts, scale, causal, cost,
                     sint, pos_offset);
  return (int)hipGetLastError();
}

KF_EXPORT int kf_attn_bwd8_dkv_fused(void* dk, void* dv, const void* q,
                                     const void* k, const void* v,
                                     const void* dout, const float* lse,
                                     const float* delta, int64_t B, int64_t S,
                                     int64_t Hq, int64_t Hkv, int64_t qts,
                                     int64_t kts, int64_t dkts, float scale,
                                     int causal, void* stream) {
  return kf_attn_bwd8_dkv_fused_rope(dk, dv, q, k, v, dout, lse, delta, B, S,
                                     Hq, Hkv, qts, kts, dkts, scale, causal,
                                     nullptr, nullptr, 0, stream);
}

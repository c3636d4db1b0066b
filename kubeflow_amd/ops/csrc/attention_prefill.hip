// attention_prefill.hip — ragged batched prefill GQA attention over the KV
// cache, on the 32x32x16 bf16 MFMA.
//
//   q      [R, Hq, 128] bf16      packed query rows of N sequences
//   kcache [SLOTS, SMAX, Hkv, 128] bf16 (same layout for vcache)
//   slots  [N] int32; starts [N+1] int32; lens [N] int32
//   out    [R, Hq, 128] bf16
//
// Rows [starts[n], starts[n+1]) of q are consecutive tokens i = 0..C_n-1 of
// sequence n, whose K/V rows are already in cache slot slots[n]. lens[n] is
// the number of keys token 0 sees (kf_attn_verify's convention); token i sees
// keys [0, vis), vis = min(max(lens[n],0)+i, SMAX); vis == 0 gives a zero
// row. With every C_n = T <= 8 this is kf_attn_verify's contract. max_rows
// (host) bounds every C_n and sizes the grid; slots, starts and lens are read
// on the device only, so a captured launch follows their contents.
//
// Grid (ceil(max_rows*g/128), Hkv, N), 4 waves. A block owns 128 tile rows of
// one (sequence, kv-head); tile row r = (token, hg) = (r / g, r % g), so the
// g q-heads of a kv-head share every staged K/V tile. A wave owns 32 tile
// rows: its Q is 8 B fragments held in registers for the whole key loop, and
// it keeps its own (m, l, O) — the four waves are independent ROW streams
// over shared keys (verify's are independent key streams). 64-key K tiles
// (kf_swz rows) and V tiles (two kf_vsub<32> halves) are double-buffered in
// LDS: 2 x (16 + 16) KiB = 64 KiB, two blocks per CU. Per tile: the next
// tile's rows are loaded from global into registers, ONE barrier, compute on
// the current buffer, then the registers are written into the other buffer.
// The write of tile t+1 follows barrier t, which every wave reaches only
// after its compute of tile t-1 on that buffer; its read follows barrier
// t+1. Per 32-key half: S^T[key,row] = 8 x mfma(K, Q); in-register online
// softmax in the exp2 domain with defer-max; P^T through kf_exchange;
// O^T[d,row] += mfma(V^T, P^T) through the ds_read_b64_tr_b16 read. The
// output goes from the accumulators straight to global: no merge, no LDS.
//
// blockIdx.x is reversed: a sequence's last tile has the most keys and is
// issued first. A block past C_n returns before any vector load; in a
// straddling block a wave wholly past C_n only stages and barriers. The key
// loop ends at the block's last visible key; a wave skips the halves wholly
// past its own last visible key; the mask compare runs only in halves that
// reach past the wave's smallest vis.
//
// Built without the packed fp32 instructions (build_ext.EXTRA_CFLAGS): first
// tokens must not depend on how the compiler pairs the softmax arithmetic.

#include "kf_attn_common.h"

#define AP_D 128
#define AP_ROWS 128                    // tile rows per block
#define AP_KT 64                       // keys per staged tile
#define AP_SUB 32                      // keys per MFMA half
#define AP_ROWB (AP_D * 2)
#define AP_TILEB (AP_KT * AP_D * 2)    // one K or V tile: 16 KiB
#define AP_HALFB (AP_SUB * AP_D * 2)   // one V half (kf_vsub<32>): 8 KiB

__global__ __launch_bounds__(256, 2) void kf_attn_prefill_kernel(
    unsigned short* __restrict__ out, const unsigned short* __restrict__ q,
    const unsigned short* __restrict__ kcache,
    const unsigned short* __restrict__ vcache,
    const int* __restrict__ slots, const int* __restrict__ starts,
    const int* __restrict__ lens, int R, int max_rows, int smax, int n_slots,
    int Hq, int Hkv, float scale) {
  // [buffer][K tile | V tile]
  __shared__ __attribute__((aligned(16)))
  unsigned char lds[2][2 * AP_TILEB];

  const int bx = gridDim.x - 1 - blockIdx.x;  // most keys first
  const int hkv = blockIdx.y, n = blockIdx.z;
  const int g = Hq / Hkv;

  // clamps are memory safety: no content of starts / lens / slots reaches
  // past q, out or the cache. 64-bit so that no difference overflows.
  const int64_t s_lo = starts[n], s_hi = starts[n + 1];
  const int row0 = (int)min(max(s_lo, (int64_t)0), (int64_t)R);
  const int C = (int)min(min(max(s_hi - s_lo, (int64_t)0), (int64_t)max_rows),
                         (int64_t)(R - row0));
  const int tok_blk = bx * AP_ROWS / g;       // g divides 32
  if (tok_blk >= C) return;                   // before any vector load

  const int w = threadIdx.x / KF_WAVE;
  const int lane = threadIdx.x & (KF_WAVE - 1);
  const int l31 = lane & 31;
  const int hi = lane >> 5;
  const float scale2 = scale * KF_LOG2E;

  const int len0 = min(max(lens[n], 0), smax);
  const int64_t slot = min(max(slots[n], 0), n_slots - 1);
  const int64_t cbase = (slot * smax * Hkv + hkv) * AP_D;
  const int64_t cstride = (int64_t)Hkv * AP_D;
  // the block's last visible key bounds its key loop
  const int tok_last = min(C - 1, (bx * AP_ROWS + AP_ROWS - 1) / g);
  const int hi_k = min(len0 + tok_last, smax);

  // ---- this wave's rows; a lane's accumulator column is one query row ----
  const int tok_w = (bx * AP_ROWS + w * AP_SUB) / g;   // wave's first token
  const bool wave_live = tok_w < C;
  const int tok_wl = min(C - 1, tok_w + AP_SUB / g - 1);
  const int vis_lo = min(len0 + tok_w, smax);          // wave's smallest vis
  const int vis_hi = wave_live ? min(len0 + tok_wl, smax) : 0;  // largest
  const int tq = tok_w + l31 / g;
  const bool row_ok = tq < C;
  const int hq = hkv * g + l31 % g;
  const int64_t orow = (int64_t)(row0 + (row_ok ? tq : 0)) * Hq + hq;
  const int vis = row_ok ? min(len0 + tq, smax) : 0;

  kf_bf16x8 qfrag[8];
  {
    const kf_short8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      kf_short8 v8 = zero8;
      if (row_ok)
        v8 = *reinterpret_cast<const kf_short8*>(q + orow * AP_D + kk * 16 +
                                                 hi * 8);
      qfrag[kk] = *reinterpret_cast<kf_bf16x8*>(&v8);
    }
  }

  kf_f32x16 oacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) oacc[i] = kf_f32x16{0.f};
  float m_run = -INFINITY, l_run = 0.f;  // m_run in exp2 units

  // staging: thread covers rows (tid>>4) + 16u, 16-byte chunk tid&15 — each
  // 16-lane group reads one whole 256-byte cache row
  const int sr0 = threadIdx.x >> 4, c8 = threadIdx.x & 15;
  const unsigned tr_off = kf_tr_lane_off<AP_SUB>(lane);
  kf_short8 kst[4], vst[4];

  auto load_tile = [&](int kb) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // rows past the slot's end re-read its last row; they are masked
      const int64_t off = cbase +
          (int64_t)min(kb + sr0 + 16 * u, smax - 1) * cstride + c8 * 8;
      kst[u] = *reinterpret_cast<const kf_short8*>(kcache + off);
      vst[u] = *reinterpret_cast<const kf_short8*>(vcache + off);
    }
  };
  auto write_tile = [&](int b) {
    unsigned char* const kt = lds[b];
    unsigned char* const vt = lds[b] + AP_TILEB;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = sr0 + 16 * u;
      *reinterpret_cast<kf_short8*>(kt + kf_swz(r, c8 * 16, AP_ROWB)) = kst[u];
      *reinterpret_cast<kf_short8*>(vt + (r >> 5) * AP_HALFB +
                                    2 * kf_vsub<AP_SUB>(r & 31, c8 * 8)) =
          vst[u];
    }
  };

  if (hi_k > 0) {
    load_tile(0);
    write_tile(0);
  }
  int buf = 0;
  for (int kb = 0; kb < hi_k; kb += AP_KT, buf ^= 1) {
    // next tile's rows fly under this one's compute
    const bool more = kb + AP_KT < hi_k;
    if (more) load_tile(kb + AP_KT);
    __syncthreads();

    if (wave_live) {
#pragma unroll
      for (int h = 0; h < AP_KT / AP_SUB; ++h) {
        const int k0 = kb + h * AP_SUB;
        if (k0 >= vis_hi) break;  // wholly past the wave's last visible key

        // ---- S^T = mfma(K, Q) ----
        const unsigned char* const kt = lds[buf];
        kf_bf16x8 af[8];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
          af[kk] = *reinterpret_cast<const kf_bf16x8*>(
              kt + kf_swz(h * AP_SUB + l31, kk * 32 + hi * 16, AP_ROWB));
        kf_f32x16 st = kf_f32x16{0.f};
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
          st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[kk], qfrag[kk], st,
                                                       0, 0, 0);
        __builtin_amdgcn_s_setprio(0);

        // ---- online softmax; the compare only where the half reaches past
        // the wave's smallest vis (wave-uniform branch) ----
        float mx = -INFINITY;
        if (k0 + AP_SUB > vis_lo) {
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

        // ---- O^T += V^T P^T ----
        const unsigned vbase =
            (unsigned)(size_t)(lds[buf] + AP_TILEB + h * AP_HALFB) + tr_off;
        kf_tr_acc_loop<true, AP_SUB>(oacc, vbase, p0, p1);
      }
    }
    if (more) write_tile(buf ^ 1);
  }

  if (!row_ok) return;  // padding rows of the last tile: never stored

  // accumulator reg r of d-block dt is d = 32dt + (r&3) + 8(r>>2) + 4hi
  const float inv_l = l_run > 0.f ? 1.f / l_run : 0.f;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      unsigned short q4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        q4[j] = kf_f32_to_bf16(oacc[dt][rq * 4 + j] * inv_l);
      *reinterpret_cast<kf_short4*>(out + orow * AP_D + dt * 32 + 8 * rq +
                                    4 * hi) =
          *reinterpret_cast<kf_short4*>(q4);
    }
}

KF_EXPORT int kf_attn_prefill(void* out, const void* q, const void* kcache,
                              const void* vcache, const int* slots,
                              const int* starts, const int* lens, int64_t N,
                              int64_t R, int64_t max_rows, int64_t smax,
                              int64_t n_slots, int64_t Hq, int64_t Hkv,
                              int64_t D, float scale, void* stream) {
  if (D != AP_D || Hkv < 1 || Hq % Hkv) return (int)hipErrorInvalidValue;
  const int64_t g = Hq / Hkv;
  if (g != 1 && g != 2 && g != 4 && g != 8) return (int)hipErrorInvalidValue;
  if (N < 0 || R < 0 || max_rows < 0 || smax < 1 || n_slots < 1)
    return (int)hipErrorInvalidValue;
  if (R > INT32_MAX / Hq || N > 65535 || Hkv > 65535 || smax > INT32_MAX / 2)
    return (int)hipErrorInvalidValue;
  if (N == 0 || R == 0 || max_rows == 0) return (int)hipSuccess;
  max_rows = max_rows < R ? max_rows : R;
  dim3 grid((unsigned)((max_rows * g + AP_ROWS - 1) / AP_ROWS), (unsigned)Hkv,
            (unsigned)N);
  hipLaunchKernelGGL(kf_attn_prefill_kernel, grid, dim3(256), 0,
                     (hipStream_t)stream, (unsigned short*)out,
                     (const unsigned short*)q, (const unsigned short*)kcache,
                     (const unsigned short*)vcache, slots, starts, lens,
                     (int)R, (int)max_rows, (int)smax, (int)n_slots, (int)Hq,
                     (int)Hkv, scale);
  return (int)hipGetLastError();
}

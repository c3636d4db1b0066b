// skinny_gemm.hip — decode-batch linear: C[M,N] = A[M,K] @ W[N,K]^T for
// M <= 32 (the serving decode step's GEMV-shaped GEMMs), plain and grouped
// over the experts of a routed MoE block.
//
// hipBLASLt runs these weight-streaming shapes at ~30-50% of HBM BW at
// M=16 (profiles/r02: decode-step GEMMs dominate the 6.3 ms step whose
// weight-read floor is ~2.5 ms). These kernels stream W exactly once:
// a block is 4 or 8 waves SHARING one 16-column N-tile with an in-block
// K-split, each wave issuing mfma_f32_16x16x32_bf16 over its K range (A
// operand rows = the M batch rows, zero-padded to the 16- or 32-row tile),
// then a reduction over the waves through LDS.
//
// Three kernel families, each with a plain and a grouped __global__ kernel:
//   direct   K % 32 == 0, M <= 16        kf_sk_direct_body<SKW>
//   LDS bf16 K % 512 == 0, M <= 32       two kernels, kept in step by hand
//   LDS q8   K % 1024 == 0, M <= 32      kf_sk_q8_body<MT>
// The direct and q8 families have one __device__ body that both kernels run.
// The LDS bf16 family does not: inlined from a shared body its 32-row
// instantiations compile to another prefetch sequence, which measured 3.6%
// slower on one grouped shape (profiles/skinny_shared_body.md).
// Grid = N/16 blocks (x n_groups); bf16 in/out, fp32 accumulate.

#include "kf_common.h"

typedef __bf16 kf_bf16x8s __attribute__((ext_vector_type(8)));
typedef float kf_f32x4s __attribute__((ext_vector_type(4)));
typedef unsigned int kf_u32x4q __attribute__((ext_vector_type(4)));

#define SK_NT 16      // N columns per block

// What one block computes, as its body sees it: rows [lo, lo + M) of c (and
// of res) from A rows lo + i, read through a_rows when it is given. The plain
// wrappers fill a_rows = nullptr, lo = 0; the grouped ones res = nullptr,
// lda = ldw = K, ldc = N. A body takes no "grouped" flag: after inlining,
// kf_sk_a_row(nullptr, ..) is the identity, lo = 0 folds out of the row
// index and `if (res)` on a null constant is gone.
struct kf_sk_prob {
  unsigned short* c;
  const unsigned short* a;
  const unsigned short* res;  // nullable, bf16, C layout: C = res + A@W^T
  const int* a_rows;          // nullable
  int a_nrows, lo, M;
  int64_t N, K, lda, ldw, ldc;
};

// A row (in a) of permuted row r; r < total_rows
__device__ __forceinline__ int64_t kf_sk_a_row(const int* __restrict__ a_rows,
                                               int r, int a_nrows) {
  if (!a_rows) return r;
  const int s = a_rows[r];
  return s < 0 ? 0 : (s >= a_nrows ? a_nrows - 1 : s);
}

// ---------------------------------------------------------------------
// Direct-load body. Lanes {l, l+16, l+32, l+48} read consecutive 8-element
// chunks of the same W row, so each wave instruction covers contiguous
// 64 B per row. K-split ways (waves/block) is a template knob: small-N
// shapes (wo: N=4096 -> 256 blocks == 1 block/CU == 1 wave/SIMD at 4 waves)
// are occupancy-starved and want 8; profiled per shape in
// profiles/r02_skinny_gemm.md.

template <int SKW>
__device__ __forceinline__ void kf_sk_direct_body(
    const kf_sk_prob& p, const unsigned short* __restrict__ w,
    float (&red)[SKW][SK_NT][SK_NT]) {
  const int64_t n0 = (int64_t)blockIdx.x * SK_NT;
  const int tid = threadIdx.x;
  const int wv = tid / KF_WAVE;
  const int lane = tid & (KF_WAVE - 1);
  const int l15 = lane & 15;
  const int hi4 = lane >> 4;  // 0..3: k-subchunk within the 32-k step

  // this wave's K range (each wave strides by SKW*32 for coalesced
  // row-chunk progression shared with its sibling lanes)
  kf_f32x4s acc = kf_f32x4s{0.f, 0.f, 0.f, 0.f};
  const unsigned short* wrow = w + (n0 + l15) * p.ldw;
  const bool arow_ok = l15 < p.M;
  const unsigned short* arow =
      p.a +
      kf_sk_a_row(p.a_rows, p.lo + (arow_ok ? l15 : 0), p.a_nrows) * p.lda;
  const kf_bf16x8s zero8 = kf_bf16x8s{0, 0, 0, 0, 0, 0, 0, 0};
  // 8-deep unrolled stream: ~256 B of W per wave in flight so the HBM
  // latency pipelines (a single outstanding load-pair left the wave
  // latency-bound at ~45% of blaslt on the big shapes)
  const int64_t step = (int64_t)SKW * 32;
  int64_t k = (int64_t)wv * 32;
  for (; k + 7 * step + 32 <= p.K; k += 8 * step) {
    kf_bf16x8s afs[8], wfs[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t ku = k + u * step + hi4 * 8;
      afs[u] = arow_ok
          ? *reinterpret_cast<const kf_bf16x8s*>(arow + ku) : zero8;
      wfs[u] = *reinterpret_cast<const kf_bf16x8s*>(wrow + ku);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afs[u], wfs[u], acc,
                                                    0, 0, 0);
  }
  for (; k < p.K; k += step) {
    kf_bf16x8s af = arow_ok
        ? *reinterpret_cast<const kf_bf16x8s*>(arow + k + hi4 * 8)
        : zero8;
    kf_bf16x8s wf =
        *reinterpret_cast<const kf_bf16x8s*>(wrow + k + hi4 * 8);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, wf, acc, 0, 0, 0);
  }
  // C/D layout (guide §3, m89): col = lane&15, row = (lane>>4)*4 + j
#pragma unroll
  for (int j = 0; j < 4; ++j) red[wv][hi4 * 4 + j][l15] = acc[j];
  __syncthreads();
  // first waves reduce + write: thread (row, col) pairs
  if (tid < SK_NT * SK_NT) {
    const int row = tid / SK_NT, col = tid % SK_NT;
    if (row < p.M && n0 + col < p.N) {
      float s = 0.f;
#pragma unroll
      for (int ww = 0; ww < SKW; ++ww) s += red[ww][row][col];
      const int64_t at = (int64_t)(p.lo + row) * p.ldc + n0 + col;
      if (p.res) s += kf_bf16_to_f32(p.res[at]);
      p.c[at] = kf_f32_to_bf16(s);
    }
  }
}

// ---------------------------------------------------------------------
// LDS-staged kernel (the plain one; kf_skinny_lds_grouped_kernel below is
// its copy and must follow every change here, tests/test_moe_decode_gpu.py
// compares the two bit for bit). The direct body's W loads put 16 rows x
// 64 B per instruction on the wire — half of every 128 B line — capping it
// at ~3 TB/s. Here the block's 8 waves stage W chunks cooperatively with
// FULL-ROW 1 KB runs (wave wv loads rows {2wv, 2wv+1}, one b128 per lane
// per row), then read their MFMA fragments from LDS. Padded row stride
// (520 elems) keeps both LDS sides at worst 2-way bank-conflicted.
// Double-buffered: one __syncthreads per 512-k chunk; the next chunk's
// global loads issue before the barrier so HBM latency overlaps MFMA.

#define SKL_W 8
#define SKL_KC 512                      // staged K elems (1 KB per row)
#define SKL_STRIDE (SKL_KC + 8)        // +8 elems: 2-way max conflicts

// MT = M-tile (16 or 32 batch rows); W traffic is identical, the wider
// tile just adds a second A fragment + accumulator (decode buckets > 16
// otherwise fell back to hipBLASLt).
template <int MT>
__global__ __launch_bounds__(SKL_W * 64, 2) void kf_skinny_lds_kernel(
    unsigned short* __restrict__ c, const unsigned short* __restrict__ a,
    const unsigned short* __restrict__ w,
    const unsigned short* __restrict__ res,
    int M, int64_t N, int64_t K, int64_t lda, int64_t ldw, int64_t ldc) {
  __shared__ unsigned short wbuf[2][SK_NT][SKL_STRIDE];
  __shared__ float red[SKL_W][MT][SK_NT];

  const int64_t n0 = (int64_t)blockIdx.x * SK_NT;
  const int tid = threadIdx.x;
  const int wv = tid / KF_WAVE;
  const int lane = tid & (KF_WAVE - 1);
  const int l15 = lane & 15;
  const int hi4 = lane >> 4;

  const int NMT = MT / 16;  // A tiles (1 or 2)
  kf_f32x4s acc[NMT];
  bool arow_ok[NMT];
  const unsigned short* arow[NMT];
#pragma unroll
  for (int t = 0; t < NMT; ++t) {
    acc[t] = kf_f32x4s{0.f, 0.f, 0.f, 0.f};
    arow_ok[t] = l15 + 16 * t < M;
    arow[t] = a + (arow_ok[t] ? l15 + 16 * t : 0) * lda;
  }
  const kf_bf16x8s zero8 = kf_bf16x8s{0, 0, 0, 0, 0, 0, 0, 0};
  // writer: wave wv stages rows {2wv, 2wv+1}, lane covers elems
  // [lane*8, lane*8+8) of each 512-elem row slice
  const unsigned short* wr0 = w + (n0 + 2 * wv) * ldw + lane * 8;
  const unsigned short* wr1 = wr0 + ldw;

  const int64_t nch = K / SKL_KC;
  const int ke0 = wv * 64 + hi4 * 8;  // this wave's k slice (s=0; s=1 at +32)
  kf_bf16x8s st0 = *reinterpret_cast<const kf_bf16x8s*>(wr0);
  kf_bf16x8s st1 = *reinterpret_cast<const kf_bf16x8s*>(wr1);
  kf_bf16x8s af0[NMT], af1[NMT];
#pragma unroll
  for (int t = 0; t < NMT; ++t) {
    af0[t] = arow_ok[t]
        ? *reinterpret_cast<const kf_bf16x8s*>(arow[t] + ke0) : zero8;
    af1[t] = arow_ok[t]
        ? *reinterpret_cast<const kf_bf16x8s*>(arow[t] + ke0 + 32) : zero8;
  }
  *reinterpret_cast<kf_bf16x8s*>(&wbuf[0][2 * wv][lane * 8]) = st0;
  *reinterpret_cast<kf_bf16x8s*>(&wbuf[0][2 * wv + 1][lane * 8]) = st1;
  for (int64_t ch = 0; ch < nch; ++ch) {
    kf_bf16x8s a0[NMT], a1[NMT];
#pragma unroll
    for (int t = 0; t < NMT; ++t) {
      a0[t] = af0[t];
      a1[t] = af1[t];
    }
    if (ch + 1 < nch) {
      st0 = *reinterpret_cast<const kf_bf16x8s*>(wr0 + (ch + 1) * SKL_KC);
      st1 = *reinterpret_cast<const kf_bf16x8s*>(wr1 + (ch + 1) * SKL_KC);
#pragma unroll
      for (int t = 0; t < NMT; ++t)
        if (arow_ok[t]) {
          af0[t] = *reinterpret_cast<const kf_bf16x8s*>(
              arow[t] + (ch + 1) * SKL_KC + ke0);
          af1[t] = *reinterpret_cast<const kf_bf16x8s*>(
              arow[t] + (ch + 1) * SKL_KC + ke0 + 32);
        }
    }
    // one barrier per chunk: makes buffer ch&1's writes visible AND
    // guarantees last iteration's readers of buffer (ch+1)&1 are done
    __syncthreads();
    kf_bf16x8s wf0 =
        *reinterpret_cast<const kf_bf16x8s*>(&wbuf[ch & 1][l15][ke0]);
    kf_bf16x8s wf1 =
        *reinterpret_cast<const kf_bf16x8s*>(&wbuf[ch & 1][l15][ke0 + 32]);
#pragma unroll
    for (int t = 0; t < NMT; ++t) {
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[t], wf0, acc[t],
                                                       0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[t], wf1, acc[t],
                                                       0, 0, 0);
    }
    if (ch + 1 < nch) {
      const int b = (int)((ch + 1) & 1);
      *reinterpret_cast<kf_bf16x8s*>(&wbuf[b][2 * wv][lane * 8]) = st0;
      *reinterpret_cast<kf_bf16x8s*>(&wbuf[b][2 * wv + 1][lane * 8]) = st1;
    }
  }
#pragma unroll
  for (int t = 0; t < NMT; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      red[wv][16 * t + hi4 * 4 + j][l15] = acc[t][j];
  __syncthreads();
  if (tid < MT * SK_NT) {
    const int row = tid / SK_NT, col = tid % SK_NT;
    if (row < M && n0 + col < N) {
      float s = 0.f;
#pragma unroll
      for (int ww = 0; ww < SKL_W; ++ww) s += red[ww][row][col];
      if (res) s += kf_bf16_to_f32(res[row * ldc + n0 + col]);
      c[row * ldc + n0 + col] = kf_f32_to_bf16(s);
    }
  }
}

// ---------------------------------------------------------------------
// W8A16 quantized body: W stored as OCP e4m3 fp8 with one fp32 scale
// per output row (absmax/448). The decode step is weight-BW-bound, so
// halving W bytes ≈ halves GEMM time; fragments convert fp8 -> f32 ->
// bf16 in-register (v_cvt_pk_f32_fp8 + v_cvt_pk_bf16_f32 — exact, since
// e4m3's 3 mantissa bits embed in bf16's 8) and MFMA stays bf16, so the
// activations keep full precision. Same LDS staging/shape rules as the
// bf16 kernel (K % 1024 == 0, N % 16 == 0, M <= 32), kept apart from it: the
// two differ in chunk size, number of k slices, staged vector type, fragment
// conversion and epilogue scale.

#define SKQ_KC 1024               // fp8 K elems per staged chunk (1 KB/row)
#define SKQ_STRIDE (SKQ_KC + 16)   // fp8 row slice bytes + pad

__device__ __forceinline__ kf_bf16x8s kf_fp8x8_to_bf16x8(
    const unsigned char* p8) {
  const unsigned int* pp = reinterpret_cast<const unsigned int*>(p8);
  const unsigned int lo = pp[0], hi = pp[1];
  typedef float kf_f32x2q __attribute__((ext_vector_type(2)));
  kf_f32x2q f0 = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false);
  kf_f32x2q f1 = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true);
  kf_f32x2q f2 = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false);
  kf_f32x2q f3 = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
  unsigned int r0, r1, r2, r3;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r0) : "v"(f0[0]), "v"(f0[1]));
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r1) : "v"(f1[0]), "v"(f1[1]));
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r2) : "v"(f2[0]), "v"(f2[1]));
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r3) : "v"(f3[0]), "v"(f3[1]));
  union {
    unsigned int u[4];
    kf_bf16x8s v;
  } out;
  out.u[0] = r0;
  out.u[1] = r1;
  out.u[2] = r2;
  out.u[3] = r3;
  return out.v;
}

template <int MT>
__device__ __forceinline__ void kf_sk_q8_body(
    const kf_sk_prob& p, const unsigned char* __restrict__ w8,
    const float* __restrict__ wscale,
    unsigned char (&wbuf8)[2][SK_NT][SKQ_STRIDE],
    float (&red)[SKL_W][MT][SK_NT]) {
  const int64_t n0 = (int64_t)blockIdx.x * SK_NT;
  const int tid = threadIdx.x;
  const int wv = tid / KF_WAVE;
  const int lane = tid & (KF_WAVE - 1);
  const int l15 = lane & 15;
  const int hi4 = lane >> 4;

  const int NMT = MT / 16;
  kf_f32x4s acc[NMT];
  bool arow_ok[NMT];
  const unsigned short* arow[NMT];
#pragma unroll
  for (int t = 0; t < NMT; ++t) {
    acc[t] = kf_f32x4s{0.f, 0.f, 0.f, 0.f};
    arow_ok[t] = l15 + 16 * t < p.M;
    arow[t] = p.a + kf_sk_a_row(p.a_rows,
                                p.lo + (arow_ok[t] ? l15 + 16 * t : 0),
                                p.a_nrows) * p.lda;
  }
  const kf_bf16x8s zero8 = kf_bf16x8s{0, 0, 0, 0, 0, 0, 0, 0};
  // 16 B per lane per row: a full 1 KB (1024 fp8) row slice per wave
  // instruction — same load width as the bf16 kernel, twice the K
  const unsigned char* wr0 = w8 + (n0 + 2 * wv) * p.ldw + lane * 16;
  const unsigned char* wr1 = wr0 + p.ldw;

  const int64_t nch = p.K / SKQ_KC;
  const int ke0 = wv * 128 + hi4 * 8;  // k slices at +0,+32,+64,+96
  kf_u32x4q st0 = *reinterpret_cast<const kf_u32x4q*>(wr0);
  kf_u32x4q st1 = *reinterpret_cast<const kf_u32x4q*>(wr1);
  kf_bf16x8s af[4][NMT];
#pragma unroll
  for (int si = 0; si < 4; ++si)
#pragma unroll
    for (int t = 0; t < NMT; ++t)
      af[si][t] = arow_ok[t]
          ? *reinterpret_cast<const kf_bf16x8s*>(arow[t] + ke0 + 32 * si)
          : zero8;
  *reinterpret_cast<kf_u32x4q*>(&wbuf8[0][2 * wv][lane * 16]) = st0;
  *reinterpret_cast<kf_u32x4q*>(&wbuf8[0][2 * wv + 1][lane * 16]) = st1;
  for (int64_t ch = 0; ch < nch; ++ch) {
    kf_bf16x8s acur[4][NMT];
#pragma unroll
    for (int si = 0; si < 4; ++si)
#pragma unroll
      for (int t = 0; t < NMT; ++t) acur[si][t] = af[si][t];
    if (ch + 1 < nch) {
      st0 = *reinterpret_cast<const kf_u32x4q*>(wr0 + (ch + 1) * SKQ_KC);
      st1 = *reinterpret_cast<const kf_u32x4q*>(wr1 + (ch + 1) * SKQ_KC);
#pragma unroll
      for (int si = 0; si < 4; ++si)
#pragma unroll
        for (int t = 0; t < NMT; ++t)
          if (arow_ok[t])
            af[si][t] = *reinterpret_cast<const kf_bf16x8s*>(
                arow[t] + (ch + 1) * SKQ_KC + ke0 + 32 * si);
    }
    __syncthreads();  // one per chunk, as in the bf16 kernel
#pragma unroll
    for (int si = 0; si < 4; ++si) {
      kf_bf16x8s wf =
          kf_fp8x8_to_bf16x8(&wbuf8[ch & 1][l15][ke0 + 32 * si]);
#pragma unroll
      for (int t = 0; t < NMT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(acur[si][t], wf,
                                                         acc[t], 0, 0, 0);
    }
    if (ch + 1 < nch) {
      const int b = (int)((ch + 1) & 1);
      *reinterpret_cast<kf_u32x4q*>(&wbuf8[b][2 * wv][lane * 16]) = st0;
      *reinterpret_cast<kf_u32x4q*>(&wbuf8[b][2 * wv + 1][lane * 16]) =
          st1;
    }
  }
#pragma unroll
  for (int t = 0; t < NMT; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      red[wv][16 * t + hi4 * 4 + j][l15] = acc[t][j];
  __syncthreads();
  if (tid < MT * SK_NT) {
    const int row = tid / SK_NT, col = tid % SK_NT;
    if (row < p.M && n0 + col < p.N) {
      float s = 0.f;
#pragma unroll
      for (int ww = 0; ww < SKL_W; ++ww) s += red[ww][row][col];
      s *= wscale[n0 + col];
      const int64_t at = (int64_t)(p.lo + row) * p.ldc + n0 + col;
      if (p.res) s += kf_bf16_to_f32(p.res[at]);
      p.c[at] = kf_f32_to_bf16(s);
    }
  }
}

// ---------------------------------------------------------------------
// Plain kernels: one problem, every block the same M rows.

template <int SKW>
__global__ __launch_bounds__(SKW * 64, 2) void kf_skinny_gemm_kernel(
    unsigned short* __restrict__ c, const unsigned short* __restrict__ a,
    const unsigned short* __restrict__ w,
    const unsigned short* __restrict__ res, int M, int64_t N, int64_t K,
    int64_t lda, int64_t ldw, int64_t ldc) {
  __shared__ float red[SKW][SK_NT][SK_NT];  // per-wave C tiles
  kf_sk_direct_body<SKW>(
      kf_sk_prob{c, a, res, nullptr, 0, 0, M, N, K, lda, ldw, ldc}, w, red);
}

template <int MT>
__global__ __launch_bounds__(SKL_W * 64, 2) void kf_skinny_q8_kernel(
    unsigned short* __restrict__ c, const unsigned short* __restrict__ a,
    const unsigned char* __restrict__ w8, const float* __restrict__ wscale,
    const unsigned short* __restrict__ res,
    int M, int64_t N, int64_t K, int64_t lda, int64_t ldw, int64_t ldc) {
  __shared__ unsigned char wbuf8[2][SK_NT][SKQ_STRIDE];
  __shared__ float red[SKL_W][MT][SK_NT];
  kf_sk_q8_body<MT>(
      kf_sk_prob{c, a, res, nullptr, 0, 0, M, N, K, lda, ldw, ldc}, w8,
      wscale, wbuf8, red);
}

KF_EXPORT int kf_skinny_gemm_q8(void* c, const void* a, const void* w8,
                                const float* wscale, const void* res,
                                int64_t M, int64_t N, int64_t K, int64_t lda,
                                int64_t ldw, int64_t ldc, void* stream) {
  if (M < 1 || M > 32 || K % SKQ_KC || N % SK_NT)
    return (int)hipErrorInvalidValue;
  if (lda == 0) lda = K;
  if (ldw == 0) ldw = K;
  if (ldc == 0) ldc = N;
  if (ldw % 8 || lda % 8) return (int)hipErrorInvalidValue;
  dim3 grid((unsigned)(N / SK_NT), 1, 1);
#define KF_SKQ_LAUNCH(MT)                                                \
  hipLaunchKernelGGL(kf_skinny_q8_kernel<MT>, grid, dim3(SKL_W * 64), 0, \
                     (hipStream_t)stream, (unsigned short*)c,            \
                     (const unsigned short*)a, (const unsigned char*)w8, \
                     wscale, (const unsigned short*)res, (int)M, N, K,   \
                     lda, ldw, ldc)
  if (M > 16) KF_SKQ_LAUNCH(32);
  else KF_SKQ_LAUNCH(16);
  return (int)hipGetLastError();
}

KF_EXPORT int kf_skinny_gemm(void* c, const void* a, const void* w,
                             const void* res, int64_t M, int64_t N,
                             int64_t K, int64_t lda, int64_t ldw,
                             int64_t ldc, void* stream) {
  if (M < 1 || M > 32 || K % 32 || N % SK_NT) return (int)hipErrorInvalidValue;
  if (lda == 0) lda = K;
  if (ldw == 0) ldw = K;
  if (ldc == 0) ldc = N;
  const bool lds_ok = K % SKL_KC == 0 && ldw % 8 == 0 && lda % 8 == 0;
  if (M > 16 && !lds_ok) return (int)hipErrorInvalidValue;
  dim3 grid((unsigned)(N / SK_NT), 1, 1);
#define KF_SKL_LAUNCH(KERNEL, THREADS)                                    \
  hipLaunchKernelGGL(KERNEL, grid, dim3(THREADS), 0, (hipStream_t)stream, \
                     (unsigned short*)c, (const unsigned short*)a,        \
                     (const unsigned short*)w, (const unsigned short*)res, \
                     (int)M, N, K, lda, ldw, ldc)
  if (lds_ok && M > 16) KF_SKL_LAUNCH(kf_skinny_lds_kernel<32>, SKL_W * 64);
  else if (lds_ok) KF_SKL_LAUNCH(kf_skinny_lds_kernel<16>, SKL_W * 64);
  // direct-load fallback: 8 waves when the grid can't fill the chip with
  // 4-wave blocks (<2 blocks/CU), 4 otherwise
  else if (N / SK_NT < 512) KF_SKL_LAUNCH(kf_skinny_gemm_kernel<8>, 8 * 64);
  else KF_SKL_LAUNCH(kf_skinny_gemm_kernel<4>, 4 * 64);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------
// Grouped kernels for routed MoE decode: one launch runs every expert's
// skinny GEMM over the permuted [total_rows, .] buffer,
//   lo = offsets[e], m = offsets[e+1] - lo
//   c[lo + i, :] = a[a_rows ? a_rows[lo + i] : lo + i, :] @ w_bank[e]^T
// with grid = (N/16, n_groups), so the expert index is block-uniform and
// each block reads its two offsets itself (the int32 array kf_moe_sort
// writes): nothing is read back to the host, and a captured graph follows
// the routing of every replay. A token's k experts are distinct, so with T
// decode tokens no expert holds more than T rows; the host passes that
// bound as max_rows (1..32) and it picks the M-tile the way M does above.
//
// Each grouped kernel is a prologue (the group's range, the early return for
// an expert without rows, the bank offset) in front of what the plain kernel
// of its family runs, with the A-row pointer going through a_rows, C rows
// offset by lo and no residual (the MoE output goes through combine). For the
// direct and q8 families that is the same __device__ body; the LDS bf16
// kernel repeats kf_skinny_lds_kernel line for line (see the file header).
// K split, LDS staging, MFMA sequence and reduction order are the plain
// kernel's, so the rows of expert e are the bits kf_skinny_gemm /
// kf_skinny_gemm_q8 give for the same rows and w_bank[e].
//
// Memory safety, not validation (as seq_lens in attention_d64.hip): m is
// clamped into [0, min(max_rows, total_rows)], lo into [0, total_rows - m]
// and every a_rows entry into [0, a_nrows), so no content of offsets or
// a_rows can cause an out-of-range access; wrong offsets give wrong rows.

struct kf_sk_group {
  int lo, m;
};

__device__ __forceinline__ kf_sk_group kf_sk_group_range(
    const int* __restrict__ offsets, int e, int max_rows, int total_rows) {
  kf_sk_group g;
  const int lo = offsets[e];
  const int cap = max_rows < total_rows ? max_rows : total_rows;
  // 64-bit difference: offsets[e+1] - lo cannot wrap for garbage offsets
  const int64_t d = (int64_t)offsets[e + 1] - lo;
  g.m = d < 0 ? 0 : (d > cap ? cap : (int)d);
  g.lo = lo < 0 ? 0 : (lo > total_rows - g.m ? total_rows - g.m : lo);
  return g;
}

// group g of a contiguous problem: c [total_rows, N], a [a_nrows, K]
__device__ __forceinline__ kf_sk_prob kf_sk_group_prob(
    unsigned short* c, const unsigned short* a, const int* a_rows,
    int a_nrows, kf_sk_group g, int64_t N, int64_t K) {
  return kf_sk_prob{c, a, nullptr, a_rows, a_nrows, g.lo, g.m, N, K, K, K, N};
}

template <int SKW>
__global__ __launch_bounds__(SKW * 64, 2) void kf_skinny_gemm_grouped_kernel(
    unsigned short* __restrict__ c, const unsigned short* __restrict__ a,
    const unsigned short* __restrict__ w_bank,
    const int* __restrict__ offsets, const int* __restrict__ a_rows,
    int max_rows, int total_rows, int a_nrows, int64_t N, int64_t K) {
  __shared__ float red[SKW][SK_NT][SK_NT];
  const kf_sk_group g =
      kf_sk_group_range(offsets, blockIdx.y, max_rows, total_rows);
  // an expert without rows leaves before any load of W: decode is
  // weight-bandwidth-bound, and the unrouted experts' banks staying in HBM
  // is the whole saving over running every expert on every token
  if (g.m == 0) return;
  kf_sk_direct_body<SKW>(kf_sk_group_prob(c, a, a_rows, a_nrows, g, N, K),
                         w_bank + (int64_t)blockIdx.y * N * K, red);
}

template <int MT>
__global__ __launch_bounds__(SKL_W * 64, 2) void kf_skinny_lds_grouped_kernel(
    unsigned short* __restrict__ c, const unsigned short* __restrict__ a,
    const unsigned short* __restrict__ w_bank,
    const int* __restrict__ offsets, const int* __restrict__ a_rows,
    int max_rows, int total_rows, int a_nrows, int64_t N, int64_t K) {
  __shared__ unsigned short wbuf[2][SK_NT][SKL_STRIDE];
  __shared__ float red[SKL_W][MT][SK_NT];
  const kf_sk_group g =
      kf_sk_group_range(offsets, blockIdx.y, max_rows, total_rows);
  if (g.m == 0) return;  // before any load of W (see the direct kernel)
  const int M = g.m;
  const unsigned short* w = w_bank + (int64_t)blockIdx.y * N * K;

  // from here on kf_skinny_lds_kernel, line for line, but for the A-row
  // pointer, lda = ldw = K, ldc = N, C rows offset by lo and no residual
  const int64_t n0 = (int64_t)blockIdx.x * SK_NT;
  const int tid = threadIdx.x;
  const int wv = tid / KF_WAVE;
  const int lane = tid & (KF_WAVE - 1);
  const int l15 = lane & 15;
  const int hi4 = lane >> 4;

  const int NMT = MT / 16;
  kf_f32x4s acc[NMT];
  bool arow_ok[NMT];
  const unsigned short* arow[NMT];
#pragma unroll
  for (int t = 0; t < NMT; ++t) {
    acc[t] = kf_f32x4s{0.f, 0.f, 0.f, 0.f};
    arow_ok[t] = l15 + 16 * t < M;
    arow[t] = a + kf_sk_a_row(a_rows,
                              g.lo + (arow_ok[t] ? l15 + 16 * t : 0),
                              a_nrows) * K;
  }
  const kf_bf16x8s zero8 = kf_bf16x8s{0, 0, 0, 0, 0, 0, 0, 0};
  const unsigned short* wr0 = w + (n0 + 2 * wv) * K + lane * 8;
  const unsigned short* wr1 = wr0 + K;

  const int64_t nch = K / SKL_KC;
  const int ke0 = wv * 64 + hi4 * 8;
  kf_bf16x8s st0 = *reinterpret_cast<const kf_bf16x8s*>(wr0);
  kf_bf16x8s st1 = *reinterpret_cast<const kf_bf16x8s*>(wr1);
  kf_bf16x8s af0[NMT], af1[NMT];
#pragma unroll
  for (int t = 0; t < NMT; ++t) {
    af0[t] = arow_ok[t]
        ? *reinterpret_cast<const kf_bf16x8s*>(arow[t] + ke0) : zero8;
    af1[t] = arow_ok[t]
        ? *reinterpret_cast<const kf_bf16x8s*>(arow[t] + ke0 + 32) : zero8;
  }
  *reinterpret_cast<kf_bf16x8s*>(&wbuf[0][2 * wv][lane * 8]) = st0;
  *reinterpret_cast<kf_bf16x8s*>(&wbuf[0][2 * wv + 1][lane * 8]) = st1;
  for (int64_t ch = 0; ch < nch; ++ch) {
    kf_bf16x8s a0[NMT], a1[NMT];
#pragma unroll
    for (int t = 0; t < NMT; ++t) {
      a0[t] = af0[t];
      a1[t] = af1[t];
    }
    if (ch + 1 < nch) {
      st0 = *reinterpret_cast<const kf_bf16x8s*>(wr0 + (ch + 1) * SKL_KC);
      st1 = *reinterpret_cast<const kf_bf16x8s*>(wr1 + (ch + 1) * SKL_KC);
#pragma unroll
      for (int t = 0; t < NMT; ++t)
        if (arow_ok[t]) {
          af0[t] = *reinterpret_cast<const kf_bf16x8s*>(
              arow[t] + (ch + 1) * SKL_KC + ke0);
          af1[t] = *reinterpret_cast<const kf_bf16x8s*>(
              arow[t] + (ch + 1) * SKL_KC + ke0 + 32);
        }
    }
    __syncthreads();
    kf_bf16x8s wf0 =
        *reinterpret_cast<const kf_bf16x8s*>(&wbuf[ch & 1][l15][ke0]);
    kf_bf16x8s wf1 =
        *reinterpret_cast<const kf_bf16x8s*>(&wbuf[ch & 1][l15][ke0 + 32]);
#pragma unroll
    for (int t = 0; t < NMT; ++t) {
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[t], wf0, acc[t],
                                                       0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[t], wf1, acc[t],
                                                       0, 0, 0);
    }
    if (ch + 1 < nch) {
      const int b = (int)((ch + 1) & 1);
      *reinterpret_cast<kf_bf16x8s*>(&wbuf[b][2 * wv][lane * 8]) = st0;
      *reinterpret_cast<kf_bf16x8s*>(&wbuf[b][2 * wv + 1][lane * 8]) = st1;
    }
  }
#pragma unroll
  for (int t = 0; t < NMT; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      red[wv][16 * t + hi4 * 4 + j][l15] = acc[t][j];
  __syncthreads();
  if (tid < MT * SK_NT) {
    const int row = tid / SK_NT, col = tid % SK_NT;
    if (row < M && n0 + col < N) {
      float s = 0.f;
#pragma unroll
      for (int ww = 0; ww < SKL_W; ++ww) s += red[ww][row][col];
      c[(int64_t)(g.lo + row) * N + n0 + col] = kf_f32_to_bf16(s);
    }
  }
}

// w8 is the bank flattened to [n_groups * N, K] fp8 rows, one fp32 scale per
// row: expert e, column n uses wscale[e * N + n]
template <int MT>
__global__ __launch_bounds__(SKL_W * 64, 2) void kf_skinny_q8_grouped_kernel(
    unsigned short* __restrict__ c, const unsigned short* __restrict__ a,
    const unsigned char* __restrict__ w8_bank,
    const float* __restrict__ wscale_bank, const int* __restrict__ offsets,
    const int* __restrict__ a_rows, int max_rows, int total_rows,
    int a_nrows, int64_t N, int64_t K) {
  __shared__ unsigned char wbuf8[2][SK_NT][SKQ_STRIDE];
  __shared__ float red[SKL_W][MT][SK_NT];
  const kf_sk_group g =
      kf_sk_group_range(offsets, blockIdx.y, max_rows, total_rows);
  if (g.m == 0) return;  // before any load of W (see the direct kernel)
  kf_sk_q8_body<MT>(kf_sk_group_prob(c, a, a_rows, a_nrows, g, N, K),
                    w8_bank + (int64_t)blockIdx.y * N * K,
                    wscale_bank + (int64_t)blockIdx.y * N, wbuf8, red);
}

// shape limits shared by the two grouped entry points; the row counts are
// int32 in the kernels
static bool kf_sk_grouped_ok(int64_t n_groups, int64_t max_rows,
                             int64_t total_rows, int64_t a_nrows, int64_t N) {
  return n_groups >= 1 && n_groups <= 65535 && max_rows >= 1 &&
         max_rows <= 32 && total_rows >= 0 && total_rows < INT32_MAX &&
         a_nrows >= 1 && a_nrows < INT32_MAX && N >= SK_NT && N % SK_NT == 0 &&
         N / SK_NT < INT32_MAX;
}

// c [total_rows, N], a [a_nrows, K] (a_rows null: a_nrows == total_rows),
// w_bank [n_groups, N, K], all contiguous bf16; offsets int32 [n_groups + 1],
// a_rows nullable int32 [total_rows]; both device arrays.
KF_EXPORT int kf_skinny_gemm_grouped(void* c, const void* a,
                                     const void* w_bank, const int* offsets,
                                     const int* a_rows, int64_t n_groups,
                                     int64_t max_rows, int64_t total_rows,
                                     int64_t a_nrows, int64_t N, int64_t K,
                                     void* stream) {
  if (!kf_sk_grouped_ok(n_groups, max_rows, total_rows, a_nrows, N) ||
      K < 32 || K % 32 || (!a_rows && a_nrows < total_rows))
    return (int)hipErrorInvalidValue;
  const bool lds_ok = K % SKL_KC == 0;
  if (max_rows > 16 && !lds_ok) return (int)hipErrorInvalidValue;
  if (total_rows == 0) return 0;
  dim3 grid((unsigned)(N / SK_NT), (unsigned)n_groups, 1);
#define KF_SKG_LAUNCH(KERNEL, THREADS)                                     \
  hipLaunchKernelGGL(KERNEL, grid, dim3(THREADS), 0, (hipStream_t)stream,  \
                     (unsigned short*)c, (const unsigned short*)a,         \
                     (const unsigned short*)w_bank, offsets, a_rows,       \
                     (int)max_rows, (int)total_rows, (int)a_nrows, N, K)
  if (lds_ok && max_rows > 16)
    KF_SKG_LAUNCH(kf_skinny_lds_grouped_kernel<32>, SKL_W * 64);
  else if (lds_ok)
    KF_SKG_LAUNCH(kf_skinny_lds_grouped_kernel<16>, SKL_W * 64);
  else if (N / SK_NT < 512)  // the direct kernels, chosen as kf_skinny_gemm does
    KF_SKG_LAUNCH(kf_skinny_gemm_grouped_kernel<8>, 8 * 64);
  else
    KF_SKG_LAUNCH(kf_skinny_gemm_grouped_kernel<4>, 4 * 64);
  return (int)hipGetLastError();
}

// as above with w8 [n_groups * N, K] e4m3 and wscale fp32 [n_groups * N]
KF_EXPORT int kf_skinny_gemm_grouped_q8(void* c, const void* a,
                                        const void* w8, const float* wscale,
                                        const int* offsets, const int* a_rows,
                                        int64_t n_groups, int64_t max_rows,
                                        int64_t total_rows, int64_t a_nrows,
                                        int64_t N, int64_t K, void* stream) {
  if (!kf_sk_grouped_ok(n_groups, max_rows, total_rows, a_nrows, N) ||
      K < SKQ_KC || K % SKQ_KC || (!a_rows && a_nrows < total_rows))
    return (int)hipErrorInvalidValue;
  if (total_rows == 0) return 0;
  dim3 grid((unsigned)(N / SK_NT), (unsigned)n_groups, 1);
#define KF_SKGQ_LAUNCH(MT)                                                   \
  hipLaunchKernelGGL(kf_skinny_q8_grouped_kernel<MT>, grid,                  \
                     dim3(SKL_W * 64), 0, (hipStream_t)stream,               \
                     (unsigned short*)c, (const unsigned short*)a,           \
                     (const unsigned char*)w8, wscale, offsets, a_rows,      \
                     (int)max_rows, (int)total_rows, (int)a_nrows, N, K)
  if (max_rows > 16) KF_SKGQ_LAUNCH(32);
  else KF_SKGQ_LAUNCH(16);
  return (int)hipGetLastError();
}

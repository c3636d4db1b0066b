// gemm_q4.hip — wide-M MXFP4 linear (W4A16): C[M,N] = A[M,K] @ dq(W4)[N,K]^T
// (+ res) for any M >= 1, the prefill-shaped sibling of skinny_gemm.hip's q4
// body. bf16 a / c / res, fp32 accumulation, one bf16 store. W is the pair
// ops.quantize_mxfp4_rows returns (e2m1 nibbles [N, K/2], low nibble first, an
// e8m0 byte per 32 along K [N, K/32]); its fragments convert to bf16 in
// registers (kf_fp4x8_to_bf16x8, exact), so the result is the bf16 product on
// the dequantized weights up to summation order. Activations stay bf16.
//
// A compute-shaped tile GEMM: 256 threads = 4 waves as 2 (M) x 2 (N), block
// tile 128 x 128, a wave 64 x 64 of C as 2 x 2 mfma_f32_32x32x16_bf16 tiles
// (64 accumulator registers). The MFMA runs swapped, C^T = mfma(W, A): W rows
// are the A operand, activation rows the B operand, so a lane's accumulator is
// one C row (m = lane&31) and 4 consecutive n per register quad, and the
// epilogue stores 8 B per quad (kf_store_row64's pattern in attention_d64.hip).
//
// K step 64, double-buffered; the loop is unrolled over the buffer pair, one
// iteration = 128 k, which is what K % 128 == 0 buys: static LDS addresses for
// both buffers and ONE aligned 32-bit word of scale bytes per W row and
// iteration, loaded straight from global by the lanes that convert that row
// (as the q4 skinny body does), never through LDS.
//   LDS per stage: A 128 rows x 128 B = 16 KB, W 128 rows x 32 B = 4 KB
//   per block:     2 x 20 KB = 40 KB  -> 4 blocks/CU of the 160 KB (the
//                  register count, below, then sets 3: 12 waves/CU)
//   a 128-k stage: 2 x 40 KB = 80 KB  -> 1 block/CU = 1 wave/SIMD, with
//                  nothing to cover a barrier. Hence 64.
// The next stage's global loads (4 b128 of A and 1 of W per thread) are issued
// before the barrier and the MFMAs of the current stage and written to LDS
// after them: one barrier per stage (attention_d64.hip's register prefetch).
//
// A tile: bf16 rows of 128 B with the family's byte ^= (row&7)<<4 swizzle
// (kf_swz); rows >= M are staged as zeros and never stored.
// W tile: the raw fp4 bytes, never a bf16 copy: a quarter of the LDS bytes and
// LDS write traffic of a bf16 B tile. A fragment of the 32x32x16 MFMA is 8
// consecutive k of one row = one 32-bit word; sub-steps start at multiples of
// 16 and a half-fragment at +0 or +8, so the 8 elements share one MX block and
// one scale byte. Layout [ks = k/16][row][2 words]: lane (l31, hi) of a wave
// reads word (ks*128 + row0 + l31)*2 + hi with row0 a multiple of 32, i.e.
// bank (2*l31 + hi) mod 64: the 64 lanes read 64 different banks, no padding.
// The writer (thread t: row t>>1, 16 B = sub-steps 2*(t&1), +1) stores two
// b64: per 32-lane pass 16 rows x 2 sub-steps on banks 2*row.., 2-way.
// Each wave converts only the fragments of its own 64 columns.
//
// Grid (ceil(M/128), ceil(N/128)): blocks that share an N tile are adjacent in
// launch order, so a 4-bit weight tile is read from HBM once and from L2 after
// that. A wave skips its 32-row / 32-column MFMA tiles past M / N; blocks with
// all tiles live run the same loop without the guards.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   168 VGPRs, scratch 0, LDS 40,960 B, 3 waves/SIMD

#include "kf_attn_common.h"
#include "kf_fp4.h"

typedef unsigned int kf_u32x4g __attribute__((ext_vector_type(4)));
typedef unsigned int kf_u32x2g __attribute__((ext_vector_type(2)));

#define GQ_BM 128                    // C rows per block
#define GQ_BN 128                    // C columns per block
#define GQ_KS 64                     // k per stage
#define GQ_THREADS 256
#define GQ_A_ROWB (GQ_KS * 2)        // 128 B per staged A row
#define GQ_A_TILEB (GQ_BM * GQ_A_ROWB)  // 16 KB
#define GQ_W_TILEB (GQ_BN * GQ_KS / 2)  // 4 KB

// What one thread stages per K step: 4 b128 of A (rows (t>>3) + 32j, 16 B
// chunk t&7: 8 lanes cover one 128 B row segment) and 1 b128 of W.
struct kf_gq_stage {
  kf_short8 a[4];
  kf_u32x4g w;

  __device__ __forceinline__ void load(const unsigned short* ag, int64_t lda,
                                       const bool (&aok)[4],
                                       const unsigned char* wg, int64_t k0) {
    const kf_short8 zero = kf_short8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      a[j] = aok[j] ? *reinterpret_cast<const kf_short8*>(
                          ag + (int64_t)(32 * j) * lda + k0)
                    : zero;
    w = *reinterpret_cast<const kf_u32x4g*>(wg + (k0 >> 1));
  }

  __device__ __forceinline__ void put(unsigned char* a_lds,
                                      unsigned char* w_lds, int tid) const {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<kf_short8*>(
          a_lds + kf_swz((tid >> 3) + 32 * j, (tid & 7) * 16, GQ_A_ROWB)) =
          a[j];
    const int row = tid >> 1, ks = (tid & 1) * 2;
    *reinterpret_cast<kf_u32x2g*>(w_lds + ((ks * GQ_BN + row) << 3)) =
        kf_u32x2g{w[0], w[1]};
    *reinterpret_cast<kf_u32x2g*>(w_lds + (((ks + 1) * GQ_BN + row) << 3)) =
        kf_u32x2g{w[2], w[3]};
  }
};

// The MFMAs of one staged K step. acc[j][i]: n-tile j, m-tile i of the wave.
// sc[j]: the scale word of this lane's row in n-tile j for the 128-k
// iteration; `half` (0 / 1) selects its low or high byte pair. GUARD: skip
// the tiles not in `live` (wave-uniform).
template <bool GUARD>
__device__ __forceinline__ void kf_gq_compute(
    kf_f32x16 (&acc)[2][2], const unsigned char* a_lds,
    const unsigned char* w_lds, const unsigned int (&sc)[2], int half,
    const bool (&live)[2][2], int arow, int wword) {
  const int hi = (threadIdx.x & 63) >> 5;
  // the LDS reads of sub-step ks + 1 are issued before the MFMAs of ks and
  // pinned there (sched_barrier): left alone the scheduler hoists the reads of
  // all four sub-steps above the first MFMA, 209 VGPRs and 2 waves/SIMD
  kf_bf16x8 xf[2][2];
  unsigned int word[2][2];
  auto read = [&](int ks) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      xf[ks & 1][i] = *reinterpret_cast<const kf_bf16x8*>(
          a_lds + kf_swz(arow + 32 * i, ks * 32 + hi * 16, GQ_A_ROWB));
#pragma unroll
    for (int j = 0; j < 2; ++j)
      word[ks & 1][j] = *reinterpret_cast<const unsigned int*>(
          w_lds + ((ks * GQ_BN + 32 * j) << 3) + wword);
  };
  read(0);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    if (ks < 3) read(ks + 1);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (GUARD && !live[j][0] && !live[j][1]) continue;
      const kf_bf16x8 wf = kf_fp4x8_to_bf16x8(
          word[ks & 1][j], (sc[j] >> (16 * half + 8 * (ks >> 1))) & 0xffu);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (GUARD && !live[j][i]) continue;
        acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            wf, xf[ks & 1][i], acc[j][i], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// One block. GUARD = false: every tile of the block is live (block-uniform,
// chosen by the kernel below). The two instantiations are whole bodies, not a
// branch per stage: with both MFMA sequences inside one K loop the register
// allocator spilled (168 VGPRs + 336 B of scratch).
template <bool GUARD>
__device__ __forceinline__ void kf_gq_body(
    unsigned short* __restrict__ c, const unsigned short* __restrict__ a,
    const unsigned char* __restrict__ w4,
    const unsigned char* __restrict__ wscale,
    const unsigned short* __restrict__ res, int64_t M, int64_t N, int64_t K,
    int64_t lda, int64_t ldw, int64_t ldc,
    unsigned char (&a_lds)[2][GQ_A_TILEB],
    unsigned char (&w_lds)[2][GQ_W_TILEB]) {
  const int tid = threadIdx.x;
  const int wv = tid / KF_WAVE, wm = wv >> 1, wn = wv & 1;
  const int lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * GQ_BM;
  const int64_t n0 = (int64_t)blockIdx.y * GQ_BN;

  // staging: this thread's 4 A rows (zeros past M) and its W row (a row past
  // N reads row N - 1: its tiles are never multiplied)
  bool aok[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) aok[j] = m0 + (tid >> 3) + 32 * j < M;
  const unsigned short* ag =
      a + (aok[0] ? m0 + (tid >> 3) : 0) * lda + (tid & 7) * 8;
  const int64_t wrow = n0 + (tid >> 1) < N ? n0 + (tid >> 1) : N - 1;
  const unsigned char* wg = w4 + wrow * (ldw >> 1) + (tid & 1) * 16;

  // this wave's tiles, and this lane's scale rows (one per n-tile)
  bool live[2][2];
  const unsigned char* sg[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t nt = n0 + wn * 64 + 32 * j;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      live[j][i] = nt < N && m0 + wm * 64 + 32 * i < M;
    sg[j] = wscale + (nt + l31 < N ? nt + l31 : N - 1) * (ldw >> 5);
  }
  const int arow = wm * 64 + l31;
  const int wword = ((wn * 64 + l31) << 3) + hi * 4;

  kf_f32x16 acc[2][2] = {{kf_f32x16{0.f}, kf_f32x16{0.f}},
                         {kf_f32x16{0.f}, kf_f32x16{0.f}}};

  const int64_t npair = K / (2 * GQ_KS);
  kf_gq_stage st;
  st.load(ag, lda, aok, wg, 0);
  unsigned int scn[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
    scn[j] = *reinterpret_cast<const unsigned int*>(sg[j]);
  st.put(a_lds[0], w_lds[0], tid);

  for (int64_t p = 0; p < npair; ++p) {
    const unsigned int sc[2] = {scn[0], scn[1]};
    // stage 2p in buffer 0; 2p + 1 exists (K % 128 == 0)
    st.load(ag, lda, aok, wg, (2 * p + 1) * GQ_KS);
    // one barrier per stage: the buffer's writes are visible, and the readers
    // of the other buffer (the stage before) are done
    __syncthreads();
    kf_gq_compute<GUARD>(acc, a_lds[0], w_lds[0], sc, 0, live, arow, wword);
    st.put(a_lds[1], w_lds[1], tid);
    // stage 2p + 1 in buffer 1
    const bool more = p + 1 < npair;
    if (more) {
      st.load(ag, lda, aok, wg, (2 * p + 2) * GQ_KS);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        scn[j] = *reinterpret_cast<const unsigned int*>(sg[j] + (p + 1) * 4);
    }
    __syncthreads();
    kf_gq_compute<GUARD>(acc, a_lds[1], w_lds[1], sc, 1, live, arow, wword);
    if (more) st.put(a_lds[0], w_lds[0], tid);
  }

  // epilogue. C^T layout of the 32x32x16 MFMA: col = lane&31 is the C row,
  // row = (reg&3) + 8*(reg>>2) + 4*hi the C column: 4 consecutive n per quad
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t m = m0 + wm * 64 + 32 * i + l31;
      if (!live[j][i] || m >= M) continue;
      const int64_t at0 = m * ldc + n0 + wn * 64 + 32 * j + 4 * hi;
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        float v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = acc[j][i][rq * 4 + t];
        if (res) {
          const kf_short4 r =
              *reinterpret_cast<const kf_short4*>(res + at0 + 8 * rq);
#pragma unroll
          for (int t = 0; t < 4; ++t)
            v[t] += kf_bf16_to_f32((unsigned short)r[t]);
        }
        unsigned int u[2] = {kf_cvt_pk_bf16_builtin(v[0], v[1]),
                             kf_cvt_pk_bf16_builtin(v[2], v[3])};
        *reinterpret_cast<kf_short4*>(c + at0 + 8 * rq) =
            *reinterpret_cast<kf_short4*>(u);
      }
    }
}

__global__ __launch_bounds__(GQ_THREADS, 3) void kf_gemm_q4_kernel(
    unsigned short* __restrict__ c, const unsigned short* __restrict__ a,
    const unsigned char* __restrict__ w4,
    const unsigned char* __restrict__ wscale,
    const unsigned short* __restrict__ res, int64_t M, int64_t N, int64_t K,
    int64_t lda, int64_t ldw, int64_t ldc) {
  __shared__ __attribute__((aligned(16))) unsigned char a_lds[2][GQ_A_TILEB];
  __shared__ __attribute__((aligned(16))) unsigned char w_lds[2][GQ_W_TILEB];
  const bool full = ((int64_t)blockIdx.x + 1) * GQ_BM <= M &&
                    ((int64_t)blockIdx.y + 1) * GQ_BN <= N;
  if (full)
    kf_gq_body<false>(c, a, w4, wscale, res, M, N, K, lda, ldw, ldc, a_lds,
                      w_lds);
  else
    kf_gq_body<true>(c, a, w4, wscale, res, M, N, K, lda, ldw, ldc, a_lds,
                     w_lds);
}

// w4 [N, ldw / 2] bytes, wscale [N, ldw / 32] e8m0 bytes; ldw in fp4
// elements; lda / ldw / ldc 0 = dense (kf_skinny_gemm_q4's conventions)
KF_EXPORT int kf_gemm_q4(void* c, const void* a, const void* w4,
                         const unsigned char* wscale, const void* res,
                         int64_t M, int64_t N, int64_t K, int64_t lda,
                         int64_t ldw, int64_t ldc, void* stream) {
  if (M < 1 || M > INT32_MAX - GQ_BM || K < 128 || K % 128 || N < 32 ||
      N % 32 || N / GQ_BN >= 65535)
    return (int)hipErrorInvalidValue;
  if (lda == 0) lda = K;
  if (ldw == 0) ldw = K;
  if (ldc == 0) ldc = N;
  // 16 B loads of A and W rows, 4 B scale words, 8 B stores of C (and loads
  // of res, which has C's layout)
  if (lda < K || lda % 8 || ldw < K || ldw % 128 || ldc < N || ldc % 4 ||
      (uintptr_t)a % 16 || (uintptr_t)w4 % 16 || (uintptr_t)wscale % 4 ||
      (uintptr_t)c % 8 || (uintptr_t)res % 8)
    return (int)hipErrorInvalidValue;
  dim3 grid((unsigned)((M + GQ_BM - 1) / GQ_BM),
            (unsigned)((N + GQ_BN - 1) / GQ_BN), 1);
  hipLaunchKernelGGL(kf_gemm_q4_kernel, grid, dim3(GQ_THREADS), 0,
                     (hipStream_t)stream, (unsigned short*)c,
                     (const unsigned short*)a, (const unsigned char*)w4,
                     wscale, (const unsigned short*)res, M, N, K, lda, ldw,
                     ldc);
  return (int)hipGetLastError();
}

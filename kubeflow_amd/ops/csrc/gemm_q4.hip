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
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), every
// kernel scratch 0, LDS 40,960 B, 3 waves/SIMD:
//   kf_gemm_q4_kernel                      168 VGPRs
//   kf_gemm_q4_grouped_kernel<rows, swiglu>
//     <0, 0> 165   <0, 1> 163   <1, 0> 147   <1, 1> 147 VGPRs
// The grouped form (kf_gemm_q4_grouped, at the end of the file) runs the same
// block per expert over device offsets; the body takes what differs between
// the two as a kf_gq_prob.

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

  // GATHER: row j is row arow[j] of the matrix ag points into (its column
  // chunk already added); else row 32 * j below ag
  template <bool GATHER>
  __device__ __forceinline__ void load(const unsigned short* ag, int64_t lda,
                                       const int (&arow)[4],
                                       const bool (&aok)[4],
                                       const unsigned char* wg, int64_t k0) {
    const kf_short8 zero = kf_short8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      a[j] = aok[j] ? *reinterpret_cast<const kf_short8*>(
                          ag + (int64_t)(GATHER ? arow[j] : 32 * j) * lda + k0)
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

// What one block computes, as its body sees it (kf_sk_prob's role in
// skinny_gemm.hip): the 128 x 128 tile (tm, tn) of C[M, N] = A W^T (+ res).
// The plain kernel fills it from its arguments and blockIdx; the grouped one
// with the rows and the bank slice of the expert its prologue found. The body
// takes no "grouped" flag.
struct kf_gq_prob {
  unsigned short* c;
  const unsigned short* a;
  const unsigned char* w4;
  const unsigned char* wscale;
  const unsigned short* res;  // nullable
  const int* a_rows;          // GATHER bodies only: entry of problem row 0
  int a_nrows;
  int64_t M, N, K, lda, ldw, ldc;
  int64_t tm, tn;  // the block's tile: rows 128 tm .., columns 128 tn ..
                   // (SWIGLU: 64 tn ..)
};

// One block. GUARD = false: every tile of the block is live (block-uniform,
// chosen by the kernel below). The two instantiations are whole bodies, not a
// branch per stage: with both MFMA sequences inside one K loop the register
// allocator spilled (168 VGPRs + 336 B of scratch).
//
// GATHER: A row m of the problem is row a_rows[m] of a, clamped into
// [0, a_nrows). Only the stager changes: its four rows become four indices.
// SWIGLU: W is a w13 bank slice [2 N, K], gate rows then up rows, and the
// block makes 64 columns (n0 = 64 tn) of silu(gate) * up. Its 128
// staged W rows are 64 gate rows and their 64 up rows, LDS row r holding
//   W row (r>>5 & 1 ? N : 0) + n0 + 32 * (r>>6) + (r & 31),
// so wave wn has gate in its n-tile j = 0 and up in j = 1 for the same 32
// columns n0 + 32 wn .., in the same lane and register index; the epilogue
// multiplies the fp32 accumulators and rounds once. The LDS layout and
// kf_gq_compute do not know.
//
// kf_gq_body (below) unpacks a kf_gq_prob into these parameters: the
// __restrict__ qualifiers have to sit on function parameters to reach the
// inlined loads and stores.
template <bool GUARD, bool GATHER, bool SWIGLU>
__device__ __forceinline__ void kf_gq_tile(
    unsigned short* __restrict__ c, const unsigned short* __restrict__ a,
    const unsigned char* __restrict__ w4,
    const unsigned char* __restrict__ wscale,
    const unsigned short* __restrict__ res, int64_t M, int64_t N, int64_t K,
    int64_t lda, int64_t ldw, int64_t ldc, int64_t tm, int64_t tn,
    const int* __restrict__ a_rows, int a_nrows,
    unsigned char (&a_lds)[2][GQ_A_TILEB],
    unsigned char (&w_lds)[2][GQ_W_TILEB]) {
  const int tid = threadIdx.x;
  const int wv = tid / KF_WAVE, wm = wv >> 1, wn = wv & 1;
  const int lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int64_t m0 = tm * GQ_BM;
  const int64_t n0 = tn * (SWIGLU ? GQ_BN / 2 : GQ_BN);

  // staging: this thread's 4 A rows (zeros past M) and its W row (a row past
  // N reads row N - 1: its tiles are never multiplied)
  bool aok[4];
  int gidx[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    aok[j] = m0 + (tid >> 3) + 32 * j < M;
    if (GATHER && aok[j]) {
      const int s = a_rows[m0 + (tid >> 3) + 32 * j];
      gidx[j] = s < 0 ? 0 : (s >= a_nrows ? a_nrows - 1 : s);
    }
  }
  const unsigned short* ag =
      GATHER ? a + (tid & 7) * 8
             : a + (aok[0] ? m0 + (tid >> 3) : 0) * lda + (tid & 7) * 8;
  int64_t wrow;
  if (SWIGLU) {
    const int r = tid >> 1;
    const int64_t o = n0 + 32 * (r >> 6) + (r & 31);
    wrow = (o < N ? o : N - 1) + ((r >> 5) & 1 ? N : 0);
  } else {
    wrow = n0 + (tid >> 1) < N ? n0 + (tid >> 1) : N - 1;
  }
  const unsigned char* wg = w4 + wrow * (ldw >> 1) + (tid & 1) * 16;

  // this wave's tiles, and this lane's scale rows (one per n-tile)
  bool live[2][2];
  const unsigned char* sg[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t nt = n0 + wn * (SWIGLU ? 32 : 64) + (SWIGLU ? 0 : 32 * j);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      live[j][i] = nt < N && m0 + wm * 64 + 32 * i < M;
    sg[j] = wscale + (nt + l31 < N ? nt + l31 : N - 1) * (ldw >> 5);
    if (SWIGLU && j) sg[j] += N * (ldw >> 5);  // the up row
  }
  const int arow = wm * 64 + l31;
  const int wword = ((wn * 64 + l31) << 3) + hi * 4;

  kf_f32x16 acc[2][2] = {{kf_f32x16{0.f}, kf_f32x16{0.f}},
                         {kf_f32x16{0.f}, kf_f32x16{0.f}}};

  const int64_t npair = K / (2 * GQ_KS);
  kf_gq_stage st;
  st.load<GATHER>(ag, lda, gidx, aok, wg, 0);
  unsigned int scn[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
    scn[j] = *reinterpret_cast<const unsigned int*>(sg[j]);
  st.put(a_lds[0], w_lds[0], tid);

  for (int64_t p = 0; p < npair; ++p) {
    const unsigned int sc[2] = {scn[0], scn[1]};
    // stage 2p in buffer 0; 2p + 1 exists (K % 128 == 0)
    st.load<GATHER>(ag, lda, gidx, aok, wg, (2 * p + 1) * GQ_KS);
    // one barrier per stage: the buffer's writes are visible, and the readers
    // of the other buffer (the stage before) are done
    __syncthreads();
    kf_gq_compute<GUARD>(acc, a_lds[0], w_lds[0], sc, 0, live, arow, wword);
    st.put(a_lds[1], w_lds[1], tid);
    // stage 2p + 1 in buffer 1
    const bool more = p + 1 < npair;
    if (more) {
      st.load<GATHER>(ag, lda, gidx, aok, wg, (2 * p + 2) * GQ_KS);
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
  if (SWIGLU) {
    // acc[0][i] is gate and acc[1][i] up of the same (row, column) per
    // register: silu(g) * u in fp32 (kf_swiglu's expression), one rounding
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t m = m0 + wm * 64 + 32 * i + l31;
      if (!live[0][i] || m >= M) continue;
      const int64_t at0 = m * ldc + n0 + wn * 32 + 4 * hi;
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        float v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float g = acc[0][i][rq * 4 + t];
          v[t] = g * (1.f / (1.f + __expf(-g))) * acc[1][i][rq * 4 + t];
        }
        unsigned int u[2] = {kf_cvt_pk_bf16_builtin(v[0], v[1]),
                             kf_cvt_pk_bf16_builtin(v[2], v[3])};
        *reinterpret_cast<kf_short4*>(c + at0 + 8 * rq) =
            *reinterpret_cast<kf_short4*>(u);
      }
    }
    return;
  }
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

template <bool GUARD, bool GATHER, bool SWIGLU>
__device__ __forceinline__ void kf_gq_body(
    const kf_gq_prob& pb, unsigned char (&a_lds)[2][GQ_A_TILEB],
    unsigned char (&w_lds)[2][GQ_W_TILEB]) {
  kf_gq_tile<GUARD, GATHER, SWIGLU>(pb.c, pb.a, pb.w4, pb.wscale, pb.res,
                                    pb.M, pb.N, pb.K, pb.lda, pb.ldw, pb.ldc,
                                    pb.tm, pb.tn, pb.a_rows, pb.a_nrows,
                                    a_lds, w_lds);
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
  // the problem is built inside each branch, and the body multiplies the tile
  // coordinates out itself: that is where the body computed its tile origin
  // when it read blockIdx, and this kernel's instruction stream is, line for
  // line, the one it had then (one kf_gq_prob in front of the branch is not)
#define KF_GQ_PLAIN_PROB                                                 \
  kf_gq_prob {                                                           \
    c, a, w4, wscale, res, nullptr, 0, M, N, K, lda, ldw, ldc,           \
        (int64_t)blockIdx.x, (int64_t)blockIdx.y                         \
  }
  if (full)
    kf_gq_body<false, false, false>(KF_GQ_PLAIN_PROB, a_lds, w_lds);
  else
    kf_gq_body<true, false, false>(KF_GQ_PLAIN_PROB, a_lds, w_lds);
#undef KF_GQ_PLAIN_PROB
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

// ---------------------------------------------------------------------
// Grouped form for routed MoE prefill and verify steps: one launch runs every
// expert's wide GEMM over the permuted [total_rows, .] buffer,
//   lo = offsets[e], m = offsets[e+1] - lo
//   c[lo + i, :] = a[a_rows ? a_rows[lo + i] : lo + i, :] @ dq(bank[e])^T
// (swiglu: silu(gate) * up of the w13 bank's [2f, K] slices, c [., f]) on the
// bank layout of kf_skinny_gemm_grouped_q4, with the body above: the k order
// is kf_gemm_q4's wherever a tile starts, so with swiglu = 0 an expert's rows
// are the bits kf_gemm_q4 gives for the same rows and bank slice.
//
// Tile map without a host sync. How many 128-row tiles an expert needs is
// known only on the device, so the grid is (mt_bound, N tiles) with
//   mt_bound = total_rows / 128 + min(E, total_rows)
//           >= sum_e ceil(m_e / 128)   (each non-empty expert adds at most one
//                                       partial tile, and there are at most
//                                       min(E, total_rows) of those)
// and M tiles fastest, so the blocks that share a weight tile are adjacent in
// launch order as in the plain kernel. Every block finds its tile in registers
// (E <= 64, one lane per expert): lane e loads and clamps its two offsets and
// takes ceil(m_e / 128); an inclusive wave prefix sum and a ballot of
// "prefix > blockIdx.x" give the expert as the first set bit, and readlane
// its lo, m and first tile, all scalars. Each wave computes the same values,
// so the result is block-uniform with no LDS and no barrier, and a block past
// the last tile returns before any load of A or W.
//
// Memory safety, not validation (as the grouped skinny kernels): lo is
// clamped into [0, total_rows], m into [0, total_rows - lo] and every a_rows
// entry into [0, a_nrows), so no content of offsets or a_rows can cause an
// out-of-range access; wrong offsets give wrong rows.

struct kf_gq_group {
  int e, lo, m, mt;  // expert, its first row and row count, the local tile
};

__device__ __forceinline__ bool kf_gq_find_tile(
    const int* __restrict__ offsets, int n_experts, int total_rows, int tile,
    kf_gq_group& g) {
  const int lane = threadIdx.x & 63;
  int lo = 0, m = 0;
  if (lane < n_experts) {
    const int o0 = offsets[lane];
    // 64-bit difference: it cannot wrap for garbage offsets
    const int64_t d = (int64_t)offsets[lane + 1] - o0;
    lo = o0 < 0 ? 0 : (o0 > total_rows ? total_rows : o0);
    m = d < 0 ? 0 : (d > total_rows - lo ? total_rows - lo : (int)d);
  }
  const int nt = (m + GQ_BM - 1) / GQ_BM;
  int incl = nt;  // <= 64 * (2^31 / 128): no overflow
#pragma unroll
  for (int off = 1; off < KF_WAVE; off <<= 1) {
    const int o = __shfl_up(incl, off, KF_WAVE);
    if (lane >= off) incl += o;
  }
  const unsigned long long hit = __ballot(incl > tile);
  if (hit == 0) return false;
  const int e = __builtin_amdgcn_readfirstlane(__builtin_ctzll(hit));
  g.e = e;
  g.lo = __builtin_amdgcn_readlane(lo, e);
  g.m = __builtin_amdgcn_readlane(m, e);
  g.mt = tile - (__builtin_amdgcn_readlane(incl, e) -
                 __builtin_amdgcn_readlane(nt, e));
  return true;
}

// N: output columns (swiglu: f, the bank slice has 2 N rows)
template <bool GATHER, bool SWIGLU>
__global__ __launch_bounds__(GQ_THREADS, 3) void kf_gemm_q4_grouped_kernel(
    unsigned short* __restrict__ c, const unsigned short* __restrict__ a,
    const unsigned char* __restrict__ w4,
    const unsigned char* __restrict__ wscale,
    const int* __restrict__ offsets, const int* __restrict__ a_rows,
    int n_experts, int total_rows, int a_nrows, int64_t N, int64_t K) {
  __shared__ __attribute__((aligned(16))) unsigned char a_lds[2][GQ_A_TILEB];
  __shared__ __attribute__((aligned(16))) unsigned char w_lds[2][GQ_W_TILEB];
  kf_gq_group g;
  if (!kf_gq_find_tile(offsets, n_experts, total_rows, (int)blockIdx.x, g))
    return;
  constexpr int BN = SWIGLU ? GQ_BN / 2 : GQ_BN;
  const int64_t wrows = (int64_t)g.e * (SWIGLU ? 2 * N : N);
  const kf_gq_prob pb{c + (int64_t)g.lo * N,
                      GATHER ? a : a + (int64_t)g.lo * K,
                      w4 + wrows * (K >> 1),
                      wscale + wrows * (K >> 5),
                      nullptr,
                      GATHER ? a_rows + g.lo : nullptr,
                      a_nrows,
                      g.m, N, K, K, K, N,
                      g.mt, (int64_t)blockIdx.y};
  const bool full = (g.mt + 1) * GQ_BM <= g.m &&
                    ((int64_t)blockIdx.y + 1) * BN <= N;
  if (full)
    kf_gq_body<false, GATHER, SWIGLU>(pb, a_lds, w_lds);
  else
    kf_gq_body<true, GATHER, SWIGLU>(pb, a_lds, w_lds);
}

// c [total_rows, swiglu ? N / 2 : N], a [a_nrows, K] (a_rows null: a_nrows >=
// total_rows), all contiguous bf16; w4 [n_experts * N, K / 2], wscale
// [n_experts * N, K / 32]; offsets int32 [n_experts + 1], a_rows nullable
// int32 [total_rows], both device arrays. K % 128 == 0, N % 32 == 0 (swiglu:
// N % 64 == 0), n_experts <= 64.
KF_EXPORT int kf_gemm_q4_grouped(void* c, const void* a, const void* w4,
                                 const unsigned char* wscale,
                                 const int* offsets, const int* a_rows,
                                 int64_t n_experts, int64_t total_rows,
                                 int64_t a_nrows, int64_t N, int64_t K,
                                 int swiglu, void* stream) {
  if (n_experts < 1 || n_experts > 64 || total_rows < 0 ||
      total_rows > INT32_MAX - GQ_BM || a_nrows < 1 || a_nrows >= INT32_MAX ||
      K < 128 || K % 128 || N < 32 || N % 32 || (swiglu && N % 64) ||
      N / (GQ_BN / 2) >= 65535 || (!a_rows && a_nrows < total_rows) ||
      !offsets || (uintptr_t)a % 16 || (uintptr_t)w4 % 16 ||
      (uintptr_t)wscale % 4 || (uintptr_t)c % 8)
    return (int)hipErrorInvalidValue;
  if (total_rows == 0) return 0;
  const int64_t n_out = swiglu ? N / 2 : N;
  const int64_t bn = swiglu ? GQ_BN / 2 : GQ_BN;
  const int64_t mt_bound =
      total_rows / GQ_BM + (n_experts < total_rows ? n_experts : total_rows);
  dim3 grid((unsigned)mt_bound, (unsigned)((n_out + bn - 1) / bn), 1);
#define KF_GQG_LAUNCH(GATHER, SWIGLU)                                         \
  hipLaunchKernelGGL((kf_gemm_q4_grouped_kernel<GATHER, SWIGLU>), grid,       \
                     dim3(GQ_THREADS), 0, (hipStream_t)stream,                \
                     (unsigned short*)c, (const unsigned short*)a,            \
                     (const unsigned char*)w4, wscale, offsets, a_rows,       \
                     (int)n_experts, (int)total_rows, (int)a_nrows, n_out, K)
  if (a_rows && swiglu) KF_GQG_LAUNCH(true, true);
  else if (a_rows) KF_GQG_LAUNCH(true, false);
  else if (swiglu) KF_GQG_LAUNCH(false, true);
  else KF_GQG_LAUNCH(false, false);
  return (int)hipGetLastError();
}

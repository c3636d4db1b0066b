// moe.hip — mixture-of-experts routing, dispatch and combine, CDNA4.
//
// The block is: route (top-k of the router logits) -> sort (a stable counting
// sort of the (token, slot) pairs by expert, giving every pair a row `pos` in
// one permuted buffer) -> gather (x rows into that buffer) -> per-expert GEMMs
// over contiguous slices (hipBLASLt, not here) -> combine (weighted sum of each
// token's k rows). Every contribution row is stored once with plain stores and
// summed per destination through the inverted index `pos` in slot order, so
// all outputs are bitwise reproducible: there is no float atomic in this file
// (the only atomics are integer LDS histogram counts, whose result does not
// depend on order).
//
//   T tokens, E experts, k = top_k, h hidden; [e_lo, e_lo + n_local) is the
//   local expert range and M the number of pairs whose expert is local.
//   Supported: 2 <= E <= 64, 1 <= k <= min(E, 8), h % 8 == 0, T * k < 2^31.
//
// Row kernels give one wave to a row (token or permuted row) and stride the
// lanes over its 16-byte vectors; grids are capped by kf_grid_for and the
// waves grid-stride over rows. Row offsets are int64.

#include "kf_common.h"

#define KF_MOE_MAX_E 64
#define KF_MOE_MAX_K 8
#define KF_MOE_BLOCK 256
#define KF_MOE_WAVES (KF_MOE_BLOCK / KF_WAVE)
// pairs per count chunk: each of the block's 4 waves owns 4 x 64 contiguous
// pairs of it
#define KF_MOE_CHUNK 1024
#define KF_MOE_SEG (KF_MOE_CHUNK / KF_MOE_WAVES)

// ------------------------------------------------------------------ route --

// bf16 bits -> an unsigned key whose integer order is the order of
// torch.sort: -inf < finite < +inf < NaN, -0 == +0, all NaNs equal. Integer
// compares cannot be poisoned by a NaN, so a selection built on them always
// yields k distinct experts.
__device__ __forceinline__ unsigned kf_moe_key(unsigned b) {
  if ((b & 0x7FFFu) > 0x7F80u) return 0xFFFFu;
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}

__device__ __forceinline__ unsigned kf_wave_umax(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    unsigned o = (unsigned)__shfl_xor((int)v, off, KF_WAVE);
    v = o > v ? o : v;
  }
  return v;
}

// One wave per token, lane e holds expert e. Round s takes the maximum of
// (key, 63 - lane) over the lanes not yet taken: the largest logit, the lowest
// expert index among equals. A taken lane and a lane >= E carry 0, below every
// live candidate, and k <= E leaves a live candidate in every round.
__global__ void kf_moe_route_kernel(int* __restrict__ topi,
                                    float* __restrict__ probs,
                                    unsigned short* __restrict__ topw,
                                    const unsigned short* __restrict__ logits,
                                    int64_t T, int E, int k) {
  const int lane = threadIdx.x & (KF_WAVE - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / KF_WAVE;
  const int64_t nwaves = gridDim.x * (int64_t)blockDim.x / KF_WAVE;
  for (int64_t t = wave; t < T; t += nwaves) {
    unsigned bits = 0, cand = 0;
    if (lane < E) {
      bits = logits[t * E + lane];
      cand = ((kf_moe_key(bits) + 1u) << 6) | (unsigned)(63 - lane);
    }
    int my_idx = 0;
    float my_v = 0.f;
    for (int s = 0; s < k; ++s) {
      const unsigned best = kf_wave_umax(cand);
      const int win = 63 - (int)(best & 63u);
      const float v = kf_bf16_to_f32((unsigned short)__shfl((int)bits, win, KF_WAVE));
      if (lane == win) cand = 0;
      if (lane == s) { my_idx = win; my_v = v; }
    }
    // softmax over the k selected logits, fp32; slot 0 holds their maximum
    const float m = __shfl(my_v, 0, KF_WAVE);
    const float ex = lane < k ? expf(my_v - m) : 0.f;
    const float p = ex / kf_wave_sum(ex);
    if (lane < k) {
      topi[t * k + lane] = my_idx;
      probs[t * k + lane] = p;
      topw[t * k + lane] = kf_f32_to_bf16(p);
    }
  }
}

// dlogits[t, topi[t,i]] = p_i * (dw_i - sum_j p_j dw_j), every other entry of
// the row an exact zero: one wave per token, lane e stores column e.
__global__ void kf_moe_route_bwd_kernel(unsigned short* __restrict__ dlogits,
                                        const unsigned short* __restrict__ dw,
                                        const float* __restrict__ probs,
                                        const int* __restrict__ topi,
                                        int64_t T, int E, int k) {
  const int lane = threadIdx.x & (KF_WAVE - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / KF_WAVE;
  const int64_t nwaves = gridDim.x * (int64_t)blockDim.x / KF_WAVE;
  for (int64_t t = wave; t < T; t += nwaves) {
    float p = 0.f, d = 0.f;
    int idx = -1;
    if (lane < k) {
      p = probs[t * k + lane];
      d = kf_bf16_to_f32(dw[t * k + lane]);
      idx = topi[t * k + lane];
    }
    const float dot = kf_wave_sum(p * d);
    const float g = p * (d - dot);
    float val = 0.f;
#pragma unroll
    for (int s = 0; s < KF_MOE_MAX_K; ++s) {
      const int si = __shfl(idx, s, KF_WAVE);
      const float sg = __shfl(g, s, KF_WAVE);
      if (s < k && si == lane) val = sg;
    }
    if (lane < E) dlogits[t * E + lane] = kf_f32_to_bf16(val);
  }
}

// ------------------------------------------------------------------- sort --

// local expert number of a pair, or >= n_local (as unsigned) if not local
__device__ __forceinline__ unsigned kf_moe_local(int e, int e_lo) {
  return (unsigned)e - (unsigned)e_lo;
}

// Stage 1: counts[c, el] = pairs of chunk c routed to local expert el.
__global__ void kf_moe_count_kernel(int* __restrict__ counts,
                                    const int* __restrict__ topi, int64_t P,
                                    int e_lo, int n_local, int64_t nchunks) {
  __shared__ int hist[KF_MOE_MAX_E];
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    if (threadIdx.x < KF_MOE_MAX_E) hist[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < KF_MOE_CHUNK; i += blockDim.x) {
      const int64_t p = c * KF_MOE_CHUNK + i;
      if (p < P) {
        const unsigned el = kf_moe_local(topi[p], e_lo);
        if (el < (unsigned)n_local) atomicAdd(&hist[el], 1);
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < n_local)
      counts[c * n_local + threadIdx.x] = hist[threadIdx.x];
    __syncthreads();
  }
}

// Stage 2 (one wave, thread el): base[c, el] = pairs of el in chunks < c;
// offsets = exclusive scan of the per-expert totals, offsets[n_local] = M.
__global__ void kf_moe_scan_kernel(int* __restrict__ base,
                                   int* __restrict__ offsets,
                                   const int* __restrict__ counts,
                                   int64_t nchunks, int n_local) {
  __shared__ int tot[KF_MOE_MAX_E];
  const int el = threadIdx.x;
  int run = 0;
  if (el < n_local) {
    for (int64_t c = 0; c < nchunks; ++c) {
      base[c * n_local + el] = run;
      run += counts[c * n_local + el];
    }
  }
  tot[el] = run;
  __syncthreads();
  int off = 0;
  for (int i = 0; i < el; ++i) off += tot[i];
  if (el < n_local) offsets[el] = off;
  if (el == n_local - 1) offsets[n_local] = off + run;
}

// Stage 3: pos / src. Wave w of a block owns pairs [w * SEG, (w + 1) * SEG) of
// its chunk and walks them 64 at a time, in order. cnt[w][el] is the next free
// row of expert el as seen by that wave: the expert's offset, plus the chunks
// before this one (base), plus the waves before this one (hist), plus what the
// wave has placed so far. Within a 64-pair step a pair's rank among the pairs
// of its own expert is the popcount, below its lane, of the ballot of lanes
// with the same expert.
__global__ void kf_moe_place_kernel(int* __restrict__ pos,
                                    int* __restrict__ src,
                                    const int* __restrict__ topi,
                                    const int* __restrict__ base,
                                    const int* __restrict__ offsets,
                                    int64_t P, int k, int e_lo, int n_local,
                                    int64_t nchunks) {
  __shared__ int hist[KF_MOE_WAVES][KF_MOE_MAX_E];
  __shared__ volatile int cnt[KF_MOE_WAVES][KF_MOE_MAX_E];
  const int lane = threadIdx.x & (KF_WAVE - 1);
  const int w = threadIdx.x / KF_WAVE;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    hist[w][lane] = 0;
    __syncthreads();
    const int64_t seg = c * KF_MOE_CHUNK + (int64_t)w * KF_MOE_SEG;
    for (int it = 0; it < KF_MOE_SEG / KF_WAVE; ++it) {
      const int64_t p = seg + it * KF_WAVE + lane;
      if (p < P) {
        const unsigned el = kf_moe_local(topi[p], e_lo);
        if (el < (unsigned)n_local) atomicAdd(&hist[w][el], 1);
      }
    }
    __syncthreads();
    if (lane < n_local) {
      int b = offsets[lane] + base[c * n_local + lane];
      for (int i = 0; i < w; ++i) b += hist[i][lane];
      cnt[w][lane] = b;
    }
    __syncthreads();
    for (int it = 0; it < KF_MOE_SEG / KF_WAVE; ++it) {
      const int64_t p = seg + it * KF_WAVE + lane;
      unsigned el = 0xFFFFFFFFu;
      if (p < P) el = kf_moe_local(topi[p], e_lo);
      const bool local = el < (unsigned)n_local;
      unsigned long long same = __ballot(local);
#pragma unroll
      for (int bit = 0; bit < 6; ++bit) {
        const bool on = (el >> bit) & 1u;
        const unsigned long long bm = __ballot(on);
        same &= on ? bm : ~bm;
      }
      if (local) {
        const int rank = __popcll(same & below);
        const int b = cnt[w][el];
        const int dst = b + rank;
        if ((int64_t)dst < P) {  // holds by construction; keeps a corrupt
          pos[p] = dst;          // index from writing out of bounds
          src[dst] = (int)(p / k);
        }
        // the group's last lane advances the counter for the next step; LDS
        // accesses of one wave execute in program order
        if (rank == __popcll(same) - 1) cnt[w][el] = dst + 1;
      } else if (p < P) {
        pos[p] = -1;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------- gather / combine --

__device__ __forceinline__ kf_short8 kf_moe_ld8(const unsigned short* p) {
  return *reinterpret_cast<const kf_short8*>(p);
}

// xp[r] = x[src[r]], r < M.
__global__ void kf_moe_gather_kernel(unsigned short* __restrict__ xp,
                                     const unsigned short* __restrict__ x,
                                     const int* __restrict__ src, int64_t M,
                                     int64_t T, int64_t h) {
  const int lane = threadIdx.x & (KF_WAVE - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / KF_WAVE;
  const int64_t nwaves = gridDim.x * (int64_t)blockDim.x / KF_WAVE;
  const int64_t hv = h / 8;
  for (int64_t r = wave; r < M; r += nwaves) {
    const int64_t t = src[r];
    const bool ok = (uint64_t)t < (uint64_t)T;
    const unsigned short* in = x + (ok ? t : 0) * h;
    unsigned short* out = xp + r * h;
#pragma unroll 4
    for (int64_t c = lane; c < hv; c += KF_WAVE) {
      kf_short8 v = kf_moe_ld8(in + c * 8);
      if (!ok) v = (kf_short8)(0);
      *reinterpret_cast<kf_short8*>(out + c * 8) = v;
    }
  }
}

// out[t] = bf16(sum_s w[t,s] * rows[pos[t,s]]) in fp32, ascending s, from 0,
// slots with pos < 0 skipped. WEIGHTED = false: w = 1 (the gather adjoint).
template <bool WEIGHTED>
__global__ void kf_moe_sum_kernel(unsigned short* __restrict__ out,
                                  const unsigned short* __restrict__ rows,
                                  const unsigned short* __restrict__ topw,
                                  const int* __restrict__ pos, int64_t T,
                                  int k, int64_t h, int64_t M) {
  const int lane = threadIdx.x & (KF_WAVE - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / KF_WAVE;
  const int64_t nwaves = gridDim.x * (int64_t)blockDim.x / KF_WAVE;
  const int64_t hv = h / 8;
  for (int64_t t = wave; t < T; t += nwaves) {
    int pl = -1;
    float wl = 1.f;
    if (lane < k) {
      pl = pos[t * k + lane];
      if ((int64_t)pl >= M) pl = -1;
      if (WEIGHTED) wl = kf_bf16_to_f32(topw[t * k + lane]);
    }
    int ps[KF_MOE_MAX_K];
    float ws[KF_MOE_MAX_K];
#pragma unroll
    for (int s = 0; s < KF_MOE_MAX_K; ++s) {
      ps[s] = __shfl(pl, s, KF_WAVE);
      ws[s] = __shfl(wl, s, KF_WAVE);
    }
    for (int64_t c = lane; c < hv; c += KF_WAVE) {
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
      for (int s = 0; s < KF_MOE_MAX_K; ++s) {
        if (s < k && ps[s] >= 0) {
          const kf_short8 v = kf_moe_ld8(rows + (int64_t)ps[s] * h + c * 8);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            acc[j] = fmaf(ws[s], kf_bf16_to_f32((unsigned short)v[j]), acc[j]);
        }
      }
      kf_short8 ov;
#pragma unroll
      for (int j = 0; j < 8; ++j) ov[j] = (short)kf_f32_to_bf16(acc[j]);
      *reinterpret_cast<kf_short8*>(out + t * h + c * 8) = ov;
    }
  }
}

// dy[pos[t,s]] = bf16(w[t,s] * dout[t]); dw[t,s] = bf16(<dout[t], y[pos[t,s]]>)
// (0 for a slot that is not local). One wave per token: each dout vector is
// loaded once and serves all k slots.
__global__ void kf_moe_combine_bwd_kernel(unsigned short* __restrict__ dy,
                                          unsigned short* __restrict__ dw,
                                          const unsigned short* __restrict__ dout,
                                          const unsigned short* __restrict__ y,
                                          const unsigned short* __restrict__ topw,
                                          const int* __restrict__ pos,
                                          int64_t T, int k, int64_t h,
                                          int64_t M) {
  const int lane = threadIdx.x & (KF_WAVE - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / KF_WAVE;
  const int64_t nwaves = gridDim.x * (int64_t)blockDim.x / KF_WAVE;
  const int64_t hv = h / 8;
  for (int64_t t = wave; t < T; t += nwaves) {
    int pl = -1;
    float wl = 0.f;
    if (lane < k) {
      pl = pos[t * k + lane];
      if ((int64_t)pl >= M) pl = -1;
      wl = kf_bf16_to_f32(topw[t * k + lane]);
    }
    int ps[KF_MOE_MAX_K];
    float ws[KF_MOE_MAX_K];
    float dot[KF_MOE_MAX_K];
#pragma unroll
    for (int s = 0; s < KF_MOE_MAX_K; ++s) {
      ps[s] = __shfl(pl, s, KF_WAVE);
      ws[s] = __shfl(wl, s, KF_WAVE);
      dot[s] = 0.f;
    }
    for (int64_t c = lane; c < hv; c += KF_WAVE) {
      const kf_short8 dv = kf_moe_ld8(dout + t * h + c * 8);
      float d[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = kf_bf16_to_f32((unsigned short)dv[j]);
#pragma unroll
      for (int s = 0; s < KF_MOE_MAX_K; ++s) {
        if (s < k && ps[s] >= 0) {
          const int64_t off = (int64_t)ps[s] * h + c * 8;
          const kf_short8 yv = kf_moe_ld8(y + off);
          kf_short8 ov;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            ov[j] = (short)kf_f32_to_bf16(ws[s] * d[j]);
            dot[s] = fmaf(d[j], kf_bf16_to_f32((unsigned short)yv[j]), dot[s]);
          }
          *reinterpret_cast<kf_short8*>(dy + off) = ov;
        }
      }
    }
    float mine = 0.f;
#pragma unroll
    for (int s = 0; s < KF_MOE_MAX_K; ++s) {
      const float tot = kf_wave_sum(dot[s]);
      if (lane == s) mine = tot;
    }
    if (lane < k) dw[t * k + lane] = pl >= 0 ? kf_f32_to_bf16(mine) : 0;
  }
}

// -------------------------------------------------------------- launchers --

static inline bool kf_moe_shape_ok(int64_t T, int64_t E, int64_t k) {
  return T >= 0 && E >= 2 && E <= KF_MOE_MAX_E && k >= 1 &&
         k <= KF_MOE_MAX_K && k <= E && T * k < (int64_t)INT32_MAX;
}

// one wave per row
static inline int kf_moe_row_grid(int64_t rows) {
  return kf_grid_for(rows * KF_WAVE, KF_MOE_BLOCK);
}

static inline int64_t kf_moe_nchunks(int64_t T, int64_t k) {
  return (T * k + KF_MOE_CHUNK - 1) / KF_MOE_CHUNK;
}

KF_EXPORT int kf_moe_route(void* topi, float* probs, void* topw,
                           const void* logits, int64_t T, int64_t E, int64_t k,
                           void* stream) {
  if (!kf_moe_shape_ok(T, E, k)) return (int)hipErrorInvalidValue;
  if (T == 0) return 0;
  hipLaunchKernelGGL(kf_moe_route_kernel, dim3(kf_moe_row_grid(T)),
                     dim3(KF_MOE_BLOCK), 0, (hipStream_t)stream, (int*)topi,
                     probs, (unsigned short*)topw,
                     (const unsigned short*)logits, T, (int)E, (int)k);
  return (int)hipGetLastError();
}

KF_EXPORT int kf_moe_route_bwd(void* dlogits, const void* dw,
                               const float* probs, const void* topi, int64_t T,
                               int64_t E, int64_t k, void* stream) {
  if (!kf_moe_shape_ok(T, E, k)) return (int)hipErrorInvalidValue;
  if (T == 0) return 0;
  hipLaunchKernelGGL(kf_moe_route_bwd_kernel, dim3(kf_moe_row_grid(T)),
                     dim3(KF_MOE_BLOCK), 0, (hipStream_t)stream,
                     (unsigned short*)dlogits, (const unsigned short*)dw,
                     probs, (const int*)topi, T, (int)E, (int)k);
  return (int)hipGetLastError();
}

// int32 elements of kf_moe_sort's workspace
KF_EXPORT int64_t kf_moe_sort_nwork(int64_t T, int64_t k, int64_t n_local) {
  const int64_t n = 2 * kf_moe_nchunks(T, k) * n_local;
  return n > 0 ? n : 1;
}

KF_EXPORT int kf_moe_sort(void* pos, void* src, void* offsets, void* work,
                          const void* topi, int64_t T, int64_t k,
                          int64_t e_lo, int64_t n_local, void* stream) {
  if (T < 0 || k < 1 || k > KF_MOE_MAX_K || T * k >= (int64_t)INT32_MAX ||
      e_lo < 0 || e_lo >= KF_MOE_MAX_E || n_local < 1 ||
      n_local > KF_MOE_MAX_E)
    return (int)hipErrorInvalidValue;
  const int64_t P = T * k;
  const int64_t nchunks = kf_moe_nchunks(T, k);
  int* counts = (int*)work;
  int* base = counts + nchunks * n_local;
  const int grid = (int)(nchunks < 1 ? 1 : (nchunks > 2048 ? 2048 : nchunks));
  hipStream_t st = (hipStream_t)stream;
  if (nchunks > 0)
    hipLaunchKernelGGL(kf_moe_count_kernel, dim3(grid), dim3(KF_MOE_BLOCK), 0,
                       st, counts, (const int*)topi, P, (int)e_lo,
                       (int)n_local, nchunks);
  hipLaunchKernelGGL(kf_moe_scan_kernel, dim3(1), dim3(KF_MOE_MAX_E), 0, st,
                     base, (int*)offsets, (const int*)counts, nchunks,
                     (int)n_local);
  if (nchunks > 0)
    hipLaunchKernelGGL(kf_moe_place_kernel, dim3(grid), dim3(KF_MOE_BLOCK), 0,
                       st, (int*)pos, (int*)src, (const int*)topi,
                       (const int*)base, (const int*)offsets, P, (int)k,
                       (int)e_lo, (int)n_local, nchunks);
  return (int)hipGetLastError();
}

KF_EXPORT int kf_moe_gather(void* xp, const void* x, const void* src,
                            int64_t M, int64_t T, int64_t h, void* stream) {
  if (M < 0 || T < 0 || h < 8 || h % 8) return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  hipLaunchKernelGGL(kf_moe_gather_kernel, dim3(kf_moe_row_grid(M)),
                     dim3(KF_MOE_BLOCK), 0, (hipStream_t)stream,
                     (unsigned short*)xp, (const unsigned short*)x,
                     (const int*)src, M, T, h);
  return (int)hipGetLastError();
}

KF_EXPORT int kf_moe_gather_bwd(void* dx, const void* dxp, const void* pos,
                                int64_t T, int64_t k, int64_t h, int64_t M,
                                void* stream) {
  if (T < 0 || k < 1 || k > KF_MOE_MAX_K || M < 0 || h < 8 || h % 8)
    return (int)hipErrorInvalidValue;
  if (T == 0) return 0;
  hipLaunchKernelGGL(kf_moe_sum_kernel<false>, dim3(kf_moe_row_grid(T)),
                     dim3(KF_MOE_BLOCK), 0, (hipStream_t)stream,
                     (unsigned short*)dx, (const unsigned short*)dxp,
                     (const unsigned short*)nullptr, (const int*)pos, T,
                     (int)k, h, M);
  return (int)hipGetLastError();
}

KF_EXPORT int kf_moe_combine(void* out, const void* y, const void* topw,
                             const void* pos, int64_t T, int64_t k, int64_t h,
                             int64_t M, void* stream) {
  if (T < 0 || k < 1 || k > KF_MOE_MAX_K || M < 0 || h < 8 || h % 8)
    return (int)hipErrorInvalidValue;
  if (T == 0) return 0;
  hipLaunchKernelGGL(kf_moe_sum_kernel<true>, dim3(kf_moe_row_grid(T)),
                     dim3(KF_MOE_BLOCK), 0, (hipStream_t)stream,
                     (unsigned short*)out, (const unsigned short*)y,
                     (const unsigned short*)topw, (const int*)pos, T, (int)k,
                     h, M);
  return (int)hipGetLastError();
}

KF_EXPORT int kf_moe_combine_bwd(void* dy, void* dw, const void* dout,
                                 const void* y, const void* topw,
                                 const void* pos, int64_t T, int64_t k,
                                 int64_t h, int64_t M, void* stream) {
  if (T < 0 || k < 1 || k > KF_MOE_MAX_K || M < 0 || h < 8 || h % 8)
    return (int)hipErrorInvalidValue;
  if (T == 0) return 0;
  hipLaunchKernelGGL(kf_moe_combine_bwd_kernel, dim3(kf_moe_row_grid(T)),
                     dim3(KF_MOE_BLOCK), 0, (hipStream_t)stream,
                     (unsigned short*)dy, (unsigned short*)dw,
                     (const unsigned short*)dout, (const unsigned short*)y,
                     (const unsigned short*)topw, (const int*)pos, T, (int)k,
                     h, M);
  return (int)hipGetLastError();
}

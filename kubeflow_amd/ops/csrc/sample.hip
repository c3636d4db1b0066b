// sample.hip — fused temperature / top-k / top-p sampling over a large vocab.
//
//   token[r] = sample(logits[r, :], temperature[r], top_k[r], top_p[r], u[r])
//
// One block of 16 waves per row, every parameter read from a device array, so
// one launch (and one captured graph) serves any mix of greedy and sampled
// rows. No [N, V] intermediate, no workspace, no float atomics.
//
// Order. A bf16 logit maps to a 16-bit integer key (sm_key) whose integer
// order is the rank order: larger logit first, -0 == +0, NaN with -inf. Equal
// keys rank by ascending index. Everything that top-k and top-p keep is then
//     { key > tau }  plus the first c entries, by index, of { key == tau },
// and the weight exp((x - x_max) / T) is a function of the key alone.
//
// Masses are integers: a weight is held as floor(w * 2^40) in 64 bits
// (w <= 1, V < 2^22, so a row sums below 2^62). Integer sums do not depend on
// their order, so histogram bins filled by LDS atomics, wave totals and the
// final scan all agree to the last bit, and count * weight(key) IS the mass of
// a plateau. The same inputs give the same token on every run.
//
// Passes over the row (the first streams it from HBM, the others hit L2):
//   1. max key and its lowest index. Greedy rows (temperature <= 0) leave.
//   2. only with top-k or top-p: a 4096-bin LDS histogram of (count, mass)
//      over the top 12 key bits, then a block scan over the bins in
//      descending order finds the bin where the count reaches k (or the mass
//      reaches top_p * kept mass).
//   3. a 16-bin count histogram of the low 4 key bits inside that bin
//      resolves tau, and c follows from counts alone. top-k and top-p together
//      resolve k first (its mass bounds p's target), then p; the second
//      low-bit pass is skipped when both land in the same bin.
//   4. draw: per-wave sums of the kept mass over 16 contiguous segments, a
//      16-entry prefix picks the wave whose segment crosses u * mass, and that
//      wave alone rescans its segment in index order (wave scans of mass and
//      of the plateau count) down to the element.
//
// Why 12 + 4 bits and not 8 + 8: the high byte of a bf16 is sign plus seven
// exponent bits, two binades per bin, and a real row of logits lives in a
// handful of them; 128k LDS atomics would serialise on those few addresses.
// Twelve bits split every binade over 8 bins, so a wave's 64 lanes rarely
// meet, and only the ~1% of the row inside the chosen bin reaches pass 3.
//
// Alignment: the 16-byte loads need every row to start 16-byte aligned:
// V % 8 == 0, stride % 8 == 0 and an aligned base. Anything else takes the
// scalar loads for the WHOLE row (the VEC = false instantiation), never a
// vector prefix at a 2-byte-aligned address.
//
// Memory safety, not validation: any content of the five inputs yields a
// token in [0, V) and no access outside them. NaN temperature counts as
// greedy, NaN top_p as off, u outside [0, 1) is clamped into the kept mass,
// and a row whose maximum is +inf or that has no finite entry returns its
// greedy token.

#include "kf_common.h"

#define SM_BLOCK 1024
#define SM_NW (SM_BLOCK / KF_WAVE)
#define SM_BINS 4096          // top 12 key bits
#define SM_LOW 16             // low 4 key bits
#define SM_ONE (1ull << 40)   // fixed-point 1.0
#define SM_KEY_NINF 0x007Fu   // key of -inf and of NaN; no real key is below
#define SM_KEY_PINF 0xFF80u

typedef unsigned long long sm_u64;

__device__ __forceinline__ unsigned sm_key(unsigned b) {
  if ((b & 0x7FFFu) > 0x7F80u) return SM_KEY_NINF;
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}

__device__ __forceinline__ float sm_key_value(unsigned key) {
  return kf_bf16_to_f32((key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu));
}

// Row parameters of the weight: w(key) = 2^((x(key) - xmax) * scale).
struct SmWeight {
  unsigned kmax;
  float xmax, scale;
  // key 0 is the padding of a partial unit; it and -inf / NaN weigh nothing.
  // kmax weighs exactly one whatever scale is (0 * inf would be NaN).
  __device__ __forceinline__ sm_u64 operator()(unsigned key) const {
    if (key <= SM_KEY_NINF) return 0;
    if (key >= kmax) return SM_ONE;
    const float w = __builtin_amdgcn_exp2f((sm_key_value(key) - xmax) * scale);
    return (sm_u64)(w * 0x1p40f);
  }
};

// The keys of unit `unit`: elements [8 * unit, 8 * unit + 8) of the row, key 0
// past the end.
template <bool VEC>
__device__ __forceinline__ void sm_load8(unsigned (&key)[8],
                                         const unsigned short* __restrict__ row,
                                         int unit, int V) {
  if (VEC) {
    const kf_short8 v = *reinterpret_cast<const kf_short8*>(row + 8 * unit);
#pragma unroll
    for (int e = 0; e < 8; ++e) key[e] = sm_key((unsigned short)v[e]);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = 8 * unit + e;
      key[e] = i < V ? sm_key(row[i]) : 0u;
    }
  }
}

__device__ __forceinline__ sm_u64 sm_wave_sum64(sm_u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, KF_WAVE);
  return v;
}

__device__ __forceinline__ unsigned sm_wave_sum32(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, KF_WAVE);
  return v;
}

__device__ __forceinline__ sm_u64 sm_wave_scan64(sm_u64 v, int lane) {
#pragma unroll
  for (int off = 1; off < KF_WAVE; off <<= 1) {
    const sm_u64 o = __shfl_up(v, off, KF_WAVE);
    if (lane >= off) v += o;
  }
  return v;
}

__device__ __forceinline__ unsigned sm_wave_scan32(unsigned v, int lane) {
#pragma unroll
  for (int off = 1; off < KF_WAVE; off <<= 1) {
    const unsigned o = __shfl_up(v, off, KF_WAVE);
    if (lane >= off) v += o;
  }
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(SM_BLOCK) void kf_sample_kernel(
    int* __restrict__ token, const unsigned short* __restrict__ logits,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const float* __restrict__ u_in, int V,
    int64_t stride) {
  __shared__ sm_u64 s_mass[SM_BINS];
  __shared__ unsigned s_cnt[SM_BINS];
  __shared__ sm_u64 s_wmass[SM_NW];
  __shared__ unsigned s_wcnt[SM_NW];
  __shared__ unsigned s_low[SM_LOW];
  __shared__ sm_u64 s_before;   // mass ranked before the chosen bin
  __shared__ sm_u64 s_mk;       // mass of the top-k set
  __shared__ unsigned s_bin, s_cbefore, s_tau, s_c;
  __shared__ int s_token;

  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (KF_WAVE - 1);
  const int wid = tid / KF_WAVE;
  const unsigned short* __restrict__ row = logits + (int64_t)r * stride;

  // wave `wid` owns the contiguous units [u0, u1); a lane walks them 64 apart
  const int NU = (V + 7) >> 3;
  const int UPW = (NU + SM_NW - 1) / SM_NW;
  const int u0 = min(wid * UPW, NU);
  const int u1 = min(u0 + UPW, NU);

  // ---- pass 1: max key, lowest index (a lane's units ascend, so > keeps
  // the first) ----
  unsigned bk = 0, bi = 0;
  for (int un = u0 + lane; un < u1; un += KF_WAVE) {
    unsigned key[8];
    sm_load8<VEC>(key, row, un, V);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (key[e] > bk) { bk = key[e]; bi = 8u * un + e; }
  }
  sm_u64 best = bk ? (((sm_u64)bk << 32) | (0xFFFFFFFFu - bi)) : 0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const sm_u64 o = __shfl_xor(best, off, KF_WAVE);
    best = o > best ? o : best;
  }
  if (lane == 0) s_wmass[wid] = best;
  __syncthreads();
  best = 0;
#pragma unroll
  for (int w = 0; w < SM_NW; ++w) best = s_wmass[w] > best ? s_wmass[w] : best;
  const unsigned kmax = (unsigned)(best >> 32);
  const int greedy = min((int)(0xFFFFFFFFu - (unsigned)best), V - 1);

  const float temp = temperature[r];
  if (!(temp > 0.f) || kmax <= SM_KEY_NINF || kmax >= SM_KEY_PINF) {
    if (tid == 0) token[r] = greedy;
    return;
  }
  const int k = top_k[r];
  const float p = top_p[r];
  const bool use_k = k > 0 && k < V;
  const bool use_p = p < 1.f;
  SmWeight wfx;
  wfx.kmax = kmax;
  wfx.xmax = sm_key_value(kmax);
  wfx.scale = (1.f / temp) * 1.44269504088896341f;

  unsigned tau = 0, c = 0;  // key > 0: every real entry is kept
  if (use_k || use_p) {
    // ---- pass 2: (count, mass) per 12-bit bin ----
    __syncthreads();  // s_wmass reads of pass 1 are done
    for (int b = tid; b < SM_BINS; b += SM_BLOCK) { s_cnt[b] = 0; s_mass[b] = 0; }
    __syncthreads();
    for (int un = u0 + lane; un < u1; un += KF_WAVE) {
      unsigned key[8];
      sm_load8<VEC>(key, row, un, V);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (key[e] == 0) continue;
        atomicAdd(&s_cnt[key[e] >> 4], 1u);
        if (use_p) {  // top-k alone selects on counts
          const sm_u64 w = wfx(key[e]);
          if (w) atomicAdd(&s_mass[key[e] >> 4], w);
        }
      }
    }
    __syncthreads();

    // block scan over the bins in descending key order: thread t owns the
    // bins 4095 - 4t .. 4092 - 4t
    unsigned c4[4];
    sm_u64 m4[4];
    unsigned tc = 0;
    sm_u64 tm = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = SM_BINS - 1 - (4 * tid + j);
      c4[j] = s_cnt[b];
      m4[j] = s_mass[b];
      tc += c4[j];
      tm += m4[j];
    }
    const unsigned ic = sm_wave_scan32(tc, lane);
    const sm_u64 im = sm_wave_scan64(tm, lane);
    if (lane == KF_WAVE - 1) { s_wcnt[wid] = ic; s_wmass[wid] = im; }
    __syncthreads();
    unsigned exc = ic - tc;
    sm_u64 exm = im - tm, total = 0;
#pragma unroll
    for (int w = 0; w < SM_NW; ++w) {
      if (w < wid) { exc += s_wcnt[w]; exm += s_wmass[w]; }
      total += s_wmass[w];
    }

    // one low-bit pass: counts of the 16 keys inside 12-bit bin `bin`
    auto low_pass = [&](unsigned bin) {
      if (tid < SM_LOW) s_low[tid] = 0;
      __syncthreads();
      for (int un = u0 + lane; un < u1; un += KF_WAVE) {
        unsigned key[8];
        sm_load8<VEC>(key, row, un, V);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (key[e] && (key[e] >> 4) == bin)
            atomicAdd(&s_low[key[e] & (SM_LOW - 1)], 1u);
      }
      __syncthreads();
    };

    sm_u64 mk = total;  // mass of the set top-p walks: all, or the top k
    unsigned kbin = SM_BINS;  // no bin
    if (use_k) {
      // the one thread whose bins take the count from < k to >= k
      if (exc < (unsigned)k && (unsigned)k <= exc + tc) {
        unsigned cc = exc;
        sm_u64 mm = exm;
        bool found = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!found && cc + c4[j] >= (unsigned)k) {
            s_bin = SM_BINS - 1 - (4 * tid + j);
            s_cbefore = cc;
            s_before = mm;
            found = true;
          }
          cc += c4[j];
          mm += m4[j];
        }
      }
      __syncthreads();
      kbin = s_bin;
      low_pass(kbin);
      if (tid == 0) {
        unsigned cc = s_cbefore;
        sm_u64 mm = s_before;
        bool found = false;
        for (int j = SM_LOW - 1; j >= 0 && !found; --j) {
          const unsigned key = (kbin << 4) | j, n = s_low[j];
          const sm_u64 w = wfx(key);
          if (cc + n >= (unsigned)k) {
            s_tau = key;
            s_c = (unsigned)k - cc;
            s_mk = mm + (sm_u64)((unsigned)k - cc) * w;
            found = true;
          }
          cc += n;
          mm += (sm_u64)n * w;
        }
      }
      __syncthreads();
      tau = s_tau;
      c = s_c;
      mk = s_mk;
    }
    if (use_p) {
      // shortest prefix with mass >= P = top_p * mk; 1 <= P <= mk keeps it
      // non-empty and inside the top-k set
      const double t = (double)p * (double)mk;
      sm_u64 P = p > 0.f ? (sm_u64)ceil(t) : 0ull;
      P = P < 1 ? 1 : (P > mk ? mk : P);
      if (exm < P && P <= exm + tm) {
        sm_u64 mm = exm;
        bool found = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!found && mm + m4[j] >= P) {
            s_bin = SM_BINS - 1 - (4 * tid + j);
            s_before = mm;
            found = true;
          }
          mm += m4[j];
        }
      }
      __syncthreads();
      const unsigned pbin = s_bin;
      if (pbin != kbin) low_pass(pbin);
      if (tid == 0) {
        sm_u64 mm = s_before;
        bool found = false;
        for (int j = SM_LOW - 1; j >= 0 && !found; --j) {
          const unsigned key = (pbin << 4) | j, n = s_low[j];
          const sm_u64 w = wfx(key);
          if (mm + (sm_u64)n * w >= P) {  // mm < P here, so n * w > 0
            const sm_u64 need = (P - mm + w - 1) / w;
            s_tau = key;
            s_c = need < 1 ? 1u : (unsigned)need;
            found = true;
          }
          mm += (sm_u64)n * w;
        }
      }
      __syncthreads();
      tau = s_tau;
      c = s_c;
    }
  }

  // ---- pass 4: the draw. Wave sums first: the mass above tau and the
  // plateau count per segment; the plateau's kept part follows from counts ----
  const sm_u64 wtau = wfx(tau);
  sm_u64 mg = 0;
  unsigned nt = 0;
  for (int un = u0 + lane; un < u1; un += KF_WAVE) {
    unsigned key[8];
    sm_load8<VEC>(key, row, un, V);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (key[e] > tau) mg += wfx(key[e]);
      else if (key[e] == tau) ++nt;
    }
  }
  mg = sm_wave_sum64(mg);
  nt = sm_wave_sum32(nt);
  __syncthreads();  // earlier readers of s_wmass / s_wcnt are done
  if (lane == 0) { s_wmass[wid] = mg; s_wcnt[wid] = nt; }
  if (tid == 0) s_token = greedy;
  __syncthreads();

  // every thread walks the 16 segment sums: M, then the crossing wave
  sm_u64 seg[SM_NW];
  sm_u64 M = 0;
  unsigned basec = 0;
#pragma unroll
  for (int w = 0; w < SM_NW; ++w) {
    const unsigned n = s_wcnt[w];
    const unsigned kept = c > basec ? min(c - basec, n) : 0u;
    seg[w] = s_wmass[w] + (sm_u64)kept * wtau;
    M += seg[w];
    basec += n;
  }
  // theta = u * M clamped into [0, M): a crossing then always exists, at an
  // entry of positive weight (M >= 2^40: the maximum is always kept)
  const float u = u_in[r];
  sm_u64 theta = 0;
  if (u > 0.f) {
    const double t = (double)u * (double)M;
    theta = t >= (double)M ? M - 1 : (sm_u64)t;
  }
  if (M && theta >= M) theta = M - 1;
  int W = -1;
  sm_u64 base = 0, cum = 0;
  unsigned rbase = 0;
  basec = 0;
#pragma unroll
  for (int w = 0; w < SM_NW; ++w) {
    if (W < 0 && cum + seg[w] > theta) { W = w; base = cum; rbase = basec; }
    cum += seg[w];
    basec += s_wcnt[w];
  }

  if (wid == W) {
    bool done = false;
    for (int ub = u0; ub < u1 && !done; ub += KF_WAVE) {
      const int un = ub + lane;
      unsigned key[8];
      if (un < u1) {
        sm_load8<VEC>(key, row, un, V);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) key[e] = 0;
      }
      unsigned ln = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) ln += (key[e] == tau);
      const unsigned lic = sm_wave_scan32(ln, lane);
      unsigned rank = rbase + lic - ln;  // plateau entries before this lane
      sm_u64 w8[8], ls = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        sm_u64 w = 0;
        if (key[e] > tau) w = wfx(key[e]);
        else if (key[e] == tau) w = rank++ < c ? wtau : 0ull;
        w8[e] = w;
        ls += w;
      }
      const sm_u64 lim = sm_wave_scan64(ls, lane);
      const sm_u64 tot = __shfl(lim, KF_WAVE - 1, KF_WAVE);
      if (base + tot > theta) {
        const unsigned long long hit = __ballot(base + lim > theta);
        if (lane == __ffsll((long long)hit) - 1) {
          sm_u64 run = base + lim - ls;
          int tok = -1;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            run += w8[e];
            if (tok < 0 && run > theta) tok = 8 * un + e;
          }
          if (tok >= 0) s_token = tok;
        }
        done = true;
      } else {
        base += tot;
        rbase += __shfl(lic, KF_WAVE - 1, KF_WAVE);
      }
    }
  }
  __syncthreads();
  if (tid == 0) token[r] = min(max(s_token, 0), V - 1);
}

KF_EXPORT int kf_sample(int* token, const void* logits,
                        const float* temperature, const int* top_k,
                        const float* top_p, const float* u, int64_t N,
                        int64_t V, int64_t stride, void* stream) {
  if (N <= 0) return 0;
  if (V < 1 || V >= (1 << 22) || stride < V) return (int)hipErrorInvalidValue;
  const bool vec = V % 8 == 0 && stride % 8 == 0 &&
                   reinterpret_cast<uintptr_t>(logits) % 16 == 0;
  auto kern = vec ? kf_sample_kernel<true> : kf_sample_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)N), dim3(SM_BLOCK), 0,
                     (hipStream_t)stream, token,
                     (const unsigned short*)logits, temperature, top_k, top_p,
                     u, (int)V, stride);
  return (int)hipGetLastError();
}

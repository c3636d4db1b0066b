// adamw.hip — fused decoupled-AdamW over one flat parameter shard, CDNA4.
//
// SURVEY.md §2.13 "fused_adamw kernel: flat 1D grid over param shards,
// master fp32". The trainer keeps ALL model parameters as views into a
// single contiguous bf16 buffer (288 GB HBM3E: big flat allocations, one
// launch per step — MI355X-first), with fp32 master weights and moments in
// matching flat buffers. One kernel updates everything:
//
//   m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g^2
//   p32 = p32*(1 - lr*wd) - lr * (m/bc1) / (sqrt(v/bc2) + eps)
//   p_bf16 = round(p32)
//
// Bias corrections are precomputed on host (no pow on device). Weight decay
// masking (no decay for norms/embeddings biases) is handled by the caller via
// a per-element fp32 `wd_mask` {0,1} buffer — optional (null => decay all).
// Memory-bound: 28-32 B/element — everything vectorized float4/short4.

#include "kf_common.h"

__global__ void kf_adamw_kernel(unsigned short* __restrict__ p16,
                                float* __restrict__ p32,
                                const unsigned short* __restrict__ g,
                                float* __restrict__ m, float* __restrict__ v,
                                const float* __restrict__ wd_mask, int64_t n4,
                                float lr, float b1, float b2, float eps,
                                float wd, float inv_bc1, float inv_bc2) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4;
       i += gridDim.x * (int64_t)blockDim.x) {
    kf_short4 gv = *reinterpret_cast<const kf_short4*>(g + i * 4);
    kf_float4 pv = *reinterpret_cast<const kf_float4*>(p32 + i * 4);
    kf_float4 mv = *reinterpret_cast<const kf_float4*>(m + i * 4);
    kf_float4 vv = *reinterpret_cast<const kf_float4*>(v + i * 4);
    kf_float4 wdv;
    if (wd_mask) wdv = *reinterpret_cast<const kf_float4*>(wd_mask + i * 4);
    kf_short4 out16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gf = kf_bf16_to_f32((unsigned short)gv[j]);
      float mf = b1 * mv[j] + (1.f - b1) * gf;
      float vf = b2 * vv[j] + (1.f - b2) * gf * gf;
      float decay = wd_mask ? wdv[j] * wd : wd;
      float pf = pv[j] * (1.f - lr * decay);
      pf -= lr * (mf * inv_bc1) * __frcp_rn(sqrtf(vf * inv_bc2) + eps);
      mv[j] = mf; vv[j] = vf; pv[j] = pf;
      out16[j] = (short)kf_f32_to_bf16(pf);
    }
    *reinterpret_cast<kf_float4*>(m + i * 4) = mv;
    *reinterpret_cast<kf_float4*>(v + i * 4) = vv;
    *reinterpret_cast<kf_float4*>(p32 + i * 4) = pv;
    *reinterpret_cast<kf_short4*>(p16 + i * 4) = out16;
  }
}

KF_EXPORT int kf_adamw(void* p16, float* p32, const void* g, float* m,
                       float* v, const float* wd_mask, int64_t n, float lr,
                       float b1, float b2, float eps, float wd, int64_t step,
                       void* stream) {
  if (n % 4) return (int)hipErrorInvalidValue;
  const float inv_bc1 = 1.f / (1.f - powf(b1, (float)step));
  const float inv_bc2 = 1.f / (1.f - powf(b2, (float)step));
  hipLaunchKernelGGL(kf_adamw_kernel, dim3(kf_grid_for(n / 4, 256)), dim3(256),
                     0, (hipStream_t)stream, (unsigned short*)p16, p32,
                     (const unsigned short*)g, m, v, wd_mask, n / 4, lr, b1,
                     b2, eps, wd, inv_bc1, inv_bc2);
  return (int)hipGetLastError();
}

// ---- step tail: clip folded into the update, compact decay mask ----------
//
// kf_adamw_clip is kf_adamw with the two passes around it removed:
//  * gscale (device scalar, may be null) holds float(bf16(clip scale)). The
//    kernel forms g' = bf16_rne(float(g) * s) — bit for bit what
//    grad.mul_(scale.to(bf16)) leaves in the buffer — updates from g', and
//    writes g' back so the gradient buffer ends the step as it did before.
//    s == 1 (nothing clipped): no multiply, no write-back.
//  * wd_groups (uint8 {0,1}, one per KF_WD_GROUP = 64 elements, may be null)
//    replaces the 4 B/element fp32 mask by 1/64 B/element. Every parameter
//    slice of the flat space starts on a 64-element boundary, and the padding
//    behind a slice holds p = g = m = v = 0, which updates to 0 under either
//    mask value. The fp32 mask is still accepted (shards whose offset is not
//    a group multiple); passing both masks is an error.
// The per-element arithmetic is kf_adamw_kernel's, expression for expression.

#define KF_WD_GROUP 64

// MASK: 0 decay all, 1 fp32 per-element mask, 2 uint8 per-group mask
template <int MASK>
__global__ void kf_adamw_clip_kernel(
    unsigned short* __restrict__ p16, float* __restrict__ p32,
    unsigned short* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, const float* __restrict__ wd_mask,
    const unsigned char* __restrict__ wd_groups,
    const float* __restrict__ gscale, int64_t n4, float lr, float b1, float b2,
    float eps, float wd, float inv_bc1, float inv_bc2) {
  const float s = gscale ? *gscale : 1.f;
  const bool clip = s != 1.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4;
       i += gridDim.x * (int64_t)blockDim.x) {
    kf_short4 gv = *reinterpret_cast<const kf_short4*>(g + i * 4);
    kf_float4 pv = *reinterpret_cast<const kf_float4*>(p32 + i * 4);
    kf_float4 mv = *reinterpret_cast<const kf_float4*>(m + i * 4);
    kf_float4 vv = *reinterpret_cast<const kf_float4*>(v + i * 4);
    kf_float4 wdv;
    if (MASK == 1) wdv = *reinterpret_cast<const kf_float4*>(wd_mask + i * 4);
    if (MASK == 2) {
      // 4 elements never straddle a 64-element group
      const float gm = (float)wd_groups[i / (KF_WD_GROUP / 4)];
      wdv = (kf_float4){gm, gm, gm, gm};
    }
    if (clip) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        gv[j] = (short)kf_f32_to_bf16(
            kf_bf16_to_f32((unsigned short)gv[j]) * s);
      *reinterpret_cast<kf_short4*>(g + i * 4) = gv;
    }
    kf_short4 out16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gf = kf_bf16_to_f32((unsigned short)gv[j]);
      float mf = b1 * mv[j] + (1.f - b1) * gf;
      float vf = b2 * vv[j] + (1.f - b2) * gf * gf;
      float decay = MASK ? wdv[j] * wd : wd;
      float pf = pv[j] * (1.f - lr * decay);
      pf -= lr * (mf * inv_bc1) * __frcp_rn(sqrtf(vf * inv_bc2) + eps);
      mv[j] = mf; vv[j] = vf; pv[j] = pf;
      out16[j] = (short)kf_f32_to_bf16(pf);
    }
    *reinterpret_cast<kf_float4*>(m + i * 4) = mv;
    *reinterpret_cast<kf_float4*>(v + i * 4) = vv;
    *reinterpret_cast<kf_float4*>(p32 + i * 4) = pv;
    *reinterpret_cast<kf_short4*>(p16 + i * 4) = out16;
  }
}

KF_EXPORT int kf_adamw_clip(void* p16, float* p32, void* g, float* m, float* v,
                            const float* wd_mask, const void* wd_groups,
                            const float* gscale, int64_t n, float lr, float b1,
                            float b2, float eps, float wd, int64_t step,
                            void* stream) {
  if (n % 4 || (wd_mask && wd_groups)) return (int)hipErrorInvalidValue;
  const float inv_bc1 = 1.f / (1.f - powf(b1, (float)step));
  const float inv_bc2 = 1.f / (1.f - powf(b2, (float)step));
  auto kernel = wd_groups ? kf_adamw_clip_kernel<2>
                : wd_mask ? kf_adamw_clip_kernel<1>
                          : kf_adamw_clip_kernel<0>;
  hipLaunchKernelGGL(kernel, dim3(kf_grid_for(n / 4, 256)), dim3(256), 0,
                     (hipStream_t)stream, (unsigned short*)p16, p32,
                     (unsigned short*)g, m, v, wd_mask,
                     (const unsigned char*)wd_groups, gscale, n / 4, lr, b1,
                     b2, eps, wd, inv_bc1, inv_bc2);
  return (int)hipGetLastError();
}

// ---- gradient norm: one streaming read, deterministic ---------------------
//
// Stage one: capped grid, grid-stride over short8 vectors, four loads in
// flight per thread; each vector's eight squares are summed pairwise before
// they join the thread's fp32 accumulator, then a block reduce and ONE plain
// store per block (no atomics: the same input gives the same bits).
// Stage two: one block sums the partials in double and writes
// float(sqrt(sum)) to out[0]. No host sync, no allocation: the caller passes
// a partials buffer of kf_grad_sumsq_nparts(n) floats.

#define SSQ_BLOCK 256

__device__ __forceinline__ float kf_sumsq8(kf_short8 gv) {
  float q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float f = kf_bf16_to_f32((unsigned short)gv[j]);
    q[j] = f * f;
  }
  return ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
}

__global__ __launch_bounds__(SSQ_BLOCK) void kf_grad_sumsq_kernel(
    float* __restrict__ partials, const unsigned short* __restrict__ g,
    int64_t n) {
  __shared__ float scratch[SSQ_BLOCK / KF_WAVE];
  const int64_t n8 = n / 8;
  const int64_t stride = gridDim.x * (int64_t)SSQ_BLOCK;
  int64_t i = blockIdx.x * (int64_t)SSQ_BLOCK + threadIdx.x;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (; i + 3 * stride < n8; i += 4 * stride) {
    kf_short8 v0 = *reinterpret_cast<const kf_short8*>(g + i * 8);
    kf_short8 v1 = *reinterpret_cast<const kf_short8*>(g + (i + stride) * 8);
    kf_short8 v2 =
        *reinterpret_cast<const kf_short8*>(g + (i + 2 * stride) * 8);
    kf_short8 v3 =
        *reinterpret_cast<const kf_short8*>(g + (i + 3 * stride) * 8);
    a0 += kf_sumsq8(v0);
    a1 += kf_sumsq8(v1);
    a2 += kf_sumsq8(v2);
    a3 += kf_sumsq8(v3);
  }
  for (; i < n8; i += stride)
    a0 += kf_sumsq8(*reinterpret_cast<const kf_short8*>(g + i * 8));
  // scalar tail (n % 8 elements), first threads of block 0
  if (blockIdx.x == 0 && n8 * 8 + threadIdx.x < n) {
    float f = kf_bf16_to_f32(g[n8 * 8 + threadIdx.x]);
    a1 += f * f;
  }
  float acc = kf_block_reduce((a0 + a1) + (a2 + a3), scratch, KfSum{}, 0.f);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

__global__ __launch_bounds__(SSQ_BLOCK) void kf_grad_norm_final_kernel(
    float* __restrict__ out, const float* __restrict__ partials, int nparts) {
  __shared__ double red[SSQ_BLOCK];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += SSQ_BLOCK)
    acc += (double)partials[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = SSQ_BLOCK / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)sqrt(red[0]);
}

KF_EXPORT int64_t kf_grad_sumsq_nparts(int64_t n) {
  return kf_grid_for(n / 8, SSQ_BLOCK);
}

// out[0] = sqrt(sum g^2) over n bf16 elements; g 16-byte aligned.
KF_EXPORT int kf_grad_sumsq(float* out, float* partials, const void* g,
                            int64_t n, void* stream) {
  if (n < 0 || ((uintptr_t)g & 15)) return (int)hipErrorInvalidValue;
  const int grid = kf_grid_for(n / 8, SSQ_BLOCK);
  hipLaunchKernelGGL(kf_grad_sumsq_kernel, dim3(grid), dim3(SSQ_BLOCK), 0,
                     (hipStream_t)stream, partials,
                     (const unsigned short*)g, n);
  int err = (int)hipGetLastError();
  if (err) return err;
  hipLaunchKernelGGL(kf_grad_norm_final_kernel, dim3(1), dim3(SSQ_BLOCK), 0,
                     (hipStream_t)stream, out, (const float*)partials, grid);
  return (int)hipGetLastError();
}

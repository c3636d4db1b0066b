// rmsnorm.hip — fused RMSNorm forward/backward for CDNA4 (gfx950).
//
// Replaces the per-token normalization of the PyTorchJob worker hot loop
// ("rmsnorm fused kernel, one workgroup per row, wave
// reduction"). Memory-bound: target is HBM BW, so all bf16 access is
// vectorized as short8 (guide G13) and forward reads x exactly once.
//
//   y = x * rsqrt(mean(x^2) + eps) * w        (fp32 math, bf16 in/out)
//
// Backward (per row, s = sum(dy*w*x)):
//   dx = rstd * dy*w - rstd^3/C * s * x
//   dw_j = sum_rows(dy_j * x_j * rstd)   — block-local LDS accumulation,
//   one fp32 atomicAdd pass per block, then a cast kernel.

#include "kf_common.h"

#include <cstdlib>

#define RN_BLOCK 256
#define RN_VEC 8

__global__ __launch_bounds__(RN_BLOCK) void kf_rmsnorm_fwd_kernel(
    unsigned short* __restrict__ y, float* __restrict__ rstd_out,
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ w,
    int64_t rows, int cols, float eps) {
  __shared__ float scratch[RN_BLOCK / KF_WAVE];
  const int nvec = cols / RN_VEC;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const unsigned short* xr = x + row * cols;
    unsigned short* yr = y + row * cols;
    float ss = 0.f;
    for (int i = threadIdx.x; i < nvec; i += RN_BLOCK) {
      kf_short8 xv = *reinterpret_cast<const kf_short8*>(xr + i * RN_VEC);
#pragma unroll
      for (int j = 0; j < RN_VEC; ++j) {
        float f = kf_bf16_to_f32((unsigned short)xv[j]);
        ss += f * f;
      }
    }
    ss = kf_block_reduce(ss, scratch, KfSum{}, 0.f);
    const float rstd = rsqrtf(ss / (float)cols + eps);
    if (threadIdx.x == 0 && rstd_out) rstd_out[row] = rstd;
    for (int i = threadIdx.x; i < nvec; i += RN_BLOCK) {
      kf_short8 xv = *reinterpret_cast<const kf_short8*>(xr + i * RN_VEC);
      kf_short8 wv = *reinterpret_cast<const kf_short8*>(w + i * RN_VEC);
      kf_short8 ov;
#pragma unroll
      for (int j = 0; j < RN_VEC; ++j) {
        float f = kf_bf16_to_f32((unsigned short)xv[j]) * rstd *
                  kf_bf16_to_f32((unsigned short)wv[j]);
        ov[j] = (short)kf_f32_to_bf16(f);
      }
      *reinterpret_cast<kf_short8*>(yr + i * RN_VEC) = ov;
    }
  }
}

// dw: each block accumulates its rows' contribution in LDS (cols * 4 B;
// hidden 4096 -> 16 KiB) and atomicAdds it once into a zeroed fp32 buffer
// (guide G12: block-level pre-reduction, one atomic pass per block — the
// earlier partials+column-sum design ran the reduction on cols/256 = 16
// blocks, 6% of the chip, ~16 ms/step in the r01 profile).
//
// RES: the residual stream's gradient `dres` [rows, cols] is added in the
// store, dx = bf16(float(bf16(rs*dy*w - k*x)) + float(dres)) — the double
// rounding of the separate bf16 add kernel this replaces, so dx keeps its bits.
template <bool RES>
__global__ __launch_bounds__(RN_BLOCK) void kf_rmsnorm_bwd_kernel(
    unsigned short* __restrict__ dx, float* __restrict__ dw_part,
    const unsigned short* __restrict__ dy, const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ w, const float* __restrict__ rstd,
    const unsigned short* __restrict__ dres, int64_t rows, int cols) {
  extern __shared__ float lds[];           // [cols] dw accum + reduce scratch
  float* dw_lds = lds;
  float* scratch = lds + cols;
  const int nvec = cols / RN_VEC;
  for (int i = threadIdx.x; i < cols; i += RN_BLOCK) dw_lds[i] = 0.f;
  __syncthreads();

  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const unsigned short* dyr = dy + row * cols;
    const unsigned short* xr = x + row * cols;
    unsigned short* dxr = dx + row * cols;
    const float rs = rstd[row];
    float dot = 0.f;
    for (int i = threadIdx.x; i < nvec; i += RN_BLOCK) {
      kf_short8 dyv = *reinterpret_cast<const kf_short8*>(dyr + i * RN_VEC);
      kf_short8 xv = *reinterpret_cast<const kf_short8*>(xr + i * RN_VEC);
      kf_short8 wv = *reinterpret_cast<const kf_short8*>(w + i * RN_VEC);
#pragma unroll
      for (int j = 0; j < RN_VEC; ++j) {
        float dyf = kf_bf16_to_f32((unsigned short)dyv[j]);
        float xf = kf_bf16_to_f32((unsigned short)xv[j]);
        float wf = kf_bf16_to_f32((unsigned short)wv[j]);
        dot += dyf * wf * xf;
        dw_lds[i * RN_VEC + j] += dyf * xf * rs;  // thread-owned slot
      }
    }
    dot = kf_block_reduce(dot, scratch, KfSum{}, 0.f);
    const float k = rs * rs * rs * dot / (float)cols;
    for (int i = threadIdx.x; i < nvec; i += RN_BLOCK) {
      kf_short8 dyv = *reinterpret_cast<const kf_short8*>(dyr + i * RN_VEC);
      kf_short8 xv = *reinterpret_cast<const kf_short8*>(xr + i * RN_VEC);
      kf_short8 wv = *reinterpret_cast<const kf_short8*>(w + i * RN_VEC);
      kf_short8 rv;
      if (RES)
        rv = *reinterpret_cast<const kf_short8*>(dres + row * cols +
                                                 i * RN_VEC);
      kf_short8 ov;
#pragma unroll
      for (int j = 0; j < RN_VEC; ++j) {
        float dyf = kf_bf16_to_f32((unsigned short)dyv[j]);
        float xf = kf_bf16_to_f32((unsigned short)xv[j]);
        float wf = kf_bf16_to_f32((unsigned short)wv[j]);
        ov[j] = (short)kf_f32_to_bf16(rs * dyf * wf - k * xf);
        if (RES)
          ov[j] = (short)kf_f32_to_bf16(
              kf_bf16_to_f32((unsigned short)ov[j]) +
              kf_bf16_to_f32((unsigned short)rv[j]));
      }
      *reinterpret_cast<kf_short8*>(dxr + i * RN_VEC) = ov;
    }
    __syncthreads();  // dw_lds writes of this row done before next row reuse
  }
  for (int i = threadIdx.x; i < cols; i += RN_BLOCK)
    atomicAdd(&dw_part[i], dw_lds[i]);
}

// cols <= RN_REG_COLS: each thread owns at most RN_REG_SLOTS fixed vectors of
// every row, so (a) the dy/x vectors of the first pass stay in registers for
// the second pass instead of being read again, (b) w is loaded once per
// block, and (c) the dw accumulators live in registers, not LDS (no
// read-modify-write of 16 KiB of LDS per row, no trailing barrier). The
// arithmetic, and the order of every sum, is kf_rmsnorm_bwd_kernel's.
#define RN_REG_SLOTS 2
#define RN_REG_COLS (RN_REG_SLOTS * RN_BLOCK * RN_VEC)  // 4096

template <bool RES>
__global__ __launch_bounds__(RN_BLOCK) void kf_rmsnorm_bwd_reg_kernel(
    unsigned short* __restrict__ dx, float* __restrict__ dw_part,
    const unsigned short* __restrict__ dy, const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ w, const float* __restrict__ rstd,
    const unsigned short* __restrict__ dres, int64_t rows, int cols) {
  extern __shared__ float dw_lds[];  // [cols], used once after the row loop
  __shared__ float scratch[RN_BLOCK / KF_WAVE];
  const int nvec = cols / RN_VEC;
  float dwacc[RN_REG_SLOTS][RN_VEC];
  float wf[RN_REG_SLOTS][RN_VEC];
#pragma unroll
  for (int t = 0; t < RN_REG_SLOTS; ++t) {
    const int i = threadIdx.x + t * RN_BLOCK;
    kf_short8 wv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < nvec) wv = *reinterpret_cast<const kf_short8*>(w + i * RN_VEC);
#pragma unroll
    for (int j = 0; j < RN_VEC; ++j) {
      wf[t][j] = kf_bf16_to_f32((unsigned short)wv[j]);
      dwacc[t][j] = 0.f;
    }
  }

  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const unsigned short* dyr = dy + row * cols;
    const unsigned short* xr = x + row * cols;
    unsigned short* dxr = dx + row * cols;
    const float rs = rstd[row];
    kf_short8 dyv[RN_REG_SLOTS], xv[RN_REG_SLOTS], rv[RN_REG_SLOTS];
#pragma unroll
    for (int t = 0; t < RN_REG_SLOTS; ++t) {
      const int i = threadIdx.x + t * RN_BLOCK;
      if (i < nvec) {
        dyv[t] = *reinterpret_cast<const kf_short8*>(dyr + i * RN_VEC);
        xv[t] = *reinterpret_cast<const kf_short8*>(xr + i * RN_VEC);
        if (RES)
          rv[t] = *reinterpret_cast<const kf_short8*>(dres + row * cols +
                                                      i * RN_VEC);
      }
    }
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < RN_REG_SLOTS; ++t) {
      if ((int)threadIdx.x + t * RN_BLOCK < nvec) {
#pragma unroll
        for (int j = 0; j < RN_VEC; ++j) {
          float dyf = kf_bf16_to_f32((unsigned short)dyv[t][j]);
          float xf = kf_bf16_to_f32((unsigned short)xv[t][j]);
          dot += dyf * wf[t][j] * xf;
          dwacc[t][j] += dyf * xf * rs;
        }
      }
    }
    dot = kf_block_reduce(dot, scratch, KfSum{}, 0.f);
    const float k = rs * rs * rs * dot / (float)cols;
#pragma unroll
    for (int t = 0; t < RN_REG_SLOTS; ++t) {
      const int i = threadIdx.x + t * RN_BLOCK;
      if (i < nvec) {
        kf_short8 ov;
#pragma unroll
        for (int j = 0; j < RN_VEC; ++j) {
          float dyf = kf_bf16_to_f32((unsigned short)dyv[t][j]);
          float xf = kf_bf16_to_f32((unsigned short)xv[t][j]);
          ov[j] = (short)kf_f32_to_bf16(rs * dyf * wf[t][j] - k * xf);
          if (RES)
            ov[j] = (short)kf_f32_to_bf16(
                kf_bf16_to_f32((unsigned short)ov[j]) +
                kf_bf16_to_f32((unsigned short)rv[t][j]));
        }
        *reinterpret_cast<kf_short8*>(dxr + i * RN_VEC) = ov;
      }
    }
  }
  // through LDS once per block, so that each wave's atomic instruction adds
  // 256 contiguous bytes as in kf_rmsnorm_bwd_kernel (guide G12)
#pragma unroll
  for (int t = 0; t < RN_REG_SLOTS; ++t) {
    const int i = threadIdx.x + t * RN_BLOCK;
    if (i < nvec) {
#pragma unroll
      for (int j = 0; j < RN_VEC; ++j) dw_lds[i * RN_VEC + j] = dwacc[t][j];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cols; i += RN_BLOCK)
    atomicAdd(&dw_part[i], dw_lds[i]);
}

// fp32 accumulator -> bf16 output.
__global__ void kf_cast_bf16_kernel(unsigned short* __restrict__ dst,
                                    const float* __restrict__ src,
                                    int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * (int64_t)blockDim.x)
    dst[i] = kf_f32_to_bf16(src[i]);
}

KF_EXPORT int kf_rmsnorm_fwd(void* y, float* rstd, const void* x, const void* w,
                             int64_t rows, int64_t cols, float eps,
                             void* stream) {
  if (cols % RN_VEC) return (int)hipErrorInvalidValue;
  int grid = kf_grid_for(rows, 1);
  hipLaunchKernelGGL(kf_rmsnorm_fwd_kernel, dim3(grid), dim3(RN_BLOCK), 0,
                     (hipStream_t)stream, (unsigned short*)y, rstd,
                     (const unsigned short*)x, (const unsigned short*)w, rows,
                     (int)cols, eps);
  return (int)hipGetLastError();
}

// dw_acc must be a ZEROED fp32 buffer of `cols` floats.
KF_EXPORT int64_t kf_rmsnorm_bwd_nparts(int64_t rows) {
  (void)rows;
  return 1;  // accumulator is [cols] now (kept for ABI compat)
}

KF_EXPORT int kf_rmsnorm_bwd(void* dx, void* dw, float* dw_acc,
                             const void* dy, const void* x, const void* w,
                             const float* rstd, int64_t rows, int64_t cols,
                             void* stream) {
  if (cols % RN_VEC) return (int)hipErrorInvalidValue;
  int grid = (int)(rows < 1024 ? rows : 1024);
  if (grid < 1) grid = 1;
  size_t lds = (cols + RN_BLOCK / KF_WAVE) * sizeof(float);
  hipLaunchKernelGGL(kf_rmsnorm_bwd_kernel<false>, dim3(grid), dim3(RN_BLOCK),
                     lds, (hipStream_t)stream, (unsigned short*)dx, dw_acc,
                     (const unsigned short*)dy, (const unsigned short*)x,
                     (const unsigned short*)w, rstd,
                     (const unsigned short*)nullptr, rows, (int)cols);
  int err = (int)hipGetLastError();
  if (err) return err;
  hipLaunchKernelGGL(kf_cast_bf16_kernel, dim3(kf_grid_for(cols, 256)),
                     dim3(256), 0, (hipStream_t)stream, (unsigned short*)dw,
                     dw_acc, cols);
  return (int)hipGetLastError();
}

// KF_RMSNORM_BWD_REGS=0: bisection switch — kf_rmsnorm_bwd_res keeps the
// LDS-accumulator kernel at every width.
static bool kf_rmsnorm_bwd_regs() {
  static int cached = -1;
  if (cached < 0) {
    const char* e = getenv("KF_RMSNORM_BWD_REGS");
    cached = (e && e[0] == '0') ? 0 : 1;
  }
  return cached == 1;
}

// kf_rmsnorm_bwd with the residual stream's gradient folded into the store:
// dres [rows, cols] bf16 or null (null: dx is kf_rmsnorm_bwd's).
KF_EXPORT int kf_rmsnorm_bwd_res(void* dx, void* dw, float* dw_acc,
                                 const void* dy, const void* x, const void* w,
                                 const float* rstd, const void* dres,
                                 int64_t rows, int64_t cols, void* stream) {
  if (cols % RN_VEC) return (int)hipErrorInvalidValue;
  int grid = (int)(rows < 1024 ? rows : 1024);
  if (grid < 1) grid = 1;
  const bool regs = cols <= RN_REG_COLS && kf_rmsnorm_bwd_regs();
  size_t lds = (cols + (regs ? 0 : RN_BLOCK / KF_WAVE)) * sizeof(float);
  auto kernel = regs ? (dres ? kf_rmsnorm_bwd_reg_kernel<true>
                             : kf_rmsnorm_bwd_reg_kernel<false>)
                     : (dres ? kf_rmsnorm_bwd_kernel<true>
                             : kf_rmsnorm_bwd_kernel<false>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(RN_BLOCK), lds,
                     (hipStream_t)stream, (unsigned short*)dx, dw_acc,
                     (const unsigned short*)dy, (const unsigned short*)x,
                     (const unsigned short*)w, rstd,
                     (const unsigned short*)dres, rows, (int)cols);
  int err = (int)hipGetLastError();
  if (err) return err;
  hipLaunchKernelGGL(kf_cast_bf16_kernel, dim3(kf_grid_for(cols, 256)),
                     dim3(256), 0, (hipStream_t)stream, (unsigned short*)dw,
                     dw_acc, cols);
  return (int)hipGetLastError();
}

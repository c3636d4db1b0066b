// kf_attn_common.h — the MFMA-attention primitives, once.
//
// Everything the 32x32x16-MFMA attention kernels share: fragment typedefs,
// softmax constants, the gfx950 instruction wrappers, the two LDS layouts
// (XOR-swizzled rows, [d/16][r/4][4][16] subtiles for the hardware transpose
// read), the accumulator -> operand exchange and the tr_read + MFMA
// accumulate loop. A new attention kernel includes this header; it does not
// grow a private copy. Whatever has one user stays in that user's file.
#pragma once

#include "kf_common.h"

typedef __bf16 kf_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 kf_bf16x2 __attribute__((ext_vector_type(2)));
typedef float kf_f32x2 __attribute__((ext_vector_type(2)));
typedef float kf_f32x4 __attribute__((ext_vector_type(4)));
typedef float kf_f32x16 __attribute__((ext_vector_type(16)));
// (kf_short4 / kf_short8 come from kf_common.h)

#define KF_LOG2E 1.44269504f
#define KF_LN2 0.69314718f
#define KF_DEFER_MAX_THR2 11.5415603f  // 8 * log2(e): defer-max, exp2 units

// two fp32 -> packed bf16 pair, round-to-nearest-even (v_cvt_pk_bf16_f32).
// Two forms on purpose: the asm one is opaque to the scheduler, the builtin
// one is visible to it. The d128 kernels were tuned with the former, the d64
// kernels with the latter; swapping either changes the generated code.
__device__ __forceinline__ unsigned int kf_cvt_pk_bf16(float lo, float hi) {
  unsigned int r;
  asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

__device__ __forceinline__ unsigned int kf_cvt_pk_bf16_builtin(float lo,
                                                               float hi) {
  kf_f32x2 x = {lo, hi};
  kf_bf16x2 y = __builtin_convertvector(x, kf_bf16x2);
  return *reinterpret_cast<unsigned int*>(&y);
}

__device__ __forceinline__ float kf_exp2(float x) {
  float r;
  asm volatile("v_exp_f32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

// hardware transpose read: each lane reads 8 B at its own address, each
// 16-lane group covers one [4][16] subtile and lane l receives column l&15
// (mapping pinned on hardware by scripts/probe_tr16.py)
#define KF_TR16(dst, addr, OFFLIT)                                      \
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:" OFFLIT               \
               : "=v"(dst) : "v"(addr))

// Row-major LDS tile with row_bytes-byte rows, XOR-swizzled (guide G4):
// byte ^= (row & 7) << 4. Rows shorter than 128 B fold in fewer row bits so
// the XOR stays inside the row (64 B -> row & 3). row_bytes is a constant at
// every call site. A plain argument, not a template parameter: with one
// instantiation per row size the compiler inlines the call sites of a kernel
// that uses two sizes in another order and allocates registers differently.
__device__ __forceinline__ int kf_swz(int row, int byte_in_row, int row_bytes) {
  const int mask = row_bytes >= 128 ? 7 : row_bytes / 16 - 1;
  return row * row_bytes + (byte_in_row ^ ((row & mask) << 4));
}

// Subtiled layout for ds_read_b64_tr_b16 (T10): element offset of X[r][d] in
// a ROWS x 128 tile = slab(d>>4)*ROWS*16 + (r>>2)*64 + (r&3)*16 + (d&15).
// Each [4][16] subtile is 128 contiguous bytes, so the tile is staged with
// plain b128 writes and read both as row chunks and through KF_TR16.
template <int ROWS>
__device__ __forceinline__ int kf_vsub(int r, int d) {
  return (d >> 4) * (ROWS * 16) + ((r >> 2) << 6) + ((r & 3) << 4) + (d & 15);
}

// tr_read per-lane base byte offset within one subtiled ROWS x 128 buffer:
// 16-lane group g covers slab (g&1), row-subtile 2*(g>>1), column lane&15
template <int ROWS>
__device__ __forceinline__ unsigned kf_tr_lane_off(int lane) {
  const int g = lane >> 4;
  return (unsigned)(((g & 1) * (ROWS * 32)) + ((g >> 1) << 8) +
                    ((lane & 15) << 3));
}

// Exchange an f32x16 accumulator half (8 regs from `base`, C layout: col =
// lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)) into one bf16x8 MFMA
// operand: the lane keeps its column and the 16 C rows become the k axis
// with chunk (lane>>5)*8. regs 0-7 cover rows {0..3, 8..11} (+4 for the hi
// lanes), regs 8-15 rows {16..19, 24..27}: 4 cvt_pk pack row pairs, 2
// permlane32_swap trade the hi lanes' first words for the lo lanes' second
// ones, which leaves 8 consecutive rows in each lane (guide T12). This is
// the P / dS re-fragmentation every swapped-QK^T kernel here uses.
template <unsigned int (*CVT)(float, float) = kf_cvt_pk_bf16>
__device__ __forceinline__ kf_bf16x8 kf_exchange(const kf_f32x16& a,
                                                 int base) {
  unsigned int w0 = CVT(a[base + 0], a[base + 1]);
  unsigned int w1 = CVT(a[base + 2], a[base + 3]);
  unsigned int w2 = CVT(a[base + 4], a[base + 5]);
  unsigned int w3 = CVT(a[base + 6], a[base + 7]);
  auto s02 = __builtin_amdgcn_permlane32_swap(w0, w2, false, false);
  auto s13 = __builtin_amdgcn_permlane32_swap(w1, w3, false, false);
  unsigned int u[4] = {(unsigned)s02[0], (unsigned)s13[0], (unsigned)s02[1],
                       (unsigned)s13[1]};
  return *reinterpret_cast<kf_bf16x8*>(u);
}

// acc[dt] += mfma over dt = 0..3 of the transposed fragment tr(dt) read at
// vbase (kf_tr_lane_off + 32-row sub-block offset, subtiled ROWS x 128
// buffer) with the two exchanged fragments p0, p1; 1-deep tr_read prefetch
// with counted lgkmcnt. TR_IS_A: the tr fragment is the MFMA A operand
// (acc^T += tr * p), else the B operand (acc += p * tr).
template <bool TR_IS_A, int ROWS>
__device__ __forceinline__ void kf_tr_acc_loop(kf_f32x16 (&acc)[4],
                                               unsigned vbase,
                                               const kf_bf16x8& p0,
                                               const kf_bf16x8& p1) {
  kf_short4 t[2][4];
  KF_TR16(t[0][0], vbase, "0");
  KF_TR16(t[0][1], vbase, "128");
  KF_TR16(t[0][2], vbase, "512");
  KF_TR16(t[0][3], vbase, "640");
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    if (dt < 3) {
      const unsigned va = vbase + (unsigned)((dt + 1) * (ROWS * 64));
      KF_TR16(t[(dt + 1) & 1][0], va, "0");
      KF_TR16(t[(dt + 1) & 1][1], va, "128");
      KF_TR16(t[(dt + 1) & 1][2], va, "512");
      KF_TR16(t[(dt + 1) & 1][3], va, "640");
      asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_sched_barrier(0);  // guide rule 18
    kf_short8 f0 = __builtin_shufflevector(t[dt & 1][0], t[dt & 1][1],
                                           0, 1, 2, 3, 4, 5, 6, 7);
    kf_short8 f1 = __builtin_shufflevector(t[dt & 1][2], t[dt & 1][3],
                                           0, 1, 2, 3, 4, 5, 6, 7);
    const kf_bf16x8 a0 = *reinterpret_cast<kf_bf16x8*>(&f0);
    const kf_bf16x8 a1 = *reinterpret_cast<kf_bf16x8*>(&f1);
    __builtin_amdgcn_s_setprio(1);
    if (TR_IS_A) {
      acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, p0, acc[dt], 0,
                                                        0, 0);
      acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, p1, acc[dt], 0,
                                                        0, 0);
    } else {
      acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p0, a0, acc[dt], 0,
                                                        0, 0);
      acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p1, a1, acc[dt], 0,
                                                        0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
  }
}

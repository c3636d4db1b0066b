// kf_fp4.h — the in-register MXFP4 -> bf16 fragment conversion shared by the
// W4A16 kernels (skinny_gemm.hip's q4 body, gemm_q4.hip).
#pragma once

#include "kf_common.h"

typedef __bf16 kf_bf16x8s __attribute__((ext_vector_type(8)));
typedef __bf16 kf_bf16x2s __attribute__((ext_vector_type(2)));

// 8 e2m1 values of one word (element j in nibble j) times 2^(sbyte - 127)
__device__ __forceinline__ kf_bf16x8s kf_fp4x8_to_bf16x8(unsigned int w,
                                                         unsigned int sbyte) {
  const float sc = __builtin_bit_cast(float, sbyte << 23);
  union {
    kf_bf16x2s p[4];
    kf_bf16x8s v;
  } out;
  out.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0);
  out.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1);
  out.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2);
  out.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3);
  return out.v;
}

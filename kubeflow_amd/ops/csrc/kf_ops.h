// kf_ops.h — the C ABI of libkfops.so: every exported entry point, once.
//
// kf_common.h includes this header, so every .hip file sees it: a definition
// that disagrees with its prototype here does not compile, and a kernel file
// that calls into another one needs no hand-copied declaration.
// kubeflow_amd/ops/_backend.py holds the ctypes side of the same table;
// tests/test_ops_abi.py parses this file and checks the two against each
// other, so keep every prototype in the plain form
//   KF_EXPORT <int|int64_t> name(type name, ...);
//
// Conventions: bf16 tensors cross as void* (ushort storage), fp32 as float*;
// sizes and strides (elements) are int64_t; every launcher takes the caller's
// hipStream_t as a trailing void* and returns hipError_t as int.
#pragma once

#include <cstdint>

#define KF_EXPORT extern "C" __attribute__((visibility("default")))

// ---- rmsnorm.hip / layernorm.hip ----
KF_EXPORT int kf_rmsnorm_fwd(void* y, float* rstd, const void* x,
    const void* w, int64_t rows, int64_t cols, float eps, void* stream);
KF_EXPORT int64_t kf_rmsnorm_bwd_nparts(int64_t rows);
KF_EXPORT int kf_rmsnorm_bwd(void* dx, void* dw, float* dw_acc, const void* dy,
    const void* x, const void* w, const float* rstd, int64_t rows,
    int64_t cols, void* stream);
// kf_rmsnorm_bwd plus dres [rows, cols] bf16 (may be null), added to dx
KF_EXPORT int kf_rmsnorm_bwd_res(void* dx, void* dw, float* dw_acc,
    const void* dy, const void* x, const void* w, const float* rstd,
    const void* dres, int64_t rows, int64_t cols, void* stream);
KF_EXPORT int kf_layernorm_fwd(void* y, float* mu, float* rstd, const void* x,
    const void* w, const void* b, int64_t rows, int64_t cols, float eps,
    void* stream);
KF_EXPORT int64_t kf_layernorm_bwd_nparts(int64_t rows);
KF_EXPORT int kf_layernorm_bwd(void* dx, void* dw, void* db, float* part,
    const void* dy, const void* x, const void* w, const float* mu,
    const float* rstd, int64_t rows, int64_t cols, void* stream);

// ---- rope.hip / swiglu.hip / adamw.hip / cross_entropy.hip ----
KF_EXPORT int kf_rope(void* q, void* k, const float* cost, const float* sint,
    const int64_t* positions, int64_t B, int64_t S, int64_t Hq, int64_t Hkv,
    int64_t D, int64_t qts, int64_t kts, int64_t pos_offset, int backward,
    void* stream);
KF_EXPORT int kf_swiglu_fwd(void* y, const void* h, int64_t T, int64_t F,
    void* stream);
KF_EXPORT int kf_swiglu_bwd(void* dh, const void* dy, const void* h, int64_t T,
    int64_t F, void* stream);
KF_EXPORT int kf_adamw(void* p16, float* p32, const void* g, float* m,
    float* v, const float* wd_mask, int64_t n, float lr, float b1, float b2,
    float eps, float wd, int64_t step, void* stream);
// step tail: kf_adamw with the clip scale (device scalar gscale, may be null;
// g is rewritten with the scaled gradient when *gscale != 1) and a uint8
// per-64-element decay mask wd_groups (may be null; not both masks);
// kf_grad_sumsq writes sqrt(sum g^2) to out[0] through a partials buffer of
// kf_grad_sumsq_nparts(n) floats
KF_EXPORT int kf_adamw_clip(void* p16, float* p32, void* g, float* m,
    float* v, const float* wd_mask, const void* wd_groups,
    const float* gscale, int64_t n, float lr, float b1, float b2, float eps,
    float wd, int64_t step, void* stream);
KF_EXPORT int64_t kf_grad_sumsq_nparts(int64_t n);
KF_EXPORT int kf_grad_sumsq(float* out, float* partials, const void* g,
    int64_t n, void* stream);
KF_EXPORT int kf_ce_fwd(float* loss_sum, float* lse, const void* logits,
    const int64_t* targets, int64_t T, int64_t V, int64_t ignore_index,
    void* stream);
KF_EXPORT int kf_ce_bwd(void* dlogits, const void* logits, const float* lse,
    const int64_t* targets, const float* scale, int64_t T, int64_t V,
    int64_t ignore_index, void* stream);

// ---- skinny_gemm.hip / kv_store.hip / decode_fused.hip ----
KF_EXPORT int kf_skinny_gemm(void* c, const void* a, const void* w,
    const void* res, int64_t M, int64_t N, int64_t K, int64_t lda,
    int64_t ldw, int64_t ldc, void* stream);
KF_EXPORT int kf_skinny_gemm_q8(void* c, const void* a, const void* w8,
    const float* wscale, const void* res, int64_t M, int64_t N, int64_t K,
    int64_t lda, int64_t ldw, int64_t ldc, void* stream);
// grouped over device offsets (routed MoE decode): group e owns rows
// [offsets[e], offsets[e+1]) of c and reads a through a_rows (nullable)
KF_EXPORT int kf_skinny_gemm_grouped(void* c, const void* a,
    const void* w_bank, const int* offsets, const int* a_rows,
    int64_t n_groups, int64_t max_rows, int64_t total_rows, int64_t a_nrows,
    int64_t N, int64_t K, void* stream);
KF_EXPORT int kf_skinny_gemm_grouped_q8(void* c, const void* a,
    const void* w8, const float* wscale, const int* offsets,
    const int* a_rows, int64_t n_groups, int64_t max_rows,
    int64_t total_rows, int64_t a_nrows, int64_t N, int64_t K, void* stream);
KF_EXPORT int kf_kv_store(void* ck, void* cv, const void* k, const void* v,
    const void* slots, const void* positions, int64_t smax, int64_t row,
    int64_t n, void* stream);
KF_EXPORT int kf_decode_rope_store(void* qout, void* ck, void* cv,
    const void* qkv, const float* cost, const float* sint, const int* slots,
    const void* positions, int64_t N, int64_t Hq, int64_t Hkv, int64_t D,
    int64_t smax, void* stream);

// ---- attention forward, D = 128 (attention_fwd.hip, attention_fwd4.hip) ----
// kf_attn_fwd dispatches on S: S % 256 == 0 -> kf_attn_fwd4, any other
// multiple of 128 -> the 4-wave kernel in attention_fwd.hip.
KF_EXPORT int kf_attn_fwd(void* o, float* lse, const void* q, const void* k,
    const void* v, int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t D,
    int64_t qts, int64_t kts, float scale, int causal, void* stream);
KF_EXPORT int kf_attn_fwd4(void* o, float* lse, const void* q, const void* k,
    const void* v, int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t D,
    int64_t qts, int64_t kts, float scale, int causal, void* stream);
KF_EXPORT int kf_attn_fwd4_rect(void* o, float* lse, const void* q,
    const void* k, const void* v, int64_t B, int64_t Sq, int64_t Skv,
    int64_t Hq, int64_t Hkv, int64_t D, int64_t qts, int64_t kts, float scale,
    int64_t qoff, void* stream);
// scripts/attn_ablate.py and scripts/probe_tr16.py
KF_EXPORT int kf_attn_fwd4_abl(int mode, void* o, float* lse, const void* q,
    const void* k, const void* v, int64_t B, int64_t S, int64_t Hq,
    int64_t Hkv, int64_t D, int64_t qts, int64_t kts, float scale, int causal,
    void* stream);
KF_EXPORT int kf_tr16_probe(void* out, const void* in, int mode, void* stream);

// ---- attention backward, D = 128 (attention_bwd.hip, attention_bwd8.hip) --
// The *_rope forms add cos, sin, pos_offset before the stream.
KF_EXPORT int kf_attn_bwd(void* dq, void* dk, void* dv, const void* dout,
    const void* q, const void* k, const void* v, const void* o,
    const float* lse, float* delta, int64_t B, int64_t S, int64_t Hq,
    int64_t Hkv, int64_t D, int64_t qts, int64_t kts, int64_t dqts,
    int64_t dkts, float scale, int causal, void* stream);
KF_EXPORT int kf_attn_bwd_rope(void* dq, void* dk, void* dv, const void* dout,
    const void* q, const void* k, const void* v, const void* o,
    const float* lse, float* delta, int64_t B, int64_t S, int64_t Hq,
    int64_t Hkv, int64_t D, int64_t qts, int64_t kts, int64_t dqts,
    int64_t dkts, float scale, int causal, const float* cost,
    const float* sint, int64_t pos_offset, void* stream);
KF_EXPORT int kf_attn_bwd8_dq(void* dq, const void* q, const void* k,
    const void* v, const void* dout, const float* lse, const float* delta,
    int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t qts, int64_t kts,
    int64_t dqts, float scale, int causal, void* stream);
KF_EXPORT int kf_attn_bwd8_dq_rope(void* dq, const void* q, const void* k,
    const void* v, const void* dout, const float* lse, const float* delta,
    int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t qts, int64_t kts,
    int64_t dqts, float scale, int causal, const float* cost,
    const float* sint, int64_t pos_offset, void* stream);
KF_EXPORT int kf_attn_bwd8_dkv(void* dk, void* dv, const void* q,
    const void* k, const void* v, const void* dout, const float* lse,
    const float* delta, int64_t B, int64_t S, int64_t Hq, int64_t Hkv,
    int64_t qts, int64_t kts, int64_t dkts, float scale, int causal,
    void* stream);
KF_EXPORT int kf_attn_bwd8_dkv_rope(void* dk, void* dv, const void* q,
    const void* k, const void* v, const void* dout, const float* lse,
    const float* delta, int64_t B, int64_t S, int64_t Hq, int64_t Hkv,
    int64_t qts, int64_t kts, int64_t dkts, float scale, int causal,
    const float* cost, const float* sint, int64_t pos_offset, void* stream);
KF_EXPORT int kf_attn_bwd8_dkv_fused(void* dk, void* dv, const void* q,
    const void* k, const void* v, const void* dout, const float* lse,
    const float* delta, int64_t B, int64_t S, int64_t Hq, int64_t Hkv,
    int64_t qts, int64_t kts, int64_t dkts, float scale, int causal,
    void* stream);
KF_EXPORT int kf_attn_bwd8_dkv_fused_rope(void* dk, void* dv, const void* q,
    const void* k, const void* v, const void* dout, const float* lse,
    const float* delta, int64_t B, int64_t S, int64_t Hq, int64_t Hkv,
    int64_t qts, int64_t kts, int64_t dkts, float scale, int causal,
    const float* cost, const float* sint, int64_t pos_offset, void* stream);

// ---- attention, D = 64 (attention_d64.hip) ----
KF_EXPORT int kf_attn64_fwd(void* o, float* lse, const void* q, const void* k,
    const void* v, int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t qts,
    int64_t kts, float scale, int causal, int64_t kv_len, void* stream);
KF_EXPORT int kf_attn64_bwd(void* dq, void* dk, void* dv, const void* dout,
    const void* q, const void* k, const void* v, const void* o,
    const float* lse, float* delta, int64_t B, int64_t S, int64_t Hq,
    int64_t Hkv, int64_t qts, int64_t kts, float scale, int causal,
    int64_t kv_len, void* stream);
// per-sequence lengths: seq_lens device int32 [B], non-causal
KF_EXPORT int kf_attn64_fwd_varlen(void* o, float* lse, const void* q,
    const void* k, const void* v, const int32_t* seq_lens, int64_t B,
    int64_t S, int64_t Hq, int64_t Hkv, int64_t qts, int64_t kts, float scale,
    void* stream);
KF_EXPORT int kf_attn64_bwd_varlen(void* dq, void* dk, void* dv,
    const void* dout, const void* q, const void* k, const void* v,
    const void* o, const float* lse, float* delta, const int32_t* seq_lens,
    int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t qts, int64_t kts,
    float scale, void* stream);

// ---- mixture-of-experts routing, dispatch, combine (moe.hip) ----
// T tokens, E experts, k = top_k, h hidden, M rows of the permuted buffer.
// topi / pos int32 [T, k], src int32 [T * k], offsets int32 [n_local + 1],
// probs fp32 [T, k], topw / dw bf16 [T, k]; work int32
// [kf_moe_sort_nwork(T, k, n_local)]. 2 <= E <= 64, k <= min(E, 8), h % 8 == 0.
KF_EXPORT int kf_moe_route(void* topi, float* probs, void* topw,
    const void* logits, int64_t T, int64_t E, int64_t k, void* stream);
KF_EXPORT int kf_moe_route_bwd(void* dlogits, const void* dw,
    const float* probs, const void* topi, int64_t T, int64_t E, int64_t k,
    void* stream);
KF_EXPORT int64_t kf_moe_sort_nwork(int64_t T, int64_t k, int64_t n_local);
KF_EXPORT int kf_moe_sort(void* pos, void* src, void* offsets, void* work,
    const void* topi, int64_t T, int64_t k, int64_t e_lo, int64_t n_local,
    void* stream);
KF_EXPORT int kf_moe_gather(void* xp, const void* x, const void* src,
    int64_t M, int64_t T, int64_t h, void* stream);
KF_EXPORT int kf_moe_gather_bwd(void* dx, const void* dxp, const void* pos,
    int64_t T, int64_t k, int64_t h, int64_t M, void* stream);
KF_EXPORT int kf_moe_combine(void* out, const void* y, const void* topw,
    const void* pos, int64_t T, int64_t k, int64_t h, int64_t M,
    void* stream);
KF_EXPORT int kf_moe_combine_bwd(void* dy, void* dw, const void* dout,
    const void* y, const void* topw, const void* pos, int64_t T, int64_t k,
    int64_t h, int64_t M, void* stream);

// ---- decode attention over the KV cache (attention_decode.hip) ----
KF_EXPORT int kf_attn_decode(void* out, void* part_o, void* part_ml,
    const void* q, const void* kcache, const void* vcache, const int* slots,
    const int* lens, int64_t N, int64_t smax, int64_t Hq, int64_t Hkv,
    int64_t D, int64_t splits, float scale, void* stream);

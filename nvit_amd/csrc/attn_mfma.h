// Entry points of the MFMA flash-attention kernels (attn_mfma.hip) for the C ABI functions in attn_ref.hip.
#pragma once
#include "common.h"

int nvit_attn_fwd_mfma(const void* qh, const void* kh, const void* vh, float scale, float qpre, const float* sqk,
                       float c_q, void* o, float* lse, int B, int H, int Tq, int Tk, int d, hipStream_t s);
int nvit_attn_bwd_mfma(const void* dout, const void* qh, const void* kh, const void* vh, const void* o, const float* lse,
                       float* delta, float scale, void* dqh, void* dkh, void* dvh, int B, int H, int Tq, int Tk,
                       int d, hipStream_t s);
// with the q/k-normalise backward fused into the epilogues (head dim 64)
int nvit_attn_bwd_mfma_fused(const void* dout, const void* qh, const void* kh, const void* vh, const void* o,
                             const float* lse, float* delta, float scale, const float* rq, const float* rk, const float* sqk,
                             float c_q, float qpre, void* dq, int ldq, void* dk, void* dv, int ldkv, float* part_q,
                             float* part_k, int B, int H, int Tq, int Tk, int d, hipStream_t s);

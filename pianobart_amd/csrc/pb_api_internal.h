// Internal: the public C ABI plus shared launch helpers.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/pianobart_hip.h"

// pb_gemm2.hip: bf16 fast path; returns 1 when it declines (caller falls back), 0 ok, <0 error.
int pb_gemm2_try(const pb_gemm_desc* d, void* stream);
// o_k[c] += sum over nblk rows of partials (nblk, nacc, d), k < nacc <= 2 (pb_norm.hip)
int pb_finalize_rows(const float* partials, int nblk, int d, float* out, void* stream, int nacc = 1, float* out1 = nullptr);
// storage for partial sums whose reduction is deferred to pb_defer_flush (NULL when no deferral is open or it is full): pass it to
// the kernel instead of the caller's workspace, then hand it to pb_finalize_rows as usual
float* pb_defer_alloc(size_t nfloats);
// pb_gemm_x3.hip: dtype PB_F32X3 -- f32 operands cut into bf16 (hi, lo) pairs, one bf16 GEMM over 3 K, f32 C
int pb_gemm_x3(const pb_gemm_desc* d, void* stream);
// The attention families behind pb_attn_fwd / pb_attn_bwd (pb_flash.hip checks the descriptor and picks one; with packed rows it has
// zeroed the batch strides, key_mask and kmax): pipelined bf16 head_dim 64 / 96 / 128 (pb_flash64.hip), its one-pass backward for
// head_dim 64 (pb_flash1.hip), split-bf16 f32 (pb_flash_x3.hip).
int pb_flash64_fwd(const pb_attn_desc& d, hipStream_t stream);
int pb_flash64_bwd(const pb_attn_desc& d, hipStream_t stream);
int pb_flash1_bwd(const pb_attn_desc& d, hipStream_t stream);
int pb_flash_x3_fwd(const pb_attn_desc& d, hipStream_t stream);
int pb_flash_x3_bwd(const pb_attn_desc& d, hipStream_t stream);
// 256 bytes of device zeros per device, allocated on first use (never freed: lives as long as the process' HIP context); NULL on failure
const void* pb_zero_page();

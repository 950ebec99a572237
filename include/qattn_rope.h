/*
 * qattn_rope.h -- rotary position embedding (RoPE) fused into the fp8 quant pre-pass of q and k (ABI 8 addition; the names are found by
 * symbol, include/qattn.h and QATTN_ABI_VERSION unchanged).  The caller hands over the UNROTATED 16-bit q and k with cos / sin tables; the
 * pre-pass rotates the values it already holds in registers, so the rotated 16-bit tensors never exist in memory.  The attention kernels
 * are untouched: they receive the same q8 / k8 / scales the unfused composition (rotate in 16 bit, then qattn_quant_fp8) would give them,
 * BIT FOR BIT.
 *
 * Semantics.  Row x[b,h,s,:] of q and of k is rotated with row s of a table pair (cos, sin) before quantisation:
 *   tables       fp32, D/2 entries per row, rows 0 .. S-1 read (the caller's table has T >= S rows; slicing cos[off:off+S] positions a chunk
 *                without a copy: pass the slice's address).  Row s of batch element b is at  base + b batch_stride + s row_stride  (floats).
 *                batch_stride = 0: one table [T, D/2] for every batch element; else the [B, T, D/2] form.  cos and sin of one pair share
 *                their strides.  Base 16-byte aligned, both strides non-negative multiples of 4 floats (the rows are read as float4).
 *                q and k have a pair each (cross-attention, or k positions offset from q's); pass the same pointers for self-attention.
 *   interleaved  0: pairs (i, i + D/2), i < D/2 (GPT-NeoX / HF rotate_half);  1: pairs (2i, 2i + 1) (GPT-J; the complex-pair form of Wan
 *                and Flux) -- flash-attn's apply_rotary_emb name and meaning.  Pair i uses table entry i.  The FULL head dim is rotated;
 *                there is no partial rotary_dim.
 *   arithmetic   a, b = fp32(x_first), fp32(x_second)                 exact up-casts of the pair
 *                y_first  = round16( fl(a c) - fl(b s) )              three separately rounded fp32 operations, no FMA contraction
 *                y_second = round16( fl(b c) + fl(a s) )              round16 = round to nearest even to the input dtype (bf16 / fp16)
 *                then abs-max, scale and fp8 bytes are those of qattn_quant_fp8 applied to y: quant8 of csrc/qattn_common.h, both `numerics`,
 *                head-wise or token-wise scales, e4m3 or e5m2; k in KFRAG with the padding rows of the last 64-key chunk as zero bytes.
 *                Rounding through 16 bits gives away some accuracy on purpose: the fused path changes time and nothing else.
 *   non-finite   an inf or NaN input poisons its head (token-wise: its row) exactly as in qattn_quant_fp8; fp16 products that overflow become
 *                inf in round16 and do the same.  A -0 input may come out +0: (-0) - (-0).
 *
 * qattn_rope_quant_qk_fp8: the pre-pass alone, q and k in ONE abs-max launch (head-wise scales only) and ONE quantise launch.
 *   q, k         [B,Hq,Sq,D] / [B,Hkv,Skv,D] bf16 / fp16 (in_fmt), 16-byte aligned.  Either may be NULL: that tensor is skipped and none of its
 *                tables, outputs or dimensions beyond being positive is used (the stand-alone use on one tensor).
 *   strides      NULL (dense) or 6 element strides {batch, head, row} of q then of k, the rules of include/qattn_strided.h: D innermost and
 *                dense, every stride a non-negative multiple of 8, row stride in [D, 2^23].
 *   q8           fp8 [B,Hq,Sq,D] row-major.   k8: k_layout = QATTN_LAYOUT_KFRAG (what the attention entries take) or QATTN_LAYOUT_ROWMAJOR.
 *   scale_q/_k   fp32 [B,H] (QATTN_SCALE_HEAD) or [B,H,S] (QATTN_SCALE_TOKEN).
 *   workspace    qattn_rope_quant_qk_workspace_bytes(B, Hq, Hkv) bytes, 4-byte aligned; needed for head-wise scales, may be NULL otherwise.
 *
 * qattn_fp8_rope_quant_attention_forward: the whole step in one call -- the pre-pass above (k8 in KFRAG), V through qattn_quant_fp8
 * (head-wise, VFRAG; v_fmt = fp8_fmt) or not at all (v_fmt = in_fmt: v8 / scale_v may be NULL, 16-bit P on the caller's V), then
 * qattn_fp8_attention_forward UNCHANGED.  Numerics: the PATH TABLE's `separate` row (`separate16` with a 16-bit V) on the rotated inputs.
 *   v            dense [B,Hkv,Skv,D] (V is not rotated; `strides` covers q and k only).   out: dense [B,Hq,Sq,D] in in_fmt.
 *   lse          NULL or the per-row log-sum-exp (lse_layout, as qattn_fp8_attention_forward).
 *   q8, k8, v8, scale_*   caller-provided outputs, all written (v8 / scale_v only with an fp8 V).
 *   workspace    qattn_fp8_rope_quant_attention_workspace_bytes(...) bytes, 16-byte aligned, always needed.
 *   Key smoothing (include/qattn_smooth.h) is not combined with RoPE: this entry has no k_mean and ignores config-level smooth_k.
 *
 * Conventions of every entry: device pointers, `stream` = hipStream_t, 0 or a negative QATTN_ERR_* code before any launch, no host sync,
 * no allocation, no environment variable, graph-capture safe.  Errors: QATTN_ERR_INVALID_ARG for a NULL or misaligned pointer, a
 * non-positive dimension, more than 65535 * 64 rows, a refused stride, an unknown enum; QATTN_ERR_UNSUPPORTED_DIM for D outside {64, 128, 256}
 * (or Hq % Hkv != 0 in the attention entry); QATTN_ERR_UNSUPPORTED_FMT for a format or k_layout; QATTN_ERR_WORKSPACE.
 * Sizes, alignment and which bytes are written: include/qattn_buffers.h.
 */
#ifndef QATTN_ROPE_H_
#define QATTN_ROPE_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t qattn_rope_quant_qk_workspace_bytes(int B, int Hq, int Hkv);
int qattn_rope_quant_qk_fp8(const void* q, const void* k, const long long* strides, int in_fmt, const float* cos_q, const float* sin_q,
                            long long table_q_batch_stride, long long table_q_row_stride, const float* cos_k, const float* sin_k,
                            long long table_k_batch_stride, long long table_k_row_stride, int interleaved, void* q8, void* k8, int k_layout,
                            float* scale_q, float* scale_k, int B, int Hq, int Hkv, int Sq, int Skv, int D, int out_fmt, int scale_mode,
                            int numerics, void* workspace, size_t workspace_bytes, void* stream);

size_t qattn_fp8_rope_quant_attention_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Skv, int D);
int qattn_fp8_rope_quant_attention_forward(const void* q, const void* k, const void* v, const long long* strides, int in_fmt,
                                           const float* cos_q, const float* sin_q, long long table_q_batch_stride,
                                           long long table_q_row_stride, const float* cos_k, const float* sin_k,
                                           long long table_k_batch_stride, long long table_k_row_stride, int interleaved, void* out,
                                           float* lse, void* q8, void* k8, void* v8, float* scale_q, float* scale_k, float* scale_v, int B,
                                           int Hq, int Hkv, int Sq, int Skv, int D, int fp8_fmt, int v_fmt, int scale_mode, int numerics,
                                           int is_causal, float sm_scale, int precision, int lse_layout, void* workspace,
                                           size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_ROPE_H_ */

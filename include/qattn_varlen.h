/*
 * qattn_varlen.h -- variable-length ("varlen") FP8 attention on PACKED sequences: the call shape of flash-attn's flash_attn_varlen_func
 * (ABI 8 addition; names found by symbol, include/qattn.h unchanged).
 *
 * B sequences are packed along the token axis: q [total_q, Hq, D], k / v [total_k, Hkv, D], bf16 or fp16 (in_fmt), with int32 tables
 * cu_seqlens_q / cu_seqlens_k [B+1] (sequence i = tokens cu[i] .. cu[i+1]-1) and an optional int32 seqused_k [B] (keys used by sequence i,
 * counted from cu_seqlens_k[i]: padded K / V without a copy; keys beyond it influence no output bit, the K scale included).
 *
 * Numerics, per sequence i and head h, bit for bit:
 *   scale_q / q8 = the head-wise quant pre-pass (qattn_quant_fp8, QATTN_SCALE_HEAD, `numerics`) of sequence i's queries alone;
 *   scale_k / k8 likewise over its USED keys;  out / lse = qattn_fp8_attention_forward_rowmajor on those operands with pv_fmt = v16_fmt
 *   (PATH TABLE row separate16: FP8 Q K^T, 16-bit P on the ORIGINAL 16-bit V -- every row QATTN_PATH_V16) and QATTN_LSE_NATURAL.
 *   is_causal: key j <= query r of the same sequence, top-left aligned (torch SDPA's is_causal; flash-attn >= 2.1 aligns bottom-right
 *   when L_q != L_k).  sm_scale <= 0: 1/sqrt(D).  A sequence with L_q = 0 has no rows; one with no used key and L_q > 0 gets zero rows
 *   and an LSE of -inf.
 *
 *   strides   NULL = dense, or 6 element strides {token, head} of q, then of k, of v: D innermost and dense, every stride a non-negative
 *             multiple of 8 (rows 16-byte aligned), q / k / v 16-byte aligned; else QATTN_ERR_INVALID_ARG.  V is read in place.
 *   out       dense [total_q, Hq, D] in in_fmt;  lse: NULL or fp32 [Hq, total_q] natural log-sum-exp (flash-attn's varlen layout).
 *   q8 / k8 / scale_q / scale_k   NULL (then they live in the workspace) or outputs:  q8 row-major, sequence i's [Hq, L_q, D] slab at
 *             byte Hq D cu_q[i];  k8 KFRAG (include/qattn.h), sequence i's [Hkv, ceil(L_k/64) 64, D] image at byte Hkv D (cu_k[i] + 64 i);
 *             sizes: qattn_varlen_tensor_bytes(QATTN_LAYOUT_ROWMAJOR / _KFRAG, ...);  scale_q fp32 [B, Hq], scale_k fp32 [B, Hkv].
 *
 * Sizes, alignment and which bytes of each buffer are written: include/qattn_buffers.h.
 * Tables are read on the device only: no host synchronisation, no allocation, graph-capture safe (a captured call follows later
 * contents of the tables).  Every extent is clamped -- start = clamp(cu[i], 0, total), end = clamp(cu[i+1], start, total), used keys
 * <= end - start -- so that no table content makes a kernel touch memory outside its tensors; results for inconsistent tables are
 * unspecified.  Errors (before any device call): QATTN_ERR_INVALID_ARG (NULL q / k / v / out / tables, B < 1, a non-positive head count,
 * a negative total, bad strides or enums), _UNSUPPORTED_DIM (D not in {64, 128, 256}, Hq % Hkv != 0), _UNSUPPORTED_FMT, _WORKSPACE.
 */
#ifndef QATTN_VARLEN_H_
#define QATTN_VARLEN_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the q8 (QATTN_LAYOUT_ROWMAJOR: H total D) or k8 (QATTN_LAYOUT_KFRAG: H D (total + 64 B)) buffer; 0 for bad arguments */
size_t qattn_varlen_tensor_bytes(int layout, int B, int H, int total, int D);
size_t qattn_fp8_quant_attention_varlen_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int D);
int qattn_fp8_quant_attention_varlen_forward(const void* q, const void* k, const void* v, const long long* strides, int in_fmt, void* out,
                                             float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k, const int* seqused_k, int B,
                                             int Hq, int Hkv, int total_q, int total_k, int D, int fp8_fmt, int numerics, int is_causal,
                                             float sm_scale, void* q8, void* k8, float* scale_q, float* scale_k, void* workspace,
                                             size_t workspace_bytes, void* stream);


/*
 * Key smoothing (include/qattn_smooth.h: K is quantised as fp32(k) - its channel mean, `out` is mathematically unchanged, the LSE is
 * corrected by sm_scale * q.m).  An ABI-8 addition, names found by symbol; the plain entry keeps its signature, launches and bits.
 * q.m is the same for every key a row attends, whichever keys a block mask lists and whichever sequence a packed row belongs to.
 *
 * qattn_fp8_quant_attention_varlen_forward_smooth: the arguments of qattn_fp8_quant_attention_varlen_forward plus k_mean (out, fp32
 * [B, Hkv, D], required, 16-byte aligned).  Per sequence i with L used keys (seqused_k honoured, extents clamped as in qattn_varlen.h),
 * bit for bit: k_mean[i], scale_k[i] and the k8 bytes of its KFRAG image are what qattn_fp8_quant_attention_forward_smooth
 * (QATTN_SCALE_HEAD, the same fp8_fmt and numerics) leaves for that sequence alone -- the mean in the summation order of a dense head of
 * L rows, evaluated per sequence on the device; padding rows of the last chunk zero bytes.  A sequence with no used key gets k_mean = 0
 * (not 0/0); keys beyond seqused_k influence no output bit, the mean included.  q8 / scale_q, the attention kernel and `out` per row are
 * those of the plain entry on the smoothed operands; lse[h, t] (when non-NULL) = what the launch writes + sm_scale * sum_d
 * fp32(q[t,h,d]) * k_mean[seq(t), kv(h), d], rows at -inf staying -inf.  total_q = 0: nothing is computed or written, k_mean included.
 * Launches: zeroing node; K's mean (two), abs-max and quantise passes; q's abs-max and quantise passes; attention; the LSE correction
 * when lse is asked for.  No length is read on the host, nothing is allocated, graph-capture safe (a captured call follows later contents
 * of the tables).
 *
 * Workspace: at least ..._smooth_workspace_bytes(...), 16-byte aligned; errors as the plain entry, and
 * QATTN_ERR_INVALID_ARG for a NULL or misaligned k_mean.
 */
size_t qattn_fp8_quant_attention_varlen_smooth_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int D);
int qattn_fp8_quant_attention_varlen_forward_smooth(const void* q, const void* k, const void* v, const long long* strides, int in_fmt, void* out,
                                                    float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k, const int* seqused_k, int B,
                                                    int Hq, int Hkv, int total_q, int total_k, int D, int fp8_fmt, int numerics, int is_causal,
                                                    float sm_scale, void* q8, void* k8, float* scale_q, float* scale_k, void* workspace,
                                                    size_t workspace_bytes, void* stream, float* k_mean);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_VARLEN_H_ */

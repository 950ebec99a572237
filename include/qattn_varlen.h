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


/*
 * FP8 P.V on packed sequences (an ABI-8 addition, names found by symbol; the entries above keep their signatures, launches and bits).
 *
 * qattn_fp8_quant_attention_varlen_forward_fp8pv: the arguments of qattn_fp8_quant_attention_varlen_forward, with after sm_scale
 *   precision   QATTN_PRECISION_FAST or _ACCURATE (_AUTO and anything else: QATTN_ERR_INVALID_ARG -- no moments, no rescue pass here);
 * after k8
 *   v8          NULL (then it lives in the workspace) or out: per-sequence VFRAG images laid out like k8's KFRAG images -- sequence i's
 *               [Hkv, ceil(L_k/64) 64, D] image at byte Hkv D (cu_k[i] + 64 i), L_k its USED keys; size qattn_varlen_tensor_bytes(
 *               QATTN_LAYOUT_KFRAG, B, Hkv, total_k, D): k8's (a 64-key chunk is 64 D bytes in both layouts; the query keeps answering 0
 *               for QATTN_LAYOUT_VFRAG, as released);
 * after scale_k
 *   scale_v     NULL or fp32 [B, Hkv];
 *   row_path    NULL or uint8 [Hq, total_q] (the LSE's layout): QATTN_PATH_* of every row of a sequence;
 *   k_mean      NULL = no smoothing; else out, fp32 [B, Hkv, D], 16-byte aligned, as in ..._forward_smooth;
 * then workspace, workspace_bytes, stream.
 *
 * NUMERICS, per sequence i and head h, bit for bit:
 *   q8 / scale_q, k8 / scale_k, k_mean   those of qattn_fp8_quant_attention_varlen_forward (with k_mean: of ..._forward_smooth, LSE
 *                correction included) for the same arguments.
 *   v8 / scale_v the head-wise quant pre-pass (qattn_quant_fp8, QATTN_SCALE_HEAD, QATTN_LAYOUT_VFRAG, `numerics`) of sequence i's USED
 *                keys alone; the padding rows of its last 64-key chunk are zero bytes.  Keys beyond seqused_k influence no output bit,
 *                V's scale included (NaN or 1e4 padding there is legal); V MUST BE FINITE on the used keys.
 *   attention    the sweep of qattn_fp8_block_sparse_attention_forward_fp8pv (include/qattn_block_sparse.h) over the sequence's 64-key
 *                chunks in ascending order, one 4-wave workgroup per 128-row tile t of the sequence, scale_v[i, kv(h)] applied in the
 *                epilogue: a non-causal sequence's rows and LSE are those of that entry on the sequence alone under an all-true mask.
 *                ACCURATE  exact exponentials and two-term (hi + lo) e4m3 P on every row; row_path QATTN_PATH_TWO_TERM.
 *                FAST      the one-term sweep (QATTN_PATH_ONE_TERM) for the tiles whose rows see n >= 1024 keys, two-term below;
 *                          n = used L_k, or with is_causal n = min(L_k, 128 (t + 1)).  One-term tiles: byte exponentials, or exact
 *                          exponentials when lse != NULL (the same bound, other bits).  No rescue: stated for score variance
 *                          sm_scale^2 D <= 1, as the block-sparse entry's FAST.
 *   is_causal    key j <= query r of the same sequence, top-left, token-exact: tile t sweeps chunks 0 .. ceil(min(L_k, 128 (t + 1)) / 64)
 *                - 1 and reads no K or V chunk beyond them.
 *   A sequence with L_q = 0 has no rows; one with queries and no used key gets zero rows, an LSE of -inf and QATTN_PATH_ONE_TERM.
 *   total_q = 0: nothing is computed or written.
 * Launches: zeroing node; [K's mean (two), abs-max and quantise passes with k_mean;] one abs-max and one quantise pass over q, k (unless
 * smoothed) and v; attention -- one launch for ACCURATE (and for FAST when total_k < 1024), two for FAST (one-term tiles, two-term tiles:
 * a workgroup of the other launch's tile returns at once); the LSE correction with k_mean and lse.  No length is read on the host, nothing
 * is allocated, graph-capture safe.  Errors, clamps and argument checks: those of the plain entry, before any device call; workspace at
 * least ..._fp8pv_workspace_bytes (with k_mean: ..._fp8pv_smooth_workspace_bytes), 16-byte aligned.
 */
size_t qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int D);
size_t qattn_fp8_quant_attention_varlen_fp8pv_smooth_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int D);
int qattn_fp8_quant_attention_varlen_forward_fp8pv(const void* q, const void* k, const void* v, const long long* strides, int in_fmt, void* out,
                                                   float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k, const int* seqused_k, int B,
                                                   int Hq, int Hkv, int total_q, int total_k, int D, int fp8_fmt, int numerics, int is_causal,
                                                   float sm_scale, int precision, void* q8, void* k8, void* v8, float* scale_q, float* scale_k,
                                                   float* scale_v, unsigned char* row_path, float* k_mean, void* workspace,
                                                   size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_VARLEN_H_ */

/*
 * qattn_window.h -- sliding-window (local) FP8 attention on PACKED sequences: flash-attn's flash_attn_varlen_func with
 * window_size = (left, right) (ABI 8 addition; names found by symbol, include/qattn.h and QATTN_ABI_VERSION unchanged).
 *
 * The arguments of qattn_fp8_quant_attention_varlen_forward (include/qattn_varlen.h) without is_causal, plus window_left, window_right
 * and k_mean.  Per sequence i with L_q queries and L_k USED keys (seqused_k honoured, extents clamped as in qattn_varlen.h) and
 * delta = L_k - L_q, query r (0-based within its sequence) attends key j iff
 *
 *     r + delta - window_left <= j <= r + delta + window_right   and   0 <= j < L_k;
 *
 * window_left = -1 / window_right = -1: unbounded on that side; values larger than any length are legal.  (-1, 0) is the causal mask
 * aligned BOTTOM-RIGHT (flash-attn >= 2.1) -- the top-left one of the packed entry's is_causal when L_q = L_k; (-1, -1) masks nothing.
 * A row whose window holds no key (rows r < -delta - window_right when L_q > L_k) gets a zero output row and an LSE of -inf, as the rows
 * of a sequence without keys.
 *
 * Numerics are the packed entry's: scale_q / q8, scale_k / k8 are the head-wise quant pre-pass per (sequence, head) over ALL its queries
 * and ALL its used keys -- keys outside every window still count toward K's scale (and K's mean), as the keys of masked tiles do in the
 * block-sparse entry -- and P.V is 16-bit P on the ORIGINAL 16-bit V, every row QATTN_PATH_V16.  For a row, out and lse are those of
 * qattn_fp8_attention_forward_rowmajor(pv_fmt = in_fmt) on the keys of its window.  Where the window masks nothing -- (-1, -1), or finite
 * values wider than every sequence -- the bits are those of qattn_fp8_quant_attention_varlen_forward(is_causal = 0); (-1, 0) with
 * cu_seqlens_q = cu_seqlens_k gives those of is_causal = 1.
 *
 * Work: a 256-row query block sweeps only the 64-key chunks that hold a key one of its rows attends -- about
 * (window_left + window_right + 256) / 64 + 1 chunks -- and V rows that no row of the block attends are never read (NaN there reaches no
 * output).  K's quantised bytes of every used key are produced by the pre-pass as before.
 *
 *   k_mean   NULL: no smoothing.  Non-NULL (fp32 [B, Hkv, D], 16-byte aligned): key smoothing with the contract of
 *            qattn_fp8_quant_attention_varlen_forward_smooth -- the mean over the sequence's used keys, k_mean / scale_k / k8 bit for bit
 *            what that entry leaves, the LSE corrected by sm_scale * q.k_mean, rows at -inf staying -inf.
 *
 * Launches: those of the packed entry (zeroing node, abs-max, quantise, with k_mean the smoothing launches and the LSE correction); only
 * the attention launch is this entry's own.  Tables are read on the device only: no host synchronisation, no allocation, graph-capture
 * safe (a captured call follows later contents of the tables); every extent is clamped.  Errors (before any device call): those of the
 * packed entry, and QATTN_ERR_INVALID_ARG for window_left < -1 or window_right < -1.
 *
 * Sizes, alignment and which bytes of each buffer are written: include/qattn_buffers.h.
 * Workspace: at least qattn_fp8_quant_attention_varlen_window_workspace_bytes(...) (enough with and without k_mean), 16-byte aligned.
 */
#ifndef QATTN_WINDOW_H_
#define QATTN_WINDOW_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t qattn_fp8_quant_attention_varlen_window_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int D);
int qattn_fp8_quant_attention_varlen_window_forward(const void* q, const void* k, const void* v, const long long* strides, int in_fmt, void* out,
                                                    float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k, const int* seqused_k, int B,
                                                    int Hq, int Hkv, int total_q, int total_k, int D, int fp8_fmt, int numerics,
                                                    int window_left, int window_right, float sm_scale, void* q8, void* k8, float* scale_q,
                                                    float* scale_k, void* workspace, size_t workspace_bytes, void* stream, float* k_mean);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_WINDOW_H_ */

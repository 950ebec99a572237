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
 *
 * qattn_fp8_quant_attention_varlen_window_forward_fp8pv -- the same mask with BOTH products on the FP8 matrix pipe: the arguments of
 * qattn_fp8_quant_attention_varlen_forward_fp8pv (include/qattn_varlen.h) with window_left, window_right in place of is_causal.
 * Per sequence i and head h:
 *   mask      the one above, unchanged: delta = L_k(used) - L_q, row r attends key j iff r + delta - window_left <= j <= r + delta +
 *             window_right and 0 <= j < L_k; -1 is unbounded; offsets are clamped so that no sum leaves 32 bits.
 *   operands  q8 / scale_q, k8 / scale_k, k_mean, v8 / scale_v are the packed FP8-PV entry's, bit for bit, by the same pre-pass launches:
 *             scales over ALL queries and ALL USED keys, windowed or not; V head-wise over the used keys.
 *   V finite  V must be FINITE on the used keys -- unlike the 16-bit entry above, which tolerates NaN in V rows no row attends: here every
 *             used V row goes through the abs-max and the quantiser.  Keys beyond seqused_k still influence no output bit.
 *   tile      one 4-wave workgroup per 128-row tile of one sequence (the block map of the packed FP8-PV entry).
 *   interval  [klo, khi] = the keys the tile's valid rows attend: from the first attended key of its first row with a key to the last
 *             attended key of its last row, clipped to [0, L_k).  The tile sweeps the 64-key chunks klo / 64 .. khi / 64 in ascending
 *             order and DMAs no other K or V chunk.
 *   accurate  QATTN_PRECISION_ACCURATE: exact exponentials and two-term e4m3 P on every row; row_path QATTN_PATH_TWO_TERM; asking for the
 *             LSE changes no bit of out.
 *   fast      QATTN_PRECISION_FAST: the one-term byte-exponential sweep (QATTN_PATH_ONE_TERM) for the tiles with
 *                 n = khi - klo + 1 >= 1024,
 *             two-term below; one-term tiles use exact exponentials when the LSE is asked for.  No rescue pass; stated for
 *             sm_scale^2 D <= 1.  This is the packed entry's own rule on this mask: (-1, 0) on equal tables gives n = min(L_k, 128 (t + 1))
 *             for tile t, (-1, -1) gives n = L_k, and every row of a tile attends at least n - 127 keys (the causal rule's worst case).
 *             Two launches (one-term tiles, two-term tiles); one when total_k < 1024.  QATTN_PRECISION_AUTO is not offered.
 *   range     sm_scale log2(e) scale_q scale_k < 3e18 (inputs whose abs-max product stays below about 1e20 at the default sm_scale): a row
 *             that meets fully masked chunks before its first key carries a finite start value times that factor.
 *   no key    a row whose window holds no key: a zero row, LSE -inf.  A tile whose interval is empty: the same with code
 *             QATTN_PATH_ONE_TERM, before any sweep.  A row without a key inside a tile that sweeps carries the tile's code.
 * Where the window masks nothing the bits (out, lse, row_path) are those of qattn_fp8_quant_attention_varlen_forward_fp8pv(is_causal = 0);
 * (-1, 0) with cu_seqlens_q = cu_seqlens_k gives those of is_causal = 1.
 * Workspace: the packed FP8-PV entry's -- the caller sizes it with qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes (with k_mean:
 * qattn_fp8_quant_attention_varlen_fp8pv_smooth_workspace_bytes); there is no size function of this entry's own.
 * Errors (before any device call): those of the packed FP8-PV entry (QATTN_PRECISION_AUTO and unknown enums: QATTN_ERR_INVALID_ARG), and
 * QATTN_ERR_INVALID_ARG for window_left < -1 or window_right < -1.  No host synchronisation, no allocation, graph-capture safe.
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
int qattn_fp8_quant_attention_varlen_window_forward_fp8pv(const void* q, const void* k, const void* v, const long long* strides, int in_fmt,
                                                          void* out, float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k,
                                                          const int* seqused_k, int B, int Hq, int Hkv, int total_q, int total_k, int D, int fp8_fmt,
                                                          int numerics, int window_left, int window_right, float sm_scale, int precision, void* q8,
                                                          void* k8, void* v8, float* scale_q, float* scale_k, float* scale_v,
                                                          unsigned char* row_path, float* k_mean, void* workspace, size_t workspace_bytes,
                                                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_WINDOW_H_ */

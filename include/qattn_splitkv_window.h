/*
 * qattn_splitkv_window.h -- SLIDING-WINDOW attention for the three split-KV entries: over contiguous prepared K / V
 * (include/qattn_splitkv.h, the appendable cache of include/qattn_kvcache.h included), over the paged cache (include/qattn_paged.h) and
 * for packed variable-length queries over the paged cache (include/qattn_paged_varlen.h).  ABI 8 addition: the names are found by symbol,
 * include/qattn.h and QATTN_ABI_VERSION are unchanged.  What Mistral, Gemma-2/3, gpt-oss and Phi-3 decode under; flash-attn's kv-cache
 * entry and vLLM take window_size next to block_table for it (vLLM's sliding_window = W is (W - 1, 0)).
 *
 * SEMANTICS: include/qattn_window.h's (flash-attn's).  window_size = (window_left, window_right), each >= -1, -1 = unbounded.  A sequence
 * has Sq queries and L = clamp(seqused_k, 0, Skv) used keys (packed: Sq_i, L_i per sequence), delta = L - Sq; position p attends the keys
 *     p + delta - window_left  <=  j  <=  p + delta + window_right,   0 <= j < L.
 * (-1, 0) is the siblings' is_causal = 1 (bottom-right), (-1, -1) their is_causal = 0.  A row whose window holds no key: a zero row, LSE
 * -inf, path byte ONE_TERM.
 *
 * Each entry has the argument list of its sibling with `is_causal` replaced by `window_left, window_right`; layouts, outputs, partial
 * buffers, launches (quant, attn, merge, path), graph-capture safety and every argument check are the sibling's; window_left or
 * window_right < -1: QATTN_ERR_INVALID_ARG.  The workspace is the sibling's: qattn_fp8_attention_splitkv_workspace_bytes,
 * qattn_fp8_attention_paged_splitkv_workspace_bytes, qattn_fp8_attention_paged_varlen_workspace_bytes.  Buffers: include/qattn_buffers.h.
 * The window entries ALWAYS run the window kernels (attn_splitkv_window_fp8_kernel and its paged / packed forms), also for (-1, 0) and
 * (-1, -1).
 *
 * THE PLAN (device side, all workgroup-uniform).
 *   interval    lo_i = window_left < 0 ? 0 : clamp(delta - window_left, 0, L): no position attends a key below lo_i.  The sequence's
 *               interval is [lo_i, L).
 *   split plan  cuts the key blocks of the interval, not of [0, L): kb0 = lo_i >> 7, nkb = ceil(L / 128) - kb0, per = ceil(nkb / ns);
 *               split s owns the keys [128 (kb0 + s per), min(128 (kb0 + (s + 1) per), L)).  A function of (L, Sq, window_left, ns)
 *               alone -- packed: of the sequence's own (L_i, Sq_i) -- and with window_left = -1 the siblings' plan.  (Over [0, L) a
 *               4096-key window on 32768 keys would leave 7 of every 8 splits empty.)
 *   tile range  a 128-row tile whose valid rows hold the positions [smin, smax] sweeps, of its split [k_begin, k_end),
 *                   klo = max(k_begin, window_left < 0 ? 0 : max(smin + delta - window_left, 0)),
 *                   khi = min(k_end - 1, window_right < 0 ? L - 1 : smax + delta + window_right),
 *               the 64-key chunks klo >> 6 .. khi >> 6 and fetches no other chunk; paged: it loads the table entry of no other page.
 *               keys = max(khi - klo + 1, 0) drives precision FAST's one-term rule (keys >= 1024) and the path byte; keys = 0: no sweep.
 *   token mask  the lane of position p keeps the keys p + delta - window_left .. min(L - 1, p + delta + window_right), applied in the
 *               chunks that cross an edge of some valid row of the tile or hold key L.
 *   arithmetic  delta -+ window is formed in 64 bits and clamped exactly (to [-Sq, L] / [-Sq - 1, L]) before it meets a 32-bit sum.
 *   dead bytes  keys below lo_i that share lo_i's 64-key chunk have P exactly 0, and 0 x NaN is NaN in the matrix pipe: the workgroup
 *               whose first chunk is lo_i >> 6 zeroes their V bytes in LDS before the stage is read.  K needs nothing (a masked score is
 *               replaced, not multiplied).
 * Host side: num_splits = 0 is the sibling's rule on min(Skv, window_left + Sq + 127) keys for window_left >= 0 (packed: max_seqlen_q for
 * Sq) -- qattn_splitkv_window_auto_splits / qattn_paged_varlen_window_auto_splits, pure functions of host ints, non-decreasing in
 * window_left, equal to the siblings' at window_left = -1; invalid arguments: 1.  FAST launches the one-term kernel whenever the interval
 * bound lets a workgroup reach 1024 keys.
 *
 * THE CONTRACT.
 *   1  No window masking anything: (-1, 0) gives the bits of the sibling with is_causal = 1, (-1, -1) those with is_causal = 0 -- out,
 *      lse, row_path and all partials, at every num_splits > 0.
 *   2  One split on contiguous prepared K / V with Hq = Hkv: out and lse are bit for bit those of
 *      qattn_fp8_quant_attention_varlen_window_forward_fp8pv (include/qattn_window.h) on the same sequence with head-wise scales: the
 *      chunks, their order, the masks (padding rows included) and the scales are the same.
 *   3  Paged = the contiguous window entry on the cache gathered through the table; packed = the paged window entry on each slot alone
 *      (the rule of include/qattn_paged_varlen.h).  Bit for bit.
 *   4  out, lse = the state merge (include/qattn_merge.h) of the partials, bit for bit.
 *   5  Bytes of keys outside [lo_i, L_i) influence no output bit: NaN patterns in K and V included, keys that share a chunk with lo_i
 *      included.  Table entries below lo_i / page_size and behind ceil(L_i / page_size) are never read; every entry that is read is
 *      clamped into the pool before it forms an address.
 *
 * WHAT A PAGED CACHE MAY FORGET.  With at most n queries per slot and window_left = W >= 0, a slot of length L reads no key below
 * L - n - W at this or any later length (lengths only grow; lo_i = L - Sq - W >= L - n - W).  So the first
 *     clamp(L - n - W, 0) / page_size
 * block-table entries of the slot are dead: the caller's allocator may hand their pages to someone else and leave the entries as they
 * are (or overwrite them with anything).  The library neither allocates nor frees pages.
 *
 * Learned attention sinks (gpt-oss): the sibling entries of include/qattn_sinks.h.  Not offered: "sink tokens + window" in one call (two
 * calls and a state merge); windows on the 16-bit P.V numerics.
 */
#ifndef QATTN_SPLITKV_WINDOW_H_
#define QATTN_SPLITKV_WINDOW_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

int qattn_splitkv_window_auto_splits(int B, int Hq, int Hkv, int Sq, int Skv, int D, int window_left, int num_cus);
int qattn_paged_varlen_window_auto_splits(int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int Skv, int D, int window_left, int num_cus);

int qattn_fp8_attention_splitkv_window_forward(const void* q16, int in_fmt, const void* k8_kfrag, const void* v8_vfrag, const float* scale_k,
                                               const float* scale_v, void* out, float* lse, const int* seqused_k, int B, int Hq, int Hkv, int Sq,
                                               int Skv, int D, int fp8_fmt, int numerics, int window_left, int window_right, float sm_scale,
                                               int precision, int num_splits, void* q8, float* scale_q, unsigned char* row_path, float* partial_o,
                                               float* partial_lse, unsigned char* partial_path, void* workspace, size_t workspace_bytes,
                                               void* stream);

int qattn_fp8_attention_paged_splitkv_window_forward(const void* q16, int in_fmt, const void* k_pool, const void* v_pool, const int* block_table,
                                                     long long table_stride, int num_pages, int page_size, int max_pages, const float* scale_k,
                                                     const float* scale_v, void* out, float* lse, const int* seqused_k, int B, int Hq, int Hkv,
                                                     int Sq, int Skv, int D, int fp8_fmt, int numerics, int window_left, int window_right,
                                                     float sm_scale, int precision, int num_splits, void* q8, float* scale_q,
                                                     unsigned char* row_path, float* partial_o, float* partial_lse, unsigned char* partial_path,
                                                     void* workspace, size_t workspace_bytes, void* stream);

int qattn_fp8_attention_paged_varlen_window_forward(const void* q16, const long long* q_strides2, int in_fmt, const void* k_pool,
                                                    const void* v_pool, const int* block_table, long long table_stride, int num_pages,
                                                    int page_size, int max_pages, const float* scale_k, const float* scale_v, void* out,
                                                    float* lse, const int* cu_seqlens_q, const int* seqused_k, int B, int Hq, int Hkv, int total_q,
                                                    int max_seqlen_q, int Skv, int D, int fp8_fmt, int numerics, int window_left, int window_right,
                                                    float sm_scale, int precision, int num_splits, void* q8, float* scale_q,
                                                    unsigned char* row_path, float* partial_o, float* partial_lse, unsigned char* partial_path,
                                                    void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_SPLITKV_WINDOW_H_ */

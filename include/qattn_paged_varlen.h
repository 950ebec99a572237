/*
 * qattn_paged_varlen.h -- PACKED variable-length queries over the paged FP8 K/V cache of include/qattn_paged.h: one call for a serving
 * step that mixes chunked prefill (hundreds of queries), decode (one query, or a few speculative ones) and idle slots (ABI 8 addition;
 * the names are found by symbol, include/qattn.h and QATTN_ABI_VERSION unchanged).  The call shape of flash-attn's / vLLM's
 * flash_attn_varlen_func(q [total_q, Hq, D], ..., cu_seqlens_q, max_seqlen_q, seqused_k, block_table, causal = True).
 *
 * qattn_fp8_attention_paged_splitkv_forward takes q [B, Hq, Sq, D]: every sequence has Sq queries.  Here sequence i owns the tokens
 *     start_i = clamp(cu_seqlens_q[i], 0, total_q)  ..  end_i = clamp(cu_seqlens_q[i + 1], start_i, total_q)
 * of q [total_q, Hq, D] (the clamps of include/qattn_varlen.h), Sq_i = end_i - start_i of them (0: an idle slot), and attends the first
 * L_i = clamp(seqused_k[i], 0, Skv) keys of slot i of the cache; causal: bottom-right PER SEQUENCE, position p of sequence i attends the
 * keys j <= p + L_i - Sq_i.  Pools, block table, scales, page rules, entries read and clamped: include/qattn_paged.h, unchanged.
 *
 * LAYOUTS (the contract).
 *   q16         [total_q, Hq, D] 16-bit through the element strides {token, head} of q_strides2 (NULL: dense {Hq D, D}); head_dim innermost.
 *   out         [total_q, Hq, D] dense, in in_fmt.          partial_o    fp32 [ns, total_q, Hq, D].
 *   lse         fp32 [Hq, total_q] (flash-attn's packed LSE layout); row_path uint8 [Hq, total_q];
 *   partial_lse fp32 [ns, Hq, total_q];                     partial_path uint8 [ns, Hq, total_q].
 *   q8          Hq total_q D bytes: sequence i's row-major [Hq, Sq_i, D] slab at byte Hq D start_i (the packed pre-pass's layout,
 *               include/qattn_varlen.h);  scale_q fp32 [B, Hq].
 * Rows of tokens that belong to no sequence (cu_seqlens_q[B] < total_q: a padded token bucket; or an inconsistent table) have
 * unspecified contents.  Whatever cu_seqlens_q, seqused_k and the block table hold, no address leaves the described tensors.
 *
 * THE RULE.  For every sequence with Sq_i > 0 the rows of out, lse, row_path and of the partials -- and its slab of q8 and row of scale_q --
 * are, bit for bit, those of qattn_fp8_attention_paged_splitkv_forward on that sequence ALONE (B = 1: its queries as [1, Hq, Sq_i, D],
 * row i of the table, of the scales and of seqused_k; the same Skv, num_splits > 0, precision and the rest): the q scales are per
 * (sequence, head), a 128-row tile of a kv head's packed rows (packed row r < G Sq_i = query head hkv G + r / Sq_i at position r % Sq_i)
 * never holds rows of two sequences, and the split plan is a function of L_i and num_splits alone.  So the contracts of
 * include/qattn_splitkv.h carry over per sequence.
 *
 * Launches, all on `stream`, none reading a table on the host (no host synchronisation, no allocation, graph-capture safe; a captured
 * call follows the later contents of cu_seqlens_q, seqused_k and the block table):
 *   quant  the packed pre-pass of include/qattn_varlen.h on q alone (a zeroing node, abs-max, quantise)
 *   attn   attn_paged_varlen_splitkv_fp8_kernel: Hkv NT ns workgroups, NT = B + ceil(G total_q / 128) tile slots per kv head, the splits of
 *          a tile neighbours.  Slot j belongs to the largest sequence i with i + floor(G start_i / 128) <= j, as its tile
 *          j - (i + floor(G start_i / 128)); a slot that is no tile of its sequence exits before it touches memory (at most B per kv
 *          head and split).  One launch for ACCURATE, two for FAST, as the paged entry.
 *   merge  num_splits > 1: the merge chain of the split-KV entries on the packed strides of include/qattn_merge.h (B = 1, S = total_q)
 *   path   row_path with num_splits > 1
 *
 * num_splits = 0: qattn_paged_varlen_auto_splits on the device's CU count -- qattn_splitkv_auto_splits (include/qattn_splitkv.h) with its
 * tile count B Hkv ceil(G Sq / 128) replaced by
 *     Hkv min(B ceil(G max_seqlen_q / 128), min(B, total_q) + floor(G total_q / 128)),
 * both terms upper bounds of the true count, the sum of ceil(G Sq_i / 128), which only the device knows.  A pure function of host ints; with
 * every sequence at Sq queries (total_q = B Sq, max_seqlen_q = Sq) it returns what qattn_splitkv_auto_splits(B, Hq, Hkv, Sq, Skv, D, cus)
 * returns.  Invalid arguments: 1.  max_seqlen_q is read by this rule only; the kernels take every count from cu_seqlens_q.
 *
 * Argument checks, before any device call: those of qattn_fp8_attention_paged_splitkv_forward (include/qattn_paged.h; QATTN_ERR_INVALID_ARG,
 * QATTN_ERR_UNSUPPORTED_DIM / _FMT, QATTN_ERR_WORKSPACE as there), and QATTN_ERR_INVALID_ARG for: cu_seqlens_q NULL or not 4-byte aligned;
 * total_q < 0; max_seqlen_q < 1; G total_q or the grid Hkv NT num_splits (num_splits = 0: the most the rule can pick) above 2^31 - 1;
 * Hq > 65535 (a grid dimension of the pre-pass and of the merge); a stride of q_strides2 that is negative or no multiple of 8 elements.
 * total_q = 0 (after these checks, before the workspace's: none is needed): QATTN_OK, nothing launched, nothing written.
 * Buffers: include/qattn_buffers.h.
 *
 * The append half of the same step, on packed [total, Hkv, D] tokens under the same cu_seqlens: qattn_paged_kv_cache_append_varlen_fp8,
 * include/qattn_paged_varlen_append.h (the padded qattn_paged_kv_cache_append_fp8 with new_lens leaves the same bytes).
 * Not offered: a per-call table whose batch differs from the scales' and lengths', the contiguous KVCacheFP8.  Sliding windows:
 * qattn_fp8_attention_paged_varlen_window_forward, include/qattn_splitkv_window.h.
 */
#ifndef QATTN_PAGED_VARLEN_H_
#define QATTN_PAGED_VARLEN_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 0 for invalid arguments; num_splits = 0 sizes it for the most splits the rule can pick */
size_t qattn_fp8_attention_paged_varlen_workspace_bytes(int B, int Hq, int Hkv, int total_q, int Skv, int D, int num_splits);

int qattn_paged_varlen_auto_splits(int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int Skv, int D, int num_cus);

int qattn_fp8_attention_paged_varlen_forward(const void* q16, const long long* q_strides2, int in_fmt, const void* k_pool, const void* v_pool,
                                             const int* block_table, long long table_stride, int num_pages, int page_size, int max_pages,
                                             const float* scale_k, const float* scale_v, void* out, float* lse, const int* cu_seqlens_q,
                                             const int* seqused_k, int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int Skv, int D,
                                             int fp8_fmt, int numerics, int is_causal, float sm_scale, int precision, int num_splits, void* q8,
                                             float* scale_q, unsigned char* row_path, float* partial_o, float* partial_lse,
                                             unsigned char* partial_path, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_PAGED_VARLEN_H_ */

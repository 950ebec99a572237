/*
 * qattn_mla_index_prefill.h -- the PREFILL form of the FP8 lightning indexer (include/qattn_mla_index.h): PACKED variable-length index
 * queries, several prompts or prompt chunks of different lengths in one call, each over its own cached prefix (ABI 8 addition; the names are
 * found by symbol, include/qattn.h and QATTN_ABI_VERSION unchanged).  The index-key cache, its append, the block table, the lengths, the
 * clamping and the selection rule are include/qattn_mla_index.h's; the dense entries there are untouched.
 *
 * LAYOUT (the contract).
 *   cu_seqlens_q int32 [B + 1] on the device, cu[0] = 0, non-decreasing: slot b owns the packed rows cu[b] .. cu[b+1] - 1 (n_b of them; every
 *                entry is read clamped to 0 .. total_q, an end below its start as the start).  Rows at or behind cu[B] -- a padded token
 *                bucket -- are NOT read: their kend is 0, their indices all -1, their logits -inf (fill_tail), their q8 / scale_q rows 0.
 *   q16          [total_q, Hi, 128] bf16 / fp16, element strides q_strides2 = {token, head} (NULL: dense), channels dense, rows 16-byte
 *                aligned; quantised in the kernel per (token, head) row by include/qattn_mla_index.h's rule and written to q8
 *                [total_q, Hi, 128] / scale_q [total_q, Hi] (both dense) when the pointers are non-NULL, every row by exactly one work item.
 *   weights      fp32 [total_q, Hi], heads dense, w_stride elements between tokens (0: dense, Hi).
 *   logits       fp32 [total_q, max_seqlen_k], logits_stride elements between rows (0: dense).
 *   kend         int32 [total_q]: written by the score launch for EVERY row.
 *
 * SCORES.  L_b = clamp(seqused_k[b], 0, max_seqlen_k); token i of slot b (packed row r = cu[b] + i) has
 *   kend(r) = L_b (is_causal = 0) or max(L_b - n_b + i + 1, 0) (bottom-right causal: the last token of the slot sees all L_b keys)
 *   logit[r, j] = scale[b] sum_h (w[r, h] scale_q[r, h]) max(sum_c q8[r, h, c] k8[b, j, c], 0)                            j < kend(r)
 * with the arithmetic of qattn_fp8_mla_index_scores OPERATION FOR OPERATION (two MFMAs per head tile in k-step order, 16 fused multiply-adds
 * in accumulator-row order, the sum of the two head tiles, the add of lanes l and l + 32, last the slot's scale): a logit is a pure function
 * of (token, key), so the packed call equals the dense entry on the same tokens bit for bit.  fill_tail as there.
 *
 * WORK SPLIT.  A work item is (slot, tile of QATTN_MLA_INDEX_PREFILL_TOKENS consecutive tokens of the slot, range of
 * QATTN_MLA_INDEX_PREFILL_WG_KEYS keys); the tile is found by a binary search on cu_seqlens_q on the device, the grid carries
 * B + ceil(total_q / TOKENS) tile slots.  Key tiles of QATTN_MLA_INDEX_PREFILL_KEYS keys go through LDS once per workgroup, double-buffered,
 * and are shared by the tile's tokens; a key tile at or behind kend of the tile's last token is neither fetched nor computed.
 *
 * qattn_fp8_mla_index_topk_varlen = the score launch, then qattn_mla_index_select on the packed rows as B = rows, Sq = 1, is_causal = 0 with
 * seqused_k = kend, in slices of at most 65 535 rows: the number of launches is a function of the shapes alone.  workspace:
 * qattn_fp8_mla_index_varlen_workspace_bytes(total_q, max_seqlen_k) bytes, 16-byte aligned: kend (total_q ints, rounded up to 256 bytes), then
 * the logits rows; with the caller's logits only the first section is needed.
 *
 * Nothing is read on the host, nothing allocated: graph-capture safe; a captured call follows the later contents of cu_seqlens_q, seqused_k,
 * the table, q and weights.
 *
 * Argument checks, before any device call, with include/qattn_mla_index.h's codes and limits: total_q, B, topk, max_seqlen_k > 0; B <= 65535;
 * total_q <= 2^31 - 1 - 65535; 1 <= Hi <= 64; topk <= QATTN_MLA_SPARSE_MAX_TOPK; max_seqlen_k <= max_pages page_size and <= 2^30; the pool
 * limits; table_stride >= max_pages; pointers non-NULL (q8, scale_q, logits of the topk entry excepted) and aligned (pool, q16, q8, workspace:
 * 16 bytes; the others: 4); strides non-negative (q: multiples of 8); workspace_bytes large enough; formats: QATTN_ERR_UNSUPPORTED_FMT.
 *
 * (Packed q for the sparse attention over these lists: include/qattn_mla_sparse_prefill.h takes the indices tensor as it is.)
 * Not offered: the selection's first histogram fused into the sweep; per-key index scales.
 */
#ifndef QATTN_MLA_INDEX_PREFILL_H_
#define QATTN_MLA_INDEX_PREFILL_H_

#include "qattn_mla_index.h"

#define QATTN_MLA_INDEX_PREFILL_TOKENS 8        /* tokens of a slot that share a key tile: 4 waves x 2 tokens */
#define QATTN_MLA_INDEX_PREFILL_KEYS 128        /* keys of a key tile in LDS (16 KiB, twice) */
#define QATTN_MLA_INDEX_PREFILL_WG_KEYS 2048    /* keys per workgroup: a multiple of the key tile */

#ifdef __cplusplus
extern "C" {
#endif

/* 0 when a limit above is broken */
size_t qattn_fp8_mla_index_varlen_workspace_bytes(int total_q, int max_seqlen_k);

int qattn_fp8_mla_index_scores_varlen(const void* q16, int in_fmt, const long long* q_strides2, const float* weights, long long w_stride,
                                      const void* pool, const int* block_table, long long table_stride, int num_pages, int page_size,
                                      int max_pages, const float* scale, const int* cu_seqlens_q, const int* seqused_k, int B, int Hi,
                                      int total_q, int max_seqlen_k, int fp8_fmt, int is_causal, float* logits, long long logits_stride,
                                      int fill_tail, int* kend, void* q8, float* scale_q, void* stream);

int qattn_fp8_mla_index_topk_varlen(const void* q16, int in_fmt, const long long* q_strides2, const float* weights, long long w_stride,
                                    const void* pool, const int* block_table, long long table_stride, int num_pages, int page_size,
                                    int max_pages, const float* scale, const int* cu_seqlens_q, const int* seqused_k, int B, int Hi,
                                    int total_q, int max_seqlen_k, int topk, int fp8_fmt, int is_causal, int* indices, float* logits, void* q8,
                                    float* scale_q, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_MLA_INDEX_PREFILL_H_ */

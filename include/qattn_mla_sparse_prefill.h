/*
 * qattn_mla_sparse_prefill.h -- SPARSE (top-k indexed) FP8 multi-head latent attention for PACKED variable-length queries: the prompt's form
 * of qattn_fp8_mla_paged_sparse_forward (include/qattn_mla_sparse.h), over the same ROW-MAJOR paged latent cache (ABI 8 addition; the name is
 * found by symbol, QATTN_ABI_VERSION unchanged).  It takes the list tensor qattn_fp8_mla_index_topk_varlen (include/qattn_mla_index_prefill.h)
 * returns as it is.  Pool, block table, lengths, clamping, scale, the q quantiser and the two-term P are include/qattn_mla_sparse.h's; what
 * differs is below.
 *
 * SHAPES.
 *   q16           [total_q, Hq, 576] in in_fmt, element strides q_strides2 = {token, head} (NULL: dense), multiples of 8, the channels dense:
 *                 a slice of a wider projection goes in as it is.
 *   indices       int32 [total_q, topk], the row stride idx_stride >= 0 in elements (topk for a dense tensor), the last dimension dense;
 *                 1 <= topk <= QATTN_MLA_SPARSE_MAX_TOPK, no multiple of 64.  indices[t][e] is a LOGICAL key position of the token's slot.
 *   cu_seqlens_q  int32 [B + 1] on the device, cu[0] = 0, non-decreasing: slot b owns the tokens cu[b] .. cu[b+1] - 1 (n_b of them, 0
 *                 allowed).  Every entry is clamped into [0, total_q] (and cu[b+1] to >= cu[b]) before it is used.
 *   out           [total_q, Hq, 512] in in_fmt; lse fp32 [Hq, total_q] (the packed convention of qattn_attention_state_merge), may be NULL;
 *                 q8 [total_q, Hq, 576] e4m3 and scale_q fp32 [total_q, Hq], both optional: what the kernel's quantiser made of q.
 *
 * VALIDITY.  include/qattn_mla_sparse.h's rule with, for token t = cu[b] + i, kend = L_b (is_causal = 0) or L_b - n_b + i + 1 (is_causal != 0:
 * bottom-right, the slot's last token sees all L_b keys), L_b = clamp(seqused_k[b], 0, max_pages page_size).  A token with kend <= 0 or
 * without a valid entry is a zero row with LSE -inf.  A token at or behind cu[B] (a padded bucket) reads neither q nor its list: zero rows,
 * LSE -inf, q8 and scale_q zero.
 *
 * WORK SPLIT.  One workgroup of 8 waves per (token, tile of QATTN_MLA_SPARSE_PREFILL_ROWS = 128 of the token's heads): one resolve, one
 * gather and one on-chip transposition per 64-entry group serve all heads of the tile.  No key splits, no combine, NO WORKSPACE; a step of a
 * handful of tokens keeps qattn_fp8_mla_paged_sparse_forward.  The arithmetic of every (row, key) and (row, channel) is that call's: out,
 * lse, q8 and scale_q of slot b equal it on the slot's tokens as [1, Hq, n_b, 576] with num_splits = 1, bit for bit.
 * Nothing is read on the host, nothing allocated: graph-capture safe; a captured call follows the later contents of cu_seqlens_q, indices,
 * table and lengths.
 *
 * Argument checks, before any device call (QATTN_ERR_INVALID_ARG unless noted): B, total_q, topk > 0; 1 <= Hq <= 2^20;
 * topk <= QATTN_MLA_SPARSE_MAX_TOPK; the grid total_q ceil(Hq / 128) <= 2^31 - 1; num_pages, max_pages, page_size > 0 with
 * num_pages page_size <= 2^31 - 1 and max_pages page_size <= 2^31 - 65; table_stride >= max_pages; pointers non-NULL (lse, q8, scale_q
 * excepted) and aligned (pool, q16, out, q8: 16 bytes; table, indices, cu_seqlens_q: 4); strides non-negative (q: multiples of 8);
 * sm_scale > 0 and finite; formats: QATTN_ERR_UNSUPPORTED_FMT.
 *
 * Not offered: key splits or a combine; a 64-row instance for Hq <= 64; physical (pre-resolved) indices; a packed row-cache append; per-token
 * cache scales or a 656-byte row; windows, sinks, soft cap or trees on MLA.
 */
#ifndef QATTN_MLA_SPARSE_PREFILL_H_
#define QATTN_MLA_SPARSE_PREFILL_H_

#include "qattn_mla_sparse.h"

#define QATTN_MLA_SPARSE_PREFILL_ROWS 128   /* heads of a token one workgroup serves */

#ifdef __cplusplus
extern "C" {
#endif

int qattn_fp8_mla_paged_sparse_varlen_forward(const void* q16, int in_fmt, const long long* q_strides2, const void* pool,
                                              const int* block_table, long long table_stride, int num_pages, int page_size, int max_pages,
                                              const float* scale, const int* indices, long long idx_stride, int topk,
                                              const int* cu_seqlens_q, void* out, float* lse, const int* seqused_k, int B, int total_q,
                                              int Hq, int fp8_fmt, int is_causal, float sm_scale, void* q8, float* scale_q, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_MLA_SPARSE_PREFILL_H_ */

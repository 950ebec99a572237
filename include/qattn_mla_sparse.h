/*
 * qattn_mla_sparse.h -- SPARSE (top-k indexed) FP8 multi-head latent attention in its absorbed decode form over a ROW-MAJOR paged latent
 * cache: the decode of DeepSeek-V3.2-style layers, where an indexer picks topk key positions per query token and all heads of the token
 * attend those keys alone (ABI 8 addition; the names are found by symbol, include/qattn.h, include/qattn_mla.h and QATTN_ABI_VERSION
 * unchanged).  Channels, scales, the q quantiser, the two-term P and the combine are include/qattn_mla.h's; what differs is below.
 *
 * LAYOUT (the contract).
 *   pool         fp8 [num_pages, page_size, 576], row-major: key k of page p is the 576 contiguous bytes (nine 64-byte sectors) at
 *                (p page_size + k) 576; channels 0..511 kv_c, 512..575 k_pe.  qattn_mla_row_pool_bytes(num_pages, page_size) bytes, 16-byte
 *                aligned.  page_size is ANY integer >= 1 (a row has no chunk constraint); num_pages page_size <= 2^31 - 1 (a physical row
 *                number is an int) and max_pages page_size <= 2^31 - 65.
 *   block table, lengths, clamping, scale   as include/qattn_mla.h: key j of slot b is row j % page_size of page table[b][j / page_size];
 *                EVERY table entry that is read is clamped into [0, num_pages - 1] before it forms an address.
 *   indices      int32 [B, Sq, topk], element strides idx_strides2 = {batch, position} (NULL: dense), the last dimension dense; topk >= 1
 *                is arbitrary (no multiple of 64), topk <= 2048 x 64.  indices[b][i][e] is a LOGICAL key position of slot b, resolved
 *                through the table on the device.
 *
 * VALIDITY.  L_b = clamp(seqused_k[b], 0, max_pages page_size).  Entry e of (b, i) with value j is VALID iff 0 <= j < kend(b, i), where
 * kend = L_b (is_causal = 0) or L_b - Sq + i + 1 (is_causal != 0).  Everything else -- -1, padding, a position at or behind the limit, the
 * tail of the last 64-entry group -- is invalid: it contributes nothing, and whatever bytes its position or a never-written page holds (NaN
 * included) influence no output bit (the score is masked, the value bytes are zeroed on the chip, and an invalid entry's load is redirected
 * to row 0 of the pool).  Entries count as often as they are listed: the result is softmax attention over the listed valid keys in list
 * order, shared by all Hq heads of (b, i).  A row with no valid entry is a zero row with LSE -inf.
 *
 * qattn_paged_mla_row_cache_append_fp8: the contract of qattn_paged_mla_cache_append_fp8 (include/qattn_mla.h) word for word -- inputs read
 * through their strides, the same quantiser, one 16-byte store per 16 channels of a token, tokens at or beyond the capacity dropped, every
 * table entry read clamped, exactly the bytes of the appended keys change, nothing read on the host -- with the destination
 * (page page_size + j % page_size) 576 + 16 piece.
 *
 * qattn_fp8_mla_paged_sparse_forward: q16 [B, Hq, Sq, 576] as in qattn_fp8_mla_paged_forward.  One workgroup per (slot, position i, 64-row
 * tile of the position's Hq heads, split of the list): Sq ceil(Hq / 64) tiles.  The list of (b, i) is cut into ceil(topk / 64) groups of 64
 * entries; split s owns the groups [s per, (s + 1) per), per = ceil(ceil(topk / 64) / ns), at most 32 of them (2048 entries), so
 * ns >= ceil(topk / 2048) is required.  num_splits = 0: qattn_mla_sparse_auto_splits(B, Hq, Sq, topk, CUs of the device).
 *   partials     one split rounds into out itself.  More write normalised fp32 partials [ns, B, Hq, Sq, 512] and their LSEs [ns, B, Hq, Sq]
 *                -- into partial_o / partial_lse when given, else into the workspace -- and ONE combine launch merges them in the order of
 *                the splits (the formula of include/qattn_mla.h).
 *   workspace    qattn_fp8_mla_paged_sparse_workspace_bytes(B, Hq, Sq, num_splits) with the RESOLVED split count, 16-byte aligned.
 * out [B, Hq, Sq, 512] in the input format, lse [B, Hq, Sq] (may be NULL); split 0 writes q8 / scale_q when the pointers are non-NULL.
 * Nothing is read on the host, nothing allocated: graph-capture safe; a captured call follows the later contents of indices, table, lengths.
 *
 * Argument checks, before any device call (QATTN_ERR_INVALID_ARG unless noted): B, Hq, Sq, T, topk > 0; Hq Sq <= 2^20; topk <= 2048 x 64;
 * the grids B Sq ceil(Hq / 64) ns and B Hq Sq <= 2^31 - 1; num_pages, max_pages, page_size > 0 with the two products above;
 * table_stride >= max_pages; pointers non-NULL (new_lens, lse, q8, scale_q, partial_*, a zero-size workspace excepted) and aligned (pool,
 * q16, ckv16, kpe16, out, q8, workspace: 16 bytes; table, indices: 4); strides non-negative (q, ckv, kpe: multiples of 8);
 * num_splits = 0 or ceil(topk / 2048) <= num_splits <= QATTN_MLA_MAX_SPLITS; sm_scale > 0 and finite; workspace_bytes large enough;
 * formats: QATTN_ERR_UNSUPPORTED_FMT.
 *
 * Not offered: dense attention over the row cache (the indexer: include/qattn_mla_index.h); physical (pre-resolved) indices; (packed variable-length q: include/qattn_mla_sparse_prefill.h);
 * per-token cache scales or a 656-byte row with 16-bit RoPE channels; windows, sinks, soft cap or trees on MLA.
 */
#ifndef QATTN_MLA_SPARSE_H_
#define QATTN_MLA_SPARSE_H_

#include "qattn_mla.h"

#define QATTN_MLA_SPARSE_SPLIT_ENTRIES 2048   /* the most list entries one split resolves */
#define QATTN_MLA_SPARSE_MAX_TOPK (QATTN_MLA_SPARSE_SPLIT_ENTRIES * QATTN_MLA_MAX_SPLITS)

#ifdef __cplusplus
extern "C" {
#endif

/* 0 when a limit above is broken */
size_t qattn_mla_row_pool_bytes(int num_pages, int page_size);

/* the largest count <= QATTN_MLA_MAX_SPLITS whose grid B Sq ceil(Hq / 64) ns the chip holds at once (one workgroup per CU) with >= 128
 * list entries (two groups) per split; never below ceil(topk / 2048), at least 1.  A pure function of its arguments. */
int qattn_mla_sparse_auto_splits(int B, int Hq, int Sq, int topk, int num_cus);

size_t qattn_fp8_mla_paged_sparse_workspace_bytes(int B, int Hq, int Sq, int num_splits);

int qattn_paged_mla_row_cache_append_fp8(const void* ckv16, const void* kpe16, int in_fmt, const long long* ckv_strides2,
                                         const long long* kpe_strides2, void* pool, const float* scale, const int* block_table,
                                         long long table_stride, int* seqlens, const int* new_lens, int advance, int B, int T, int num_pages,
                                         int page_size, int max_pages, int fp8_fmt, void* stream);

int qattn_fp8_mla_paged_sparse_forward(const void* q16, int in_fmt, const long long* q_strides3, const void* pool, const int* block_table,
                                       long long table_stride, int num_pages, int page_size, int max_pages, const float* scale,
                                       const int* indices, const long long* idx_strides2, int topk, void* out, float* lse,
                                       const int* seqused_k, int B, int Hq, int Sq, int fp8_fmt, int is_causal, float sm_scale, int num_splits,
                                       void* q8, float* scale_q, float* partial_o, float* partial_lse, void* workspace, size_t workspace_bytes,
                                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_MLA_SPARSE_H_ */

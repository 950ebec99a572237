/*
 * qattn_mla_index.h -- the FP8 LIGHTNING INDEXER of sparse multi-head latent attention (DeepSeek-V3.2-style layers): the index-key cache and
 * its append, the index scores and the exact top-k selection that produces the `indices` of include/qattn_mla_sparse.h (ABI 8 addition; the
 * names are found by symbol, include/qattn.h and QATTN_ABI_VERSION unchanged).  Block table, lengths and clamping: include/qattn_mla.h.
 *
 * LAYOUT (the contract).
 *   pool         fp8 [num_pages, page_size, 128], row-major: index key k of page p is the 128 contiguous bytes at (p page_size + k) 128, ONE
 *                key vector shared by all index heads.  qattn_mla_index_pool_bytes(num_pages, page_size) bytes, 16-byte aligned; page_size
 *                is ANY integer >= 1; num_pages page_size <= 2^31 - 1 and max_pages page_size <= 2^31 - 65.
 *   scale        fp32 [B], FIXED, one per slot.  (The selection does not depend on it -- a positive factor keeps the order -- only the
 *                logits do.)
 *   q16          [B, Hi, Sq, 128] bf16 / fp16, element strides q_strides3 = {batch, head, position} (NULL: dense), channels dense, rows
 *                16-byte aligned; 1 <= Hi <= QATTN_MLA_INDEX_MAX_HEADS.  Quantised in the kernel per (token, head) row: scale_q =
 *                max(amax / 448, 2^-23), q8 = e4m3(clamp(q (1 / scale_q), +-448)), include/qattn_mla.h's q quantiser; written to q8
 *                [B, Hi, Sq, 128] / scale_q [B, Hi, Sq] when the pointers are non-NULL.
 *   weights      fp32 [B, Sq, Hi], element strides w_strides2 = {batch, position} (NULL: dense), heads dense: the caller's head weights
 *                with the model's d^-1/2 and Hi^-1/2 folded in.
 *
 * SCORES.  L_b = clamp(seqused_k[b], 0, max_seqlen_k); kend(b, i) = L_b (is_causal = 0) or max(L_b - Sq + i + 1, 0) (bottom-right).
 *   logit[b, i, j] = scale[b] sum_h (w[b, i, h] scale_q[b, h, i]) max(sum_c q8[b, h, i, c] k8[b, j, c], 0)        j < kend(b, i)
 * in fp32: the 128-channel products on v_mfma_f32_32x32x64_f8f6f4, the head sum as fused multiply-adds in the order of the accumulator rows
 * (a NaN score counts as 0: the maximum is v_max_f32).  No softmax, no LSE.  logits is fp32 [B, Sq, max_seqlen_k], element strides
 * logits_strides2 = {batch, position} (NULL: dense).  Elements j < kend hold the logits; with fill_tail != 0 every element kend <= j <
 * max_seqlen_k is written -inf, else those elements are left as they are (ALL of them: the tail of the key group that kend cuts too).
 * Keys at or behind kend and never-written pages (NaN bytes included) influence no element below kend: a key is one column of the matrix
 * product.  One workgroup per (b, i, range of QATTN_MLA_INDEX_WG_KEYS keys); a range at or behind kend only fills.  No merge, no splits.
 *
 * SELECTION (the contract).  indices int32 [B, Sq, topk] (dense) receives, per (b, i), the positions of the min(topk, kend) largest logits
 * among j < kend in ASCENDING position order, then -1 up to topk.  A larger logit wins; equal logits are won by the LOWER position; -0.0
 * equals +0.0; a NaN logit ranks as -inf (and ties with it).  kend <= topk gives 0 .. kend - 1 followed by -1s without reading a logit.
 * The output is a pure function of the logits below kend -- no sort, no atomics on the output -- so a replayed graph equals the eager call
 * bit for bit, and the order is the one in which qattn_fp8_mla_paged_sparse_forward reproduces the dense kernel's chunks.  One workgroup per
 * (b, i) row: radix select on order-preserving 32-bit keys (8 bits a pass, LDS histograms; the threshold bin's candidates in LDS when at most
 * QATTN_MLA_INDEX_LDS_CANDIDATES, else further passes over the row), then an ordered stream compaction over positions.  Correct for any
 * distribution, all-equal rows included.  qattn_mla_index_select runs it alone on the caller's logits [B, Sq, N]: L_b = clamp(seqused_k[b], 0, N).
 *
 * qattn_fp8_mla_index_topk = the scores launch and the selection launch.  logits NULL: the rows live in the workspace,
 * qattn_fp8_mla_index_workspace_bytes(B, Sq, max_seqlen_k) bytes, 16-byte aligned (0 bytes are needed with the caller's logits).
 *
 * qattn_paged_mla_index_cache_append_fp8: the contract of qattn_paged_mla_row_cache_append_fp8 (include/qattn_mla_sparse.h) word for word, on
 * k16 [B, T, 128] with 8 pieces of 16 channels per token: a thread owns one piece -- two 16-byte loads, the cache quantiser, ONE 16-byte
 * store at (page page_size + j % page_size) 128 + 16 piece; tokens at or beyond the capacity dropped, every table entry read clamped,
 * exactly the appended bytes change, nothing read on the host.
 *
 * Nothing is read on the host, nothing allocated: graph-capture safe; a captured call follows the later contents of q, weights, table, lengths.
 *
 * Argument checks, before any device call (QATTN_ERR_INVALID_ARG unless noted): B, Sq, T, topk, max_seqlen_k / N > 0; B, Sq <= 65535 (grid
 * axes) and B Sq <= 2^31 - 1; 1 <= Hi <= 64; topk <= QATTN_MLA_SPARSE_MAX_TOPK; max_seqlen_k <= max_pages page_size; N <= 2^30; num_pages,
 * max_pages, page_size > 0 with the two products above; table_stride >= max_pages; pointers non-NULL (new_lens, q8, scale_q, logits, a
 * zero-size workspace excepted) and aligned (pool, q16, k16, q8, workspace: 16 bytes; table, weights, logits, indices: 4); strides
 * non-negative (q, k: multiples of 8); workspace_bytes large enough; formats: QATTN_ERR_UNSUPPORTED_FMT.
 *
 * Not offered: per-key cache scales (DeepSeek's own 132-byte index row: 128 fp8 bytes + an fp32 scale); RoPE or the LayerNorm of the index
 * key (the caller applies them before the append).  (A selection that cuts a row across workgroups -- few rows over many keys: at B Sq = 1
 * one CU selects here -- is include/qattn_mla_index_split.h; packed variable-length q -- a prompt -- is include/qattn_mla_index_prefill.h.)
 */
#ifndef QATTN_MLA_INDEX_H_
#define QATTN_MLA_INDEX_H_

#include "qattn_mla_sparse.h"

#define QATTN_MLA_INDEX_D 128
#define QATTN_MLA_INDEX_MAX_HEADS 64
#ifndef QATTN_MLA_INDEX_WG_KEYS
#define QATTN_MLA_INDEX_WG_KEYS 512            /* keys per workgroup of the score sweep: a multiple of 128 */
#endif
#define QATTN_MLA_INDEX_LDS_CANDIDATES 8192    /* threshold-bin candidates the selection keeps in LDS (32 KiB) */

#ifdef __cplusplus
extern "C" {
#endif

/* 0 when a limit above is broken */
size_t qattn_mla_index_pool_bytes(int num_pages, int page_size);

size_t qattn_fp8_mla_index_workspace_bytes(int B, int Sq, int max_seqlen_k);

int qattn_paged_mla_index_cache_append_fp8(const void* k16, int in_fmt, const long long* k_strides2, void* pool, const float* scale,
                                           const int* block_table, long long table_stride, int* seqlens, const int* new_lens, int advance,
                                           int B, int T, int num_pages, int page_size, int max_pages, int fp8_fmt, void* stream);

int qattn_fp8_mla_index_scores(const void* q16, int in_fmt, const long long* q_strides3, const float* weights, const long long* w_strides2,
                               const void* pool, const int* block_table, long long table_stride, int num_pages, int page_size, int max_pages,
                               const float* scale, const int* seqused_k, int B, int Hi, int Sq, int max_seqlen_k, int fp8_fmt, int is_causal,
                               float* logits, const long long* logits_strides2, int fill_tail, void* q8, float* scale_q, void* stream);

int qattn_mla_index_select(const float* logits, const long long* logits_strides2, const int* seqused_k, int B, int Sq, int N, int topk,
                           int is_causal, int* indices, void* stream);

int qattn_fp8_mla_index_topk(const void* q16, int in_fmt, const long long* q_strides3, const float* weights, const long long* w_strides2,
                             const void* pool, const int* block_table, long long table_stride, int num_pages, int page_size, int max_pages,
                             const float* scale, const int* seqused_k, int B, int Hi, int Sq, int max_seqlen_k, int topk, int fp8_fmt,
                             int is_causal, int* indices, float* logits, void* q8, float* scale_q, void* workspace, size_t workspace_bytes,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_MLA_INDEX_H_ */

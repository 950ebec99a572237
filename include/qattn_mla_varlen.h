/*
 * qattn_mla_varlen.h -- absorbed FP8 multi-head latent attention for PACKED variable-length queries over the one-image paged latent cache:
 * qattn_fp8_mla_paged_forward (include/qattn_mla.h) for a continuous-batching step whose slots carry different numbers of new tokens -- one
 * decode token, a few speculative drafts, a prompt chunk (ABI 8 addition; the names are found by symbol, QATTN_ABI_VERSION unchanged).  Pool,
 * block table, lengths, clamping, scale, the q quantiser, the two-term P and the split plan are include/qattn_mla.h's; what differs is below.
 *
 * SHAPES.
 *   q16           [total_q, Hq, 576] in in_fmt, element strides q_strides2 = {token, head} (NULL: dense), multiples of 8, the channels dense:
 *                 a slice of a wider projection goes in as it is.
 *   cu_seqlens_q  int32 [B + 1] on the device, cu[0] = 0, non-decreasing: slot b owns the tokens cu[b] .. cu[b+1] - 1 (n_b of them, 0
 *                 allowed).  Every entry is clamped into [0, total_q] (and cu[b+1] to >= cu[b]) before it is used.
 *   max_seqlen_q  a host int in 1 .. total_q that bounds n_b.  It is checked and never read back from the device; the grid is sized by
 *                 total_q, which bounds every slot (TILE MAP below).
 *   out           [total_q, Hq, 512] in in_fmt; lse fp32 [Hq, total_q] (the packed convention of qattn_attention_state_merge), may be NULL;
 *                 q8 [total_q, Hq, 576] e4m3 and scale_q fp32 [total_q, Hq], both optional: what the kernel's quantiser made of q.
 *   partial_o, partial_lse  optional fp32 [ns, total_q, Hq, 512] and [ns, total_q, Hq], indexed by the OUTPUT row token Hq + h.
 *
 * RULE.  Token i of slot b attends the keys j < kend = L_b (is_causal = 0) or j <= L_b - n_b + i (is_causal != 0: bottom-right, the slot's
 * last token sees all L_b keys), L_b = clamp(seqused_k[b], 0, Skv).  A row without a key is a zero row with LSE -inf.  A token at or behind
 * cu[B] (a padded bucket) is never read from q: zero rows, LSE -inf, q8 and scale_q zero, zero / -inf partials.
 *
 * WORK SPLIT.  One workgroup of 8 waves per (tile slot, key split); a tile is QATTN_MLA_VARLEN_ROWS = 128 rows of ONE slot, in the slot's
 * head-major row order R = h n_b + i.
 *   TILE MAP    tile_slots = ceil(total_q Hq / 128) + B bounds the tiles of any cu_seqlens_q; slot b's tiles start at tile slot
 *               floor(cu[b] Hq / 128) + b, found on the device by a binary search; a tile slot without rows exits at once.
 *   splits      num_splits is ONE count for all slots; slot b uses include/qattn_mla.h's plan on its own L_b.  num_splits = 0:
 *               qattn_mla_varlen_auto_splits(tile_slots, Skv, CUs of the device).  More than one split: ONE combine launch over the
 *               total_q Hq output rows with qattn_mla.h's formula and order, which also writes lse as [Hq, total_q] and the zero rows
 *               behind cu[B].
 *   workspace   qattn_fp8_mla_paged_varlen_workspace_bytes(total_q, Hq, ns) with the RESOLVED split count (0 for one split), 16-byte aligned.
 * The arithmetic of every (row, key) and (row, channel) is qattn_fp8_mla_paged_forward's, and a 32-row block holds the rows it holds there:
 * out, lse, q8, scale_q and the partials of slot b equal that call on the slot's tokens as [1, Hq, n_b, 576] with Sq = n_b and the same
 * num_splits, bit for bit.
 * Nothing is read on the host, nothing allocated: graph-capture safe; a captured call follows the later contents of cu_seqlens_q, table and
 * lengths.
 *
 * Argument checks, before any device call (QATTN_ERR_INVALID_ARG unless noted): the paging checks of include/qattn_mla.h; B, total_q, Skv > 0;
 * 1 <= Hq <= 2^20; 1 <= max_seqlen_q <= total_q; total_q Hq + 128 (B + 1) <= 2^31 - 1 and tile_slots ns <= 2^31 - 1 (the grids); pointers
 * non-NULL (lse, q8, scale_q, partial_*, a zero-size workspace excepted) and aligned (pool, q16, out, q8, workspace: 16 bytes; table,
 * cu_seqlens_q: 4); strides non-negative multiples of 8; 0 <= num_splits <= QATTN_MLA_MAX_SPLITS; sm_scale > 0 and finite; workspace_bytes
 * large enough; formats: QATTN_ERR_UNSUPPORTED_FMT.  Buffers: include/qattn_buffers.h.
 *
 * Not offered: the row-major cache; a 64-row instance for slots of <= 64 rows (a pure decode step keeps qattn_fp8_mla_paged_forward);
 * per-slot split counts; windows, sinks, soft cap or trees on MLA; per-token cache scales.
 */
#ifndef QATTN_MLA_VARLEN_H_
#define QATTN_MLA_VARLEN_H_

#include "qattn_mla.h"

#define QATTN_MLA_VARLEN_ROWS 128   /* rows of a slot one workgroup serves */

#ifdef __cplusplus
extern "C" {
#endif

/* the largest count <= QATTN_MLA_MAX_SPLITS with tile_slots ns <= num_cus and >= 1024 keys of Skv per split; at least 1.  A pure function of
 * its arguments; tile_slots = ceil(total_q Hq / 128) + B. */
int qattn_mla_varlen_auto_splits(int tile_slots, int Skv, int num_cus);

size_t qattn_fp8_mla_paged_varlen_workspace_bytes(int total_q, int Hq, int num_splits);

int qattn_fp8_mla_paged_varlen_forward(const void* q16, int in_fmt, const long long* q_strides2, const void* pool, const int* block_table,
                                       long long table_stride, int num_pages, int page_size, int max_pages, const float* scale,
                                       const int* cu_seqlens_q, int max_seqlen_q, void* out, float* lse, const int* seqused_k, int B,
                                       int total_q, int Hq, int Skv, int fp8_fmt, int is_causal, float sm_scale, int num_splits, void* q8,
                                       float* scale_q, float* partial_o, float* partial_lse, void* workspace, size_t workspace_bytes,
                                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_MLA_VARLEN_H_ */

/*
 * qattn_paged_varlen_tree_window.h -- the verify pass of tree-shaped speculative decoding (include/qattn_paged_varlen_tree.h) on WINDOWED
 * layers and on layers with learned SINKS (include/qattn_splitkv_window.h, include/qattn_sinks.h): gpt-oss, Mistral, Gemma-2/3, Phi-3.
 * One addition, found by symbol; include/qattn.h and QATTN_ABI_VERSION unchanged.
 *
 * qattn_fp8_attention_paged_varlen_tree_window_forward
 *
 * The arguments, outputs, buffers and workspace (qattn_fp8_attention_paged_varlen_workspace_bytes) of
 * qattn_fp8_attention_paged_varlen_tree_forward, with `int window_left, int window_right, const float* sinks` after `tree_mask`.  sinks:
 * fp32 [Hq] on the device, 4-byte aligned, as qattn_fp8_attention_paged_varlen_sink_forward takes them -- or NULL: no sinks, the sink-free
 * kernels.  num_splits = 0: the rule of qattn_paged_varlen_window_auto_splits(..., window_left, num_cus) -- the driver evaluates it in
 * the form that function is defined by, qattn_paged_varlen_auto_splits on skv_window_keys(Skv, max_seqlen_q, window_left) keys: the same
 * number for every argument the entry accepts.
 *
 * THE RULE.  Slot b has Sq_b queries and L_b keys (both clamped as include/qattn_paged_varlen.h clamps them); delta = L_b - Sq_b.  w_p is
 * the word of the token at position p, tree_mask[cu[b] + p], read as unsigned.
 *   For a slot with 1 <= Sq_b <= 64:  depth_p = popcount(w_p & (2^p - 1)) -- the set bits BELOW p; the self bit does not count.
 *   For a slot with Sq_b > 64:        depth_p = p.  Its words are not read, as in the tree entry.
 * The query at position p sits at sequence position delta + depth_p.  It attends key j iff all of
 *   1. the tree entry's rule: j <= min(L_b - 1, p + delta), and for j >= max(delta, 0) bit j - delta of w_p is set (Sq_b <= 64);
 *   2. for window_left >= 0 and a committed key j < delta:  j >= delta + depth_p - window_left;
 *   3. draft keys j >= delta get no window test.
 * Accepted windows: window_right == 0 and window_left == -1 or window_left >= 63; anything else is QATTN_ERR_INVALID_ARG.  At
 * window_left >= 63 every ancestor of a draft token lies inside its window -- two tokens of a slot differ by at most 63 in depth --, so
 * rule 3 costs nothing: delta + depth_p - window_left <= delta, and one comparison serves committed and draft keys.  window_right != 0
 * has no meaning under a causal tree.  A slot with Sq_b > 64 is a prefill chunk: no tree, depth = position, and the window test runs on
 * all of its keys -- it is the window entry's slot, bit for bit.
 * A row without a key is a zero row with LSE -inf; with sinks its LSE is sink_h.  With sinks, L = log(exp(sink_h) + sum_j exp(x_j)) over
 * the attended keys j, exactly as include/qattn_sinks.h defines it: -inf is no sink, +inf and NaN poison their head alone, and the sink
 * kernels never take the byte sweep.
 *
 * IDENTITIES, bit for bit in out, lse, row_path and the partials, under both precisions, every num_splits and page size:
 *   1. window_left = -1, no sinks: qattn_fp8_attention_paged_varlen_tree_forward.
 *   2. a chain (w_p = bits 0 .. p), no sinks: qattn_fp8_attention_paged_varlen_window_forward under (window_left, 0); with sinks:
 *      qattn_fp8_attention_paged_varlen_sink_forward under (window_left, 0).
 *   3. with sinks and num_splits > 1 the partials are the sink-free call's, and qattn_attention_state_merge_sink of them gives out, lse.
 *   4. every slot's rows are those of the call on that slot alone: mask, depth and window are functions of the token and its slot.
 *
 * THE KERNELS are two more compilations of csrc/qattn_splitkv_body.h, the tree over the packed paged window text.  The split plan is the
 * window entry's -- lo_i = max(delta - window_left, 0): position 0 has depth 0 --, a function of (L_b, Sq_b, window_left, num_splits)
 * alone.  Where the window text takes a row's position for the window's lower edge, this text takes the row's depth: a tile's first key
 * klo comes from the least depth of its valid rows, the chunk range of the lower-edge token test from the greatest.  Every wave reduces
 * both from the tile's words (two loads per lane, lane shuffles: no LDS beside the ring, no barrier) before the plan's key count and the
 * precision selection, so that a chain reproduces the window kernel's work items exactly.  A word is read only at a token of a slot with
 * 1 <= Sq_b <= 64, inside [0, total_q).  A chunk takes the token branch iff it holds key L_b, crosses the causal edge or the lower window
 * edge of some valid row, or holds a draft key.  The V bytes below lo_i in its chunk are zeroed in LDS and the pages walked as in the window
 * text; the sink epilogue and the merge chain are the sink text's.
 *
 * Everything is read on the device: no host synchronisation, graph-capture safe; a captured call follows the later contents of
 * tree_mask, cu_seqlens_q, seqused_k, the table and sinks.
 *
 * Argument checks, before any device call: QATTN_ERR_INVALID_ARG for tree_mask NULL or not 8-byte aligned, a window outside the accepted
 * values, sinks not 4-byte aligned; then those of qattn_fp8_attention_paged_varlen_window_forward.
 *
 * The rotary embedding of the drafts at the tree's positions, delta + depth_p -- the packed append and q's packed rotation with a positions
 * tensor -- is include/qattn_paged_varlen_rope_pos.h.
 *
 * Not offered: window_left < 63 under a tree (an ancestor could fall out of the window: the draft keys would need the window test by
 * depth); trees above 64 tokens per slot; a partial rotary_dim, multi-axis (M-RoPE) positions and positions in the padded and the
 * contiguous appends (include/qattn_paged_varlen_rope_pos.h); the contiguous KVCacheFP8.
 */
#ifndef QATTN_PAGED_VARLEN_TREE_WINDOW_H_
#define QATTN_PAGED_VARLEN_TREE_WINDOW_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

int qattn_fp8_attention_paged_varlen_tree_window_forward(const void* q16, const long long* q_strides2, int in_fmt, const void* k_pool,
                                                         const void* v_pool, const int* block_table, long long table_stride, int num_pages,
                                                         int page_size, int max_pages, const float* scale_k, const float* scale_v,
                                                         void* out, float* lse, const int* cu_seqlens_q, const int* seqused_k, int B, int Hq,
                                                         int Hkv, int total_q, int max_seqlen_q, int Skv, int D, int fp8_fmt, int numerics,
                                                         const unsigned long long* tree_mask, int window_left, int window_right,
                                                         const float* sinks, float sm_scale, int precision, int num_splits, void* q8,
                                                         float* scale_q, unsigned char* row_path, float* partial_o, float* partial_lse,
                                                         unsigned char* partial_path, void* workspace, size_t workspace_bytes,
                                                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_PAGED_VARLEN_TREE_WINDOW_H_ */

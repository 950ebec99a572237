/*
 * qattn_paged_varlen_tree.h -- tree-shaped speculative decoding on the paged FP8 K/V cache of include/qattn_paged.h: the verify pass under a
 * draft TREE per sequence slot, and the compaction of the accepted root-to-leaf path into the contiguous tail of the slot's keys (ABI 8
 * additions; the names are found by symbol, include/qattn.h and QATTN_ABI_VERSION unchanged).
 *
 * The step: append the drafts (qattn_paged_kv_cache_append_varlen_fp8) -> tree attend (here) -> verify (the caller) -> compact (here).
 *
 * 1. qattn_fp8_attention_paged_varlen_tree_forward
 *
 * The arguments, outputs, buffers, workspace (qattn_fp8_attention_paged_varlen_workspace_bytes) and the num_splits = 0 rule
 * (qattn_paged_varlen_auto_splits) of qattn_fp8_attention_paged_varlen_forward (include/qattn_paged_varlen.h) with is_causal = 1, and
 * `tree_mask` in is_causal's place: one 64-bit word per packed token, [total_q] on the device, 8-byte aligned, read as unsigned.
 *
 * THE MASK RULE.  Slot b has Sq_b queries and L_b keys (both clamped as include/qattn_paged_varlen.h clamps them), delta = L_b - Sq_b.  Its
 * draft tokens are its LAST Sq_b keys: they have been appended, as for the causal call.  Position p attends key j iff
 *     j <= min(L_b - 1, p + delta)                                    -- the causal rule -- and,
 *     for j >= max(delta, 0): bit j - delta of tree_mask[cu[b] + p] is set.
 * Bits above p are ignored (the causal rule excludes those keys); the self bit p is honoured as given; committed keys (j < delta) are
 * always attended.  A slot with Sq_b > 64 (a prefill chunk of a mixed step) ignores its words and is plain causal.  A row whose mask
 * leaves no key is a zero row with LSE -inf.  With grouped queries the word belongs to the TOKEN: packed row r of a kv head's group is
 * head r / Sq_b at position r % Sq_b, and all Hq / Hkv heads of a token read the same word.  Padding rows read nothing; a word is read
 * only at a token of a slot with 1 <= Sq_b <= 64, that is inside [0, total_q).
 *
 * The split plan, the trip range of every workgroup, the chunks fetched, the table entries read and the merge chain are the causal
 * call's: the words are tested token by token in the chunks that hold a key >= delta -- at most two per slot -- and nowhere else.
 * A chain (word p = bits 0 .. p) therefore gives the outputs of qattn_fp8_attention_paged_varlen_forward(is_causal = 1) bit for bit:
 * out, lse, row_path and the partials.  Both precisions as there: FAST takes the byte sweep for tiles with >= 1024 keys.
 *
 * Everything is read on the device: no host synchronisation, graph-capture safe; a captured call follows the later contents of
 * tree_mask, cu_seqlens_q, seqused_k and the table.
 *
 * Argument checks, before any device call: QATTN_ERR_INVALID_ARG for tree_mask NULL or not 8-byte aligned, then those of
 * qattn_fp8_attention_paged_varlen_forward.
 *
 * 2. qattn_paged_kv_cache_compact_fp8
 *
 * cu_seqlens int32 [B + 1] is the verify step's; accept_index int32 [total], packed like the tokens: slot b's entries cu[b] ..
 * cu[b] + n_b - 1 are in-slot draft indices; accept_lens int32 [B].  All on the device, 4-byte aligned.
 *
 * THE RULE.  With start_b, Sq_b from cu_seqlens (clamped as the append clamps them) and L_b = clamp(seqlens[b], 0, capacity), capacity =
 * max_pages page_size, a slot is compactable iff 1 <= Sq_b <= 64 and L_b >= Sq_b.  Then base = L_b - Sq_b, n_b = clamp(accept_lens[b], 0,
 * Sq_b), idx_i = clamp(accept_index[start_b + i], 0, Sq_b - 1), and for i < n_b key base + i receives the K and V bytes key base + idx_i
 * held BEFORE the call: all reads happen before all writes, so any index list is well defined.  Then seqlens[b] = base + n_b.  Other
 * slots keep their bytes and their seqlens.  Exactly the bytes of the keys base + i, i < n_b, may change; every other byte of both pools
 * keeps its value.  The scales are fixed per (slot, head): the bytes move unchanged.  Two slots whose draft regions share a page:
 * undefined, as for the append.
 *
 * Launches, both on `stream`, nothing read on the host (no host synchronisation, no allocation, graph-capture safe):
 *   move     grid (B Hkv, 2) -- y: K, V -- of 256 threads.  A workgroup stages the at most two 64-key chunks that hold the draft region
 *            (they may lie in two pages; table entries are clamped into the pool as the append clamps them) in LDS, and after a barrier
 *            stores the destination keys: K as the 16-byte KFRAG pieces of a key, V as bytes, or as whole words where all four keys of a
 *            VFRAG word are destinations.  One writer per piece, word or byte.
 *   lengths  one thread per slot writes seqlens[b] = base + n_b for the compactable slots.  Stream order puts it behind the move, so
 *            that no workgroup reads a rewritten length.
 * No address leaves the tensors: cu_seqlens is read at [b] and [b + 1], seqlens and accept_lens at [b], accept_index at start_b + i for
 * i < n_b <= Sq_b, that is inside [0, total); the table entries read are those of the chunks floor(base / 64) and floor((L_b - 1) / 64),
 * below max_pages.
 *
 * Argument checks, before any device call: QATTN_ERR_INVALID_ARG for a NULL or misaligned pointer (pools 16 bytes, the int tensors 4),
 * num_pages, max_pages, Hkv, B <= 0, total < 0, page_size no positive multiple of 64, table_stride < max_pages, a capacity or a grid
 * B Hkv above 2^31 - 1; QATTN_ERR_UNSUPPORTED_DIM for D not in {64, 128, 256}.  total = 0 (after these checks): QATTN_OK, nothing launched.
 *
 * Offered elsewhere, not by these two entries: sliding windows under a tree mask and sinks folded into the tree unit -- both are
 * qattn_fp8_attention_paged_varlen_tree_window_forward (include/qattn_paged_varlen_tree_window.h), for windows (left, 0) with left = -1
 * or left >= 63; a positions tensor for the fused RoPE append and for q's packed rotation (a tree node's position is base + depth, not
 * base + index) -- include/qattn_paged_varlen_rope_pos.h.
 * Not offered: a window with left < 63 under a tree; trees above 64 tokens per slot; the contiguous KVCacheFP8; masks for the dense,
 * 16-bit and block-sparse entries.
 */
#ifndef QATTN_PAGED_VARLEN_TREE_H_
#define QATTN_PAGED_VARLEN_TREE_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

int qattn_fp8_attention_paged_varlen_tree_forward(const void* q16, const long long* q_strides2, int in_fmt, const void* k_pool,
                                                  const void* v_pool, const int* block_table, long long table_stride, int num_pages,
                                                  int page_size, int max_pages, const float* scale_k, const float* scale_v, void* out,
                                                  float* lse, const int* cu_seqlens_q, const int* seqused_k, int B, int Hq, int Hkv,
                                                  int total_q, int max_seqlen_q, int Skv, int D, int fp8_fmt, int numerics,
                                                  const unsigned long long* tree_mask, float sm_scale, int precision, int num_splits,
                                                  void* q8, float* scale_q, unsigned char* row_path, float* partial_o, float* partial_lse,
                                                  unsigned char* partial_path, void* workspace, size_t workspace_bytes, void* stream);

int qattn_paged_kv_cache_compact_fp8(void* k_pool, void* v_pool, const int* block_table, long long table_stride, int* seqlens,
                                     const int* cu_seqlens, const int* accept_index, const int* accept_lens, int B, int Hkv, int total,
                                     int num_pages, int page_size, int max_pages, int D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_PAGED_VARLEN_TREE_H_ */

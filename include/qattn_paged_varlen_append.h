/*
 * qattn_paged_varlen_append.h -- appending PACKED variable-length tokens to the paged FP8 K/V cache of include/qattn_paged.h: the append
 * half of a serving step that mixes chunked prefill, decode and idle slots, in the call shape of its attention half,
 * include/qattn_paged_varlen.h (ABI 8 addition; the name is found by symbol, include/qattn.h and QATTN_ABI_VERSION unchanged).
 *
 * qattn_paged_kv_cache_append_fp8 takes k16 / v16 [B, Hkv, T, D]: every sequence slot owns T rows, of which new_lens[b] are used, so a
 * step with one 512-token chunk and 31 decodes hands over 32 x 512 rows for 543 tokens.  Here the tokens are packed as the QKV projection
 * leaves them: sequence i owns the rows
 *     start_i = clamp(cu_seqlens[i], 0, total)  ..  end_i = clamp(cu_seqlens[i + 1], start_i, total)
 * of k16 / v16 [total, Hkv, D] (the clamps of include/qattn_paged_varlen.h: cu_seqlens is the tensor the attention takes as
 * cu_seqlens_q), n_i = end_i - start_i of them (0: an idle slot).  With p_i = clamp(seqlens[i], 0, capacity), capacity = max_pages
 * page_size, token start_i + t becomes key p_i + t of slot i; tokens at or beyond the capacity are dropped; seqlens[i] becomes
 * min(p_i + n_i, capacity) unless advance = 0.  Pools, block table, scales, page rules, entries read and clamped: include/qattn_paged.h,
 * unchanged.
 *
 * LAYOUTS (the contract).
 *   k16, v16    [total, Hkv, D] 16-bit through the element strides {token, head} of k_strides2 / v_strides2; head_dim innermost and dense;
 *               both strides non-negative multiples of 8 elements, the base 16-byte aligned (16-byte row loads).  The K and V slices of a
 *               packed [total, (Hq + 2 Hkv) D] projection go in as they are.  Exactly `total` rows are addressable.
 *   cu_seqlens  int32 [B + 1] on the device.       seqlens  int32 [B] on the device.
 *   pools, block_table, scale_k / scale_v [B, Hkv]: include/qattn_paged.h.
 *
 * THE RULE.  From the same starting state the call leaves k_pool, v_pool and seqlens byte for byte as
 *     qattn_paged_kv_cache_append_fp8(pad(k16), pad(v16), ..., new_lens = n, T = max_i n_i)
 * leaves them, pad(x)[i][h][t] = x[start_i + t][h] for t < n_i: the quantiser's bytes, saturation, NaN and +-inf handling, the store
 * schemes of a wholly and of a partly covered chunk (one writer per word or byte, nothing read back), the table entries read and
 * clamped are that entry's, because the kernel is that entry's body (csrc/qattn_kvcache_append_body.h) compiled a third time.  Exactly the
 * bytes of the appended keys change.  Two slots that append into the same page in one call have two writers: undefined.
 *
 * Launches, both on `stream`, nothing read on the host (no host synchronisation, no allocation, graph-capture safe; a captured call
 * follows the later contents of cu_seqlens, seqlens and the block table):
 *   append   kv_paged_varlen_append_kernel: grid (Hkv NS, 2) -- y: K, V -- of 256 threads, NS = 2 B + floor(total / 64) chunk slots per kv
 *            head.  Slot j belongs to the largest sequence i with base_i = 2 i + floor(start_i / 64) <= j, as its chunk j - base_i counted
 *            from the 64-key chunk that holds key p_i.  base is non-decreasing and base_{i+1} - base_i >= floor(n_i / 64) + 2, at least the
 *            number of chunks n_i consecutive keys can touch, so every touched chunk has exactly one slot; base_B <= NS.  The sequence is
 *            found by a binary search over cu_seqlens (workgroup-uniform, ceil(log2 B) + 2 dword loads); a slot that is no chunk of its
 *            sequence exits before it touches other memory (at most 2 B + total / 64 - the touched chunks, per kv head).
 *   advance  advance != 0: one thread per slot writes seqlens[i] = min(p_i + n_i, capacity) (every slot, idle ones included: a value
 *            outside [0, capacity] is clamped, as qattn_paged_kv_cache_append_fp8 does).  Stream order puts it behind the append.
 *
 * No address leaves the tensors, whatever cu_seqlens, seqlens and the block table hold: the search reads cu_seqlens[1 .. B - 1], then
 * [i] and [i + 1] for an i in [0, B - 1]; seqlens is read at that i; a workgroup loads the rows start_i + (k - p_i) for keys k in
 * [p_i, end) of its chunk, end = min(p_i + n_i, capacity), that is rows in [start_i, start_i + n_i) = [start_i, end_i) within [0, total); it
 * reads the table entry floor(k0 / page_size) < max_pages of row i for a chunk start k0 < end <= capacity and clamps it into
 * [0, num_pages - 1] before it forms the chunk's address.  A cu_seqlens that is not non-decreasing can give a sequence's chunk two
 * slots or none: unspecified pool contents in the slots concerned, and nothing worse.  Rows behind cu_seqlens[B] (a padded token
 * bucket) are not read.
 *
 * Argument checks, before any device call: those of qattn_paged_kv_cache_append_fp8 (include/qattn_paged.h, include/qattn_kvcache.h;
 * QATTN_ERR_INVALID_ARG, QATTN_ERR_UNSUPPORTED_DIM / _FMT as there) with total in T's place, and QATTN_ERR_INVALID_ARG for: cu_seqlens
 * NULL or not 4-byte aligned; total < 0; the grid Hkv NS above 2^31 - 1.  total = 0 (after these checks): QATTN_OK, nothing launched,
 * nothing written.  Buffers: as listed above; no workspace.
 *
 * Rotary embedding of K inside the append: the sibling qattn_paged_kv_cache_append_varlen_rope_fp8 (include/qattn_paged_varlen_rope.h), this
 * entry's body compiled once more with the rotation between its load and its quantiser.
 * Not offered: a per-token slot_mapping form, the contiguous KVCacheFP8, page allocation.
 */
#ifndef QATTN_PAGED_VARLEN_APPEND_H_
#define QATTN_PAGED_VARLEN_APPEND_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

int qattn_paged_kv_cache_append_varlen_fp8(const void* k16, const void* v16, int in_fmt, const long long* k_strides2,
                                           const long long* v_strides2, /* {token, head}, elements */
                                           void* k_pool, void* v_pool, const float* scale_k, const float* scale_v, const int* block_table,
                                           long long table_stride, int* seqlens, const int* cu_seqlens, int advance, int B, int Hkv, int total,
                                           int num_pages, int page_size, int max_pages, int D, int fp8_fmt, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_PAGED_VARLEN_APPEND_H_ */

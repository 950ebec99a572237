/*
 * qattn_paged_varlen_rope_pos.h -- the rotary embedding of include/qattn_paged_varlen_rope.h at the CALLER's positions: one 64-bit position
 * per packed token (vLLM's `positions`) in the place of "a key's index in its sequence is its position".  Two additions, found by symbol;
 * include/qattn.h and QATTN_ABI_VERSION unchanged.
 *
 * Why: under tree-shaped speculative decoding (include/qattn_paged_varlen_tree.h, include/qattn_paged_varlen_tree_window.h) a draft token's
 * position is base + DEPTH, so two siblings share a position while their keys are stored next to each other.  With these entries the step
 * is   rotate q and append K at the tree's positions -> tree attend -> verify -> compact   with nothing read on the host.
 *
 * 1. qattn_paged_kv_cache_append_varlen_rope_pos_fp8
 *
 * The arguments of qattn_paged_kv_cache_append_varlen_rope_fp8, and `const long long* positions` before `stream`: [total] on the device,
 * 8-byte aligned.  Token t of the call (0 <= t < total) is rotated with table row clamp(positions[t], 0, T - 1) -- the clamp in 64 bits,
 * so that no value leaves the tables.  WHERE a key is stored does not change: token start_b + t becomes key p_b + t of slot b, exactly as
 * the packed append stores it.  positions is read only at tokens that are appended; rows behind cu[B] are not read.
 * THE RULE.  Pools and seqlens end, byte for byte, as "apply_rope_eager on K at those positions, then
 * qattn_paged_kv_cache_append_varlen_fp8" leaves them: the rotated value is rounded to the input dtype before the quantiser, non-finite
 * values are handled as the composition handles them, and exactly the bytes of the appended keys change.  With
 * positions[start_b + t] = p_b + t the bits are those of qattn_paged_kv_cache_append_varlen_rope_fp8.
 * The kernel is a fifth compilation of csrc/qattn_kvcache_append_body.h (QATTN_KVA_POS on top of QATTN_KVA_ROPE): one line differs.
 *
 * 2. qattn_rope_packed_positions
 *
 * x16 [total, H, D] bf16 / fp16 read through x_strides2 (elements between tokens and heads: non-negative multiples of 8, the base 16-byte
 * aligned: the q slice of a packed projection goes in as it is), out16 dense [total, H, D], 16-byte aligned.  Row t is rotated with table
 * row clamp(positions[t], 0, T - 1): bit for bit apply_rope_eager at those positions, and with the positions of qattn_rope_paged_varlen
 * its bits.  Every row of [0, total) is read and written: there is no cu_seqlens here.  One launch, one (row, head, 16-channel pair of
 * pieces) per thread, no slot search.
 *
 * Tables: cos / sin fp32 [T, D/2], both bases 16-byte aligned, table_row_stride floats between rows (a non-negative multiple of 4), T >= 1;
 * interleaved 0 pairs (i, i + D/2), 1 pairs (2i, 2i + 1).  Both entries share csrc/qattn_rope_dev.h with the entries of
 * include/qattn_paged_varlen_rope.h.  Everything is read on the device: no host synchronisation, no allocation, graph-capture safe.
 *
 * Argument checks, before any device call: those of the siblings, then QATTN_ERR_INVALID_ARG for positions NULL or not 8-byte aligned.
 * total = 0 (after the checks): QATTN_OK, nothing launched.
 *
 * Not offered: a partial rotary_dim; multi-axis (M-RoPE) positions; positions in the padded and the contiguous appends.
 */
#ifndef QATTN_PAGED_VARLEN_ROPE_POS_H_
#define QATTN_PAGED_VARLEN_ROPE_POS_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

int qattn_paged_kv_cache_append_varlen_rope_pos_fp8(const void* k16, const void* v16, int in_fmt, const long long* k_strides2,
                                                    const long long* v_strides2, void* k_pool, void* v_pool, const float* scale_k,
                                                    const float* scale_v, const int* block_table, long long table_stride, int* seqlens,
                                                    const int* cu_seqlens, int advance, int B, int Hkv, int total, int num_pages,
                                                    int page_size, int max_pages, int D, int fp8_fmt, const float* cos, const float* sin,
                                                    long long table_row_stride, int T, int interleaved, const long long* positions,
                                                    void* stream);

int qattn_rope_packed_positions(const void* x16, int in_fmt, const long long* x_strides2, void* out16, const long long* positions, int H,
                                int total, int D, const float* cos, const float* sin, long long table_row_stride, int T, int interleaved,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_PAGED_VARLEN_ROPE_POS_H_ */

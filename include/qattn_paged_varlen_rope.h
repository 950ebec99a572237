/*
 * qattn_paged_varlen_rope.h -- the rotary position embedding (RoPE) of a serving step on the paged FP8 K/V cache: K rotated INSIDE the
 * packed append of include/qattn_paged_varlen_append.h, and the packed rotation q needs at the same positions (ABI 8 addition; the names
 * are found by symbol, include/qattn.h and QATTN_ABI_VERSION unchanged).
 *
 * Every model that decodes on this path rotates q and k by position before attention.  The append knows each key's position -- token
 * start_i + t of slot i becomes key p_i + t, p_i = clamp(seqlens[i], 0, capacity) -- so the caller hands over the UNROTATED K slice of the
 * projection and one cos / sin table pair; the kernel rotates the values it already holds in registers, and the rotated 16-bit K never
 * exists in memory.  No positions tensor, nothing read on the host.
 *
 * THE ROTATION is include/qattn_rope.h's, operation for operation: for a pair (a, b) with table entry (c, s),
 *     y_first = round16(fl(a c) - fl(b s)),   y_second = round16(fl(b c) + fl(a s))
 * -- three separately rounded fp32 operations, no fused multiply-add, one rounding to the input dtype.  interleaved = 0 pairs
 * (i, i + D/2), interleaved = 1 pairs (2i, 2i + 1).  Only the full head dim is rotated.
 *
 * TABLES.  cos, sin: fp32 [T, D/2], ONE pair for every slot, both through the row stride table_row_stride (floats; a non-negative
 * multiple of 4), both bases 16-byte aligned (rows are read as float4).  A slice cos[:, :D/2] of a wider table is read in place.  Exactly
 * T rows of D/2 floats are addressable.  T >= 1; the row read for position j is min(j, T - 1), so no address leaves the tables whatever
 * seqlens holds (a caller keeps T >= capacity; the Python entry requires it).
 *
 * ---- qattn_paged_kv_cache_append_varlen_rope_fp8 -------------------------------------------------------------------------------------
 * The arguments of qattn_paged_kv_cache_append_varlen_fp8, then cos, sin, table_row_stride, T, interleaved.  Key p_i + t of slot i is
 * rotated with table row min(p_i + t, T - 1): a key's index in its sequence is its position.  V is not rotated.
 *
 * THE RULE.  From the same starting state the call leaves k_pool, v_pool and seqlens byte for byte as
 *     k_rot[start_i + t] = rope(k16[start_i + t], row min(p_i + t, T - 1));   qattn_paged_kv_cache_append_varlen_fp8(k_rot, v16, ...)
 * leaves them.  So: the rotated value is rounded to the input dtype before the quantiser sees it; the quantiser's non-finite test is
 * taken on the ROTATED vector (an inf input makes NaN through inf x 0, an fp16 product can overflow, exactly as in the composition);
 * saturation, NaN bytes, the store schemes of whole and partial chunks, the table entries read and clamped are the packed append's,
 * because the kernel is its body (csrc/qattn_kvcache_append_body.h) compiled a fourth time, switch QATTN_KVA_ROPE on.  Exactly the bytes
 * of the appended keys change.
 *
 * Launches, both on `stream`; no workspace, nothing read on the host, graph-capture safe (a captured call follows the later contents of
 * cu_seqlens, seqlens, the block table and the tables):
 *   append   kv_paged_varlen_rope_append_kernel: the packed append's grid (Hkv NS, 2) of 256 threads and its slot search.  The V half
 *            (y = 1) is the packed append's.  The K half (y = 0) holds work units instead of single vectors: the 16-byte pieces dvh and
 *            dvh + D/16 of one chunk row in one thread, so that no value crosses lanes; 64 D/16 units per chunk, 1 / 2 / 4 per thread at
 *            D = 64 / 128 / 256, in the registers the plain mapping uses.  A unit of chunk row r in [lo, hi) reads two float4 of cos and
 *            two of sin from table row min(key0 + r, T - 1) -- the float4 2 dvh, 2 dvh + 1 (pairs (i, i + D/2)) or dvh, dvh + D/16
 *            (interleaved) -- rotates, and quantises each piece into the LDS image at the offsets of the plain mapping.  Rows outside
 *            [lo, hi) stay zero vectors and read no table.  Behind the barrier: shared text.
 *   advance  kv_varlen_advance_kernel, as it is.
 *
 * Argument checks, before any device call: those of qattn_paged_kv_cache_append_varlen_fp8, then QATTN_ERR_INVALID_ARG for: cos or sin
 * NULL or not 16-byte aligned; table_row_stride negative or no multiple of 4; T < 1; interleaved outside {0, 1}.  total = 0 (after these
 * checks): QATTN_OK, nothing launched, nothing written.
 *
 * ---- qattn_rope_paged_varlen ---------------------------------------------------------------------------------------------------------
 * x16 [total, H, D] 16-bit through the element strides {token, head} of x_strides2 (the packed append's stride rules: head_dim dense,
 * both strides non-negative multiples of 8 elements, base 16-byte aligned): the q slice of the projection goes in as it is.  out16:
 * dense [total, H, D] in the same dtype, 16-byte aligned, not overlapping x16.  Row start_i + t is rotated with table row
 *     min(max(base_i, 0) + t, T - 1),   base_i = clamp(seqlens[i], 0, capacity) - (appended ? n_i : 0)
 * appended = 0: a call made BEFORE the step's append (the query gets the position of the key the same token becomes); appended = 1: a
 * call made AFTER an advancing append.  Rows behind cu_seqlens[B] are neither read nor written.  The result is bit for bit the rotation
 * above at these positions.  One launch (rope_paged_varlen_kernel: one work unit per thread; every row finds its sequence by a binary
 * search on cu_seqlens, ceil(log2 B) + 2 dword loads, because a block of rows can hold several sequences); no workspace, nothing read on
 * the host, graph-capture safe.  QATTN_ERR_INVALID_ARG for: a NULL pointer; cu_seqlens or seqlens not 4-byte aligned; x16 or out16 not
 * 16-byte aligned; a stride that is negative or no multiple of 8; B, H or capacity < 1, capacity above 2^31 - 65, total < 0; appended
 * outside {0, 1}; the table rules above; more than 2^31 - 1 blocks of 256 units.  QATTN_ERR_UNSUPPORTED_DIM / _FMT as the append.
 * total = 0 (after these checks): QATTN_OK, nothing launched.
 *
 * A positions tensor (vLLM's `positions`; a tree node of a speculative step sits at base + depth) is taken by the siblings of
 * include/qattn_paged_varlen_rope_pos.h, not by these entries.
 * Not offered: RoPE fused into the q pre-pass of the paged attention (the pre-pass is shared by every split-KV entry); per-slot position
 * offsets; a [B, T, D/2] table per slot; a partial rotary_dim; multi-axis (M-RoPE) positions; scaled / YaRN tables beyond what the caller
 * puts into cos / sin; the padded and the contiguous appends, with or without positions.
 */
#ifndef QATTN_PAGED_VARLEN_ROPE_H_
#define QATTN_PAGED_VARLEN_ROPE_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

int qattn_paged_kv_cache_append_varlen_rope_fp8(const void* k16, const void* v16, int in_fmt, const long long* k_strides2,
                                                const long long* v_strides2, /* {token, head}, elements */
                                                void* k_pool, void* v_pool, const float* scale_k, const float* scale_v,
                                                const int* block_table, long long table_stride, int* seqlens, const int* cu_seqlens,
                                                int advance, int B, int Hkv, int total, int num_pages, int page_size, int max_pages, int D,
                                                int fp8_fmt, const float* cos, const float* sin, long long table_row_stride, int T,
                                                int interleaved, void* stream);

int qattn_rope_paged_varlen(const void* x16, int in_fmt, const long long* x_strides2, /* {token, head}, elements */
                            void* out16, const int* cu_seqlens, const int* seqlens, int appended, int B, int H, int total,
                            long long capacity, int D, const float* cos, const float* sin, long long table_row_stride, int T,
                            int interleaved, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_PAGED_VARLEN_ROPE_H_ */

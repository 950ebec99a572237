/*
 * qattn_kvcache.h -- an APPENDABLE FP8 K/V cache with FIXED scales for qattn_fp8_attention_splitkv_forward (include/qattn_splitkv.h): new
 * tokens are quantised with the cache's scales and written into the KFRAG / VFRAG images at positions read on the device (ABI 8 addition;
 * the name is found by symbol, include/qattn.h and QATTN_ABI_VERSION unchanged).
 *
 * The prepared images of qattn_splitkv.h carry head-wise scales over the WHOLE tensor, which cannot grow with it.  A cache's scales are
 * fixed when it is made -- calibrated, or taken from the prefill with headroom -- and a value outside scale * qmax saturates: its byte is
 * +-qmax, its error the excess, never a NaN.  The attention entry needs nothing new: it reads seqused_k (= seqlens here) on the device and
 * ignores every byte behind it.
 *
 * Semantics.  k16 / v16: T new tokens of every (batch element, kv head), 16-bit (in_fmt), head_dim innermost and dense, addressed through
 * the ELEMENT strides k_strides3 / v_strides3 = {batch, head, token}; every row 16-byte aligned (base pointer 16-byte aligned, strides
 * non-negative multiples of 8).  k8_kfrag / v8_vfrag: the images of [B, Hkv, capacity, D] in fp8_fmt, qattn_fp8_tensor_bytes(QATTN_LAYOUT_KFRAG / _VFRAG,
 * B, Hkv, capacity, D) bytes each; scale_k / scale_v fp32 [B, Hkv], finite and > 0.  seqlens int32 [B]; new_lens NULL or int32 [B].
 *   positions   p_b = clamp(seqlens[b], 0, capacity);  n_b = T (new_lens NULL) or clamp(new_lens[b], 0, T).  Token t < n_b of batch element
 *               b becomes key p_b + t of every kv head; a token whose position is >= capacity is dropped.
 *   advance     != 0: after all writes seqlens[b] = min(p_b + n_b, capacity).  A cache that reaches capacity saturates there.
 *   bytes       key j of the K image: fp8_rne(clamp(round_to_in_fmt(fp32(x) / scale_k[b,h]), +-qmax)) at the KFRAG offset of (j, d); V the same
 *               with scale_v at the VFRAG offset -- the quantiser of qattn_quant_fp8 under the given scale (no `numerics`: that argument
 *               only shapes how qattn_quant_fp8 derives a scale).  A vector that holds a non-finite element takes the quantiser's exact
 *               path, as the formula says: a NaN becomes a NaN byte, +-inf clamps to +-qmax.  V must be finite.
 *   written     exactly the bytes of the appended keys, and seqlens under advance.  No other byte of either image changes, and no result
 *               depends on what the images held.  Bytes behind seqlens influence no output bit of the attention entry, so a rollback is
 *               seqlens[b] -= n (speculative decoding: rejected tokens are overwritten by the next append).
 *
 * Launches, both on `stream`, nothing read on the host, no allocation, no workspace; graph-capture safe, and a captured call follows the
 * later contents of seqlens / new_lens:
 *   1  kv_append_kernel: one 256-thread workgroup per (b, kv head, c, K or V), c the c-th 64-key chunk touched by [p_b, p_b + n_b) -- a grid of
 *      B Hkv (ceil(T / 64) + 1) x 2; a batch element that appends nothing (n_b = 0, a full cache) costs its workgroups two loads.  A chunk
 *      the range covers completely is stored as the quant pre-pass stores it.  A partly covered K chunk stores the 16-byte pieces of its own keys (a KFRAG piece belongs to one key).  A partly covered V chunk stores a 32-bit word
 *      where the aligned 4-key group lies wholly inside the range and single bytes otherwise: a word or a byte has one writer, nothing is
 *      read back from the images.
 *   2  advance only: kv_advance_kernel, ceil(B / 256) workgroups, rewrites seqlens.  A launch of its own because stream order is the one
 *      cheap guarantee that every workgroup of launch 1 has read the old value.
 *
 * Errors (negative QATTN_ERR_* before any device call): QATTN_ERR_INVALID_ARG for a NULL pointer (new_lens excepted), an image pointer
 * that is not 16-byte aligned, a misaligned row (k16 / v16 not 16-byte aligned, a stride that is no multiple of 8), a negative stride,
 * a non-positive dimension, a capacity above 2^31 - 64, a grid beyond 2^31 - 1 workgroups; QATTN_ERR_UNSUPPORTED_DIM for D outside {64, 128, 256};
 * QATTN_ERR_UNSUPPORTED_FMT.  Buffers: include/qattn_buffers.h.
 *
 * A PAGED cache (a pool of fixed-size pages behind a block table) is include/qattn_paged.h: qattn_paged_kv_cache_append_fp8 is this entry
 * with another store address per chunk, and an image of shape (num_pages, Hkv, page_size, D) made here is a pool there, byte for byte.
 */
#ifndef QATTN_KVCACHE_H_
#define QATTN_KVCACHE_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

int qattn_kv_cache_append_fp8(const void* k16, const void* v16, int in_fmt, const long long* k_strides3, const long long* v_strides3,
                              void* k8_kfrag, void* v8_vfrag, const float* scale_k, const float* scale_v, int* seqlens, const int* new_lens,
                              int advance, int B, int Hkv, int T, int capacity, int D, int fp8_fmt, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_KVCACHE_H_ */

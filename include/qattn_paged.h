/*
 * qattn_paged.h -- a PAGED FP8 K/V cache (pool + block table) for split-KV decode: the append of include/qattn_kvcache.h and the attention
 * of include/qattn_splitkv.h on keys that live in fixed-size pages of a shared pool (ABI 8 addition; the names are found by symbol,
 * include/qattn.h and QATTN_ABI_VERSION unchanged).
 *
 * A contiguous cache [B, Hkv, capacity, D] reserves `capacity` keys for every sequence, cannot share a prompt prefix between sequences and
 * cannot hand a finished sequence's memory to a new one without a copy.  Here a sequence's keys are looked up through a table of page
 * numbers; which chunk a kernel fetches or stores is all that changes -- the sweep, the numerics and the DMA granularity (one contiguous
 * 64 D-byte chunk per fetch) are those of the contiguous entries.
 *
 * LAYOUT (the contract).
 *   pool         k_pool: the KFRAG image of a [num_pages, Hkv, page_size, D] tensor; v_pool: the VFRAG image of the same shape.  Each
 *                qattn_fp8_tensor_bytes(QATTN_LAYOUT_KFRAG / _VFRAG, num_pages, Hkv, page_size, D) bytes, 16-byte aligned.  page_size is a
 *                positive multiple of 64 (64, 128, 256, ...): an image is an array of self-contained 64-key chunks of 64 D bytes and no chunk
 *                straddles a page.  With pc = page_size / 64, chunk c < pc of kv head h of page p starts at byte
 *                    ((p Hkv + h) pc + c) 64 D.
 *                A KVCacheFP8 (include/qattn_kvcache.h) of shape (num_pages, Hkv, page_size, D) therefore IS a pool, byte for byte: its
 *                "batch element" p is page p.
 *   block table  int32 [B, max_pages] on the device, row stride table_stride >= max_pages in elements.  Key j of sequence b is key
 *                j % page_size of page table[b][j / page_size].
 *   scales       scale_k / scale_v fp32 [B, Hkv], fixed, as a KVCacheFP8's: per SEQUENCE, not per page.  A page that several sequences
 *                share (a common prompt prefix) needs equal scales in all of them: the caller's responsibility, nothing checks it.
 *   logical bound  every entry takes Skv (the append: capacity = max_pages page_size) <= max_pages page_size; L_b = clamp(seqused_k[b], 0, Skv).
 *                seqused_k is REQUIRED by the attention entry.
 *   entries read   the attention reads only the table entries below ceil(L_b / page_size) that the chunks of its splits touch (causal: up to
 *                the last chunk a row attends); the append only the entries of the pages that hold the keys [p_b, end_b).  Every other
 *                entry may hold anything.
 *   entries clamped  EVERY entry that is read is clamped into [0, num_pages - 1] before it forms an address: no table content can make a
 *                kernel address a byte outside the pool.  (A clamped entry reads or writes the wrong page -- garbage in, garbage out --
 *                but never faults.)
 * The library allocates no pages, copies none on write and never re-scales; the table is the caller's allocator's to write, in place,
 * between calls -- both entries read it on the device, so a captured graph follows its later contents.
 *
 * qattn_paged_kv_cache_append_fp8: qattn_kv_cache_append_fp8 (include/qattn_kvcache.h) with capacity = max_pages page_size, word for word --
 * positions, new_lens, advance (a launch of its own), the quantiser's bytes, saturation, NaN and +-inf handling, tokens at or beyond the
 * capacity dropped, the store schemes of a wholly and of a partly covered chunk (one writer per word or byte, nothing read back) -- except
 * for WHERE a touched chunk is stored: chunk c of the sequence goes to chunk c % pc of page clamp(table[b][c / pc]).  The pages that cover
 * [seqlens[b], seqlens[b] + n_b) must have been assigned before the call.  Two sequences that append into the same page in one call have
 * two writers: undefined.  Errors: those of qattn_kv_cache_append_fp8, and QATTN_ERR_INVALID_ARG for the argument checks below.
 *
 * qattn_fp8_attention_paged_splitkv_forward: qattn_fp8_attention_splitkv_forward (include/qattn_splitkv.h) with k_pool, v_pool, block_table,
 * table_stride, num_pages, page_size, max_pages in place of the contiguous images; the split plan, the masks, the zeroing of the V bytes
 * behind L_b in the chunk that holds key L_b, the partial buffers, the merge chain, row_path, the error codes and "no host synchronisation,
 * no allocation, graph-capture safe" are that entry's, and so are its bits: a call equals the contiguous call on the images gathered
 * through the table (tests/test_gpu_paged.py), which carries contracts (a) .. (g) of include/qattn_splitkv.h over.  num_splits = 0 is
 * qattn_splitkv_auto_splits on the LOGICAL Skv; pass the longest live sequence (rounded up as you like), not max_pages page_size, or the
 * rule over-splits.  Workspace: qattn_fp8_attention_paged_splitkv_workspace_bytes, which is the contiguous entry's function (neither
 * depends on where the keys live).  Step t of a workgroup sweeps logical chunk c; a workgroup keeps page and chunk-in-page counters (one
 * division per workgroup, none per step) and loads a table entry -- one dword, workgroup-uniform -- when its sweep enters a page, a
 * step before the DMA that needs it.
 *
 * Argument checks of both entries, before any device call (QATTN_ERR_INVALID_ARG): page_size >= 64 and page_size % 64 == 0; num_pages > 0,
 * max_pages > 0; table_stride >= max_pages; num_pages Hkv (page_size / 64) <= 2^31 - 1 (the physical chunk index is an int);
 * max_pages page_size <= 2^31 - 65; Skv <= max_pages page_size; every pointer non-NULL (new_lens and the optional outputs excepted) and
 * aligned (pools 16 bytes, block_table 4 bytes).  Buffers: include/qattn_buffers.h.
 *
 * Not offered: page allocation, copy-on-write, re-scaling, a per-call table whose batch differs from the scales' and lengths', sliding
 * windows.  Queries of a DIFFERENT count per sequence (a serving step that mixes prefill chunks and decodes), packed as [total_q, Hq, D]
 * under cu_seqlens_q: include/qattn_paged_varlen.h.
 */
#ifndef QATTN_PAGED_H_
#define QATTN_PAGED_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

int qattn_paged_kv_cache_append_fp8(const void* k16, const void* v16, int in_fmt, const long long* k_strides3, const long long* v_strides3,
                                    void* k_pool, void* v_pool, const float* scale_k, const float* scale_v, const int* block_table,
                                    long long table_stride, int* seqlens, const int* new_lens, int advance, int B, int Hkv, int T,
                                    int num_pages, int page_size, int max_pages, int D, int fp8_fmt, void* stream);

/* = qattn_fp8_attention_splitkv_workspace_bytes(B, Hq, Hkv, Sq, Skv, D, num_splits) */
size_t qattn_fp8_attention_paged_splitkv_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Skv, int D, int num_splits);

int qattn_fp8_attention_paged_splitkv_forward(const void* q16, int in_fmt, const void* k_pool, const void* v_pool, const int* block_table,
                                              long long table_stride, int num_pages, int page_size, int max_pages, const float* scale_k,
                                              const float* scale_v, void* out, float* lse, const int* seqused_k, int B, int Hq, int Hkv,
                                              int Sq, int Skv, int D, int fp8_fmt, int numerics, int is_causal, float sm_scale,
                                              int precision, int num_splits, void* q8, float* scale_q, unsigned char* row_path,
                                              float* partial_o, float* partial_lse, unsigned char* partial_path, void* workspace,
                                              size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_PAGED_H_ */

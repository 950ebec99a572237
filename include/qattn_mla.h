/*
 * qattn_mla.h -- FP8 multi-head latent attention (MLA, the attention of DeepSeek-V2 / V3 / R1 and Kimi-K2) in its ABSORBED decode form over a
 * paged latent cache (ABI 8 addition; the names are found by symbol, include/qattn.h and QATTN_ABI_VERSION unchanged).
 *
 * In the absorbed form every query head of a token attends ONE shared vector per key: 512 latent channels (kv_c) followed by 64 rotary
 * channels (k_pe, rotated by the caller).  A score is a 576-channel dot product; the value of a key is the first 512 channels of the same
 * vector.  Hq (head, position) pairs of a slot therefore form one group over one "kv head" whose K and V are the same bytes.
 *
 * LAYOUT (the contract).
 *   pool         ONE image, [num_pages, page_size / 64] chunks of 64 keys x 576 bytes = 36 864 bytes, 16-byte aligned, no head axis:
 *                qattn_mla_pool_bytes(num_pages, page_size) bytes.  A chunk is the KFRAG order of csrc/qattn_common.h with s over the 9
 *                slices of 64 channels:  [t:2][s:9][hh:2][half:2][key:32][16 B],  byte j of a piece = X[64c + 32t + key][64s + 32hh + 16half + j],
 *                i.e. byte (key k < 64, channel d < 576) of a chunk lies at
 *                    (((k >> 5) * 9 + (d >> 6)) << 11) + (((d >> 5) & 1) << 10) + (((d >> 4) & 1) << 9) + ((k & 31) << 4) + (d & 15).
 *                Channels 0..511 are kv_c, 512..575 k_pe.  The value operand is read from the SAME bytes (the kernel transposes each chunk
 *                on the chip): there is no second image.  page_size is a positive multiple of 64; chunk c of page p starts at byte
 *                (p (page_size / 64) + c) 36 864.
 *   block table, lengths, clamping   as include/qattn_paged.h: int32 [B, max_pages] with row stride table_stride; key j of slot b is key
 *                j % page_size of page table[b][j / page_size]; L_b = clamp(seqused_k[b], 0, Skv), Skv <= max_pages page_size; only the
 *                entries below ceil(L_b / page_size) that a split touches are read (the append: the pages that hold the appended keys), and
 *                EVERY entry that is read is clamped into [0, num_pages - 1] before it forms an address.
 *   scale        fp32 [B]: ONE fixed scale per slot for all 576 channels (the value bytes are the key bytes: there is no room for two).  A
 *                caller whose k_pe range differs from the latent's may pre-multiply k_pe by a constant and q_pe by its inverse: the scores do
 *                not change and the values never see k_pe.
 *
 * qattn_paged_mla_cache_append_fp8: reads ckv16 [B, T, 512] and kpe16 [B, T, 64] (bf16 / fp16, the two slices of the model's projection) through
 * their element strides {batch, token} (channels dense, rows 16-byte aligned, strides multiples of 8, nothing is copied), quantises with the
 * slot's scale -- the quantiser, saturation, NaN and +-inf handling of qattn_kv_cache_append_fp8 (include/qattn_kvcache.h) -- and stores token t
 * of slot b as key seqlens[b] + t through the table.  new_lens, advance (a launch of its own) and "tokens at or beyond the capacity
 * max_pages page_size are dropped" as in qattn_paged_kv_cache_append_fp8.  A call changes exactly the bytes of the keys it appends (one 16-byte
 * store per 16 channels of a key, nothing read back).  Everything is read on the device: graph-capture safe.
 *
 * qattn_fp8_mla_paged_forward: q16 [B, Hq, Sq, 576] (element strides q_strides3 = {batch, head, position}, NULL: dense; channels dense, rows
 * 16-byte aligned) over the pool.  One workgroup per (slot, 64-row tile of the slot's Hq Sq (head, position) rows, key split).  q is quantised
 * INSIDE the kernel, token-wise: scale_q = max(amax / 448, 2^-23) per row, q8 = e4m3(clamp(fp32(q) * (1 / scale_q), +-448)) -- always e4m3,
 * whatever the cache's format; every split produces the same bytes, and split 0 writes q8 [B, Hq, Sq, 576] and scale_q [B, Hq, Sq] when the
 * pointers are non-NULL.  Scores are sm_scale scale_q scale[b] (q8 . k8); sm_scale must be > 0 and finite -- MLA's scale is the MODEL's
 * (1/sqrt(192) times its YaRN factor), never 1/sqrt(576), so there is no default.  P is two-term e4m3 with the 2^5 gain of csrc/qattn_attn.h,
 * both products run on v_mfma_f32_32x32x64_f8f6f4.  is_causal: bottom-right over Sq (position i attends keys j <= L_b - Sq + i).  Keys at or
 * behind L_b influence no bit: their scores are masked and their value bytes zeroed on the chip, NaN bytes of never-written pages included.
 * A row without a key is a zero row with LSE -inf.  out [B, Hq, Sq, 512] in the input format, lse [B, Hq, Sq] (may be NULL) in natural-log
 * units of the scaled scores.
 *   splits       num_splits = 0: qattn_mla_auto_splits(B, Hq, Sq, Skv, CUs of the device).  Split s of slot b owns the chunks
 *                [s per, (s + 1) per) of its ceil(L_b / 64), per = ceil(ceil(L_b / 64) / num_splits).  One split rounds into out itself.  More
 *                write normalised fp32 partials [ns, B, Hq, Sq, 512] and their LSEs [ns, B, Hq, Sq] -- into partial_o / partial_lse when given,
 *                else into the workspace -- and ONE launch of the combine kernel merges all ns <= QATTN_MLA_MAX_SPLITS of them:
 *                L = log sum exp(lse_i), O = sum_i exp(lse_i - L) O_i in fp32 in the order of i, one rounding; a -inf partial contributes
 *                nothing, all -inf gives a zero row and LSE -inf.
 *   workspace    qattn_fp8_mla_paged_workspace_bytes(B, Hq, Sq, num_splits) with the RESOLVED split count (0 for one split), 16-byte aligned.
 * Nothing is read on the host, nothing allocated: graph-capture safe; a captured call follows the later contents of the table and lengths.
 *
 * Argument checks, before any device call (QATTN_ERR_INVALID_ARG unless noted): the paging checks of include/qattn_paged.h with Hkv = 1; B, Hq,
 * Sq, T > 0; Hq Sq <= 2^20; B Hq Sq and B ceil(Hq Sq / 64) ns <= 2^31 - 1 (the grids); pointers non-NULL (new_lens, lse, q8, scale_q, partial_*, a zero-size workspace excepted) and aligned (pool, q16,
 * ckv16, kpe16, out, q8: 16 bytes); strides non-negative multiples of 8; 0 <= num_splits <= QATTN_MLA_MAX_SPLITS; sm_scale > 0; workspace_bytes
 * large enough; formats: QATTN_ERR_UNSUPPORTED_FMT.  Buffers: include/qattn_buffers.h.
 *
 * Not offered: windows, sinks, soft cap or trees on MLA; RoPE inside the append (the caller rotates k_pe);
 * precision "fast" / "auto"; per-token cache scales.  (Packed variable-length q: include/qattn_mla_varlen.h.  DeepSeek-V3.2's sparse indexer: include/qattn_mla_index.h.  The non-absorbed prefill
 * form -- ordinary MHA at D 192 / 128 -- is include/qattn_mla_prefill.h)
 */
#ifndef QATTN_MLA_H_
#define QATTN_MLA_H_

#include "qattn.h"

#define QATTN_MLA_D_LATENT 512
#define QATTN_MLA_D_ROPE 64
#define QATTN_MLA_D 576
#define QATTN_MLA_MAX_SPLITS 64

#ifdef __cplusplus
extern "C" {
#endif

size_t qattn_mla_pool_bytes(int num_pages, int page_size);

/* the largest count <= QATTN_MLA_MAX_SPLITS whose grid B ceil(Hq Sq / 64) ns the chip holds at once (one workgroup per CU) with >= 1024 keys
 * of Skv per split; at least 1.  A pure function of its arguments. */
int qattn_mla_auto_splits(int B, int Hq, int Sq, int Skv, int num_cus);

size_t qattn_fp8_mla_paged_workspace_bytes(int B, int Hq, int Sq, int num_splits);

int qattn_paged_mla_cache_append_fp8(const void* ckv16, const void* kpe16, int in_fmt, const long long* ckv_strides2,
                                     const long long* kpe_strides2, void* pool, const float* scale, const int* block_table,
                                     long long table_stride, int* seqlens, const int* new_lens, int advance, int B, int T, int num_pages,
                                     int page_size, int max_pages, int fp8_fmt, void* stream);

int qattn_fp8_mla_paged_forward(const void* q16, int in_fmt, const long long* q_strides3, const void* pool, const int* block_table,
                                long long table_stride, int num_pages, int page_size, int max_pages, const float* scale, void* out, float* lse,
                                const int* seqused_k, int B, int Hq, int Sq, int Skv, int fp8_fmt, int is_causal, float sm_scale,
                                int num_splits, void* q8, float* scale_q, float* partial_o, float* partial_lse, void* workspace,
                                size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_MLA_H_ */

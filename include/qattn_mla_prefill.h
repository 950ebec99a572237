/*
 * qattn_mla_prefill.h -- FP8 multi-head latent attention (include/qattn_mla.h) in its NON-ABSORBED prefill form: packed variable-length
 * multi-head attention whose score product has 192 channels (128 "nope" channels of the head followed by 64 rotary channels) and whose value
 * product has 128, with the rotary slice of K stored ONCE per token and shared by all heads.  The names are found by symbol; include/qattn.h and
 * QATTN_ABI_VERSION are unchanged.
 *
 * TENSORS (16-bit, one format in_fmt = QATTN_FMT_BF16 / _FP16; channels dense, rows 16-byte aligned, nothing is copied)
 *   q       [total_q, H, 192]   q_nope | q_pe, already rotated
 *   k_nope  [total_k, H, 128]
 *   k_pe    [total_k, 64]       one row per token, already rotated, attended by EVERY head
 *   v       [total_k, H, 128]
 *   strides7 = element strides {q token, q head, k_nope token, k_nope head, k_pe token, v token, v head}, NULL: dense.  Non-negative multiples
 *   of 8.  k_nope and v may be the two halves of one [total_k, H, 256] projection.  MHA only: one head count H.
 *   out     [total_q, H, 128] dense, in_fmt;   lse fp32 [H, total_q] (may be NULL): the natural log-sum-exp of the scaled scores, the packed
 *   layout of include/qattn_varlen.h, which qattn_attention_state_merge (include/qattn_merge.h) takes as it is.  out and lse are written
 *   for the rows of sequences only: a token at or behind cu_seqlens_q[B] (a padded bucket) has no work item and keeps what it held.
 *
 * TABLES.  cu_seqlens_q / cu_seqlens_k int32 [B + 1], seqused_k int32 [B] or NULL, on the device; every extent is clamped as in
 * include/qattn_varlen.h (start = clamp(cu[i], 0, total), end = clamp(cu[i + 1], start, total), used keys clamp(seqused_k[i], 0, end - start)).
 * Nothing is read on the host and nothing allocated: graph-capture safe; a replayed graph follows the later contents of the tables.
 *
 * MASK.  is_causal is BOTTOM-RIGHT, as in the MLA decode entries: row r of a sequence with L_q rows and L_k used keys attends the keys
 * j <= r + L_k - L_q.  A row without a key (L_k = 0; the first L_q - L_k rows when L_q > L_k) is a zero row with LSE -inf.  Chunked prefill is
 * one call over the context (is_causal = 0) and one over the chunk (is_causal = 1), merged by their LSEs.
 *
 * NUMERICS.
 *   q    quantised token-wise INSIDE the attention kernel, over the 192 channels of a (token, head) row: scale_q = max(amax / 448, 2^-23),
 *        q8 = e4m3(clamp(fp32(q) * (1 / scale_q), +-448)) -- always e4m3 (the quantiser of qattn_fp8_mla_paged_forward); no launch of its own.
 *        q8 [total_q, H, 192] and scale_q [total_q, H] are written when the pointers are non-NULL (rows of sequences only).
 *   K    ONE scale per (sequence, head): amax over the head's 128 k_nope channels AND the shared 64 k_pe channels of the sequence's USED keys,
 *        scale_k = max(amax * (1 / fmax), 2^-23) in fp32, k8 = fp8(clamp(round16(fp32(k) / scale_k), +-fmax)) -- the head-wise quantiser of
 *        the library (QATTN_NUMERICS_COMPILED, saturating) in fp8_fmt = QATTN_FMT_E4M3 / _E5M2.  k_pe is quantised once per head, with that
 *        head's scale, while the image is written: neither the 16-bit concatenation nor the head broadcast exists in memory.
 *   V    ONE scale per (sequence, head) over its used keys, the same quantiser.  scale_k / scale_v fp32 [B, H] are written when non-NULL.
 *   P    two-term (hi + lo) e4m3 with the 2^5 gain of csrc/qattn_attn.h on exact exponentials; there is no "fast" / "auto".  Both products
 *        run on v_mfma_f32_32x32x64_f8f6f4.  Scores are sm_scale scale_q scale_k (q8 . k8); sm_scale must be finite and > 0 -- MLA's softmax
 *        scale is the model's (1/sqrt(192) times its YaRN factor), so there is no default.
 * Keys at or behind the used length and tokens outside every sequence influence no output bit, the scales included: they are never read.
 *
 * IMAGES (workspace, private).  Per (sequence i, head h) a K image of 64-key chunks of 64 x 192 = 12 288 bytes in the KFRAG order of
 * csrc/qattn_common.h with s over the 3 slices of 64 channels -- [t:2][s:3][hh:2][half:2][key:32][16 B], the order include/qattn_mla.h spells out
 * for 9 slices; channels 0..127 = k_nope[:, h], 128..191 = k_pe -- and beside it a V image of 64 x 128 = 8 192-byte chunks in VFRAG order.  The
 * rows of the last chunk behind the used length are zero bytes.  Sequence i's images start at byte H D (start_i + 64 i), D = 192 / 128.
 *
 * LAUNCHES: a zeroing node, one abs-max launch, one quantise launch (k_nope, k_pe and v together, on the packed tile map), the attention sweep:
 * one 4-wave workgroup per (head, 128-row tile of a sequence) over the sequence's 64-key chunks in ascending order, up to the tile's
 * bottom-right diagonal when causal.
 *
 * WORKSPACE.  qattn_fp8_mla_prefill_varlen_workspace_bytes(B, H, total_q, total_k) bytes, 16-byte aligned (0 when a limit is broken).
 *
 * Argument checks, before any device call, with the codes of include/qattn_varlen.h: QATTN_ERR_INVALID_ARG for a NULL q / k_nope / k_pe / v /
 * out / table, B < 1, H < 1, a negative total, a pointer (q, k_nope, k_pe, v, out, q8) that is not 16-byte aligned, a stride that is negative
 * or no multiple of 8, sm_scale not finite or <= 0, a grid beyond 2^31 - 1 workgroups; QATTN_ERR_UNSUPPORTED_FMT for the formats;
 * QATTN_ERR_WORKSPACE for a NULL or short workspace.  total_q = 0 returns QATTN_OK and writes nothing.
 *
 * Not offered: grouped heads (Hq != Hkv), windows, sinks, soft cap, key smoothing, precision "fast" / "auto", a backward pass.
 */
#ifndef QATTN_MLA_PREFILL_H_
#define QATTN_MLA_PREFILL_H_

#include "qattn.h"

#define QATTN_MLA_PREFILL_D_QK 192    /* 128 nope + 64 rotary channels */
#define QATTN_MLA_PREFILL_D_NOPE 128
#define QATTN_MLA_PREFILL_D_ROPE 64
#define QATTN_MLA_PREFILL_D_V 128

#ifdef __cplusplus
extern "C" {
#endif

size_t qattn_fp8_mla_prefill_varlen_workspace_bytes(int B, int H, int total_q, int total_k);

int qattn_fp8_mla_prefill_varlen_forward(const void* q, const void* k_nope, const void* k_pe, const void* v, const long long* strides7, int in_fmt,
                                         void* out, float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k, const int* seqused_k, int B,
                                         int H, int total_q, int total_k, int fp8_fmt, int is_causal, float sm_scale, void* q8, float* scale_q,
                                         float* scale_k, float* scale_v, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_MLA_PREFILL_H_ */

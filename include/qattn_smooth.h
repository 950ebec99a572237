/*
 * qattn_smooth.h -- the fused entry of include/qattn.h / qattn_strided.h with KEY SMOOTHING (an ABI-8 addition).
 *
 * The keys of image / video DiTs carry a large per-channel offset shared by all tokens of a head.  e4m3 keeps 3 mantissa bits, so an
 * offset b on a channel costs about b/16 of absolute error on every key of that channel, while the part of K that decides the softmax --
 * the deviation from the channel mean -- is much smaller.  SageAttention's "smooth-K": subtract the mean of K over the sequence, per
 * (batch, kv head, channel), before quantising.  q.(k_j - m) = q.k_j - q.m and q.m is the same for every key j of a row, so the softmax
 * rows -- and `out` -- are mathematically unchanged (causal or not, GQA, head-wise or token-wise scales); only the LSE moves, by
 * sm_scale * q_i.m, which this entry adds back.
 *
 * Numerics, for every (b, kv head) g and channel d:
 *   1. m[g,d] = fp32 mean over the Skv rows of fp32(k[g,:,d]).  Deterministic: per-block partial sums in the workspace, added in a fixed
 *      order (no float atomics); the same input gives the same bits on every call, eager or graph replay.  m is written to `k_mean`.
 *   2. ks = fp32(k) - m: one fp32 subtraction per element, never rounded to 16 bits.
 *   3. K's abs-max (per head, or per token), its sum of squares (the score-spread forecast of QATTN_PRECISION_AUTO), scale_k and the fp8
 *      bytes are those of the quantiser of qattn_quant_fp8 applied to ks: scale = clamp_min(amax * (1/fmax), eps) (QATTN_NUMERICS_EAGER:
 *      scale and eps rounded to the input dtype), byte = fp8(clamp(round16(ks / scale), +-fmax)) with the IEEE fp32 quotient, KFRAG layout,
 *      the padding rows of the last 64-key chunk zero bytes (not -m).
 *   4. The attention kernels run unchanged on q (or q8), the smoothed k8, scale_k and V.
 *   5. lse (when non-NULL) = what the launch writes + sm_scale * sum_d fp32(q[b,h,i,d]) * m[g,d] (the caller's 16-bit q, fp32
 *      accumulation; sm_scale the effective one, 1/sqrt(D) by default), i.e. the LSE of the TRUE scores, in both layouts (REFERENCE scales
 *      the correction by -sqrt(D) like the rest).  One small kernel after the attention launch, only when lse is asked for: `out` depends on
 *      `lse` no more than it does in qattn_fp8_quant_attention_forward_ex.
 *   6. A NaN or inf anywhere in a head's K makes m non-finite and the whole head's output NaN (without smoothing such a K poisons the
 *      head through its scale as well).
 *
 * Arguments: those of qattn_fp8_quant_attention_forward_strided (`strides` may be NULL = dense [B,H,S,D]) plus
 *   k_mean    out: fp32 [B, Hkv, D], required.
 *   amax_k, ssq_k   describe the UNSMOOTHED K: must be NULL, else QATTN_ERR_INVALID_ARG.  amax_q and amax_v work as in ..._forward_ex;
 *             ssq_q is accepted and not used (without K's sum the forecast takes both from the pre-pass: q is read for its own).
 *   workspace at least qattn_fp8_quant_attention_smooth_workspace_bytes(...) bytes, 16-byte aligned.
 * Sizes, alignment and which bytes of each buffer are written: include/qattn_buffers.h.
 * Costs one more read of K than the plain entry (mean pass, abs-max pass, quantise pass instead of the last two); K rides in launches of
 * its own, q and V in the plain pre-pass.  No host synchronisation, no allocation, graph-capture safe, like every entry.
 */
#ifndef QATTN_SMOOTH_H_
#define QATTN_SMOOTH_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t qattn_fp8_quant_attention_smooth_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Skv, int D);

int qattn_fp8_quant_attention_forward_smooth(const void* q, const void* k, const void* v, const long long* strides, int in_fmt, void* out,
                                             void* q8, void* k8, void* v8, float* scale_q, float* scale_k, float* scale_v,
                                             const float* amax_q, const float* amax_k, const float* amax_v, const float* ssq_q,
                                             const float* ssq_k, int B, int Hq, int Hkv, int Sq, int Skv, int D, int fp8_fmt, int scale_mode,
                                             int numerics, int is_causal, float sm_scale, int precision, float* lse, int lse_layout,
                                             unsigned char* row_path, void* workspace, size_t workspace_bytes, void* stream, float* k_mean);

/* The packed variable-length and block-sparse entries with key smoothing (qattn_fp8_quant_attention_varlen_forward_smooth,
 * qattn_fp8_block_sparse_attention_forward_smooth) are declared beside their plain entries: include/qattn_varlen.h,
 * include/qattn_block_sparse.h. */

#ifdef __cplusplus
}
#endif
#endif /* QATTN_SMOOTH_H_ */

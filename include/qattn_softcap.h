/*
 * qattn_softcap.h -- LOGIT SOFT-CAPPING for the three split-KV window entries (include/qattn_splitkv_window.h).  ABI 8 addition: the names
 * are found by symbol, include/qattn.h and QATTN_ABI_VERSION are unchanged.  What every Gemma-2 attention layer applies to its scores
 * (attn_logit_softcapping = 50, on its 4096-key window layers (4095, 0) and its full layers (-1, 0) alike) and Grok-1 with 30; flash-attn
 * and vLLM pass it as softcap=.
 *
 * SEMANTICS.  softcap is a host float, finite and > 0.  For a row with scaled scores x_j = sm_scale q.k_j -- computed on the quantised q
 * and k, as in the window sibling:
 *     y_j = softcap tanh(x_j / softcap)
 *     L   = log sum_j exp(y_j)            over the keys j the window admits
 *     out = sum_j exp(y_j - L) v_j
 *   cap before mask  the cap is applied to the score, the mask to the capped score: a masked key weighs exactly 0 (-inf after the cap),
 *                    never exp(-softcap).  Key bytes outside the window -- below it, behind seqused_k, in the window's first chunk below its
 *                    first key; NaN patterns included -- influence no output bit.
 *   returned LSE     is L of the CAPPED scores.  The partials of a call with more splits are ordinary attention states over capped scores:
 *                    the merge chain is the window sibling's, unchanged, and merge(partials) is out, lse bit for bit.
 *   empty rows       a row that attends no key is a zero row with lse = -inf and the sibling's path byte.
 *   NaN              a NaN score among the attended keys makes the row NaN, as in the sibling (tanh(NaN) = NaN).
 *   a kernel argument  softcap is a model constant and travels by value: no device read, no host synchronisation, graph-capture safe -- and a
 *                    captured graph keeps the value it was captured with (capture one graph per distinct cap).
 * Everything else -- the mask, the split plan, the chunks fetched, the paged table reads and clamps, seqused_k, row_path, the workspace size
 * functions and every other argument check -- is the window sibling's.
 *
 * WHERE THE CAP ENTERS.  In the sweep kernel, between the K.Q^T product of a 64-key chunk and the token mask, on all 32 scores a lane
 * holds, on every chunk.  A raw score s (the product of the quantised bytes) becomes
 *     t = tanh(s kin),    kin = sm_scale scale_q[the row's head] scale_k / softcap,
 * a value in [-1, 1], and the sweep runs on t with c = softcap log2e where it runs on s with c = sm_scale log2e scale_q scale_k otherwise:
 * the running maximum, the rescale limit, P' = 2^(t c - base), the two-term split of P' and the epilogue lse = ln2 base + log l are the
 * sibling's statements.
 *
 * THE TANH.  t = 1 - 2 / (1 + 2^(2 log2e u)), u = s kin: one multiply, v_exp_f32, one add, v_rcp_f32, one fma per score.  2^(+large) = +inf
 * gives 2 / inf = 0 and t = 1; 2^(-large) = 0 gives t = -1: saturation without a NaN at any finite u.  Absolute error in t: v_exp_f32 and
 * v_rcp_f32 are good to 1 ulp and the quotient 2 / (1 + E) lies in [0, 2], so
 *     |t - tanh(u)| <= 2 (2^-23 [exp] + 2^-24 [add] + 2^-23 [rcp]) + 2^-24 [fma] + 2^-24 |u| sech^2(u) [the product s kin2] < 2^-20 = 9.5e-7
 * at every u (for |u| < 2^-20 this is also the formula's relative collapse: such scores are returned as multiples of 2^-24 -- an absolute
 * error the bound covers).  The error of a capped logit is softcap times that: 4.8e-5 at softcap = 50, 2.9e-5 at 30 -- against the 2^-8
 * relative step of the two-term e4m3 P, a logit error of 3.9e-3.  There is no small-|u| branch: the tanh error reaches that step from
 * softcap ~ 4000 on, and at such caps scores of ordinary size are not capped at all (|x| = 20 moves by 2e-4) -- call the window sibling.
 *
 * Precision FAST: the soft-cap entries run the EXACT one-term sweep wherever the sibling would pick the byte-exponential one (whose formula
 * is fitted to raw scores): their bits are those of themselves called with an LSE.  ACCURATE is the two-term e4m3 P, as in the sibling.
 *
 * Each forward entry has the argument list of its window sibling plus `float softcap` after window_right; the workspace is the sibling's
 * (qattn_fp8_attention_splitkv_workspace_bytes, ..._paged_splitkv_workspace_bytes, ..._paged_varlen_workspace_bytes).  A softcap that is
 * not finite or not > 0 (NaN, +-inf, 0, negative): QATTN_ERR_INVALID_ARG, before any device call.  ("softcap = 0 means off" is the Python
 * surface's: it calls the window sibling.)
 *
 * Not offered: a soft cap with sinks or under a draft tree; on the dense, packed 16-bit and block-sparse entries; ALiBi; a device-side
 * softcap tensor.
 */
#ifndef QATTN_SOFTCAP_H_
#define QATTN_SOFTCAP_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

int qattn_fp8_attention_splitkv_softcap_forward(const void* q16, int in_fmt, const void* k8_kfrag, const void* v8_vfrag, const float* scale_k,
                                                const float* scale_v, void* out, float* lse, const int* seqused_k, int B, int Hq, int Hkv,
                                                int Sq, int Skv, int D, int fp8_fmt, int numerics, int window_left, int window_right,
                                                float softcap, float sm_scale, int precision, int num_splits, void* q8, float* scale_q,
                                                unsigned char* row_path, float* partial_o, float* partial_lse, unsigned char* partial_path,
                                                void* workspace, size_t workspace_bytes, void* stream);

int qattn_fp8_attention_paged_splitkv_softcap_forward(const void* q16, int in_fmt, const void* k_pool, const void* v_pool,
                                                      const int* block_table, long long table_stride, int num_pages, int page_size,
                                                      int max_pages, const float* scale_k, const float* scale_v, void* out, float* lse,
                                                      const int* seqused_k, int B, int Hq, int Hkv, int Sq, int Skv, int D, int fp8_fmt,
                                                      int numerics, int window_left, int window_right, float softcap, float sm_scale,
                                                      int precision, int num_splits, void* q8, float* scale_q, unsigned char* row_path,
                                                      float* partial_o, float* partial_lse, unsigned char* partial_path, void* workspace,
                                                      size_t workspace_bytes, void* stream);

int qattn_fp8_attention_paged_varlen_softcap_forward(const void* q16, const long long* q_strides2, int in_fmt, const void* k_pool,
                                                     const void* v_pool, const int* block_table, long long table_stride, int num_pages,
                                                     int page_size, int max_pages, const float* scale_k, const float* scale_v, void* out,
                                                     float* lse, const int* cu_seqlens_q, const int* seqused_k, int B, int Hq, int Hkv,
                                                     int total_q, int max_seqlen_q, int Skv, int D, int fp8_fmt, int numerics, int window_left,
                                                     int window_right, float softcap, float sm_scale, int precision, int num_splits, void* q8,
                                                     float* scale_q, unsigned char* row_path, float* partial_o, float* partial_lse,
                                                     unsigned char* partial_path, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_SOFTCAP_H_ */

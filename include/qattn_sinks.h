/*
 * qattn_sinks.h -- LEARNED ATTENTION SINKS for the three split-KV window entries (include/qattn_splitkv_window.h) and for the state merge
 * (include/qattn_merge.h).  ABI 8 addition: the names are found by symbol, include/qattn.h and QATTN_ABI_VERSION are unchanged.  What
 * every gpt-oss attention layer adds to its softmax, windowed (128 keys: (127, 0)) and full ((-1, 0)) alike; vLLM passes it as sinks=,
 * flash-attn 3 as s_aux.
 *
 * SEMANTICS.  sinks is fp32 [Hq] on the device, 4-byte aligned: one logit per QUERY head, in the units of the scaled scores -- natural
 * log, sm_scale applied to the scores and NOT to the sink.  For a row of head h with attended keys j and scores x_j = sm_scale q.k_j:
 *     L   = log( exp(sink_h) + sum_j exp(x_j) )
 *     out = sum_j exp(x_j - L) v_j
 * The sink adds to the denominator and has no value row: it scales the row by 1 - p_sink.
 *   returned LSE   is L, sink included.  Such a state must not be merged with another state that also counted the sink.
 *   empty rows     a row that attends no key is a zero row with lse = sink_h (not -inf); its path byte is ONE_TERM as before.
 *   sink_h = -inf  no sink for that head.  With every sink -inf, out, lse, row_path and all partials are bit for bit those of the window
 *                  entry -- called WITH an LSE under precision FAST, see below -- at every num_splits > 0 (l + 0.0f and den + 0.0f are exact).
 *   +inf or NaN    the rows of that head are NaN in out and lse.
 *   device-only    sinks is read by the kernels alone: no host synchronisation, no allocation, graph-capture safe; a captured call follows
 *                  rewritten sink values.
 * Everything else -- the mask, the split plan, the dead bytes, the paged table reads, seqused_k, row_path, the workspace size functions and
 * every argument check -- is the window sibling's.
 *
 * WHERE THE SINK ENTERS.  One split: the sweep kernel's epilogue.  With the row's maximum m (raw scores), c = sm_scale log2e scale_q
 * scale_k and the sum l of P' = 2^(x c - base), base = m c - 5:
 *     e = 2^(sink_h log2e - base),  l' = l + e,  out = O scale_v / l',  lse = ln2 base + log l'
 * (a sink more than 64 octaves above base is summed under its own shift instead, so that e cannot overflow).  More splits: the sweep
 * writes the partials WITHOUT the sink -- bit for bit the window sibling's partials -- and the sink enters the LAST launch of the merge
 * chain (qattn_attention_state_merge_sink); in a chain of more than 8 partials the launches before it are the plain merge.
 * Precision FAST: the sink entries run the EXACT one-term sweep wherever the sibling would pick the byte-exponential one (the sibling does
 * so with one split and no LSE): their bits are those of the sibling called with an LSE.
 *
 * Each forward entry has the argument list of its window sibling plus `sinks` after window_right; the workspace is the sibling's
 * (qattn_fp8_attention_splitkv_workspace_bytes, ..._paged_splitkv_workspace_bytes, ..._paged_varlen_workspace_bytes).  sinks == NULL or
 * not 4-byte aligned: QATTN_ERR_INVALID_ARG, before any device call.  Exactly Hq floats of it are read.
 *
 * qattn_attention_state_merge_sink: qattn_attention_state_merge (arguments, arithmetic, summation order, NaN rules, aliasing, buffer
 * contract) with 1 <= n <= 8 partials and `sink`, fp32 [H] on the device, 4-byte aligned, indexed by the kernel's head coordinate h (dense
 * and packed stride conventions alike).  The sink is one more state with lse = sink_h and no O row, summed after the partials:
 *     m = max(max_i lse_i, sink_h),  den = sum_i exp(lse_i - m) + exp(sink_h - m),  out = (sum_i e_i O_i) / den,  lse_out = m + log den.
 * It takes part in the "all partials empty" decision: every lse_i = -inf with a finite sink is a zero row with lse_out = sink_h exactly;
 * with sink_h = -inf too, a zero row with lse_out = -inf.  sink_h = -inf: the bits of qattn_attention_state_merge (n >= 2).
 *
 * Not offered: sinks on the dense, packed 16-bit and block-sparse entries; "sink tokens + window" in one call (two calls and a state
 * merge); sink gradients.
 */
#ifndef QATTN_SINKS_H_
#define QATTN_SINKS_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

int qattn_attention_state_merge_sink(int n, const void* const* o, const int* o_fmt, const long long* o_strides, const float* const* lse,
                                     const long long* lse_strides, void* out, int out_fmt, const long long* out_strides, float* lse_out,
                                     const long long* lse_out_strides, int B, int H, int S, int D, void* stream, const float* sink);

int qattn_fp8_attention_splitkv_sink_forward(const void* q16, int in_fmt, const void* k8_kfrag, const void* v8_vfrag, const float* scale_k,
                                             const float* scale_v, void* out, float* lse, const int* seqused_k, int B, int Hq, int Hkv, int Sq,
                                             int Skv, int D, int fp8_fmt, int numerics, int window_left, int window_right, const float* sinks,
                                             float sm_scale, int precision, int num_splits, void* q8, float* scale_q, unsigned char* row_path,
                                             float* partial_o, float* partial_lse, unsigned char* partial_path, void* workspace,
                                             size_t workspace_bytes, void* stream);

int qattn_fp8_attention_paged_splitkv_sink_forward(const void* q16, int in_fmt, const void* k_pool, const void* v_pool, const int* block_table,
                                                   long long table_stride, int num_pages, int page_size, int max_pages, const float* scale_k,
                                                   const float* scale_v, void* out, float* lse, const int* seqused_k, int B, int Hq, int Hkv,
                                                   int Sq, int Skv, int D, int fp8_fmt, int numerics, int window_left, int window_right,
                                                   const float* sinks, float sm_scale, int precision, int num_splits, void* q8, float* scale_q,
                                                   unsigned char* row_path, float* partial_o, float* partial_lse, unsigned char* partial_path,
                                                   void* workspace, size_t workspace_bytes, void* stream);

int qattn_fp8_attention_paged_varlen_sink_forward(const void* q16, const long long* q_strides2, int in_fmt, const void* k_pool,
                                                  const void* v_pool, const int* block_table, long long table_stride, int num_pages,
                                                  int page_size, int max_pages, const float* scale_k, const float* scale_v, void* out,
                                                  float* lse, const int* cu_seqlens_q, const int* seqused_k, int B, int Hq, int Hkv, int total_q,
                                                  int max_seqlen_q, int Skv, int D, int fp8_fmt, int numerics, int window_left, int window_right,
                                                  const float* sinks, float sm_scale, int precision, int num_splits, void* q8, float* scale_q,
                                                  unsigned char* row_path, float* partial_o, float* partial_lse, unsigned char* partial_path,
                                                  void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_SINKS_H_ */

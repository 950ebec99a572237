// qattn_paged_varlen_splitkv_softcap_fp8.hip -- qattn_fp8_attention_paged_varlen_softcap_forward (include/qattn_softcap.h): packed
// variable-length queries over the paged cache under a sliding window per sequence, with the scaled scores soft-capped,
// y = softcap tanh(x / softcap), before the mask and the softmax.
//
// The kernel is the compilation of qattn_splitkv_body.h with QATTN_SKV_PAGED, QATTN_SKV_VARQ, QATTN_SKV_WINDOW and QATTN_SKV_SOFTCAP on; the
// driver is qattn_paged_varlen_attn.h's with WINDOW = SOFTCAP = true.  The cap is a function of the score alone, so a sequence's bits are
// those of the paged soft-cap entry on it alone.
#include "qattn_paged_varlen_attn.h"

using namespace qattn;

extern "C" int qattn_fp8_attention_paged_varlen_softcap_forward(const void* q16, const long long* q_strides2, int in_fmt, const void* k_pool,
                                                                const void* v_pool, const int* block_table, long long table_stride,
                                                                int num_pages, int page_size, int max_pages, const float* scale_k,
                                                                const float* scale_v, void* out, float* lse, const int* cu_seqlens_q,
                                                                const int* seqused_k, int B, int Hq, int Hkv, int total_q, int max_seqlen_q,
                                                                int Skv, int D, int fp8_fmt, int numerics, int window_left, int window_right,
                                                                float softcap, float sm_scale, int precision, int num_splits, void* q8,
                                                                float* scale_q, unsigned char* row_path, float* partial_o, float* partial_lse,
                                                                unsigned char* partial_path, void* workspace, size_t workspace_bytes,
                                                                void* stream) {
    return pvq_forward<true, false, false, true>(q16, q_strides2, in_fmt, k_pool, v_pool, block_table, table_stride, num_pages, page_size,
                                                 max_pages, scale_k, scale_v, out, lse, cu_seqlens_q, seqused_k, B, Hq, Hkv, total_q,
                                                 max_seqlen_q, Skv, D, fp8_fmt, numerics, 0, window_left, window_right, sm_scale, precision,
                                                 num_splits, q8, scale_q, row_path, partial_o, partial_lse, partial_path, workspace,
                                                 workspace_bytes, stream, nullptr, nullptr, softcap);
}

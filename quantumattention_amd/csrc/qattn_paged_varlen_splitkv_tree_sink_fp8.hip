// qattn_paged_varlen_splitkv_tree_sink_fp8.hip -- the sink half of qattn_fp8_attention_paged_varlen_tree_window_forward
// (include/qattn_paged_varlen_tree_window.h): the tree over the packed paged window kernel with a learned sink logit per query head.
//
// The kernel is the compilation of qattn_splitkv_body.h with all five switches on, the exact instances only (the sink kernels never take
// the byte sweep); the driver is qattn_paged_varlen_attn.h's with WINDOW = SINK = TREE = true: one split folds the sink into the sweep's
// epilogue, more splits write sink-free partials and the sink enters the last launch of the merge chain.
#include "qattn_paged_varlen_attn.h"

namespace qattn {

int pvq_tree_window_sink_forward(const void* q16, const long long* q_strides2, int in_fmt, const void* k_pool, const void* v_pool,
                                 const int* block_table, long long table_stride, int num_pages, int page_size, int max_pages,
                                 const float* scale_k, const float* scale_v, void* out, float* lse, const int* cu_seqlens_q,
                                 const int* seqused_k, int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int Skv, int D, int fp8_fmt,
                                 int numerics, const unsigned long long* tree_mask, int window_left, int window_right, const float* sinks,
                                 float sm_scale, int precision, int num_splits, void* q8, float* scale_q, unsigned char* row_path,
                                 float* partial_o, float* partial_lse, unsigned char* partial_path, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    return pvq_forward<true, true, true>(q16, q_strides2, in_fmt, k_pool, v_pool, block_table, table_stride, num_pages, page_size, max_pages,
                                         scale_k, scale_v, out, lse, cu_seqlens_q, seqused_k, B, Hq, Hkv, total_q, max_seqlen_q, Skv, D, fp8_fmt,
                                         numerics, 1, window_left, window_right, sm_scale, precision, num_splits, q8, scale_q, row_path,
                                         partial_o, partial_lse, partial_path, workspace, workspace_bytes, stream, sinks, tree_mask);
}

}  // namespace qattn

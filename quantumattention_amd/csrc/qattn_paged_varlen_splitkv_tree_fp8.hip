// qattn_paged_varlen_splitkv_tree_fp8.hip -- qattn_fp8_attention_paged_varlen_tree_forward (include/qattn_paged_varlen_tree.h): packed
// variable-length queries over the paged cache under a draft TREE per sequence -- the verify pass of tree-shaped speculative decoding.
//
// The kernel is the compilation of qattn_splitkv_body.h with QATTN_SKV_PAGED, QATTN_SKV_VARQ and QATTN_SKV_TREE on: the causal packed
// kernel with one 64-bit word per lane, loaded before the sweep loop and tested in the token branch of the chunks that hold a draft key.
// The driver is qattn_paged_varlen_attn.h's with TREE = true: split plan, workspace, merge chain and path launch are the causal entry's,
// so a chain-shaped tree gives that entry's bits.  The mask is a function of the token, so a sequence's bits are those of the call on it
// alone.
#include "qattn_paged_varlen_attn.h"
#include "../../include/qattn_paged_varlen_tree.h"

using namespace qattn;

extern "C" int qattn_fp8_attention_paged_varlen_tree_forward(const void* q16, const long long* q_strides2, int in_fmt, const void* k_pool,
                                                             const void* v_pool, const int* block_table, long long table_stride,
                                                             int num_pages, int page_size, int max_pages, const float* scale_k,
                                                             const float* scale_v, void* out, float* lse, const int* cu_seqlens_q,
                                                             const int* seqused_k, int B, int Hq, int Hkv, int total_q, int max_seqlen_q,
                                                             int Skv, int D, int fp8_fmt, int numerics, const unsigned long long* tree_mask,
                                                             float sm_scale, int precision, int num_splits, void* q8, float* scale_q,
                                                             unsigned char* row_path, float* partial_o, float* partial_lse,
                                                             unsigned char* partial_path, void* workspace, size_t workspace_bytes,
                                                             void* stream) {
    return pvq_forward<false, false, true>(q16, q_strides2, in_fmt, k_pool, v_pool, block_table, table_stride, num_pages, page_size, max_pages,
                                           scale_k, scale_v, out, lse, cu_seqlens_q, seqused_k, B, Hq, Hkv, total_q, max_seqlen_q, Skv, D, fp8_fmt,
                                           numerics, 1, -1, -1, sm_scale, precision, num_splits, q8, scale_q, row_path, partial_o, partial_lse,
                                           partial_path, workspace, workspace_bytes, stream, nullptr, tree_mask);
}

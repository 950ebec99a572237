// qattn_paged_varlen_splitkv_fp8.hip -- qattn_fp8_attention_paged_varlen_forward (include/qattn_paged_varlen.h): the paged split-KV entry
// for PACKED queries, a different count per sequence -- one call for a serving step that mixes chunked prefill, decode and idle slots.
//
// The kernel is the third compilation of qattn_splitkv_body.h (QATTN_SKV_PAGED and QATTN_SKV_VARQ): the paged kernel's sweep, split plan,
// masks, V-tail zeroing, page walk and sel / two_term_keys rule, on the sequence's own Sq_i and L_i.  What differs is the work-item map --
// (kv head, tile slot of the packed-row space, split), the slot resolved to (sequence, tile) by the binary search of qattn_varlen_tile.h
// on G cu_seqlens_q[i] -- and the row addresses: q8 in the packed pre-pass's slabs, out / partial_o token-major [total_q, Hq, D], the
// LSE-like outputs [Hq, total_q].  A sequence's tiles hold its rows alone, so its bits are those of the paged entry on it alone.
// The host driver: the packed q pre-pass (qattn_varlen.hip's abs-max and quantise launches on q alone), the launch ladder, the merge chain
// and the path launch of qattn_splitkv_attn.h -- the latter two on flat rows / the packed strides of include/qattn_merge.h.
#include "qattn_paged_varlen_attn.h"

using namespace qattn;

extern "C" size_t qattn_fp8_attention_paged_varlen_workspace_bytes(int B, int Hq, int Hkv, int total_q, int Skv, int D, int num_splits) {
    if (!pvq_dims_ok(B, Hq, Hkv, total_q, Skv, D) || num_splits < 0 || num_splits > QATTN_SPLITKV_MAX_SPLITS) return 0;
    return pvq_ws(B, Hq, total_q, D, pvq_most_splits(Skv, num_splits)).total();
}

extern "C" int qattn_paged_varlen_auto_splits(int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int Skv, int D, int num_cus) {
    if (!pvq_dims_ok(B, Hq, Hkv, total_q, Skv, D) || total_q < 1 || max_seqlen_q < 1 || num_cus <= 0) return 1;
    // two upper bounds of the tiles per kv head, sum of ceil(G Sq_i / 128): every sequence at the longest count; one ragged tile per
    // non-empty sequence on top of the full ones
    const long long G = Hq / Hkv;
    const long long by_max = (long long)B * ((G * max_seqlen_q + kFpvTile - 1) / kFpvTile);
    const long long by_total = (B < total_q ? B : total_q) + G * total_q / kFpvTile;
    return skv_auto_splits_of_tiles(Hkv * (by_max < by_total ? by_max : by_total), Skv, D, num_cus);
}

extern "C" int qattn_fp8_attention_paged_varlen_forward(const void* q16, const long long* q_strides2, int in_fmt, const void* k_pool,
                                                        const void* v_pool, const int* block_table, long long table_stride, int num_pages,
                                                        int page_size, int max_pages, const float* scale_k, const float* scale_v, void* out,
                                                        float* lse, const int* cu_seqlens_q, const int* seqused_k, int B, int Hq, int Hkv,
                                                        int total_q, int max_seqlen_q, int Skv, int D, int fp8_fmt, int numerics, int is_causal,
                                                        float sm_scale, int precision, int num_splits, void* q8, float* scale_q,
                                                        unsigned char* row_path, float* partial_o, float* partial_lse,
                                                        unsigned char* partial_path, void* workspace, size_t workspace_bytes, void* stream) {
    return pvq_forward<false>(q16, q_strides2, in_fmt, k_pool, v_pool, block_table, table_stride, num_pages, page_size, max_pages, scale_k, scale_v,
                              out, lse, cu_seqlens_q, seqused_k, B, Hq, Hkv, total_q, max_seqlen_q, Skv, D, fp8_fmt, numerics, is_causal, -1, -1,
                              sm_scale, precision, num_splits, q8, scale_q, row_path, partial_o, partial_lse, partial_path, workspace,
                              workspace_bytes, stream);
}

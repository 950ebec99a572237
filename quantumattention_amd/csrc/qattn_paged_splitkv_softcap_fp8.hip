// qattn_paged_splitkv_softcap_fp8.hip -- qattn_fp8_attention_paged_splitkv_softcap_forward (include/qattn_softcap.h): the paged split-KV
// window entry with the scaled scores soft-capped, y = softcap tanh(x / softcap), before the mask and the softmax.
//
// qattn_paged_splitkv_window_fp8.hip with QATTN_SKV_SOFTCAP on: the same paging checks, the same page walk, and skv_forward with WINDOW =
// SOFTCAP = true.
#include "qattn_splitkv_attn.h"
#include "../../include/qattn_paged.h"

using namespace qattn;

extern "C" int qattn_fp8_attention_paged_splitkv_softcap_forward(const void* q16, int in_fmt, const void* k_pool, const void* v_pool,
                                                                 const int* block_table, long long table_stride, int num_pages,
                                                                 int page_size, int max_pages, const float* scale_k, const float* scale_v,
                                                                 void* out, float* lse, const int* seqused_k, int B, int Hq, int Hkv, int Sq,
                                                                 int Skv, int D, int fp8_fmt, int numerics, int window_left, int window_right,
                                                                 float softcap, float sm_scale, int precision, int num_splits, void* q8,
                                                                 float* scale_q, unsigned char* row_path, float* partial_o,
                                                                 float* partial_lse, unsigned char* partial_path, void* workspace,
                                                                 size_t workspace_bytes, void* stream) {
    // the cap first, then the paging arguments (include/qattn_paged.h); everything else is checked by skv_forward, still before any device call
    if (!skv_softcap_ok(softcap)) return QATTN_ERR_INVALID_ARG;
    if (!block_table || !seqused_k || (size_t)block_table % 4 != 0) return QATTN_ERR_INVALID_ARG;
    if (num_pages <= 0 || max_pages <= 0 || Hkv <= 0 || page_size < 64 || page_size % 64 != 0) return QATTN_ERR_INVALID_ARG;
    if (table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    const int pc = page_size / 64;
    if ((long long)num_pages * Hkv * pc > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (the physical chunk index is an int)
    if ((long long)Skv > (long long)max_pages * page_size) return QATTN_ERR_INVALID_ARG;
    SkvPages pg;
    pg.table = block_table; pg.stride = (long)table_stride; pg.num_pages = num_pages; pg.pc = pc;
    return skv_forward<true, true, false, true>(q16, in_fmt, k_pool, v_pool, pg, scale_k, scale_v, out, lse, seqused_k, B, Hq, Hkv, Sq, Skv, D,
                                                fp8_fmt, numerics, 0, sm_scale, precision, num_splits, q8, scale_q, row_path, partial_o,
                                                partial_lse, partial_path, workspace, workspace_bytes, stream, window_left, window_right, nullptr,
                                                softcap);
}

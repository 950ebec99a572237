// qattn_paged_splitkv_fp8.hip -- qattn_fp8_attention_paged_splitkv_forward (include/qattn_paged.h): the split-KV entry over a pool of
// fixed-size pages behind a block table.
//
// The kernel is qattn_splitkv_attn.h's body with PAGED = true, the host driver that header's skv_forward: the quant pre-pass of q, the
// split plan, the masks, the partial buffers, the merge chain and the path launch are the contiguous entry's, unchanged.  What differs is
// the chunk a step fetches: logical chunk c of (b, hkv) is chunk c % pc of page clamp(table[b][c / pc], 0, num_pages - 1), pc = page_size /
// 64 -- physical chunk (page Hkv + hkv) pc + c % pc of the pool, handed to FpvRing::dma_chunk whose base is the pool itself.  A fetched
// chunk stays one contiguous 64 D-byte block, so the DMA pieces, the LDS images and everything behind them are the same.  The table index
// is workgroup-uniform: one dword load per PAGE the sweep enters, issued a step ahead of the DMA that needs its value; page and
// chunk-in-page are counters, so no step divides (qattn_splitkv_body.h; what the divisions cost: DESIGN.md section 4.19).
#include "qattn_splitkv_attn.h"
#include "../../include/qattn_paged.h"

using namespace qattn;

extern "C" size_t qattn_fp8_attention_paged_splitkv_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Skv, int D, int num_splits) {
    return qattn_fp8_attention_splitkv_workspace_bytes(B, Hq, Hkv, Sq, Skv, D, num_splits);
}

extern "C" int qattn_fp8_attention_paged_splitkv_forward(const void* q16, int in_fmt, const void* k_pool, const void* v_pool,
                                                         const int* block_table, long long table_stride, int num_pages, int page_size,
                                                         int max_pages, const float* scale_k, const float* scale_v, void* out, float* lse,
                                                         const int* seqused_k, int B, int Hq, int Hkv, int Sq, int Skv, int D, int fp8_fmt,
                                                         int numerics, int is_causal, float sm_scale, int precision, int num_splits, void* q8,
                                                         float* scale_q, unsigned char* row_path, float* partial_o, float* partial_lse,
                                                         unsigned char* partial_path, void* workspace, size_t workspace_bytes, void* stream) {
    // the paging arguments (include/qattn_paged.h); everything else is checked by skv_forward, still before any device call
    if (!block_table || !seqused_k || (size_t)block_table % 4 != 0) return QATTN_ERR_INVALID_ARG;
    if (num_pages <= 0 || max_pages <= 0 || Hkv <= 0 || page_size < 64 || page_size % 64 != 0) return QATTN_ERR_INVALID_ARG;
    if (table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    const int pc = page_size / 64;
    if ((long long)num_pages * Hkv * pc > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (the physical chunk index is an int)
    if ((long long)Skv > (long long)max_pages * page_size) return QATTN_ERR_INVALID_ARG;
    SkvPages pg;
    pg.table = block_table; pg.stride = (long)table_stride; pg.num_pages = num_pages; pg.pc = pc;
    return skv_forward<true>(q16, in_fmt, k_pool, v_pool, pg, scale_k, scale_v, out, lse, seqused_k, B, Hq, Hkv, Sq, Skv, D, fp8_fmt, numerics,
                             is_causal, sm_scale, precision, num_splits, q8, scale_q, row_path, partial_o, partial_lse, partial_path, workspace,
                             workspace_bytes, stream);
}

// qattn_paged_append.hip -- qattn_paged_kv_cache_append_fp8 (include/qattn_paged.h): appending tokens to a PAGED FP8 K/V cache, gfx950.
//
// The kernel is qattn_kvcache_append.h's body with PAGED = true: the contiguous append's tile, quantiser, staging images and store schemes,
// with one difference -- the address of the workgroup's chunk (`og`): chunk c of the sequence is chunk c % pc of page
// clamp(table[b][c / pc], 0, num_pages - 1), pc = page_size / 64.  The advance launch is the contiguous entry's, on capacity =
// max_pages page_size.
#include "qattn_kvcache_append.h"
#include "../../include/qattn_paged.h"

using namespace qattn;

extern "C" int qattn_paged_kv_cache_append_fp8(const void* k16, const void* v16, int in_fmt, const long long* k_strides3,
                                               const long long* v_strides3, void* k_pool, void* v_pool, const float* scale_k,
                                               const float* scale_v, const int* block_table, long long table_stride, int* seqlens,
                                               const int* new_lens, int advance, int B, int Hkv, int T, int num_pages, int page_size,
                                               int max_pages, int D, int fp8_fmt, void* stream) {
    // the paging arguments (include/qattn_paged.h); everything else is checked by kv_append, still before any device call
    if (!block_table || (size_t)block_table % 4 != 0) return QATTN_ERR_INVALID_ARG;
    if (num_pages <= 0 || max_pages <= 0 || Hkv <= 0 || page_size < 64 || page_size % 64 != 0) return QATTN_ERR_INVALID_ARG;
    if (table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    const int pc = page_size / 64;
    if ((long long)num_pages * Hkv * pc > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (the physical chunk index is an int)
    const long long capacity = (long long)max_pages * page_size;
    if (capacity > 0x7fffffffLL - 64) return QATTN_ERR_INVALID_ARG;
    KvPages pg;
    pg.table = block_table; pg.stride = (long)table_stride; pg.num_pages = num_pages; pg.pc = pc;
    return kv_append<true>(k16, v16, in_fmt, k_strides3, v_strides3, k_pool, v_pool, pg, scale_k, scale_v, seqlens, new_lens, advance, B, Hkv, T,
                           (int)capacity, D, fp8_fmt, stream);
}

// qattn_mla_index_append.hip -- qattn_paged_mla_index_cache_append_fp8 (include/qattn_mla_index.h): appending index keys to the row-major
// paged FP8 index-key cache of the lightning indexer, gfx950.
//
// The body of csrc/qattn_mla_row_append.hip on 128-channel rows in a unit of its own (that unit's device code stays as it is): a thread owns
// one 16-channel piece of one token -- two 16-byte loads of the 16-bit row, the cache quantiser quant8 and ONE 16-byte store at
// (page page_size + key % page_size) 128 + 16 piece.
#include "qattn_kvcache_append.h"
#include "../../include/qattn_mla_index.h"

using namespace qattn;

namespace {

constexpr int kIdxD = QATTN_MLA_INDEX_D, kIdxPieces = kIdxD / 16;

struct MlaIndexAppendArgs {
    const uint4* k;       // rows of 128 16-bit channels
    long kb, kt;          // batch / token strides in 16-byte vectors
    unsigned char* pool;
    const float* scale;   // [B]
    const int* table;
    long tstride;
    int* seqlens;
    const int* new_lens;
    int T, capacity, num_pages, page_size;
};

// grid = (ceil(T 8 / 256), B), block = 256: thread -> (token t, piece)
template <int IN_FMT, int OUT_FMT>
__global__ __launch_bounds__(256) void mla_index_append_kernel(const MlaIndexAppendArgs a) {
    const int b = blockIdx.y;
    const int u = blockIdx.x * 256 + threadIdx.x;
    const int t = u / kIdxPieces, piece = u % kIdxPieces;
    int p, end;
    kv_append_range(a.seqlens, a.new_lens, b, a.T, a.capacity, p, end);
    if (t >= a.T || t >= end - p) return;   // not a token of the call, or dropped at the capacity
    const int key = p + t;                  // < end <= capacity
    const uint4* src = a.k + (long)b * a.kb + (long)t * a.kt + 2 * piece;
    const uint4 x0 = load_nt(src), x1 = load_nt(src + 1);
    const float scale = a.scale[b];
    const float rinv = 1.0f / scale;
    const int2 lo = quant8<IN_FMT, OUT_FMT>(x0, scale, rinv, has_nonfinite16<IN_FMT>(x0));   // NaN stays NaN, +-inf clamps to +-qmax
    const int2 hi = quant8<IN_FMT, OUT_FMT>(x1, scale, rinv, has_nonfinite16<IN_FMT>(x1));
    // the entry read is one of the pages that cover [p, end); its clamp keeps the row inside the pool whatever the table holds
    int page = a.table[(long)b * a.tstride + key / a.page_size];
    page = page < 0 ? 0 : page > a.num_pages - 1 ? a.num_pages - 1 : page;
    unsigned char* og = a.pool + ((long)page * a.page_size + key % a.page_size) * (long)kIdxD;
    *reinterpret_cast<int4*>(og + 16 * piece) = make_int4(lo.x, lo.y, hi.x, hi.y);
}

}  // namespace

extern "C" size_t qattn_mla_index_pool_bytes(int num_pages, int page_size) {
    if (num_pages <= 0 || page_size <= 0 || (long long)num_pages * page_size > 0x7fffffffLL) return 0;
    return (size_t)num_pages * (size_t)page_size * kIdxD;
}

extern "C" int qattn_paged_mla_index_cache_append_fp8(const void* k16, int in_fmt, const long long* k_strides2, void* pool, const float* scale,
                                                      const int* block_table, long long table_stride, int* seqlens, const int* new_lens,
                                                      int advance, int B, int T, int num_pages, int page_size, int max_pages, int fp8_fmt,
                                                      void* stream) {
    if (!k16 || !k_strides2 || !pool || !scale || !block_table || !seqlens) return QATTN_ERR_INVALID_ARG;
    if ((size_t)block_table % 4 != 0 || ((size_t)pool | (size_t)k16) % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || T <= 0 || num_pages <= 0 || max_pages <= 0 || page_size <= 0) return QATTN_ERR_INVALID_ARG;
    if (table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    if ((long long)num_pages * page_size > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (the physical row number is an int)
    const long long capacity = (long long)max_pages * page_size;
    if (capacity > 0x7fffffffLL - 64) return QATTN_ERR_INVALID_ARG;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    for (int i = 0; i < 2; i++)   // (a negative stride would read in front of the base pointer)
        if (k_strides2[i] < 0 || k_strides2[i] % 8 != 0) return QATTN_ERR_INVALID_ARG;
    const long long blocks = ((long long)T * kIdxPieces + 255) / 256;
    if (blocks > 0x7fffffffLL || B > 65535) return QATTN_ERR_INVALID_ARG;
    MlaIndexAppendArgs a;
    a.k = (const uint4*)k16;
    a.kb = (long)(k_strides2[0] / 8); a.kt = (long)(k_strides2[1] / 8);
    a.pool = (unsigned char*)pool; a.scale = scale; a.table = block_table; a.tstride = (long)table_stride;
    a.seqlens = seqlens; a.new_lens = new_lens;
    a.T = T; a.capacity = (int)capacity; a.num_pages = num_pages; a.page_size = page_size;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)blocks, (unsigned)B, 1), block(256);
    if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E4M3) hipLaunchKernelGGL((mla_index_append_kernel<QATTN_FMT_BF16, QATTN_FMT_E4M3>), grid, block, 0, st, a);
    else if (in_fmt == QATTN_FMT_BF16) hipLaunchKernelGGL((mla_index_append_kernel<QATTN_FMT_BF16, QATTN_FMT_E5M2>), grid, block, 0, st, a);
    else if (fp8_fmt == QATTN_FMT_E4M3) hipLaunchKernelGGL((mla_index_append_kernel<QATTN_FMT_FP16, QATTN_FMT_E4M3>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((mla_index_append_kernel<QATTN_FMT_FP16, QATTN_FMT_E5M2>), grid, block, 0, st, a);
    if (advance) kv_launch_advance(seqlens, new_lens, B, T, (int)capacity, st);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

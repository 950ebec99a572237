// qattn_paged_varlen_append.hip -- qattn_paged_kv_cache_append_varlen_fp8 (include/qattn_paged_varlen_append.h): appending PACKED tokens
// [total, Hkv, D], a count per sequence slot under cu_seqlens, to a paged FP8 K/V cache, gfx950.
//
// The kernel is a third compilation of qattn_kvcache_append_body.h (QATTN_KVA_PAGED and QATTN_KVA_VARQ on): the paged append's tile,
// quantiser, staging images, store schemes and table lookup, with two differences -- which (sequence, chunk) a workgroup serves (a binary
// search on cu_seqlens instead of a division by the padded chunk count) and the row its tokens start at (start_i instead of b T).  The
// advance is a kernel of this unit: kv_launch_advance (qattn_kvcache_append.hip) takes new_lens and stays as it is.
#include "qattn_kvcache_append.h"
#include "../../include/qattn_paged_varlen_append.h"

namespace qattn {

// grid = (Hkv NS, 2), block = 256.  blockIdx.y: 0 = K, 1 = V.  blockIdx.x = h NS + j: chunk slot j of kv head h.
template <int D, int IN_FMT, int OUT_FMT>
__global__ __launch_bounds__(256) void kv_paged_varlen_append_kernel(const KvAppendArgs a, const KvPages pg, const KvVarq vq) {
#define QATTN_KVA_PAGED 1
#define QATTN_KVA_VARQ 1
#include "qattn_kvcache_append_body.h"
#undef QATTN_KVA_VARQ
#undef QATTN_KVA_PAGED
}

// the second launch of an advancing call (stream order puts it behind every workgroup that had to read the old positions):
// kv_advance_kernel on the counts of cu_seqlens
__global__ __launch_bounds__(256) void kv_varlen_advance_kernel(int* seqlens, const int* cu, int B, int total, int capacity) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int start = kv_clampi(cu[b], 0, total);
    const int n = kv_clampi(cu[b + 1], start, total) - start;
    const int p = kv_clampi(seqlens[b], 0, capacity);
    seqlens[b] = capacity - p >= n ? p + n : capacity;
}

template <int D>
static int launch_kv_varlen_append(const KvAppendArgs& a, const KvPages& pg, const KvVarq& vq, int in_fmt, int fp8_fmt, dim3 grid, hipStream_t st) {
    dim3 block(256);
    if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E4M3)
        hipLaunchKernelGGL((kv_paged_varlen_append_kernel<D, QATTN_FMT_BF16, QATTN_FMT_E4M3>), grid, block, 0, st, a, pg, vq);
    else if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E5M2)
        hipLaunchKernelGGL((kv_paged_varlen_append_kernel<D, QATTN_FMT_BF16, QATTN_FMT_E5M2>), grid, block, 0, st, a, pg, vq);
    else if (in_fmt == QATTN_FMT_FP16 && fp8_fmt == QATTN_FMT_E4M3)
        hipLaunchKernelGGL((kv_paged_varlen_append_kernel<D, QATTN_FMT_FP16, QATTN_FMT_E4M3>), grid, block, 0, st, a, pg, vq);
    else if (in_fmt == QATTN_FMT_FP16 && fp8_fmt == QATTN_FMT_E5M2)
        hipLaunchKernelGGL((kv_paged_varlen_append_kernel<D, QATTN_FMT_FP16, QATTN_FMT_E5M2>), grid, block, 0, st, a, pg, vq);
    else return QATTN_ERR_UNSUPPORTED_FMT;
    return QATTN_OK;
}

}  // namespace qattn

using namespace qattn;

extern "C" int qattn_paged_kv_cache_append_varlen_fp8(const void* k16, const void* v16, int in_fmt, const long long* k_strides2,
                                                      const long long* v_strides2, void* k_pool, void* v_pool, const float* scale_k,
                                                      const float* scale_v, const int* block_table, long long table_stride, int* seqlens,
                                                      const int* cu_seqlens, int advance, int B, int Hkv, int total, int num_pages,
                                                      int page_size, int max_pages, int D, int fp8_fmt, void* stream) {
    // the paging arguments, as qattn_paged_kv_cache_append_fp8 checks them
    if (!block_table || (size_t)block_table % 4 != 0) return QATTN_ERR_INVALID_ARG;
    if (num_pages <= 0 || max_pages <= 0 || Hkv <= 0 || page_size < 64 || page_size % 64 != 0) return QATTN_ERR_INVALID_ARG;
    if (table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    const int pc = page_size / 64;
    if ((long long)num_pages * Hkv * pc > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (the physical chunk index is an int)
    const long long capacity = (long long)max_pages * page_size;
    if (capacity > 0x7fffffffLL - 64) return QATTN_ERR_INVALID_ARG;   // (p_i + n_i stays in 32 bits)
    // the packed arguments
    if (!cu_seqlens || (size_t)cu_seqlens % 4 != 0) return QATTN_ERR_INVALID_ARG;
    if (total < 0) return QATTN_ERR_INVALID_ARG;
    // kv_append's checks (qattn_kvcache_append.h), T > 0 excepted
    if (!k16 || !v16 || !k_strides2 || !v_strides2 || !k_pool || !v_pool || !scale_k || !scale_v || !seqlens) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || D <= 0) return QATTN_ERR_INVALID_ARG;
    if (D != 64 && D != 128 && D != 256) return QATTN_ERR_UNSUPPORTED_DIM;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (((size_t)k_pool | (size_t)v_pool) % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if (((size_t)k16 | (size_t)v16) % 16 != 0) return QATTN_ERR_INVALID_ARG;   // rows: 16-byte loads
    for (int i = 0; i < 2; i++)   // (a negative stride would read in front of the base pointer)
        if (k_strides2[i] < 0 || v_strides2[i] < 0 || k_strides2[i] % 8 != 0 || v_strides2[i] % 8 != 0) return QATTN_ERR_INVALID_ARG;
    const long long NS = 2LL * B + total / 64;   // chunk slots per kv head
    if (NS * Hkv > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (one workgroup per (kv head, slot): a 32-bit grid; NS itself an int)
    if (total == 0) return QATTN_OK;   // nothing launched, nothing written
    KvAppendArgs a;
    a.x[0] = (const uint4*)k16; a.x[1] = (const uint4*)v16;
    a.img[0] = (unsigned char*)k_pool; a.img[1] = (unsigned char*)v_pool;
    a.scale[0] = scale_k; a.scale[1] = scale_v;
    a.sb[0] = a.sb[1] = 0;   // (no batch axis: the sequence's rows start at start_i)
    a.st[0] = (long)(k_strides2[0] / 8); a.sh[0] = (long)(k_strides2[1] / 8);
    a.st[1] = (long)(v_strides2[0] / 8); a.sh[1] = (long)(v_strides2[1] / 8);
    a.seqlens = seqlens; a.new_lens = nullptr;
    a.Hkv = Hkv; a.T = total; a.capacity = (int)capacity; a.nchunk = (int)NS;
    KvPages pg;
    pg.table = block_table; pg.stride = (long)table_stride; pg.num_pages = num_pages; pg.pc = pc;
    KvVarq vq;
    vq.cu = cu_seqlens; vq.B = B; vq.total = total; vq.NS = (int)NS;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)(NS * Hkv), 2, 1);
    int rc;
    if (D == 64) rc = launch_kv_varlen_append<64>(a, pg, vq, in_fmt, fp8_fmt, grid, st);
    else if (D == 128) rc = launch_kv_varlen_append<128>(a, pg, vq, in_fmt, fp8_fmt, grid, st);
    else rc = launch_kv_varlen_append<256>(a, pg, vq, in_fmt, fp8_fmt, grid, st);
    if (rc != QATTN_OK) return rc;
    if (advance)
        hipLaunchKernelGGL(kv_varlen_advance_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, seqlens, cu_seqlens, B, total,
                           (int)capacity);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

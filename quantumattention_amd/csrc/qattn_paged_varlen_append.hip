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
#define QATTN_KVA_ROPE 0
#include "qattn_kvcache_append_body.h"
#undef QATTN_KVA_ROPE
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

void kv_launch_varlen_advance(int* seqlens, const int* cu, int B, int total, int capacity, hipStream_t st) {
    hipLaunchKernelGGL(kv_varlen_advance_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, seqlens, cu, B, total, capacity);
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
    KvAppendArgs a;
    KvPages pg;
    KvVarq vq;
    const int ok = kv_varlen_append_args(k16, v16, in_fmt, k_strides2, v_strides2, k_pool, v_pool, scale_k, scale_v, block_table, table_stride, seqlens,
                                         cu_seqlens, B, Hkv, total, num_pages, page_size, max_pages, D, fp8_fmt, a, pg, vq);
    if (ok != QATTN_OK) return ok;
    if (total == 0) return QATTN_OK;   // nothing launched, nothing written
    const long long NS = vq.NS, capacity = a.capacity;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)(NS * Hkv), 2, 1);
    int rc;
    if (D == 64) rc = launch_kv_varlen_append<64>(a, pg, vq, in_fmt, fp8_fmt, grid, st);
    else if (D == 128) rc = launch_kv_varlen_append<128>(a, pg, vq, in_fmt, fp8_fmt, grid, st);
    else rc = launch_kv_varlen_append<256>(a, pg, vq, in_fmt, fp8_fmt, grid, st);
    if (rc != QATTN_OK) return rc;
    if (advance) kv_launch_varlen_advance(seqlens, cu_seqlens, B, total, (int)capacity, st);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

// qattn_kvcache_append.hip -- appending tokens to an FP8 K/V cache with fixed scales (include/qattn_kvcache.h), gfx950.
//
// quant_multi_kernel's tile (qattn_quant.hip) with three differences: the scale is the cache's, not the tensor's abs-max; the first key is
// read from seqlens on the device, so the tokens of a call do not start at a chunk boundary; and a chunk that the call covers only in
// part is stored key by key, because the bytes of the keys that are already there must not change.  quant8, the LDS staging images and the
// copy-out of a whole chunk (vfrag_copy_out) are qattn_common.h's.
// The kernel and the host driver are qattn_kvcache_append.h's (shared with the paged entry, qattn_paged_append.hip); this unit
// instantiates the contiguous kernels and holds the advance launch both entries use.
#include "qattn_kvcache_append.h"

namespace qattn {

// the second launch of an advancing call: stream order puts it behind every workgroup that had to read the old positions
__global__ __launch_bounds__(256) void kv_advance_kernel(int* seqlens, const int* new_lens, int B, int T, int capacity) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int p, end;
    kv_append_range(seqlens, new_lens, b, T, capacity, p, end);
    seqlens[b] = end;
}

void kv_launch_advance(int* seqlens, const int* new_lens, int B, int T, int capacity, hipStream_t st) {
    hipLaunchKernelGGL(kv_advance_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, seqlens, new_lens, B, T, capacity);
}

}  // namespace qattn

using namespace qattn;

extern "C" int qattn_kv_cache_append_fp8(const void* k16, const void* v16, int in_fmt, const long long* k_strides3, const long long* v_strides3,
                                         void* k8_kfrag, void* v8_vfrag, const float* scale_k, const float* scale_v, int* seqlens,
                                         const int* new_lens, int advance, int B, int Hkv, int T, int capacity, int D, int fp8_fmt, void* stream) {
    return kv_append<false>(k16, v16, in_fmt, k_strides3, v_strides3, k8_kfrag, v8_vfrag, KvPages{}, scale_k, scale_v, seqlens, new_lens, advance, B,
                            Hkv, T, capacity, D, fp8_fmt, stream);
}

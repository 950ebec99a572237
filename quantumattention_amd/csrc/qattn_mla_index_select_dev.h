// qattn_mla_index_select_dev.h -- what the two selection units of the lightning indexer share on the device (qattn_mla_index_select.hip: one
// workgroup per row; qattn_mla_index_select_split.hip: a row cut across workgroups): the order-preserving key of a logit and the histogram
// increment that does not serialise on rows of equal values.
#pragma once
#include <hip/hip_runtime.h>

namespace qattn {

__device__ __forceinline__ unsigned order_key(float f) {
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = 0xff800000u;   // a NaN ranks as -inf
    if (u == 0x80000000u) u = 0u;                           // -0.0 equals +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// one count per participating lane; the lanes that share the leading lane's digit go in with one atomic
__device__ __forceinline__ void hist_add(unsigned* hist, bool on, unsigned digit, int lane) {
    const unsigned long long act = __ballot(on);
    if (act == 0ull) return;   // (wave-uniform)
    const int first = __builtin_ctzll(act);
    const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)digit, first);
    const bool same = on && digit == d0;
    const unsigned long long m = __ballot(same);
    if (lane == first) atomicAdd(&hist[d0], (unsigned)__builtin_popcountll(m));
    if (on && !same) atomicAdd(&hist[digit], 1u);
}

}  // namespace qattn

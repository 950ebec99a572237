// qattn_smooth_dev.h -- device helpers of key smoothing shared by the dense unit (qattn_smooth_k.hip) and the packed variable-length unit
// (qattn_varlen_smooth.hip): the row walk and register sums of the mean pass, and the fp32-input quantiser.  One definition of each, so
// that "the sums and bytes of the dense smoothing entry on that sequence alone" is a statement about the same code.
#pragma once
#include "qattn_common.h"

namespace qattn {

template <int IN_FMT>
__device__ __forceinline__ void unpack8(const uint4& raw, float (&f)[8]) {
    const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (IN_FMT == QATTN_FMT_BF16) {
            f[2 * i] = __uint_as_float(w[i] << 16);
            f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        } else {
            typedef _Float16 h2 __attribute__((ext_vector_type(2)));
            h2 x;
            __builtin_memcpy(&x, &w[i], 4);
            f[2 * i] = (float)x[0];
            f[2 * i + 1] = (float)x[1];
        }
    }
}

// The rows of a head are dealt to `nblk` blocks in contiguous shares of `per` rows, `per` a multiple of the 256 / VPR rows that the block's
// threads cover per step: thread tid reads 16-byte piece tid % VPR (channels 8 (tid % VPR) .. +7) of rows first + tid / VPR + n 256 / VPR.
template <int D>
__device__ __forceinline__ int rows_per_block(int S, int nblk) {
    constexpr int RPI = 256 / (D / 8);
    return ((S + nblk - 1) / nblk + RPI - 1) / RPI * RPI;
}

// walk a block's share of rows with kAmaxInFlight loads in flight per thread
template <int D, bool SV, typename F>
__device__ __forceinline__ void for_my_rows(const uint4* xg, long row_vecs, int first, int last, F&& fold) {
    constexpr int VPR = D / 8, RPI = 256 / VPR;
    const int dv = threadIdx.x % VPR;
    int r = first + (int)threadIdx.x / VPR;
    auto at = [&](int row) { return xg + (SV ? (long)row * row_vecs : (long)row * VPR) + dv; };
    for (; r + (kAmaxInFlight - 1) * RPI < last; r += kAmaxInFlight * RPI) {
        uint4 v[kAmaxInFlight];
#pragma unroll
        for (int u = 0; u < kAmaxInFlight; u++) v[u] = load_nt(at(r + u * RPI));
#pragma unroll
        for (int u = 0; u < kAmaxInFlight; u++) fold(v[u]);
    }
    for (; r < last; r += RPI) fold(load_nt(at(r)));
}

__device__ __forceinline__ void load_mean8(const float* mean, float (&m)[8]) {
    const float4 a = reinterpret_cast<const float4*>(mean)[0], b = reinterpret_cast<const float4*>(mean)[1];
    m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w; m[4] = b.x; m[5] = b.y; m[6] = b.z; m[7] = b.w;
}

// ---- 8 fp32 values -> 8 fp8 bytes, bit-exact to  fp8(clamp(round16(x / scale), +-qmax))  (quant8 of qattn_common.h on fp32 inputs).
template <int IN_FMT, int OUT_FMT>
__device__ __attribute__((noinline)) int2 quant8_f32_exact(const float4 lo, const float4 hi, float scale) {
    const float qmax = OUT_FMT == QATTN_FMT_E4M3 ? 448.0f : 57344.0f;
    const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    float q[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        float t = round16<IN_FMT>(x[j] / scale);   // IEEE fp32 divide, then the rounding to the input dtype
        t = t > qmax ? qmax : t;
        t = t < -qmax ? -qmax : t;
        q[j] = t;
    }
    return make_int2(cvt4_fp8<OUT_FMT>(q[0], q[1], q[2], q[3]), cvt4_fp8<OUT_FMT>(q[4], q[5], q[6], q[7]));
}

template <int IN_FMT, int OUT_FMT>
__device__ __forceinline__ int2 quant8_f32(const float (&x)[8], float scale, float rinv) {
    const float4 xlo = make_float4(x[0], x[1], x[2], x[3]), xhi = make_float4(x[4], x[5], x[6], x[7]);
    // fp16: the exact sequence (the fast form of quant8_f16_fast leans on its exhaustive check over all fp16 inputs, which fp32 inputs have not)
    if (IN_FMT != QATTN_FMT_BF16) return quant8_f32_exact<IN_FMT, OUT_FMT>(xlo, xhi, scale);
    // bf16: quant8's fast path from the product on -- x * rinv is within 3 fp32 ulps of RNE(x / scale) for every fp32 x (rinv = RNE(1 / scale)
    // of a normal scale), both round to the same bf16 unless the product lies within 4 ulps of a bf16 tie; those vectors, and a
    // non-finite scale (which a non-finite ks implies), take the exact sequence.
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    typedef short s2 __attribute__((ext_vector_type(2)));
    const unsigned qbits = OUT_FMT == QATTN_FMT_E4M3 ? 0x43e043e0u : 0x47604760u;   // bf16(448) / bf16(57344), both halves
    const unsigned tie = 0x80048004u;
    u16x2 pq, ptie, pnear = {0xffff, 0xffff};
    __builtin_memcpy(&pq, &qbits, 4);
    __builtin_memcpy(&ptie, &tie, 4);
    b2 cl[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const f2 q = f2{x[2 * i], x[2 * i + 1]} * rinv;
        const unsigned lows = __builtin_amdgcn_perm(__float_as_uint(q.y), __float_as_uint(q.x), 0x05040100u);
        u16x2 pl;
        __builtin_memcpy(&pl, &lows, 4);
        pnear = __builtin_elementwise_min(pnear, (u16x2)(pl + ptie));
        const b2 h = __builtin_convertvector(q, b2);  // v_cvt_pk_bf16_f32: RNE
        unsigned u;
        __builtin_memcpy(&u, &h, 4);
        unsigned mag = u & 0x7fff7fffu;
        u16x2 pm;
        __builtin_memcpy(&pm, &mag, 4);
        pm = __builtin_elementwise_min(pm, pq);
        __builtin_memcpy(&mag, &pm, 4);
        const unsigned c = mag | (u & 0x80008000u);
        __builtin_memcpy(&cl[i], &c, 4);
    }
    const unsigned near = min((unsigned)pnear.x, (unsigned)pnear.y);
    const bool slow = near < 9u || !((__float_as_uint(scale) & 0x7f800000u) != 0x7f800000u);
    if (__builtin_expect(slow, 0)) return quant8_f32_exact<IN_FMT, OUT_FMT>(xlo, xhi, scale);
    s2 lo = {0, 0}, hi = {0, 0};
    if (OUT_FMT == QATTN_FMT_E4M3) {
        lo = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(lo, cl[0], 1.0f, false);
        lo = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(lo, cl[1], 1.0f, true);
        hi = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(hi, cl[2], 1.0f, false);
        hi = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(hi, cl[3], 1.0f, true);
    } else {
        lo = __builtin_amdgcn_cvt_scalef32_pk_bf8_bf16(lo, cl[0], 1.0f, false);
        lo = __builtin_amdgcn_cvt_scalef32_pk_bf8_bf16(lo, cl[1], 1.0f, true);
        hi = __builtin_amdgcn_cvt_scalef32_pk_bf8_bf16(hi, cl[2], 1.0f, false);
        hi = __builtin_amdgcn_cvt_scalef32_pk_bf8_bf16(hi, cl[3], 1.0f, true);
    }
    int2 r;
    __builtin_memcpy(&r.x, &lo, 4);
    __builtin_memcpy(&r.y, &hi, 4);
    return r;
}

// blocks per head of the mean pass: a pure integer function of (rows, head dim), evaluated on the host for a dense head and on the device
// per packed sequence
__host__ __device__ inline int mean_splits(int Skv, int D) {
    const int s = amax_splits(Skv, Skv, D);
    return s > kMeanSplits ? kMeanSplits : s;
}

}  // namespace qattn

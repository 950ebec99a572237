// qattn_rope_dev.h -- the rotation of the RoPE contract (include/qattn_rope.h; quantumattention_amd/rope.py apply_rope_eager) as device
// functions, shared by the units that rotate values they hold in registers: qattn_rope_quant.hip (the dense quant pre-pass) and
// qattn_paged_varlen_rope_append.hip (the packed append to the paged cache, and the packed rotation at the cache's positions).
//
// Work unit: the two 16-byte pieces dvh and dvh + D/16 of one row (dvh < D/16), in ONE thread.
//   interleaved = 0   pairs (i, i + D/2): element j of the first piece rotates with element j of the second; the unit needs the
//                     table entries 8 dvh .. 8 dvh + 7 (the float4 2 dvh and 2 dvh + 1 of the cos row, the same of the sin row)
//   interleaved = 1   pairs (2i, 2i + 1) lie inside a piece; piece dv needs the entries 4 dv .. 4 dv + 3 (the float4 dvh and dvh + D/16)
// Either way a unit reads 32 bytes of data and 64 bytes of tables, and no value crosses lanes.
#pragma once
#include "qattn_common.h"

namespace qattn {

// the rotation of one pair, as the contract states it: three separately rounded fp32 operations (no contraction)
__device__ __forceinline__ void rot(float a, float b, float c, float s, float& y0, float& y1) {
    y0 = __fsub_rn(__fmul_rn(a, c), __fmul_rn(b, s));
    y1 = __fadd_rn(__fmul_rn(b, c), __fmul_rn(a, s));
}

// 8 floats -> 8 values of the input dtype, round to nearest even (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32)
template <int IN_FMT>
__device__ __forceinline__ uint4 pack16x8(const float (&f)[8]) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const f2 v = {f[2 * i], f[2 * i + 1]};
        if (IN_FMT == QATTN_FMT_BF16) {
            const b2 h = __builtin_convertvector(v, b2);
            __builtin_memcpy(&w[i], &h, 4);
        } else {
            const h2 h = __builtin_convertvector(v, h2);
            __builtin_memcpy(&w[i], &h, 4);
        }
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// one unit in place: A = piece dvh, B = piece dvh + D/16; c / s: the unit's two float4 of cos / sin (see the head of the file)
template <int IN_FMT, bool IL>
__device__ __forceinline__ void rope_unit(uint4& A, uint4& B, const float4 (&c)[2], const float4 (&s)[2]) {
    unsigned short ea[8], eb[8];
    float cc[8], sv[8], fa[8], fb[8];
    __builtin_memcpy(ea, &A, 16); __builtin_memcpy(eb, &B, 16);
    __builtin_memcpy(cc, c, 32); __builtin_memcpy(sv, s, 32);
    if (!IL) {
#pragma unroll
        for (int j = 0; j < 8; j++) rot(load16f<IN_FMT>(ea[j]), load16f<IN_FMT>(eb[j]), cc[j], sv[j], fa[j], fb[j]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            rot(load16f<IN_FMT>(ea[2 * i]), load16f<IN_FMT>(ea[2 * i + 1]), cc[i], sv[i], fa[2 * i], fa[2 * i + 1]);
            rot(load16f<IN_FMT>(eb[2 * i]), load16f<IN_FMT>(eb[2 * i + 1]), cc[4 + i], sv[4 + i], fb[2 * i], fb[2 * i + 1]);
        }
    }
    A = pack16x8<IN_FMT>(fa);
    B = pack16x8<IN_FMT>(fb);
}

}  // namespace qattn

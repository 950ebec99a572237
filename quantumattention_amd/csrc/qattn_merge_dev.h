// qattn_merge_dev.h -- what the two state-merge units share: qattn_merge.hip (include/qattn_merge.h) and qattn_merge_sink.hip
// (qattn_attention_state_merge_sink, include/qattn_sinks.h).  The kernel's parameter block, the 16-bit pack / unpack helpers, and the host
// side of an entry: the argument checks that fill the block, and the grid.  The kernel body itself is qattn_merge_body.h.
#pragma once
#include <math.h>

#include "qattn_common.h"
#include "../../include/qattn_merge.h"

namespace qattn {

struct MergeParams {
    const void* o[QATTN_MERGE_MAX_PARTIALS];
    const float* lse[QATTN_MERGE_MAX_PARTIALS];
    long long os[QATTN_MERGE_MAX_PARTIALS][3];   // element strides {batch, head, row}
    long long ls[QATTN_MERGE_MAX_PARTIALS][3];
    int fmt[QATTN_MERGE_MAX_PARTIALS];
    void* out;
    float* lse_out;
    long long outs[3], louts[3];
    int out_fmt, S;
};

__device__ inline unsigned short f32_to_bf16_bits(float x) {   // round to nearest even; NaN stays NaN (quiet)
    const unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x0040u);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ inline unsigned short f32_to_fp16_bits(float x) {
    const _Float16 h = (_Float16)x;
    unsigned short b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}
template <int FMT16>
__device__ inline unsigned merge_pack16(float a, float b) {
    if (FMT16 == QATTN_FMT_BF16) return (unsigned)f32_to_bf16_bits(a) | ((unsigned)f32_to_bf16_bits(b) << 16);
    return (unsigned)f32_to_fp16_bits(a) | ((unsigned)f32_to_fp16_bits(b) << 16);
}
template <int FMT16>
__device__ inline void merge_unpack16(const uint4& r, float (&x)[8]) {
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        x[2 * j] = load16f<FMT16>((unsigned short)(w[j] & 0xffffu));
        x[2 * j + 1] = load16f<FMT16>((unsigned short)(w[j] >> 16));
    }
}

static inline int elem_bytes(int fmt) { return fmt == QATTN_FMT_FP32 ? 4 : 2; }
static inline bool merge_fmt_ok(int fmt) { return fmt == QATTN_FMT_BF16 || fmt == QATTN_FMT_FP16 || fmt == QATTN_FMT_FP32; }

// a tensor of rows of `row` elements under strides st[3] over `ext[3]` indices: strides >= 0 and, for an O tensor, base and rows on 16 bytes
static inline bool merge_view_ok(const void* base, const long long* st, const int* ext, int bytes, bool rows16) {
    if ((reinterpret_cast<uintptr_t>(base) & (rows16 ? 15u : 3u)) != 0) return false;
    for (int i = 0; i < 3; i++) {
        if (ext[i] <= 1) continue;
        if (st[i] < 0) return false;
        if (rows16 && (st[i] * bytes) % 16 != 0) return false;
    }
    return true;
}

// what the strides alone show about an OUTPUT: no broadcast, and the dimensions nest -- ordered by stride, each stride covers the span of
// the narrower ones (rows of `row` elements).  Dimensions with one index do not count.
static inline bool merge_output_ok(const long long* st, const int* ext, int row) {
    int order[3], nd = 0;
    for (int i = 0; i < 3; i++)
        if (ext[i] > 1) order[nd++] = i;
    for (int a = 0; a < nd; a++)
        for (int c = a + 1; c < nd; c++)
            if (st[order[c]] < st[order[a]]) { const int t = order[a]; order[a] = order[c]; order[c] = t; }
    long long span = row;   // elements one index of the dimension in hand reaches over
    for (int a = 0; a < nd; a++) {
        const long long s = st[order[a]];
        if (s < span) return false;
        span = s * (ext[order[a]] - 1) + span;
    }
    return true;
}

// The argument checks of a merge entry that takes n_min .. QATTN_MERGE_MAX_PARTIALS partials, in the order include/qattn_merge.h's entry
// always made them; on QATTN_OK `p` is filled in and `grid` is the launch's.
static inline int merge_check_and_fill(int n_min, int n, const void* const* o, const int* o_fmt, const long long* o_strides,
                                       const float* const* lse, const long long* lse_strides, void* out, int out_fmt,
                                       const long long* out_strides, float* lse_out, const long long* lse_out_strides, int B, int H, int S, int D,
                                       MergeParams& p, dim3& grid) {
    if (n < n_min || n > QATTN_MERGE_MAX_PARTIALS) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || H <= 0 || S <= 0 || B > 65535 || H > 65535) return QATTN_ERR_INVALID_ARG;
    if (D != 64 && D != 128 && D != 256) return QATTN_ERR_UNSUPPORTED_DIM;
    if (!o || !o_fmt || !o_strides || !lse || !lse_strides || !out || !out_strides) return QATTN_ERR_INVALID_ARG;
    if (lse_out && !lse_out_strides) return QATTN_ERR_INVALID_ARG;
    if (!merge_fmt_ok(out_fmt)) return QATTN_ERR_UNSUPPORTED_FMT;
    const int ext[3] = {B, H, S};
    p = MergeParams{};
    for (int i = 0; i < n; i++) {
        if (!o[i] || !lse[i]) return QATTN_ERR_INVALID_ARG;
        if (!merge_fmt_ok(o_fmt[i])) return QATTN_ERR_UNSUPPORTED_FMT;
        if (!merge_view_ok(o[i], o_strides + 3 * i, ext, elem_bytes(o_fmt[i]), true)) return QATTN_ERR_INVALID_ARG;
        if (!merge_view_ok(lse[i], lse_strides + 3 * i, ext, 4, false)) return QATTN_ERR_INVALID_ARG;
        p.o[i] = o[i];
        p.lse[i] = lse[i];
        p.fmt[i] = o_fmt[i];
        for (int j = 0; j < 3; j++) {   // (a dimension with one index: its stride is not read, and 0 keeps the offsets in bounds)
            p.os[i][j] = ext[j] > 1 ? o_strides[3 * i + j] : 0;
            p.ls[i][j] = ext[j] > 1 ? lse_strides[3 * i + j] : 0;
        }
    }
    if (!merge_view_ok(out, out_strides, ext, elem_bytes(out_fmt), true) || !merge_output_ok(out_strides, ext, D)) return QATTN_ERR_INVALID_ARG;
    if (lse_out && (!merge_view_ok(lse_out, lse_out_strides, ext, 4, false) || !merge_output_ok(lse_out_strides, ext, 1)))
        return QATTN_ERR_INVALID_ARG;
    p.out = out;
    p.lse_out = lse_out;
    p.out_fmt = out_fmt;
    p.S = S;
    for (int j = 0; j < 3; j++) {
        p.outs[j] = ext[j] > 1 ? out_strides[j] : 0;
        p.louts[j] = (lse_out && ext[j] > 1) ? lse_out_strides[j] : 0;
    }
    const int rows = 256 / (D / 8);
    grid = dim3((unsigned)((S + rows - 1) / rows), (unsigned)H, (unsigned)B);
    return QATTN_OK;
}

}  // namespace qattn

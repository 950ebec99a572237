// qattn_merge.hip -- merging of attention states (include/qattn_merge.h): out = sum_i exp(lse_i - L) O_i, L = log sum_i exp(lse_i), for the
// partial results of one set of queries over disjoint key sets.  One launch, fp32 arithmetic, bandwidth-bound.
//
// Shape: a lane owns 8 consecutive elements of one row -- 16 bytes of a 16-bit tensor, 32 of an fp32 one -- so a row of D elements is D / 8
// neighbouring lanes of ONE wave (8 / 16 / 32) and a wave's request covers whole rows.  256 threads = 32 / 16 / 8 rows of one (b, h); the
// grid is (row tiles, H, B): no division, the batch and head offsets are scalar.  N is a template argument: the N row pieces are N
// independent 16-byte loads in flight per lane before the first use, and every register array is indexed statically (no scratch).  The
// FORMAT of a partial is a launch-uniform runtime branch (not 3^8 instantiations).  No LDS: the N log-sum-exps of a row are read by the
// row's lanes from one address each (a broadcast within the request) and the weights are computed per lane.
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

template <int D, int N>
__global__ __launch_bounds__(256) void merge_states_kernel(const MergeParams p) {
    constexpr int kLanes = D / 8;          // lanes of one row
    constexpr int kRows = 256 / kLanes;    // rows of one workgroup
    const int piece = (int)threadIdx.x % kLanes;
    const long long s = (long long)blockIdx.x * kRows + (int)threadIdx.x / kLanes;
    if (s >= p.S) return;
    const long long b = blockIdx.z, h = blockIdx.y;

    // every load of the row first: N floats and N (fp32: 2 N) 16-byte pieces, none depending on another
    float l[N];
    uint4 ra[N], rb[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        l[i] = p.lse[i][b * p.ls[i][0] + h * p.ls[i][1] + s * p.ls[i][2]];
        const long long e = b * p.os[i][0] + h * p.os[i][1] + s * p.os[i][2] + piece * 8;
        if (p.fmt[i] == QATTN_FMT_FP32) {
            const uint4* src = reinterpret_cast<const uint4*>(static_cast<const float*>(p.o[i]) + e);
            ra[i] = src[0];
            rb[i] = src[1];
        } else {
            ra[i] = *reinterpret_cast<const uint4*>(static_cast<const unsigned short*>(p.o[i]) + e);
            rb[i] = ra[i];
        }
    }

    // m = max_i lse_i; a NaN stays (fmaxf would drop it)
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < N; i++) m = (l[i] > m || l[i] != l[i]) ? l[i] : m;

    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float lse_row = -INFINITY;
    if (m != -INFINITY) {   // (all partials empty: the zero row and -inf above)
        float den = 0.f;
#pragma unroll
        for (int i = 0; i < N; i++) {
            const float w = expf(l[i] - m);   // +inf - +inf, NaN: NaN, and it spreads over the row
            den += w;
            float x[8];
            if (p.fmt[i] == QATTN_FMT_FP32) {
                const float t[8] = {__uint_as_float(ra[i].x), __uint_as_float(ra[i].y), __uint_as_float(ra[i].z), __uint_as_float(ra[i].w),
                                    __uint_as_float(rb[i].x), __uint_as_float(rb[i].y), __uint_as_float(rb[i].z), __uint_as_float(rb[i].w)};
#pragma unroll
                for (int j = 0; j < 8; j++) x[j] = t[j];
            } else if (p.fmt[i] == QATTN_FMT_BF16) {
                merge_unpack16<QATTN_FMT_BF16>(ra[i], x);
            } else {
                merge_unpack16<QATTN_FMT_FP16>(ra[i], x);
            }
            // a partial of weight zero (lse_i = -inf, or too far below m) contributes nothing WHATEVER its row holds: 0 * NaN would be NaN
            const bool live = w != 0.f;
#pragma unroll
            for (int j = 0; j < 8; j++) acc[j] += w * (live ? x[j] : 0.f);
        }
        const float inv = 1.0f / den;
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j] *= inv;
        lse_row = m + logf(den);
    }

    const long long eo = b * p.outs[0] + h * p.outs[1] + s * p.outs[2] + piece * 8;
    if (p.out_fmt == QATTN_FMT_FP32) {
        float4* dst = reinterpret_cast<float4*>(static_cast<float*>(p.out) + eo);
        dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else {
        uint4 r;
        if (p.out_fmt == QATTN_FMT_BF16) {
            r = make_uint4(merge_pack16<QATTN_FMT_BF16>(acc[0], acc[1]), merge_pack16<QATTN_FMT_BF16>(acc[2], acc[3]),
                           merge_pack16<QATTN_FMT_BF16>(acc[4], acc[5]), merge_pack16<QATTN_FMT_BF16>(acc[6], acc[7]));
        } else {
            r = make_uint4(merge_pack16<QATTN_FMT_FP16>(acc[0], acc[1]), merge_pack16<QATTN_FMT_FP16>(acc[2], acc[3]),
                           merge_pack16<QATTN_FMT_FP16>(acc[4], acc[5]), merge_pack16<QATTN_FMT_FP16>(acc[6], acc[7]));
        }
        *reinterpret_cast<uint4*>(static_cast<unsigned short*>(p.out) + eo) = r;
    }
    // in place (lse_out = lse[0]): the lanes of a row sit in one wave and have all read lse[0] of the row above
    if (p.lse_out != nullptr && piece == 0) p.lse_out[b * p.louts[0] + h * p.louts[1] + s * p.louts[2]] = lse_row;
}

template <int D>
static void launch_merge(int n, const MergeParams& p, dim3 grid, hipStream_t st) {
    switch (n) {
#define QATTN_MERGE_CASE(NN) case NN: hipLaunchKernelGGL((merge_states_kernel<D, NN>), grid, dim3(256), 0, st, p); break
        QATTN_MERGE_CASE(2);
        QATTN_MERGE_CASE(3);
        QATTN_MERGE_CASE(4);
        QATTN_MERGE_CASE(5);
        QATTN_MERGE_CASE(6);
        QATTN_MERGE_CASE(7);
        QATTN_MERGE_CASE(8);
#undef QATTN_MERGE_CASE
    }
}

static int elem_bytes(int fmt) { return fmt == QATTN_FMT_FP32 ? 4 : 2; }
static bool merge_fmt_ok(int fmt) { return fmt == QATTN_FMT_BF16 || fmt == QATTN_FMT_FP16 || fmt == QATTN_FMT_FP32; }

// a tensor of rows of `row` elements under strides st[3] over `ext[3]` indices: strides >= 0 and, for an O tensor, base and rows on 16 bytes
static bool merge_view_ok(const void* base, const long long* st, const int* ext, int bytes, bool rows16) {
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
static bool merge_output_ok(const long long* st, const int* ext, int row) {
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

}  // namespace qattn

using namespace qattn;

extern "C" int qattn_attention_state_merge(int n, const void* const* o, const int* o_fmt, const long long* o_strides, const float* const* lse,
                                           const long long* lse_strides, void* out, int out_fmt, const long long* out_strides,
                                           float* lse_out, const long long* lse_out_strides, int B, int H, int S, int D, void* stream) {
    if (n < 2 || n > QATTN_MERGE_MAX_PARTIALS) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || H <= 0 || S <= 0 || B > 65535 || H > 65535) return QATTN_ERR_INVALID_ARG;
    if (D != 64 && D != 128 && D != 256) return QATTN_ERR_UNSUPPORTED_DIM;
    if (!o || !o_fmt || !o_strides || !lse || !lse_strides || !out || !out_strides) return QATTN_ERR_INVALID_ARG;
    if (lse_out && !lse_out_strides) return QATTN_ERR_INVALID_ARG;
    if (!merge_fmt_ok(out_fmt)) return QATTN_ERR_UNSUPPORTED_FMT;
    const int ext[3] = {B, H, S};
    MergeParams p = {};
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
    hipStream_t st = (hipStream_t)stream;
    const int rows = 256 / (D / 8);
    const dim3 grid((unsigned)((S + rows - 1) / rows), (unsigned)H, (unsigned)B);
    if (D == 64) launch_merge<64>(n, p, grid, st);
    else if (D == 128) launch_merge<128>(n, p, grid, st);
    else launch_merge<256>(n, p, grid, st);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

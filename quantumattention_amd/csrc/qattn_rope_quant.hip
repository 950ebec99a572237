// qattn_rope_quant.hip -- rotary position embedding fused into the bf16/fp16 -> fp8 quant pre-pass of q and k, gfx950
// (include/qattn_rope.h).
//
// The rotated 16-bit q and k never exist in memory: both passes of the pre-pass (abs-max, quantise) rotate the values they hold in
// registers, round them to the input dtype -- so that every byte is the one the unfused composition gives -- and go on as
// qattn_quant.hip's kernels do (quant8, the KFRAG image and the scale rule come from qattn_common.h).
//
// Work unit of both kernels: the two 16-byte pieces dvh and dvh + D/16 of one row (dvh < D/16), in ONE thread.
//   interleaved = 0   pairs (i, i + D/2): element j of the first piece rotates with element j of the second; the unit needs the
//                     table entries 8 dvh .. 8 dvh + 7 (two consecutive float4 of cos, two of sin)
//   interleaved = 1   pairs (2i, 2i + 1) lie inside a piece; piece dv needs the entries 4 dv .. 4 dv + 3 (one float4 each)
// Either way a unit reads 32 bytes of data and 64 bytes of tables, and no value crosses lanes.  The tables are shared by every head of a
// batch element: blockIdx.x is the head, so that the workgroups in flight together read the same table rows (L2 / Infinity Cache).
#include "qattn_common.h"
#include "qattn_rope_dev.h"
#include "../../include/qattn_rope.h"

namespace qattn {

struct RopeJob {
    const uint4* x;        // [B,H,S,D] 16-bit, dense or a view (sb / sh / ss)
    uint4* out;            // fp8 payload: ROWMAJOR or KFRAG
    float* scale;          // [G] (head) or [G,S] (token)
    unsigned* amax_part;   // [G][kMomentSplits] workspace (head-wise): fp32 bits of every abs-max block's share
    const float* cs;       // row s of batch element b: cs + b tb + s tr, D/2 floats
    const float* sn;
    long tb, tr;           // table strides in floats (multiples of 4)
    int G, S, H, layout;
    long sb, sh, ss;       // 16-byte vectors between batch elements, heads, rows (SV kernels)
};
struct RopeJobs {
    RopeJob j[2];          // q, k
    int nsplit;            // abs-max blocks per head = valid words of amax_part per head
    int token;
};

__device__ __forceinline__ const uint4* rope_head(const RopeJob& jb, int g) { return jb.x + (long)(g / jb.H) * jb.sb + (long)(g % jb.H) * jb.sh; }

// rope + abs-max, q and k in one launch.  grid = (heads, splits, tensors), block = 256.  SV: heads and rows through sb / sh / ss (a strided
// view), else compile-time-free dense rows -- the split the pre-pass kernels of qattn_quant.hip have.
template <int IN_FMT, bool IL, bool SV>
__global__ __launch_bounds__(256) void rope_amax_kernel(const RopeJobs jobs, int D, int zbase) {
    const RopeJob& jb = jobs.j[zbase + blockIdx.z];
    const int g = blockIdx.x;
    if (g >= jb.G) return;
    const int hv = D >> 4, lg = 31 - __builtin_clz((unsigned)hv);   // units per row
    const long units = (long)jb.S * hv;
    const long per = (units + gridDim.y - 1) / gridDim.y;
    const long beg = (long)blockIdx.y * per;
    long end = beg + per;
    if (end > units) end = units;
    const uint4* xg = SV ? rope_head(jb, g) : jb.x + (long)g * jb.S * (2 * hv);
    const long rs = SV ? jb.ss : (long)(2 * hv);
    const long tbase = (long)(g / jb.H) * jb.tb;
    const float4* cg = reinterpret_cast<const float4*>(jb.cs + tbase);
    const float4* sg = reinterpret_cast<const float4*>(jb.sn + tbase);
    const long tr4 = jb.tr >> 2;
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    unsigned m0 = 0, m1 = 0;
    auto fold = [&](const uint4& v) {
        unsigned a = v.x & 0x7fff7fffu, b = v.y & 0x7fff7fffu, c = v.z & 0x7fff7fffu, d = v.w & 0x7fff7fffu;
        u16x2 pa, pb, pc, pd, p0, p1;
        __builtin_memcpy(&pa, &a, 4); __builtin_memcpy(&pb, &b, 4); __builtin_memcpy(&pc, &c, 4); __builtin_memcpy(&pd, &d, 4);
        __builtin_memcpy(&p0, &m0, 4); __builtin_memcpy(&p1, &m1, 4);
        p0 = __builtin_elementwise_max(p0, __builtin_elementwise_max(pa, pb));
        p1 = __builtin_elementwise_max(p1, __builtin_elementwise_max(pc, pd));
        __builtin_memcpy(&m0, &p0, 4); __builtin_memcpy(&m1, &p1, 4);
    };
    auto fetch = [&](long idx, uint4& a, uint4& b, float4 (&c)[2], float4 (&s)[2]) {
        const long row = idx >> lg;
        const int dvh = (int)(idx & (hv - 1));
        const uint4* p = xg + row * rs + dvh;
        a = load_nt(p);
        b = load_nt(p + hv);
        const int t0 = IL ? dvh : 2 * dvh, t1 = IL ? dvh + hv : 2 * dvh + 1;
        c[0] = cg[row * tr4 + t0]; c[1] = cg[row * tr4 + t1];
        s[0] = sg[row * tr4 + t0]; s[1] = sg[row * tr4 + t1];
    };
    constexpr int U = kAmaxInFlight / 2 > 0 ? kAmaxInFlight / 2 : 1;   // units per burst: kAmaxInFlight 16-byte data loads in flight per thread
    long i = beg + threadIdx.x;
    for (; i + (U - 1) * 256 < end; i += U * 256) {
        uint4 a[U], b[U];
        float4 c[U][2], s[U][2];
#pragma unroll
        for (int u = 0; u < U; u++) fetch(i + u * 256, a[u], b[u], c[u], s[u]);
#pragma unroll
        for (int u = 0; u < U; u++) {
            rope_unit<IN_FMT, IL>(a[u], b[u], c[u], s[u]);
            fold(a[u]);
            fold(b[u]);
        }
    }
    for (; i < end; i += 256) {
        uint4 a, b;
        float4 c[2], s[2];
        fetch(i, a, b, c, s);
        rope_unit<IN_FMT, IL>(a, b, c, s);
        fold(a);
        fold(b);
    }
    unsigned m = wave_allmax_u32(max(max(m0 & 0xffffu, m0 >> 16), max(m1 & 0xffffu, m1 >> 16)));
    __shared__ unsigned red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        // every block leaves its word (an empty share: 0); the quantise pass takes the maximum of a head's nsplit words
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        jb.amax_part[(long)g * kMomentSplits + blockIdx.y] = __float_as_uint(load16f<IN_FMT>((unsigned short)m));
    }
}

// rope + quantise: q to row-major q8, k to KFRAG k8 (or row-major), the same rotation and therefore the same bytes.
// grid = (heads, 64-row tiles, tensors), block = 256.
template <int D, int IN_FMT, int OUT_FMT, bool IL, bool SV>
__global__ __launch_bounds__(256) void rope_quant_kernel(const RopeJobs jobs, int numerics, int zbase) {
    constexpr int VPR = D / 8;              // 16-byte input vectors per row
    constexpr int HV = D / 16;              // units per row
    constexpr int ITERS = 64 * HV / 256;    // units per thread
    constexpr int KPAD = 64 * D + (64 * D / 512) * 16;  // KFRAG image + 16 B per 512 B (conflict-free 8-byte writes, as quant_multi_kernel)
    __shared__ __attribute__((aligned(16))) unsigned char img[KPAD];
    const RopeJob& jb = jobs.j[zbase + blockIdx.z];
    const int tid = threadIdx.x, S = jb.S;
    const int g = blockIdx.x, tile = blockIdx.y, row0 = tile * 64;
    if (g >= jb.G || row0 >= S) return;   // (block-uniform)
    const int layout = jb.layout;
    const bool token = jobs.token != 0;
    const float inv_qmax = (float)(1.0 / (double)(OUT_FMT == QATTN_FMT_E4M3 ? 448.0 : 57344.0));
    float scale = 1.0f;
    if (!token) {
        const unsigned amax_bits = max_partials(jb.amax_part + (long)g * kMomentSplits, jobs.nsplit, tid & 63);
        scale = make_scale(__uint_as_float(amax_bits), inv_qmax, numerics, IN_FMT);
        if (tile == 0 && tid == 0) jb.scale[g] = scale;
    }
    float rinv = 1.0f / scale;
    const uint4* xg = SV ? rope_head(jb, g) : jb.x + (long)g * S * VPR;
    const long rs = SV ? jb.ss : (long)VPR;
    const long tbase = (long)(g / jb.H) * jb.tb;
    const float4* cg = reinterpret_cast<const float4*>(jb.cs + tbase);
    const float4* sg = reinterpret_cast<const float4*>(jb.sn + tbase);
    const long tr4 = jb.tr >> 2;
    uint4 a[ITERS], b[ITERS];
    float4 c[ITERS][2], s[ITERS][2];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int vec = it * 256 + tid;
        const int r = vec / HV, dvh = vec % HV, row = row0 + r;
        a[it] = b[it] = make_uint4(0, 0, 0, 0);
        c[it][0] = c[it][1] = s[it][0] = s[it][1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (row < S) {   // (rows past the end: zeros, no table row is read for them -- T >= S is all the contract promises)
            const uint4* p = xg + (long)row * rs + dvh;
            a[it] = load_nt(p);
            b[it] = load_nt(p + HV);
            const int t0 = IL ? dvh : 2 * dvh, t1 = IL ? dvh + HV : 2 * dvh + 1;
            c[it][0] = cg[(long)row * tr4 + t0]; c[it][1] = cg[(long)row * tr4 + t1];
            s[it][0] = sg[(long)row * tr4 + t0]; s[it][1] = sg[(long)row * tr4 + t1];
        }
    }
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int vec = it * 256 + tid;
        const int r = vec / HV, dvh = vec % HV, row = row0 + r;
        rope_unit<IN_FMT, IL>(a[it], b[it], c[it], s[it]);
        if (token) {
            unsigned short e[16];
            __builtin_memcpy(e, &a[it], 16);
            __builtin_memcpy(e + 8, &b[it], 16);
            float am = 0.0f;
            bool nan = false;
#pragma unroll
            for (int j = 0; j < 16; j++) { const float f = load16f<IN_FMT>(e[j]); am = fmaxf(am, fabsf(f)); nan |= (f != f); }
            unsigned ab = nan ? 0x7fc00000u : __float_as_uint(am);
#pragma unroll
            for (int off = HV / 2; off > 0; off >>= 1) ab = max(ab, (unsigned)__shfl_xor((int)ab, off));   // the HV lanes of a row are neighbours
            scale = make_scale(__uint_as_float(ab), inv_qmax, numerics, IN_FMT);
            if (dvh == 0 && row < S) jb.scale[(long)g * S + row] = scale;
            rinv = 1.0f / scale;
        }
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int2 lohi = quant8<IN_FMT, OUT_FMT>(half ? b[it] : a[it], scale, rinv);
            const int dv = dvh + half * HV;
            if (layout == QATTN_LAYOUT_ROWMAJOR) {
                if (row < S) reinterpret_cast<int2*>(jb.out)[((long)g * S + row) * VPR + dv] = lohi;
            } else {
                const int o = kfrag_offset<D>(r, dv * 8);
                *reinterpret_cast<int2*>(img + o + ((o >> 9) << 4)) = lohi;
            }
        }
    }
    if (layout != QATTN_LAYOUT_ROWMAJOR) {   // (block-uniform: one layout per tensor)
        __syncthreads();
        const long Sp = (long)((S + 63) / 64) * 64;
        uint4* og = jb.out + ((long)g * Sp + row0) * (D / 16);
        for (int i = tid; i < 64 * D / 16; i += 256) og[i] = *reinterpret_cast<const uint4*>(img + i * 16 + ((i >> 5) << 4));
    }
}

template <int D, int IN, int OUT>
static void launch_rope_quant3(const RopeJobs& jobs, bool il, bool sv, int numerics, dim3 grid, int zbase, hipStream_t st) {
    dim3 block(256);
    if (il) {
        if (sv) hipLaunchKernelGGL((rope_quant_kernel<D, IN, OUT, true, true>), grid, block, 0, st, jobs, numerics, zbase);
        else hipLaunchKernelGGL((rope_quant_kernel<D, IN, OUT, true, false>), grid, block, 0, st, jobs, numerics, zbase);
    } else {
        if (sv) hipLaunchKernelGGL((rope_quant_kernel<D, IN, OUT, false, true>), grid, block, 0, st, jobs, numerics, zbase);
        else hipLaunchKernelGGL((rope_quant_kernel<D, IN, OUT, false, false>), grid, block, 0, st, jobs, numerics, zbase);
    }
}

template <int D>
static void launch_rope_quant(const RopeJobs& jobs, int in_fmt, int out_fmt, bool il, bool sv, int numerics, dim3 grid, int zbase, hipStream_t st) {
    if (in_fmt == QATTN_FMT_BF16) {
        if (out_fmt == QATTN_FMT_E4M3) launch_rope_quant3<D, QATTN_FMT_BF16, QATTN_FMT_E4M3>(jobs, il, sv, numerics, grid, zbase, st);
        else launch_rope_quant3<D, QATTN_FMT_BF16, QATTN_FMT_E5M2>(jobs, il, sv, numerics, grid, zbase, st);
    } else {
        if (out_fmt == QATTN_FMT_E4M3) launch_rope_quant3<D, QATTN_FMT_FP16, QATTN_FMT_E4M3>(jobs, il, sv, numerics, grid, zbase, st);
        else launch_rope_quant3<D, QATTN_FMT_FP16, QATTN_FMT_E5M2>(jobs, il, sv, numerics, grid, zbase, st);
    }
}

template <int IN>
static void launch_rope_amax(const RopeJobs& jobs, bool il, bool sv, int D, dim3 grid, int zbase, hipStream_t st) {
    dim3 block(256);
    if (il) {
        if (sv) hipLaunchKernelGGL((rope_amax_kernel<IN, true, true>), grid, block, 0, st, jobs, D, zbase);
        else hipLaunchKernelGGL((rope_amax_kernel<IN, true, false>), grid, block, 0, st, jobs, D, zbase);
    } else {
        if (sv) hipLaunchKernelGGL((rope_amax_kernel<IN, false, true>), grid, block, 0, st, jobs, D, zbase);
        else hipLaunchKernelGGL((rope_amax_kernel<IN, false, false>), grid, block, 0, st, jobs, D, zbase);
    }
}

}  // namespace qattn

using namespace qattn;

extern "C" size_t qattn_rope_quant_qk_workspace_bytes(int B, int Hq, int Hkv) {
    if (B <= 0 || Hq <= 0 || Hkv <= 0) return 0;
    // per-block abs-max words of q, then of k: kMomentSplits per head (nothing to zero beforehand; unused with token-wise scales)
    return (size_t)kMomentSplits * ((size_t)B * Hq + (size_t)B * Hkv) * sizeof(unsigned);
}

static bool rope_table_ok(const float* c, const float* s, long long tb, long long tr) {
    return c && s && ((uintptr_t)c & 15) == 0 && ((uintptr_t)s & 15) == 0 && tb >= 0 && tr >= 0 && tb % 4 == 0 && tr % 4 == 0;
}

extern "C" int qattn_rope_quant_qk_fp8(const void* q, const void* k, const long long* strides, int in_fmt, const float* cos_q,
                                       const float* sin_q, long long table_q_batch_stride, long long table_q_row_stride,
                                       const float* cos_k, const float* sin_k, long long table_k_batch_stride,
                                       long long table_k_row_stride, int interleaved, void* q8, void* k8, int k_layout, float* scale_q,
                                       float* scale_k, int B, int Hq, int Hkv, int Sq, int Skv, int D, int out_fmt, int scale_mode,
                                       int numerics, void* workspace, size_t workspace_bytes, void* stream) {
    if (!q && !k) return QATTN_ERR_INVALID_ARG;
    if ((q && (!q8 || !scale_q)) || (k && (!k8 || !scale_k))) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || Hq <= 0 || Hkv <= 0 || Sq <= 0 || Skv <= 0) return QATTN_ERR_INVALID_ARG;
    if (D != 64 && D != 128 && D != 256) return QATTN_ERR_UNSUPPORTED_DIM;
    if (scale_mode != QATTN_SCALE_HEAD && scale_mode != QATTN_SCALE_TOKEN) return QATTN_ERR_INVALID_ARG;
    if (numerics != QATTN_NUMERICS_COMPILED && numerics != QATTN_NUMERICS_EAGER) return QATTN_ERR_INVALID_ARG;
    if (interleaved != 0 && interleaved != 1) return QATTN_ERR_INVALID_ARG;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (out_fmt != QATTN_FMT_E4M3 && out_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (k_layout != QATTN_LAYOUT_KFRAG && k_layout != QATTN_LAYOUT_ROWMAJOR) return QATTN_ERR_UNSUPPORTED_FMT;
    if (q && !rope_table_ok(cos_q, sin_q, table_q_batch_stride, table_q_row_stride)) return QATTN_ERR_INVALID_ARG;
    if (k && !rope_table_ok(cos_k, sin_k, table_k_batch_stride, table_k_row_stride)) return QATTN_ERR_INVALID_ARG;
    if (((uintptr_t)q & 15) || ((uintptr_t)k & 15) || ((uintptr_t)q8 & 15) || ((uintptr_t)k8 & 15)) return QATTN_ERR_INVALID_ARG;
    if ((Sq + 63) / 64 > 65535 || (Skv + 63) / 64 > 65535) return QATTN_ERR_INVALID_ARG;   // (a grid dimension)
    if (strides)
        for (int t = 0; t < 6; t++)
            if (strides[t] < 0 || strides[t] % 8 != 0 || (t % 3 == 2 && (strides[t] < D || strides[t] > (1LL << 23)))) return QATTN_ERR_INVALID_ARG;
    const bool head = scale_mode == QATTN_SCALE_HEAD;
    if (head && (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < qattn_rope_quant_qk_workspace_bytes(B, Hq, Hkv))) return QATTN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    unsigned* ws = (unsigned*)workspace;
    const long vd = D / 8;
    auto sv3 = [&](int t, int H, int S, int i) { return strides ? (long)(strides[3 * t + i] / 8) : i == 0 ? (long)H * S * vd : i == 1 ? (long)S * vd : vd; };
    RopeJobs jobs;
    jobs.nsplit = amax_splits(Sq, Skv, D);
    jobs.token = head ? 0 : 1;
    jobs.j[0] = RopeJob{(const uint4*)q, (uint4*)q8, scale_q, ws, cos_q, sin_q, (long)table_q_batch_stride, (long)table_q_row_stride,
                        B * Hq, Sq, Hq, QATTN_LAYOUT_ROWMAJOR, sv3(0, Hq, Sq, 0), sv3(0, Hq, Sq, 1), sv3(0, Hq, Sq, 2)};
    jobs.j[1] = RopeJob{(const uint4*)k, (uint4*)k8, scale_k, head ? ws + (size_t)kMomentSplits * B * Hq : nullptr, cos_k, sin_k,
                        (long)table_k_batch_stride, (long)table_k_row_stride, B * Hkv, Skv, Hkv, k_layout, sv3(1, Hkv, Skv, 0),
                        sv3(1, Hkv, Skv, 1), sv3(1, Hkv, Skv, 2)};
    // one tensor only: the launches cover its slot alone
    const int zbase = q ? 0 : 1, nz = (q && k) ? 2 : 1;
    const int Gmax = !k ? B * Hq : !q ? B * Hkv : B * (Hq > Hkv ? Hq : Hkv);
    const int Smax = !k ? Sq : !q ? Skv : (Sq > Skv ? Sq : Skv);
    if (!q || !k) jobs.nsplit = amax_splits(Smax, Smax, D);
    const bool il = interleaved != 0, sv = strides != nullptr;
    if (head) {
        dim3 grid(Gmax, jobs.nsplit, nz);
        if (in_fmt == QATTN_FMT_BF16) launch_rope_amax<QATTN_FMT_BF16>(jobs, il, sv, D, grid, zbase, st);
        else launch_rope_amax<QATTN_FMT_FP16>(jobs, il, sv, D, grid, zbase, st);
    }
    dim3 grid(Gmax, (Smax + 63) / 64, nz);
    if (D == 64) launch_rope_quant<64>(jobs, in_fmt, out_fmt, il, sv, numerics, grid, zbase, st);
    else if (D == 128) launch_rope_quant<128>(jobs, in_fmt, out_fmt, il, sv, numerics, grid, zbase, st);
    else launch_rope_quant<256>(jobs, in_fmt, out_fmt, il, sv, numerics, grid, zbase, st);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

// ---- the whole step: rope + quantise q and k, V through the head-wise quantiser (or kept 16-bit), then the existing attention entry
static size_t up256(size_t x) { return (x + 255) / 256 * 256; }

extern "C" size_t qattn_fp8_rope_quant_attention_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Skv, int D) {
    if (B <= 0 || Hq <= 0 || Hkv <= 0 || Sq <= 0 || Skv <= 0 || (D != 64 && D != 128 && D != 256)) return 0;
    // [abs-max words of q and k | abs-max words of V's quantiser | the attention call's workspace], each part 256-byte aligned
    return up256(qattn_rope_quant_qk_workspace_bytes(B, Hq, Hkv)) + up256(qattn_quant_workspace_bytes(B, Hkv, Skv, D, QATTN_SCALE_HEAD)) +
           up256(qattn_attention_workspace_bytes(B, Hq, Sq));
}

extern "C" int qattn_fp8_rope_quant_attention_forward(const void* q, const void* k, const void* v, const long long* strides, int in_fmt,
                                                      const float* cos_q, const float* sin_q, long long table_q_batch_stride,
                                                      long long table_q_row_stride, const float* cos_k, const float* sin_k,
                                                      long long table_k_batch_stride, long long table_k_row_stride, int interleaved,
                                                      void* out, float* lse, void* q8, void* k8, void* v8, float* scale_q, float* scale_k,
                                                      float* scale_v, int B, int Hq, int Hkv, int Sq, int Skv, int D, int fp8_fmt, int v_fmt,
                                                      int scale_mode, int numerics, int is_causal, float sm_scale, int precision,
                                                      int lse_layout, void* workspace, size_t workspace_bytes, void* stream) {
    if (!q || !k || !v || !out || !q8 || !k8 || !scale_q || !scale_k) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || Hq <= 0 || Hkv <= 0 || Sq <= 0 || Skv <= 0) return QATTN_ERR_INVALID_ARG;
    if ((D != 64 && D != 128 && D != 256) || Hq % Hkv != 0) return QATTN_ERR_UNSUPPORTED_DIM;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (v_fmt != fp8_fmt && v_fmt != in_fmt) return QATTN_ERR_UNSUPPORTED_FMT;   // both products on FP8 MFMA, or 16-bit P on the caller's V
    if (v_fmt == fp8_fmt && (!v8 || !scale_v)) return QATTN_ERR_INVALID_ARG;
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < qattn_fp8_rope_quant_attention_workspace_bytes(B, Hq, Hkv, Sq, Skv, D))
        return QATTN_ERR_WORKSPACE;
    unsigned char* w = (unsigned char*)workspace;
    void* rope_ws = w;   const size_t rope_ws_bytes = qattn_rope_quant_qk_workspace_bytes(B, Hq, Hkv);
    w += up256(rope_ws_bytes);
    void* vq_ws = w;     const size_t vq_ws_bytes = qattn_quant_workspace_bytes(B, Hkv, Skv, D, QATTN_SCALE_HEAD);
    w += up256(vq_ws_bytes);
    void* attn_ws = w;   const size_t attn_ws_bytes = qattn_attention_workspace_bytes(B, Hq, Sq);
    int rc = qattn_rope_quant_qk_fp8(q, k, strides, in_fmt, cos_q, sin_q, table_q_batch_stride, table_q_row_stride, cos_k, sin_k,
                                     table_k_batch_stride, table_k_row_stride, interleaved, q8, k8, QATTN_LAYOUT_KFRAG, scale_q, scale_k, B, Hq,
                                     Hkv, Sq, Skv, D, fp8_fmt, scale_mode, numerics, rope_ws, rope_ws_bytes, stream);
    if (rc != QATTN_OK) return rc;
    if (v_fmt == fp8_fmt) {
        rc = qattn_quant_fp8(v, in_fmt, v8, scale_v, B, Hkv, Skv, D, fp8_fmt, QATTN_SCALE_HEAD, numerics, QATTN_LAYOUT_VFRAG, vq_ws, vq_ws_bytes, stream);
        if (rc != QATTN_OK) return rc;
        return qattn_fp8_attention_forward(q8, k8, v8, out, lse, scale_q, scale_k, scale_v, B, Hq, Hkv, Sq, Skv, D, fp8_fmt, fp8_fmt, in_fmt,
                                           scale_mode, is_causal, sm_scale, precision, lse_layout, attn_ws, attn_ws_bytes, stream);
    }
    return qattn_fp8_attention_forward(q8, k8, v, out, lse, scale_q, scale_k, nullptr, B, Hq, Hkv, Sq, Skv, D, fp8_fmt, in_fmt, in_fmt, scale_mode,
                                       is_causal, sm_scale, precision, lse_layout, attn_ws, attn_ws_bytes, stream);
}

// qattn_varlen.hip -- qattn_fp8_quant_attention_varlen_forward (include/qattn_varlen.h): FP8 attention on B sequences packed along the
// token axis, with per-(sequence, head) scales and the reference kernel's own P.V numerics (16-bit P on the original 16-bit V).
//
// Three launches after a zeroing node, none of which reads a length on the host:
//   amax   per (sequence, head) abs-max of q and of k (used keys only): 256-row tiles, one atomicMax per tile on the fp32 bits of the
//          tile's abs-max (non-negative floats order like their bits; the words are zeroed by the node before, so the result does not
//          depend on the order of the atomics)
//   quant  64-row tiles: q into a dense [Hq, L_q, D] slab per sequence, k into its KFRAG image, with quant8 / kfrag_offset of the dense
//          pre-pass (qattn_common.h, quant_multi_kernel) -- so the bytes are those of qattn_quant_fp8 on the sequence alone
//   attn   one workgroup per (head, 256-row query block of a sequence): pv16_block_pass_at (qattn_pv16.h) on the sequence's B = 1
//          parameters, with the loop form of the whole-tensor launch (launch_one, qattn_attn_pv16.hip) -- the same bits per row
//
// Block -> sequence without a scan: with R rows per tile, f(i) = i + floor(start_i / R) is strictly increasing over the sequences of a
// consistent table and f(i + 1) - f(i) >= ceil(L_i / R), so workgroup j belongs to the largest i with f(i) <= j (binary search over the
// table) as its tile j - f(i) -- or to no tile, and exits.  B + ceil(total / R) workgroups per head cover every tile and waste at most B.
// Built with strided addressing (QATTN_STRIDED16 = 1: V and `out` through byte strides).
#include "qattn_pv16.h"
#include "qattn_varlen_tile.h"
#include "qattn_varlen_attn.h"
#include "../../include/qattn_varlen.h"

namespace qattn {

static_assert(kStrided16, "the varlen unit addresses V and the output through strides");

// q (z = 0) and k (z = 1) of one call
struct VarlenQuant {
    const unsigned char* x[2];   // 16-bit inputs
    long ts[2], hs[2];           // element strides of token and head
    const int* cu[2];
    const int* used;             // seqused_k or nullptr
    int total[2], H[2];
    int B;
    unsigned* amax[2];           // [B][H] fp32 bits, zeroed before the abs-max pass
    unsigned char* x8[2];        // q8 row-major slabs / k8 KFRAG images
    float* scale[2];             // [B][H]
};

template <int D, int IN_FMT>
__global__ __launch_bounds__(256) void varlen_amax_kernel(const VarlenQuant a) {
    constexpr int VPR = D / 8;   // 16-byte vectors per row
    const int z = blockIdx.z, h = blockIdx.y;
    if (h >= a.H[z]) return;
    const VarlenTile t = varlen_tile<kVarlenAmaxRows>(a.cu[z], z ? a.used : nullptr, a.B, a.total[z], (int)blockIdx.x);
    if (t.tile < 0 || t.tile * kVarlenAmaxRows >= t.len) return;
    const int row0 = t.tile * kVarlenAmaxRows, rows = min(kVarlenAmaxRows, t.len - row0);
    const unsigned char* xh = a.x[z] + 2 * ((long)(t.start + row0) * a.ts[z] + (long)h * a.hs[z]);
    const int nvec = rows * VPR;
    unsigned m0 = 0, m1 = 0;
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    auto fold = [&](const uint4& v) {
        unsigned w[4] = {v.x & 0x7fff7fffu, v.y & 0x7fff7fffu, v.z & 0x7fff7fffu, v.w & 0x7fff7fffu};
        u16x2 pa, pb, pc, pd, p0, p1;
        __builtin_memcpy(&pa, &w[0], 4); __builtin_memcpy(&pb, &w[1], 4); __builtin_memcpy(&pc, &w[2], 4); __builtin_memcpy(&pd, &w[3], 4);
        __builtin_memcpy(&p0, &m0, 4); __builtin_memcpy(&p1, &m1, 4);
        p0 = __builtin_elementwise_max(p0, __builtin_elementwise_max(pa, pb));
        p1 = __builtin_elementwise_max(p1, __builtin_elementwise_max(pc, pd));
        __builtin_memcpy(&m0, &p0, 4); __builtin_memcpy(&m1, &p1, 4);
    };
    for (int base = threadIdx.x; base < nvec; base += 4 * 256) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int idx = base + u * 256;
            v[u] = make_uint4(0, 0, 0, 0);
            if (idx < nvec) v[u] = load_nt(reinterpret_cast<const uint4*>(xh + 2 * (long)(idx / VPR) * a.ts[z]) + idx % VPR);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) fold(v[u]);
    }
    unsigned m = wave_allmax_u32(max(max(m0 & 0xffffu, m0 >> 16), max(m1 & 0xffffu, m1 >> 16)));
    __shared__ unsigned red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        atomicMax(a.amax[z] + (long)t.i * a.H[z] + h, __float_as_uint(load16f<IN_FMT>((unsigned short)m)));
    }
}

template <int D, int IN_FMT, int OUT_FMT>
__global__ __launch_bounds__(256) void varlen_quant_kernel(const VarlenQuant a, int numerics) {
    constexpr int VPR = D / 8;
    constexpr int ITERS = 64 * VPR / 256;
    constexpr int KPAD = 64 * D + (64 * D / 512) * 16;   // the KFRAG image of quant_multi_kernel, padded by 16 B per 512 B
    __shared__ __attribute__((aligned(16))) unsigned char img[KPAD];
    const int z = blockIdx.z, h = blockIdx.y, tid = threadIdx.x;
    if (h >= a.H[z]) return;
    const int H = a.H[z];
    const VarlenTile t = varlen_tile<kVarlenQuantRows>(a.cu[z], z ? a.used : nullptr, a.B, a.total[z], (int)blockIdx.x);
    if (t.tile < 0) return;
    const float inv_qmax = (float)(1.0 / (double)(OUT_FMT == QATTN_FMT_E4M3 ? 448.0 : 57344.0));
    const float scale = make_scale(__uint_as_float(a.amax[z][(long)t.i * H + h] & 0x7fffffffu), inv_qmax, numerics, IN_FMT);
    if (t.tile == 0 && tid == 0) a.scale[z][(long)t.i * H + h] = scale;   // (also for an empty sequence: amax 0 -> eps)
    if (t.tile * kVarlenQuantRows >= t.len) return;
    const float rinv = 1.0f / scale;
    const int row0 = t.tile * kVarlenQuantRows;
    const unsigned char* xh = a.x[z] + 2 * ((long)t.start * a.ts[z] + (long)h * a.hs[z]);
    uint4 held[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int vec = it * 256 + tid, row = row0 + vec / VPR;
        held[it] = make_uint4(0, 0, 0, 0);   // (rows beyond the used length: the zero padding of the dense pack)
        if (row < t.len) held[it] = load_nt(reinterpret_cast<const uint4*>(xh + 2 * (long)row * a.ts[z]) + vec % VPR);
    }
    if (z == 0) {   // q: row-major slab [Hq, L_q, D] at element Hq D start
        int2* og = reinterpret_cast<int2*>(a.x8[0] + (long)H * D * t.start + ((long)h * t.len + row0) * D);
#pragma unroll
        for (int it = 0; it < ITERS; it++) {
            const int vec = it * 256 + tid, r = vec / VPR;
            const int2 lohi = quant8<IN_FMT, OUT_FMT>(held[it], scale, rinv);
            if (row0 + r < t.len) og[(long)r * (D / 8) + vec % VPR] = lohi;
        }
        return;
    }
    // k: KFRAG image of the sequence, [Hkv, ceil(L/64) 64, D] at element Hkv D (start + 64 i)
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int vec = it * 256 + tid, r = vec / VPR, dv = vec % VPR;
        const int2 lohi = quant8<IN_FMT, OUT_FMT>(held[it], scale, rinv);
        const int o = kfrag_offset<D>(r, dv * 8);
        *reinterpret_cast<int2*>(img + o + ((o >> 9) << 4)) = lohi;
    }
    __syncthreads();
    const long Lp = (long)((t.len + 63) / 64) * 64;
    uint4* og = reinterpret_cast<uint4*>(a.x8[1] + (long)H * D * (t.start + 64L * t.i) + ((long)h * Lp + row0) * D);
    for (int i = tid; i < 64 * D / 16; i += 256) og[i] = *reinterpret_cast<const uint4*>(img + i * 16 + ((i >> 5) << 4));
}

// PP: the two-group loop, as launch_one picks it for a whole-tensor launch (D = 128); else the one-group loop with three stages
template <int D, int QK_FMT, int V16_FMT, bool CAUSAL, bool PP>
__global__ __launch_bounds__(kThreads, 2) void attn_pv16_varlen_kernel(const VarlenAttn a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int bid = blockIdx.x;
    int h, j;
    if (a.xcd_remap) {   // (speed only) every XCD takes a contiguous range of heads, all sequences of each: their K / V stay in its L2
        const int idx = bid >> 3, hpx = a.Hq >> 3;
        h = (bid & 7) * hpx + idx / a.nblk;
        j = idx % a.nblk;
    } else {
        h = bid / a.nblk;
        j = bid % a.nblk;
    }
    if (CAUSAL) j = a.nblk - 1 - j;   // (the last blocks of a sequence see the most keys: roughly longest first)
    const VarlenTile tq = varlen_tile<kQPerWG>(a.cu_q, nullptr, a.B, a.total_q, j);
    if (tq.tile < 0 || tq.tile * kQPerWG >= tq.len) return;
    const int i = tq.i;
    const int sk0 = clampi(__builtin_amdgcn_readfirstlane(a.cu_k[i]), 0, a.total_k);
    int lk = clampi(__builtin_amdgcn_readfirstlane(a.cu_k[i + 1]), sk0, a.total_k) - sk0;
    if (a.used) lk = clampi(__builtin_amdgcn_readfirstlane(a.used[i]), 0, lk);
    constexpr int RB = 2 * D;   // bytes of a 16-bit row
    const long o_rs = (long)a.Hq * RB;
    unsigned char* out = reinterpret_cast<unsigned char*>(a.out) + (long)tq.start * o_rs;
    if (lk == 0) {   // no key: zero rows, LSE -inf (pv16_block_pass would index chunk -1)
        const int row = tq.tile * kQPerWG + (int)threadIdx.x / 2, half = threadIdx.x & 1;
        if (threadIdx.x < 2 * kQPerWG && row < tq.len) {
            uint4* op = reinterpret_cast<uint4*>(out + (long)row * o_rs + (long)h * RB + half * (RB / 2));
#pragma unroll
            for (int c = 0; c < RB / 32; c++) op[c] = make_uint4(0, 0, 0, 0);
            if (a.lse && half == 0) a.lse[(long)h * a.total_q + tq.start + row] = -INFINITY;
        }
        return;
    }
    AttnParams p;
    __builtin_memset(&p, 0, sizeof(p));
    p.B = 1; p.Hq = a.Hq; p.Hkv = a.Hkv; p.Sq = tq.len; p.Skv = lk;
    p.nqb = ceil_div(tq.len, kQPerWG);
    p.nchunks = ceil_div(lk, 64);
    p.q = a.q8 + (long)a.Hq * D * tq.start;
    p.k = a.k8 + (long)a.Hkv * D * (sk0 + 64L * i);
    p.sq = a.sq + (long)i * a.Hq;
    p.sk = a.sk + (long)i * a.Hkv;
    p.sm_log2e = a.sm_log2e;
    p.out = out; p.out_fmt = a.out_fmt;
    p.o_rs = o_rs; p.o_hs = RB; p.o_bs = 0;
    p.lse = a.lse ? a.lse + tq.start : nullptr;
    p.lse_stride = a.total_q; p.lse_mul = 1.0f;
    p.v16 = a.v + (long)sk0 * a.v_ts;
    p.v16_rs = a.v_ts; p.v16_hs = a.v_hs; p.v16_bs = 0;
    pv16_block_pass_at<D, kWaves, QK_FMT, V16_FMT, CAUSAL, false, false, PP ? 4 : 3, PP>(p, smem, (int)threadIdx.x, h, tq.tile, []() { return 0u; },
                                                                                       [](unsigned) {});
}

template <int D, int QK_FMT, int V16_FMT, bool CAUSAL>
static int launch_varlen_attn(const VarlenAttn& a, hipStream_t st) {
    constexpr bool PP = D == 128;
    constexpr int lds = (PP ? 4 : 3) * (64 * D + 64 * D * 2);
    auto kern = attn_pv16_varlen_kernel<D, QK_FMT, V16_FMT, CAUSAL, PP>;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return QATTN_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3((unsigned)(a.Hq * a.nblk)), dim3(kThreads), lds, st, a);
    return QATTN_OK;
}
template <int D, int QK_FMT, int V16_FMT>
static int launch_varlen_attn_c(const VarlenAttn& a, int causal, hipStream_t st) {
    return causal ? launch_varlen_attn<D, QK_FMT, V16_FMT, true>(a, st) : launch_varlen_attn<D, QK_FMT, V16_FMT, false>(a, st);
}
// skip_k (key smoothing): K takes no part in the abs-max and quantise launches -- their grids shrink to q's slice (z = 0) -- and is
// quantised by the launches of qattn_varlen_smooth.hip instead, as launch_quant_qkv's skip_k
template <int D, int IN_FMT, int OUT_FMT>
static int launch_varlen_d(const VarlenQuant& qa, const VarlenAttn& a, int numerics, int causal, hipStream_t st, bool skip_k, const int* window) {
    const int tmax = skip_k || qa.total[0] > qa.total[1] ? qa.total[0] : qa.total[1];
    const int hmax = skip_k || qa.H[0] > qa.H[1] ? qa.H[0] : qa.H[1];
    const unsigned nz = skip_k ? 1 : 2;
    hipLaunchKernelGGL((varlen_amax_kernel<D, IN_FMT>), dim3((unsigned)(qa.B + ceil_div(tmax, kVarlenAmaxRows)), hmax, nz), dim3(256), 0, st, qa);
    hipLaunchKernelGGL((varlen_quant_kernel<D, IN_FMT, OUT_FMT>), dim3((unsigned)(qa.B + ceil_div(tmax, kVarlenQuantRows)), hmax, nz), dim3(256), 0, st,
                       qa, numerics);
    // window: the sliding-window attention launch (qattn_varlen_window.hip) behind the same pre-pass
    if (window) return launch_varlen_window_attn(a, D, OUT_FMT, IN_FMT, window[0], window[1], st);
    return launch_varlen_attn_c<D, OUT_FMT, IN_FMT>(a, causal, st);
}
template <int D>
static int launch_varlen(const VarlenQuant& qa, const VarlenAttn& a, int in_fmt, int fp8_fmt, int numerics, int causal, hipStream_t st, bool skip_k,
                         const int* window) {
    if (in_fmt == QATTN_FMT_BF16)
        return fp8_fmt == QATTN_FMT_E4M3 ? launch_varlen_d<D, QATTN_FMT_BF16, QATTN_FMT_E4M3>(qa, a, numerics, causal, st, skip_k, window)
                                         : launch_varlen_d<D, QATTN_FMT_BF16, QATTN_FMT_E5M2>(qa, a, numerics, causal, st, skip_k, window);
    return fp8_fmt == QATTN_FMT_E4M3 ? launch_varlen_d<D, QATTN_FMT_FP16, QATTN_FMT_E4M3>(qa, a, numerics, causal, st, skip_k, window)
                                     : launch_varlen_d<D, QATTN_FMT_FP16, QATTN_FMT_E5M2>(qa, a, numerics, causal, st, skip_k, window);
}

}  // namespace qattn

using namespace qattn;

namespace {
size_t up256(size_t x) { return (x + 255) / 256 * 256; }
bool varlen_dims_ok(int B, int Hq, int Hkv, int total_q, int total_k) { return B >= 1 && Hq > 0 && Hkv > 0 && total_q >= 0 && total_k >= 0; }
}  // namespace

extern "C" size_t qattn_varlen_tensor_bytes(int layout, int B, int H, int total, int D) {
    if (B < 1 || H <= 0 || total < 0 || (D != 64 && D != 128 && D != 256)) return 0;
    if (layout == QATTN_LAYOUT_ROWMAJOR) return (size_t)H * total * D;
    if (layout == QATTN_LAYOUT_KFRAG) return (size_t)H * D * ((size_t)total + 64 * (size_t)B);   // ceil(L/64) 64 <= L + 63 per sequence
    return 0;
}

extern "C" size_t qattn_fp8_quant_attention_varlen_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int D) {
    if (!varlen_dims_ok(B, Hq, Hkv, total_q, total_k) || (D != 64 && D != 128 && D != 256)) return 0;
    // [q8 | k8 | scale_q | scale_k | abs-max words of q, k]: the first four only used where the caller passes no buffer of its own
    return up256(qattn_varlen_tensor_bytes(QATTN_LAYOUT_ROWMAJOR, B, Hq, total_q, D)) + up256(qattn_varlen_tensor_bytes(QATTN_LAYOUT_KFRAG, B, Hkv, total_k, D)) +
           2 * up256(sizeof(float) * (size_t)B * (Hq + Hkv));
}

extern "C" size_t qattn_fp8_quant_attention_varlen_smooth_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int D) {
    const size_t plain = qattn_fp8_quant_attention_varlen_workspace_bytes(B, Hq, Hkv, total_q, total_k, D);
    // [the plain entry's workspace | per-block channel sums of the mean pass]
    return plain ? up256(plain) + varlen_smooth_k_workspace_bytes(B, Hkv, D) : 0;
}

// k_mean != nullptr: key smoothing (include/qattn_smooth.h); window != nullptr: {left, right} of the sliding-window entry
// (include/qattn_window.h, validated there), whose attention launch replaces this unit's -- is_causal is then not read
int qattn::varlen_forward_impl(const void* q, const void* k, const void* v, const long long* strides, int in_fmt, void* out, float* lse,
                               const int* cu_seqlens_q, const int* cu_seqlens_k, const int* seqused_k, int B, int Hq, int Hkv, int total_q,
                               int total_k, int D, int fp8_fmt, int numerics, int is_causal, float sm_scale, void* q8, void* k8, float* scale_q,
                               float* scale_k, void* workspace, size_t workspace_bytes, void* stream, float* k_mean, const int* window) {
    if (!q || !k || !v || !out || !cu_seqlens_q || !cu_seqlens_k) return QATTN_ERR_INVALID_ARG;
    if (!varlen_dims_ok(B, Hq, Hkv, total_q, total_k)) return QATTN_ERR_INVALID_ARG;
    if ((D != 64 && D != 128 && D != 256) || Hq % Hkv != 0) return QATTN_ERR_UNSUPPORTED_DIM;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (numerics != QATTN_NUMERICS_COMPILED && numerics != QATTN_NUMERICS_EAGER) return QATTN_ERR_INVALID_ARG;
    long long st6[6] = {(long long)Hq * D, D, (long long)Hkv * D, D, (long long)Hkv * D, D};   // dense [total, H, D]
    if (strides)
        for (int s = 0; s < 6; s++) {
            if (strides[s] < 0 || strides[s] % 8 != 0) return QATTN_ERR_INVALID_ARG;
            st6[s] = strides[s];
        }
    if (((size_t)q | (size_t)k | (size_t)v | (size_t)out) % 16 != 0) return QATTN_ERR_INVALID_ARG;
    // grids: Hq (B + ceil(total_q / 256)) attention workgroups, B + ceil(total / 64) quantise tiles per head (32-bit dimensions)
    if ((long long)Hq * (B + ceil_div(total_q, kQPerWG)) > 0x7fffffffLL || (long long)B + ceil_div(total_q > total_k ? total_q : total_k, 64) > 0x7fffffffLL)
        return QATTN_ERR_INVALID_ARG;
    const bool smooth = k_mean != nullptr;
    if (smooth && (reinterpret_cast<uintptr_t>(k_mean) & 15u) != 0) return QATTN_ERR_INVALID_ARG;
    const size_t plain_bytes = qattn_fp8_quant_attention_varlen_workspace_bytes(B, Hq, Hkv, total_q, total_k, D);
    const size_t need = smooth ? qattn_fp8_quant_attention_varlen_smooth_workspace_bytes(B, Hq, Hkv, total_q, total_k, D) : plain_bytes;
    if (!workspace || workspace_bytes < need) return QATTN_ERR_WORKSPACE;
    if (total_q == 0) return QATTN_OK;   // no query row: nothing to compute or write
    hipStream_t st = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)workspace;
    unsigned char* q8w = w;   w += up256(qattn_varlen_tensor_bytes(QATTN_LAYOUT_ROWMAJOR, B, Hq, total_q, D));
    unsigned char* k8w = w;   w += up256(qattn_varlen_tensor_bytes(QATTN_LAYOUT_KFRAG, B, Hkv, total_k, D));
    float* sw = (float*)w;    w += up256(sizeof(float) * (size_t)B * (Hq + Hkv));
    unsigned* amax = (unsigned*)w;
    VarlenQuant qa;
    qa.x[0] = (const unsigned char*)q; qa.x[1] = (const unsigned char*)k;
    qa.ts[0] = st6[0]; qa.hs[0] = st6[1]; qa.ts[1] = st6[2]; qa.hs[1] = st6[3];
    qa.cu[0] = cu_seqlens_q; qa.cu[1] = cu_seqlens_k; qa.used = seqused_k;
    qa.total[0] = total_q; qa.total[1] = total_k; qa.H[0] = Hq; qa.H[1] = Hkv; qa.B = B;
    qa.amax[0] = amax; qa.amax[1] = amax + (size_t)B * Hq;
    qa.x8[0] = q8 ? (unsigned char*)q8 : q8w; qa.x8[1] = k8 ? (unsigned char*)k8 : k8w;
    qa.scale[0] = scale_q ? scale_q : sw; qa.scale[1] = scale_k ? scale_k : sw + (size_t)B * Hq;
    VarlenAttn a;
    a.q8 = qa.x8[0]; a.k8 = qa.x8[1]; a.v = (const unsigned char*)v;
    a.v_ts = 2 * st6[4]; a.v_hs = 2 * st6[5];
    a.out = out; a.lse = lse; a.sq = qa.scale[0]; a.sk = qa.scale[1];
    a.cu_q = cu_seqlens_q; a.cu_k = cu_seqlens_k; a.used = seqused_k;
    a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.total_q = total_q; a.total_k = total_k;
    a.nblk = B + ceil_div(total_q, kQPerWG);
    a.out_fmt = in_fmt;
    a.xcd_remap = (Hq % 8 == 0 && xcd_count() == 8) ? 1 : 0;   // (the XCD-contiguous map assumes 8 XCDs; a speed assumption only)
    const float sm = sm_scale > 0.0f ? sm_scale : 1.0f / sqrtf((float)D);
    a.sm_log2e = sm * 1.4426950408889634f;
    if (zero_words(amax, (long)B * (Hq + Hkv), st) != hipSuccess) return QATTN_ERR_LAUNCH;
    int rc;
    if (smooth) {   // K first, in launches of its own (mean, abs-max, quantise on k - mean), then q through the plain two
        rc = launch_varlen_smooth_k(k, (long)st6[2], (long)st6[3], in_fmt, cu_seqlens_k, seqused_k, B, Hkv, total_k, D, fp8_fmt, numerics, qa.x8[1],
                                    qa.scale[1], k_mean, qa.amax[1], reinterpret_cast<float*>((unsigned char*)workspace + up256(plain_bytes)), st);
        if (rc != QATTN_OK) return rc;
    }
    if (D == 64) rc = launch_varlen<64>(qa, a, in_fmt, fp8_fmt, numerics, is_causal, st, smooth, window);
    else if (D == 128) rc = launch_varlen<128>(qa, a, in_fmt, fp8_fmt, numerics, is_causal, st, smooth, window);
    else rc = launch_varlen<256>(qa, a, in_fmt, fp8_fmt, numerics, is_causal, st, smooth, window);
    if (rc != QATTN_OK) return rc;
    if (hipGetLastError() != hipSuccess) return QATTN_ERR_LAUNCH;
    if (!smooth || !lse) return QATTN_OK;
    // the launch wrote the LSE of the smoothed scores; the true scores of a row lie sm_scale * q.m higher
    return launch_varlen_smooth_lse(q, (long)st6[0], (long)st6[1], in_fmt, cu_seqlens_q, k_mean, lse, B, Hq, Hkv, total_q, D, sm, st);
}

extern "C" int qattn_fp8_quant_attention_varlen_forward(const void* q, const void* k, const void* v, const long long* strides, int in_fmt, void* out,
                                                        float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k, const int* seqused_k, int B,
                                                        int Hq, int Hkv, int total_q, int total_k, int D, int fp8_fmt, int numerics, int is_causal,
                                                        float sm_scale, void* q8, void* k8, float* scale_q, float* scale_k, void* workspace,
                                                        size_t workspace_bytes, void* stream) {
    return varlen_forward_impl(q, k, v, strides, in_fmt, out, lse, cu_seqlens_q, cu_seqlens_k, seqused_k, B, Hq, Hkv, total_q, total_k, D, fp8_fmt,
                               numerics, is_causal, sm_scale, q8, k8, scale_q, scale_k, workspace, workspace_bytes, stream, nullptr, nullptr);
}

// The varlen entry with key smoothing (include/qattn_varlen.h; the idea: include/qattn_smooth.h): every sequence's K is quantised as fp32(k) - the channel mean of its used keys.
extern "C" int qattn_fp8_quant_attention_varlen_forward_smooth(const void* q, const void* k, const void* v, const long long* strides, int in_fmt,
                                                               void* out, float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k,
                                                               const int* seqused_k, int B, int Hq, int Hkv, int total_q, int total_k, int D,
                                                               int fp8_fmt, int numerics, int is_causal, float sm_scale, void* q8, void* k8,
                                                               float* scale_q, float* scale_k, void* workspace, size_t workspace_bytes, void* stream,
                                                               float* k_mean) {
    if (!k_mean) return QATTN_ERR_INVALID_ARG;
    return varlen_forward_impl(q, k, v, strides, in_fmt, out, lse, cu_seqlens_q, cu_seqlens_k, seqused_k, B, Hq, Hkv, total_q, total_k, D, fp8_fmt,
                               numerics, is_causal, sm_scale, q8, k8, scale_q, scale_k, workspace, workspace_bytes, stream, k_mean, nullptr);
}

// (at the end of the unit: the kernels above keep the order in which the entries first ask for them, and with it the unit's device code)
// q's slice (z = 0) of the two pre-pass launches: the skip_k grids of launch_varlen_d
template <int D, int IN_FMT, int OUT_FMT>
static void launch_varlen_quant_q_fmt(const VarlenQuant& qa, int numerics, hipStream_t st) {
    hipLaunchKernelGGL((varlen_amax_kernel<D, IN_FMT>), dim3((unsigned)(qa.B + ceil_div(qa.total[0], kVarlenAmaxRows)), qa.H[0], 1), dim3(256), 0, st, qa);
    hipLaunchKernelGGL((varlen_quant_kernel<D, IN_FMT, OUT_FMT>), dim3((unsigned)(qa.B + ceil_div(qa.total[0], kVarlenQuantRows)), qa.H[0], 1), dim3(256),
                       0, st, qa, numerics);
}
template <int D>
static void launch_varlen_quant_q(const VarlenQuant& qa, int in_fmt, int fp8_fmt, int numerics, hipStream_t st) {
    if (in_fmt == QATTN_FMT_BF16) {
        if (fp8_fmt == QATTN_FMT_E4M3) launch_varlen_quant_q_fmt<D, QATTN_FMT_BF16, QATTN_FMT_E4M3>(qa, numerics, st);
        else launch_varlen_quant_q_fmt<D, QATTN_FMT_BF16, QATTN_FMT_E5M2>(qa, numerics, st);
    } else {
        if (fp8_fmt == QATTN_FMT_E4M3) launch_varlen_quant_q_fmt<D, QATTN_FMT_FP16, QATTN_FMT_E4M3>(qa, numerics, st);
        else launch_varlen_quant_q_fmt<D, QATTN_FMT_FP16, QATTN_FMT_E5M2>(qa, numerics, st);
    }
}

// The packed pre-pass on q ALONE (the skip_k grids): zeroing node, abs-max, quantise -- for a caller whose keys are prepared already
// (qattn_paged_varlen_splitkv_fp8.hip).  Arguments are the caller's to check: D supported, formats valid, total >= 1, B >= 1.
int qattn::varlen_quant_q(const void* q16, long token_stride, long head_stride, int in_fmt, const int* cu_seqlens_q, int B, int Hq, int total_q, int D,
                   int fp8_fmt, int numerics, unsigned* amax, void* q8, float* scale_q, hipStream_t st) {
    VarlenQuant qa;
    __builtin_memset(&qa, 0, sizeof(qa));
    qa.x[0] = (const unsigned char*)q16;
    qa.ts[0] = token_stride; qa.hs[0] = head_stride;
    qa.cu[0] = cu_seqlens_q;
    qa.total[0] = total_q; qa.H[0] = Hq; qa.B = B;
    qa.amax[0] = amax; qa.x8[0] = (unsigned char*)q8; qa.scale[0] = scale_q;
    if (zero_words(amax, (long)B * Hq, st) != hipSuccess) return QATTN_ERR_LAUNCH;
    if (D == 64) launch_varlen_quant_q<64>(qa, in_fmt, fp8_fmt, numerics, st);
    else if (D == 128) launch_varlen_quant_q<128>(qa, in_fmt, fp8_fmt, numerics, st);
    else launch_varlen_quant_q<256>(qa, in_fmt, fp8_fmt, numerics, st);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

// qattn_smooth_k.hip -- key smoothing for the fused fp8 step (include/qattn_smooth.h), gfx950: the channel mean of K over the sequence,
// and K's abs-max pass and quantise pass on ks = fp32(k) - mean.  q and V keep going through the pre-pass of qattn_quant.hip; K rides in
// the launches below.  All of them are HBM-bound byte work like the pre-pass: 16-byte non-temporal loads, kAmaxInFlight of them in
// flight per thread, per-channel sums kept in REGISTERS (a thread always sees the same 8 channels) and folded across lanes by __shfl_xor;
// LDS only carries the four wave results of a block (and the KFRAG image of the quantise pass, padded as in quant_multi_kernel).
// Deterministic: per-block partials in the workspace, added in a fixed order by the consumer (as QuantJob::part); no atomics.
#include "qattn_smooth_dev.h"
#include "../../include/qattn_smooth.h"

namespace qattn {

struct SmoothK {
    const uint4* k;        // 16-bit K, [B,Hkv,Skv,D] or a strided view of it
    int G, H, S;           // G = B * Hkv heads of S rows
    long sb, sh, ss;       // 16-byte vectors between batches, heads, rows
    float* mean_part;      // [G][nmean][D] per-block channel sums
    int nmean;
    float* mean;           // [G][D]
    unsigned* amax_part;   // head-wise: [G][kMomentSplits] fp32 bits of every block's max |ks| (nsplit valid per head)
    float* part;           // head-wise AUTO (else nullptr): [G][kMomentSplits] every block's sum of ks^2
    int nsplit;
    uint4* k8;             // KFRAG payload
    float* scale;          // [G] or [G][S]
    int token;
};
__device__ __forceinline__ const uint4* smooth_head(const SmoothK& p, int g) { return p.k + (long)(g / p.H) * p.sb + (long)(g % p.H) * p.sh; }

// ---- pass 1: per-block channel sums.  grid = (nmean, G), block = 256.
template <int IN_FMT, int D, bool SV>
__global__ __launch_bounds__(256) void kmean_partial_kernel(const SmoothK p) {
    constexpr int VPR = D / 8;
    const int g = blockIdx.y, tid = threadIdx.x;
    const int per = rows_per_block<D>(p.S, p.nmean);
    const int first = (int)blockIdx.x * per, last = min(p.S, first + per);
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for_my_rows<D, SV>(smooth_head(p, g), p.ss, first, last, [&](const uint4& raw) {
        float f[8];
        unpack8<IN_FMT>(raw, f);
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j] += f[j];
    });
    // lanes l, l + VPR, l + 2 VPR, ... of a wave hold the same channels
#pragma unroll
    for (int off = 32; off >= VPR; off >>= 1) {
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j] += __shfl_xor(acc[j], off);
    }
    __shared__ __attribute__((aligned(16))) float red[4][D];
    if ((tid & 63) < VPR) {
        float4* dst = reinterpret_cast<float4*>(&red[tid >> 6][(tid & 63) * 8]);
        dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
    __syncthreads();
    // (a block past the end of the head writes zeros: nothing is cleared beforehand)
    if (tid < D) p.mean_part[((long)g * p.nmean + blockIdx.x) * D + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// ---- pass 1b: the partial sums of a head in block order, divided by the number of rows.  grid = G, block = D.
__global__ void kmean_final_kernel(const SmoothK p, int D) {
    const int g = blockIdx.x, d = threadIdx.x;
    const float* part = p.mean_part + (long)g * p.nmean * D + d;
    float s = 0.0f;
    for (int i = 0; i < p.nmean; i++) s += part[(long)i * D];
    p.mean[(long)g * D + d] = s / (float)p.S;
}

// ---- pass 2 (head-wise scales): max |ks| and, for the score-spread forecast, the sum of ks^2 of every block's share.
// grid = (nsplit, G), block = 256; the results land where amax_multi_kernel leaves K's (the quantise pass below and the attention
// prologue read them from there).  |ks| as fp32 bits under an unsigned max: a NaN outranks everything, as in the pre-pass.
template <int IN_FMT, int D, bool SV>
__global__ __launch_bounds__(256) void smooth_amax_kernel(const SmoothK p) {
    constexpr int VPR = D / 8;
    const int g = blockIdx.y, tid = threadIdx.x;
    const int per = rows_per_block<D>(p.S, p.nsplit);
    const int first = (int)blockIdx.x * per, last = min(p.S, first + per);
    float m[8];
    load_mean8(p.mean + (long)g * D + (tid % VPR) * 8, m);
    const bool moments = p.part != nullptr;
    unsigned amax = 0u;
    float s0 = 0.0f, s1 = 0.0f;
    for_my_rows<D, SV>(smooth_head(p, g), p.ss, first, last, [&](const uint4& raw) {
        float f[8];
        unpack8<IN_FMT>(raw, f);
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const float a = f[j] - m[j], b = f[j + 1] - m[j + 1];
            amax = max(amax, max(__float_as_uint(a) & 0x7fffffffu, __float_as_uint(b) & 0x7fffffffu));
            if (moments) { s0 = __builtin_fmaf(a, a, s0); s1 = __builtin_fmaf(b, b, s1); }
        }
    });
    float ss = s0 + s1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        amax = max(amax, (unsigned)__shfl_xor((int)amax, off));
        if (moments) ss += __shfl_xor(ss, off);
    }
    __shared__ unsigned red[4];
    __shared__ float red_ss[4];
    if ((tid & 63) == 0) { red[tid >> 6] = amax; red_ss[tid >> 6] = ss; }
    __syncthreads();
    if (tid == 0) {
        p.amax_part[(long)g * kMomentSplits + blockIdx.x] = max(max(red[0], red[1]), max(red[2], red[3]));
        if (moments) p.part[(long)g * kMomentSplits + blockIdx.x] = (red_ss[0] + red_ss[1]) + (red_ss[2] + red_ss[3]);
    }
}

// ---- pass 3: ks -> fp8 in KFRAG order, one 64-key chunk per block (K's share of quant_multi_kernel).  grid = (ceil(S / 64), G), block = 256.
template <int D, int IN_FMT, int OUT_FMT, bool SV>
__global__ __launch_bounds__(256) void smooth_quant_k_kernel(const SmoothK p, int numerics) {
    constexpr int VPR = D / 8;
    constexpr int ITERS = 64 * VPR / 256;
    constexpr int KPAD = 64 * D + (64 * D / 512) * 16;   // KFRAG image + 16 B per 512 B (conflict-free 8-byte writes, linear copy-out)
    __shared__ __attribute__((aligned(16))) unsigned char img[KPAD];
    const int tid = threadIdx.x, S = p.S;
    const int g = p.G - 1 - (int)blockIdx.y, tile = (S + 63) / 64 - 1 - (int)blockIdx.x;   // (downwards, as the pre-pass: the abs-max pass's last bytes first)
    const bool token = p.token != 0;
    const float inv_qmax = (float)(1.0 / (double)(OUT_FMT == QATTN_FMT_E4M3 ? 448.0 : 57344.0));
    float scale = 1.0f;
    if (!token) {
        const unsigned amax_bits = max_partials(p.amax_part + (long)g * kMomentSplits, p.nsplit, tid & 63);
        scale = make_scale(__uint_as_float(amax_bits), inv_qmax, numerics, IN_FMT);
        if (tile == 0 && tid == 0) p.scale[g] = scale;
    }
    float rinv = 1.0f / scale;
    const int dv = tid % VPR, row0 = tile * 64;
    float m[8];
    load_mean8(p.mean + (long)g * D + dv * 8, m);
    const uint4* xg = smooth_head(p, g);
    const long row_vecs = SV ? p.ss : (long)VPR;
    uint4 held[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int row = row0 + (it * 256 + tid) / VPR;
        held[it] = make_uint4(0, 0, 0, 0);
        if (row < S) held[it] = load_nt(xg + (long)row * row_vecs + dv);
    }
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int r = (it * 256 + tid) / VPR, row = row0 + r;
        float ks[8];
        unpack8<IN_FMT>(held[it], ks);
#pragma unroll
        for (int j = 0; j < 8; j++) ks[j] = row < S ? ks[j] - m[j] : 0.0f;   // the padding rows of the last chunk stay zero bytes
        if (token) {
            unsigned ab = 0u;
#pragma unroll
            for (int j = 0; j < 8; j++) ab = max(ab, __float_as_uint(ks[j]) & 0x7fffffffu);
#pragma unroll
            for (int off = VPR / 2; off > 0; off >>= 1) ab = max(ab, (unsigned)__shfl_xor((int)ab, off));
            scale = make_scale(__uint_as_float(ab), inv_qmax, numerics, IN_FMT);
            if (dv == 0 && row < S) p.scale[(long)g * S + row] = scale;
            rinv = 1.0f / scale;
        }
        const int2 lohi = quant8_f32<IN_FMT, OUT_FMT>(ks, scale, rinv);
        const int o = kfrag_offset<D>(r, dv * 8);
        *reinterpret_cast<int2*>(img + o + ((o >> 9) << 4)) = lohi;
    }
    __syncthreads();
    const long Sp = (long)((S + 63) / 64) * 64;
    uint4* og = p.k8 + ((long)g * Sp + row0) * (D / 16);
    for (int i = tid; i < 64 * D / 16; i += 256) og[i] = *reinterpret_cast<const uint4*>(img + i * 16 + ((i >> 5) << 4));
}

// ---- LSE of the true scores: lse[b,h,i] += mul * sum_d fp32(q[b,h,i,d]) * m[kv head of h, d].  grid = (ceil(Sq / (256 / VPR)), B * Hq).
template <int IN_FMT, int D>
__global__ __launch_bounds__(256) void smooth_lse_kernel(const uint4* q, long sb, long sh, long ss, const float* mean, float* lse, long lse_stride,
                                                         int Hq, int Hkv, int Sq, float mul) {
    constexpr int VPR = D / 8, RPB = 256 / VPR;
    const int tid = threadIdx.x, dv = tid % VPR, row = (int)blockIdx.x * RPB + tid / VPR;
    const int bh = blockIdx.y, b = bh / Hq, h = bh % Hq;
    const long kv_head = (long)b * Hkv + h / (Hq / Hkv);
    float m[8], f[8];
    load_mean8(mean + kv_head * D + dv * 8, m);
    uint4 raw = make_uint4(0, 0, 0, 0);
    if (row < Sq) raw = q[(long)b * sb + (long)h * sh + (long)row * ss + dv];
    unpack8<IN_FMT>(raw, f);
    float dot = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++) dot = __builtin_fmaf(f[j], m[j], dot);
#pragma unroll
    for (int off = VPR / 2; off > 0; off >>= 1) dot += __shfl_xor(dot, off);
    if (dv == 0 && row < Sq) lse[(long)bh * lse_stride + row] += mul * dot;
}

// ---------------------------------------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------------------------------------

size_t smooth_k_workspace_bytes(int B, int Hkv, int D) { return sizeof(float) * (size_t)B * Hkv * kMeanSplits * D; }

template <int IN_FMT, int D, bool SV>
static void launch_smooth_passes(const SmoothK& p, int out_fmt, int numerics, hipStream_t st) {
    hipLaunchKernelGGL((kmean_partial_kernel<IN_FMT, D, SV>), dim3(p.nmean, p.G), dim3(256), 0, st, p);
    hipLaunchKernelGGL(kmean_final_kernel, dim3(p.G), dim3(D), 0, st, p, D);
    if (!p.token) hipLaunchKernelGGL((smooth_amax_kernel<IN_FMT, D, SV>), dim3(p.nsplit, p.G), dim3(256), 0, st, p);
    const dim3 grid((p.S + 63) / 64, p.G);
    if (out_fmt == QATTN_FMT_E4M3) hipLaunchKernelGGL((smooth_quant_k_kernel<D, IN_FMT, QATTN_FMT_E4M3, SV>), grid, dim3(256), 0, st, p, numerics);
    else hipLaunchKernelGGL((smooth_quant_k_kernel<D, IN_FMT, QATTN_FMT_E5M2, SV>), grid, dim3(256), 0, st, p, numerics);
}

template <int IN_FMT, int D>
static void launch_smooth_passes_sv(const SmoothK& p, int out_fmt, int numerics, bool sv, hipStream_t st) {
    if (sv) launch_smooth_passes<IN_FMT, D, true>(p, out_fmt, numerics, st);
    else launch_smooth_passes<IN_FMT, D, false>(p, out_fmt, numerics, st);
}

int launch_smooth_k(const void* k, int in_fmt, void* k8, float* scale_k, float* k_mean, int B, int Hkv, int Skv, int D, int out_fmt,
                    int scale_mode, int numerics, unsigned* amax_part_k, float* part_k, int nsplit, float* mean_part, hipStream_t st,
                    const long long* kstrides) {
    const long vd = D / 8;
    SmoothK p;
    p.k = (const uint4*)k;
    p.G = B * Hkv; p.H = Hkv; p.S = Skv;
    p.sb = kstrides ? (long)(kstrides[0] / 8) : (long)Hkv * Skv * vd;
    p.sh = kstrides ? (long)(kstrides[1] / 8) : (long)Skv * vd;
    p.ss = kstrides ? (long)(kstrides[2] / 8) : vd;
    p.mean_part = mean_part; p.nmean = mean_splits(Skv, D); p.mean = k_mean;
    p.amax_part = amax_part_k; p.part = part_k; p.nsplit = nsplit;
    p.k8 = (uint4*)k8; p.scale = scale_k; p.token = scale_mode == QATTN_SCALE_TOKEN;
    const bool sv = kstrides != nullptr;
    const bool bf = in_fmt == QATTN_FMT_BF16;
    if (D == 64) { if (bf) launch_smooth_passes_sv<QATTN_FMT_BF16, 64>(p, out_fmt, numerics, sv, st); else launch_smooth_passes_sv<QATTN_FMT_FP16, 64>(p, out_fmt, numerics, sv, st); }
    else if (D == 128) { if (bf) launch_smooth_passes_sv<QATTN_FMT_BF16, 128>(p, out_fmt, numerics, sv, st); else launch_smooth_passes_sv<QATTN_FMT_FP16, 128>(p, out_fmt, numerics, sv, st); }
    else if (D == 256) { if (bf) launch_smooth_passes_sv<QATTN_FMT_BF16, 256>(p, out_fmt, numerics, sv, st); else launch_smooth_passes_sv<QATTN_FMT_FP16, 256>(p, out_fmt, numerics, sv, st); }
    else return QATTN_ERR_UNSUPPORTED_DIM;
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

int launch_smooth_lse(const void* q, int in_fmt, const float* k_mean, float* lse, long lse_stride, int B, int Hq, int Hkv, int Sq, int D,
                      float mul, hipStream_t st, const long long* qstrides) {
    const long vd = D / 8;
    const long sb = qstrides ? (long)(qstrides[0] / 8) : (long)Hq * Sq * vd, sh = qstrides ? (long)(qstrides[1] / 8) : (long)Sq * vd;
    const long ss = qstrides ? (long)(qstrides[2] / 8) : vd;
    const int rpb = 256 / (D / 8);
    const dim3 grid((Sq + rpb - 1) / rpb, B * Hq), block(256);
    const uint4* qp = (const uint4*)q;
#define QATTN_SL(FMT, DD) hipLaunchKernelGGL((smooth_lse_kernel<FMT, DD>), grid, block, 0, st, qp, sb, sh, ss, k_mean, lse, lse_stride, Hq, Hkv, Sq, mul)
    const bool bf = in_fmt == QATTN_FMT_BF16;
    if (D == 64) { if (bf) QATTN_SL(QATTN_FMT_BF16, 64); else QATTN_SL(QATTN_FMT_FP16, 64); }
    else if (D == 128) { if (bf) QATTN_SL(QATTN_FMT_BF16, 128); else QATTN_SL(QATTN_FMT_FP16, 128); }
    else if (D == 256) { if (bf) QATTN_SL(QATTN_FMT_BF16, 256); else QATTN_SL(QATTN_FMT_FP16, 256); }
    else return QATTN_ERR_UNSUPPORTED_DIM;
#undef QATTN_SL
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

}  // namespace qattn

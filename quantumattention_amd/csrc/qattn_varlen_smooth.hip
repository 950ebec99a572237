// qattn_varlen_smooth.hip -- key smoothing for packed variable-length sequences (qattn_fp8_quant_attention_varlen_forward_smooth,
// include/qattn_varlen.h), gfx950: K's share of the varlen quant launches on ks = fp32(k) - the channel mean of the sequence's USED keys.
//
// The contract is "per sequence, bit for bit, what the dense smoothing entry (qattn_smooth_k.hip) leaves for that sequence alone":
//   mean   the sums of kmean_partial_kernel / kmean_final_kernel on a head of L rows: mean_splits(L, D) blocks with rows_per_block<D>
//          shares, evaluated per sequence ON THE DEVICE from the clamped tables (grid (kMeanSplits, Hkv, B): blocks at or past a
//          sequence's split count write nothing), the same row walk and shuffle / LDS folds (qattn_smooth_dev.h), the valid partials
//          added in block order, one division by L.  No used key: mean 0.
//   amax   max |ks| per (sequence, kv head) over the 256-row varlen tiles: one atomicMax per tile on fp32 bits (order-independent, so
//          the maximum over the dense entry's per-block words)
//   quant  64-row varlen tiles into the sequence's KFRAG image with quant8_f32 of the dense quantise pass; padding rows zero bytes
//   lse    lse[h, t] += mul * sum_d fp32(q[t,h,d]) * mean[seq(t), kv(h), d] with the per-row arithmetic of smooth_lse_kernel
// All of it HBM-bound byte work: 16-byte non-temporal loads, kAmaxInFlight in flight per thread, channel sums in registers, no float
// atomics.  No length is read on the host.
#include "qattn_smooth_dev.h"
#include "qattn_varlen_tile.h"

namespace qattn {

struct VarlenSmoothK {
    const unsigned char* k;   // 16-bit K [total_k, Hkv, D] or a strided view
    long ts, hs;              // element strides of token and head (multiples of 8)
    const int* cu;            // cu_seqlens_k
    const int* used;          // seqused_k or nullptr
    int total, H, B;          // total_k, Hkv, sequences
    float* mean_part;         // [B][Hkv][kMeanSplits][D] per-block channel sums (mean_splits(L, D) valid per sequence)
    float* mean;              // [B][Hkv][D]
    unsigned* amax;           // [B][Hkv] fp32 bits of max |ks|, zeroed before the abs-max pass
    unsigned char* k8;        // KFRAG images
    float* scale;             // [B][Hkv]
};

// sequence i's clamped first key and used length (include/qattn_varlen.h; as varlen_tile)
__device__ __forceinline__ void varlen_extent(const int* cu, const int* used, int total, int i, int& start, int& len) {
    start = clampi(__builtin_amdgcn_readfirstlane(cu[i]), 0, total);
    len = clampi(__builtin_amdgcn_readfirstlane(cu[i + 1]), start, total) - start;
    if (used) len = clampi(__builtin_amdgcn_readfirstlane(used[i]), 0, len);
}

// ---- pass 1: kmean_partial_kernel on sequence blockIdx.z as a head of `len` rows.  grid = (kMeanSplits, Hkv, B), block = 256.
template <int IN_FMT, int D>
__global__ __launch_bounds__(256) void varlen_kmean_partial_kernel(const VarlenSmoothK p) {
    constexpr int VPR = D / 8;
    const int i = blockIdx.z, h = blockIdx.y, tid = threadIdx.x;
    int start, len;
    varlen_extent(p.cu, p.used, p.total, i, start, len);
    const int nmean = mean_splits(len, D);
    if ((int)blockIdx.x >= nmean) return;
    const int per = rows_per_block<D>(len, nmean);
    const int first = (int)blockIdx.x * per, last = min(len, first + per);
    const uint4* xg = reinterpret_cast<const uint4*>(p.k + 2 * ((long)start * p.ts + (long)h * p.hs));
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for_my_rows<D, true>(xg, p.ts / 8, first, last, [&](const uint4& raw) {
        float f[8];
        unpack8<IN_FMT>(raw, f);
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j] += f[j];
    });
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
    // (a block past the end of the sequence but below its split count writes zeros, as in the dense pass)
    if (tid < D) p.mean_part[(((long)i * p.H + h) * kMeanSplits + blockIdx.x) * D + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// ---- pass 1b: kmean_final_kernel per sequence: its valid partials in block order, one division by its length.  grid = (Hkv, B), block = D.
__global__ void varlen_kmean_final_kernel(const VarlenSmoothK p, int D) {
    const int i = blockIdx.y, h = blockIdx.x, d = threadIdx.x;
    int start, len;
    varlen_extent(p.cu, p.used, p.total, i, start, len);
    const long g = (long)i * p.H + h;
    float m = 0.0f;   // no used key: 0, not 0 / 0
    if (len > 0) {
        const int nmean = mean_splits(len, D);
        const float* part = p.mean_part + g * kMeanSplits * D + d;
        float s = 0.0f;
        for (int b = 0; b < nmean; b++) s += part[(long)b * D];
        m = s / (float)len;
    }
    p.mean[g * D + d] = m;
}

// ---- pass 2: max |fp32(k) - mean| of a 256-row tile.  grid = (B + ceil(total_k / 256), Hkv), block = 256.
template <int IN_FMT, int D>
__global__ __launch_bounds__(256) void varlen_smooth_amax_kernel(const VarlenSmoothK p) {
    constexpr int VPR = D / 8, RPI = 256 / VPR;
    const int h = blockIdx.y, tid = threadIdx.x;
    const VarlenTile t = varlen_tile<kVarlenAmaxRows>(p.cu, p.used, p.B, p.total, (int)blockIdx.x);
    if (t.tile < 0 || t.tile * kVarlenAmaxRows >= t.len) return;
    const int first = t.tile * kVarlenAmaxRows, last = min(t.len, first + kVarlenAmaxRows);
    const long g = (long)t.i * p.H + h;
    float m[8];
    load_mean8(p.mean + g * D + (tid % VPR) * 8, m);
    const uint4* xg = reinterpret_cast<const uint4*>(p.k + 2 * ((long)t.start * p.ts + (long)h * p.hs));
    unsigned amax = 0u;
    static_assert(kVarlenAmaxRows % RPI == 0, "a tile is a whole number of block steps");
    for_my_rows<D, true>(xg, p.ts / 8, first, last, [&](const uint4& raw) {
        float f[8];
        unpack8<IN_FMT>(raw, f);
#pragma unroll
        for (int j = 0; j < 8; j++) amax = max(amax, __float_as_uint(f[j] - m[j]) & 0x7fffffffu);   // (a NaN outranks everything, as in the dense pass)
    });
    amax = wave_allmax_u32(amax);
    __shared__ unsigned red[4];
    if ((tid & 63) == 0) red[tid >> 6] = amax;
    __syncthreads();
    if (tid == 0) atomicMax(p.amax + g, max(max(red[0], red[1]), max(red[2], red[3])));
}

// ---- pass 3: ks -> fp8, one 64-key chunk of a sequence's KFRAG image per block (smooth_quant_k_kernel, head-wise, on the varlen tile map).
// grid = (B + ceil(total_k / 64), Hkv), block = 256.
template <int D, int IN_FMT, int OUT_FMT>
__global__ __launch_bounds__(256) void varlen_smooth_quant_k_kernel(const VarlenSmoothK p, int numerics) {
    constexpr int VPR = D / 8;
    constexpr int ITERS = 64 * VPR / 256;
    constexpr int KPAD = 64 * D + (64 * D / 512) * 16;   // KFRAG image + 16 B per 512 B, as the dense pass
    __shared__ __attribute__((aligned(16))) unsigned char img[KPAD];
    const int h = blockIdx.y, tid = threadIdx.x, H = p.H;
    const VarlenTile t = varlen_tile<kVarlenQuantRows>(p.cu, p.used, p.B, p.total, (int)blockIdx.x);
    if (t.tile < 0) return;
    const long g = (long)t.i * H + h;
    const float inv_qmax = (float)(1.0 / (double)(OUT_FMT == QATTN_FMT_E4M3 ? 448.0 : 57344.0));
    const float scale = make_scale(__uint_as_float(p.amax[g]), inv_qmax, numerics, IN_FMT);
    if (t.tile == 0 && tid == 0) p.scale[g] = scale;   // (also for a sequence without used keys: amax 0 -> eps)
    if (t.tile * kVarlenQuantRows >= t.len) return;
    const float rinv = 1.0f / scale;
    const int dv = tid % VPR, row0 = t.tile * kVarlenQuantRows, S = t.len;
    float m[8];
    load_mean8(p.mean + g * D + dv * 8, m);
    const uint4* xg = reinterpret_cast<const uint4*>(p.k + 2 * ((long)t.start * p.ts + (long)h * p.hs));
    const long row_vecs = p.ts / 8;
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
        const int2 lohi = quant8_f32<IN_FMT, OUT_FMT>(ks, scale, rinv);
        const int o = kfrag_offset<D>(r, dv * 8);
        *reinterpret_cast<int2*>(img + o + ((o >> 9) << 4)) = lohi;
    }
    __syncthreads();
    // sequence i's image: [Hkv, ceil(L/64) 64, D] at element Hkv D (start + 64 i)
    const long Lp = (long)((S + 63) / 64) * 64;
    uint4* og = reinterpret_cast<uint4*>(p.k8 + (long)H * D * (t.start + 64L * t.i) + ((long)h * Lp + row0) * D);
    for (int i = tid; i < 64 * D / 16; i += 256) og[i] = *reinterpret_cast<const uint4*>(img + i * 16 + ((i >> 5) << 4));
}

// ---- LSE of the true scores in the packed layout: lse[h, t] += mul * sum_d fp32(q[t,h,d]) * mean[seq(t), kv head of h, d].
// grid = (ceil(total_q / (256 / VPR)), Hq), block = 256.  Tokens outside every sequence and rows whose LSE is -inf are left alone.
template <int IN_FMT, int D>
__global__ __launch_bounds__(256) void varlen_smooth_lse_kernel(const unsigned char* q, long ts, long hs, const int* cu_q, const float* mean,
                                                                float* lse, int B, int Hq, int Hkv, int total_q, float mul) {
    constexpr int VPR = D / 8, RPB = 256 / VPR;
    const int tid = threadIdx.x, dv = tid % VPR, row = (int)blockIdx.x * RPB + tid / VPR, h = blockIdx.y;
    const int tok = min(row, total_q - 1);
    int lo = 0, hi = B - 1;
    while (lo < hi) {   // the largest i with start_i <= tok (the rows of a block may lie in different sequences: per lane)
        const int mid = (lo + hi + 1) >> 1;
        if (clampi(cu_q[mid], 0, total_q) <= tok) lo = mid;
        else hi = mid - 1;
    }
    const int start = clampi(cu_q[lo], 0, total_q), end = clampi(cu_q[lo + 1], start, total_q);
    const bool live = row < total_q && tok >= start && tok < end;
    float m[8], f[8];
    load_mean8(mean + ((long)lo * Hkv + h / (Hq / Hkv)) * D + dv * 8, m);
    uint4 raw = make_uint4(0, 0, 0, 0);
    if (live) raw = *reinterpret_cast<const uint4*>(q + 2 * ((long)tok * ts + (long)h * hs) + 16 * dv);
    unpack8<IN_FMT>(raw, f);
    float dot = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++) dot = __builtin_fmaf(f[j], m[j], dot);
#pragma unroll
    for (int off = VPR / 2; off > 0; off >>= 1) dot += __shfl_xor(dot, off);
    if (dv == 0 && live) {
        float* l = lse + (long)h * total_q + tok;
        const float old = *l;
        if (old != -INFINITY) *l = old + mul * dot;
    }
}

// ---------------------------------------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------------------------------------
size_t varlen_smooth_k_workspace_bytes(int B, int Hkv, int D) { return sizeof(float) * (size_t)B * Hkv * kMeanSplits * D; }

template <int IN_FMT, int D>
static void launch_varlen_smooth_passes(const VarlenSmoothK& p, int out_fmt, int numerics, hipStream_t st) {
    hipLaunchKernelGGL((varlen_kmean_partial_kernel<IN_FMT, D>), dim3(kMeanSplits, p.H, p.B), dim3(256), 0, st, p);
    hipLaunchKernelGGL(varlen_kmean_final_kernel, dim3(p.H, p.B), dim3(D), 0, st, p, D);
    hipLaunchKernelGGL((varlen_smooth_amax_kernel<IN_FMT, D>), dim3((unsigned)(p.B + ceil_div(p.total, kVarlenAmaxRows)), p.H), dim3(256), 0, st, p);
    const dim3 grid((unsigned)(p.B + ceil_div(p.total, kVarlenQuantRows)), p.H);
    if (out_fmt == QATTN_FMT_E4M3) hipLaunchKernelGGL((varlen_smooth_quant_k_kernel<D, IN_FMT, QATTN_FMT_E4M3>), grid, dim3(256), 0, st, p, numerics);
    else hipLaunchKernelGGL((varlen_smooth_quant_k_kernel<D, IN_FMT, QATTN_FMT_E5M2>), grid, dim3(256), 0, st, p, numerics);
}

int launch_varlen_smooth_k(const void* k, long ts, long hs, int in_fmt, const int* cu_k, const int* used, int B, int Hkv, int total_k, int D,
                           int out_fmt, int numerics, void* k8, float* scale_k, float* k_mean, unsigned* amax_k, float* mean_part, hipStream_t st) {
    VarlenSmoothK p;
    p.k = (const unsigned char*)k; p.ts = ts; p.hs = hs; p.cu = cu_k; p.used = used;
    p.total = total_k; p.H = Hkv; p.B = B;
    p.mean_part = mean_part; p.mean = k_mean; p.amax = amax_k; p.k8 = (unsigned char*)k8; p.scale = scale_k;
    const bool bf = in_fmt == QATTN_FMT_BF16;
    if (D == 64) { if (bf) launch_varlen_smooth_passes<QATTN_FMT_BF16, 64>(p, out_fmt, numerics, st); else launch_varlen_smooth_passes<QATTN_FMT_FP16, 64>(p, out_fmt, numerics, st); }
    else if (D == 128) { if (bf) launch_varlen_smooth_passes<QATTN_FMT_BF16, 128>(p, out_fmt, numerics, st); else launch_varlen_smooth_passes<QATTN_FMT_FP16, 128>(p, out_fmt, numerics, st); }
    else if (D == 256) { if (bf) launch_varlen_smooth_passes<QATTN_FMT_BF16, 256>(p, out_fmt, numerics, st); else launch_varlen_smooth_passes<QATTN_FMT_FP16, 256>(p, out_fmt, numerics, st); }
    else return QATTN_ERR_UNSUPPORTED_DIM;
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

int launch_varlen_smooth_lse(const void* q, long ts, long hs, int in_fmt, const int* cu_q, const float* k_mean, float* lse, int B, int Hq, int Hkv,
                             int total_q, int D, float mul, hipStream_t st) {
    if (total_q <= 0) return QATTN_OK;
    const int rpb = 256 / (D / 8);
    const dim3 grid((unsigned)ceil_div(total_q, rpb), Hq), block(256);
    const unsigned char* qp = (const unsigned char*)q;
#define QATTN_VSL(FMT, DD) hipLaunchKernelGGL((varlen_smooth_lse_kernel<FMT, DD>), grid, block, 0, st, qp, ts, hs, cu_q, k_mean, lse, B, Hq, Hkv, total_q, mul)
    const bool bf = in_fmt == QATTN_FMT_BF16;
    if (D == 64) { if (bf) QATTN_VSL(QATTN_FMT_BF16, 64); else QATTN_VSL(QATTN_FMT_FP16, 64); }
    else if (D == 128) { if (bf) QATTN_VSL(QATTN_FMT_BF16, 128); else QATTN_VSL(QATTN_FMT_FP16, 128); }
    else if (D == 256) { if (bf) QATTN_VSL(QATTN_FMT_BF16, 256); else QATTN_VSL(QATTN_FMT_FP16, 256); }
    else return QATTN_ERR_UNSUPPORTED_DIM;
#undef QATTN_VSL
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

}  // namespace qattn

// qattn_varlen_fp8.hip -- qattn_fp8_quant_attention_varlen_forward_fp8pv (include/qattn_varlen.h): FP8 attention on packed sequences with
// BOTH products on the FP8 matrix pipe -- Q K^T as the 16-bit-PV packed entry (qattn_varlen.hip), P.V as e4m3 P on a FP8 V that is
// quantised head-wise per (sequence, kv head) over the sequence's USED keys.
//
// Launches after a zeroing node, none of which reads a length on the host:
//   amax   per (sequence, head) abs-max of q, k and v (used keys only): qattn_varlen.hip's pass (256-row tiles, atomicMax on the fp32
//          bits) with V as a third z slice
//   quant  64-row tiles: q into its row-major slab, k into its KFRAG image -- statement for statement qattn_varlen.hip's pass, so the
//          bytes and scales are the 16-bit-PV entry's -- and v into a VFRAG image beside k's (quant8 / vfrag_offset of the dense pre-pass)
//          With key smoothing K is left out of both (qattn_varlen_smooth.hip's launches quantise it), as in the 16-bit-PV entry.
//   attn   attn_vfp8_kernel: the FP8-PV chunk sweep of qattn_fp8pv_sweep.h (shared with the block-sparse and the sliding-window kernels)
//          under the packed block map -- one 4-wave workgroup per (head, 128-row tile of a sequence) sweeps the 64-key chunks 0 .. n - 1
//          of that sequence (causal: up to the tile's diagonal), the chunk number being the loop counter; this unit keeps the map, the
//          tail / diagonal mask and the token-stride offsets.  ACCURATE: one launch.  FAST: two launches (fpv_precision_ladder) --
//          the one-term sweep for the tiles whose rows see >= kTwoTermKeys keys, the two-term sweep for the rest; a workgroup whose tile
//          belongs to the other launch returns before any DMA or barrier.  With total_k < kTwoTermKeys no tile can be one-term: one launch.
//
// Block -> (sequence, tile): qattn_varlen_tile.h with R = 128.
// The body of the entry below (varlen_fp8pv_forward_impl, declared in qattn_varlen_fp8.h with the launch's arguments) runs the
// sliding-window unit's attention launch (qattn_varlen_window_fp8.hip) behind this unit's pre-pass when it is given a window.
#include "qattn_varlen_fp8.h"
#include "qattn_varlen_tile.h"
#include "../../include/qattn_varlen.h"

namespace qattn {

// q (z = 0), k (z = 1) and v (z = 2) of one call
struct VfpQuant {
    const unsigned char* x[3];   // 16-bit inputs
    long ts[3], hs[3];           // element strides of token and head
    const int* cu[3];
    const int* used;             // seqused_k or nullptr (k and v)
    int total[3], H[3];
    int B, skip_k;               // skip_k: key smoothing quantises K in launches of its own
    unsigned* amax[3];           // [B][H] fp32 bits, zeroed before the abs-max pass
    unsigned char* x8[3];        // q8 row-major slabs / k8 KFRAG images / v8 VFRAG images
    float* scale[3];             // [B][H]
};

template <int D, int IN_FMT>
__global__ __launch_bounds__(256) void vfp_amax_kernel(const VfpQuant a) {
    constexpr int VPR = D / 8;   // 16-byte vectors per row
    const int z = blockIdx.z, h = blockIdx.y;
    if (h >= a.H[z] || (z == 1 && a.skip_k)) return;
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
__global__ __launch_bounds__(256) void vfp_quant_kernel(const VfpQuant a, int numerics) {
    constexpr int VPR = D / 8;
    constexpr int ITERS = 64 * VPR / 256;
    constexpr int KPAD = 64 * D + (64 * D / 512) * 16;   // the KFRAG image of quant_multi_kernel, padded by 16 B per 512 B
    __shared__ __attribute__((aligned(16))) unsigned char img[KPAD];
    const int z = blockIdx.z, h = blockIdx.y, tid = threadIdx.x;
    if (h >= a.H[z] || (z == 1 && a.skip_k)) return;
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
    // k / v: KFRAG / VFRAG image of the sequence, [Hkv, ceil(L/64) 64, D] at element Hkv D (start + 64 i)
    const long Lp = (long)((t.len + 63) / 64) * 64;
    uint4* og = reinterpret_cast<uint4*>(a.x8[z] + (long)H * D * (t.start + 64L * t.i) + ((long)h * Lp + row0) * D);
    if (z == 1) {
#pragma unroll
        for (int it = 0; it < ITERS; it++) {
            const int vec = it * 256 + tid, r = vec / VPR, dv = vec % VPR;
            const int2 lohi = quant8<IN_FMT, OUT_FMT>(held[it], scale, rinv);
            const int o = kfrag_offset<D>(r, dv * 8);
            *reinterpret_cast<int2*>(img + o + ((o >> 9) << 4)) = lohi;
        }
        __syncthreads();
        for (int i = tid; i < 64 * D / 16; i += 256) og[i] = *reinterpret_cast<const uint4*>(img + i * 16 + ((i >> 5) << 4));
        return;
    }
    // v: 8 consecutive d of one key land 16 bytes apart in the image (vfrag_offset); byte scatter as pack_tile_kernel (a pre-pass, not hot)
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int vec = it * 256 + tid, r = vec / VPR, dv = vec % VPR;
        const int2 lohi = quant8<IN_FMT, OUT_FMT>(held[it], scale, rinv);
        unsigned char b[8];
        __builtin_memcpy(b, &lohi, 8);
#pragma unroll
        for (int j = 0; j < 8; j++) img[vfrag_offset<D>(r, dv * 8 + j)] = b[j];
    }
    __syncthreads();
    for (int i = tid; i < 64 * D / 16; i += 256) og[i] = reinterpret_cast<const uint4*>(img)[i];
}

// BYTE / two: FpvSweep (qattn_fp8pv_sweep.h).  sel: the launch (kFpvSel*).  The sweep is the block-sparse kernel's: a non-causal
// sequence comes out with the bits of the block-sparse FP8-PV call on that sequence alone under an all-true mask.
template <int D, int FMT, bool BYTE, bool CAUSAL>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_vfp8_kernel(const VfpAttn a, const int two, const int sel) {
    constexpr int CH = 64 * D, MB = D / 32, KS = D / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    FpvSweep<D, FMT, BYTE> sw(smem);
    const int lane = sw.lane, wave = sw.wave, ql = sw.ql, hh = sw.hh;

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
    if (CAUSAL) j = a.nblk - 1 - j;   // (the last tiles of a sequence see the most keys: roughly longest first)
    const VarlenTile tq = varlen_tile<kFpvTile>(a.cu_q, nullptr, a.B, a.total_q, j);
    if (tq.tile < 0 || tq.tile * kFpvTile >= tq.len) return;   // no tile of any sequence
    const int i = tq.i;
    const int sk0 = clampi(__builtin_amdgcn_readfirstlane(a.cu_k[i]), 0, a.total_k);
    int lk = clampi(__builtin_amdgcn_readfirstlane(a.cu_k[i + 1]), sk0, a.total_k) - sk0;
    if (a.used) lk = clampi(__builtin_amdgcn_readfirstlane(a.used[i]), 0, lk);
    // keys the tile's rows see (its last row, when causal): the rule of the one-term sweep and the trip count, both workgroup-uniform
    const int keys = CAUSAL ? min(lk, kFpvTile * (tq.tile + 1)) : lk;
    if (sel == kFpvSelMany && keys < a.two_term_keys) return;
    if (sel == kFpvSelFew && keys >= a.two_term_keys) return;

    const int kvh = h / (a.Hq / a.Hkv);
    const int qrow = tq.tile * kFpvTile + wave * kQPerWave + ql;   // row within the sequence
    const bool qvalid = qrow < tq.len;
    const long orow = ((long)(tq.start + (qvalid ? qrow : 0)) * a.Hq + h) * (2L * D);   // bytes: rows are a token stride apart
    const long lrow = (long)h * a.total_q + tq.start + qrow;                           // lse / path: [Hq, total_q]
    if (keys == 0) {   // a sequence with queries and no used key
        fpv_store_empty<D>(a.out, a.out_fmt, orow, a.lse, lrow, a.path, lrow, hh, qvalid);
        return;
    }
    const int n_wg = (keys + 63) >> 6;        // chunks 0 .. n_wg - 1 (a causal tile: up to its diagonal)
    const int nch = (lk + 63) >> 6;           // chunks of the sequence's images

    const long img = (long)a.Hkv * D * (sk0 + 64L * i) + (long)kvh * nch * CH + (wave << 10);
    FpvRing<D> ring(smem, wave, lane, a.k8 + img, a.v8 + img);
    ring.dma_chunk(0);
    sw.park_q(a.q8 + (long)a.Hq * D * tq.start + ((long)h * tq.len + (qvalid ? qrow : 0)) * D + hh * 32, qvalid);
    sw.init_state(a.sm_log2e * a.sq[(long)i * a.Hq + h] * a.sk[(long)i * a.Hkv + kvh], -1.0e30f);
    const v8i ones = fpv_ones(lane);
    const int kend = CAUSAL ? min(lk, qrow + 1) : lk;   // this lane's row attends keys 0 .. kend - 1 (token-exact)
    const int diag = 2 * tq.tile;                       // causal: chunks >= diag hold keys beyond the tile's first row

    for (int t = 0; t < n_wg; t++) {   // step t sweeps chunk t
        v8i qf[KS];
        sw.read_q(qf);
        sw.wait_stage();
        if (t + 1 < n_wg) ring.dma_chunk(t + 1);
        v16f s0, s1;
        v8i vf0, vf1;
        sw.qk(t, qf, s0, s1, vf0, vf1);
        // ---- ragged tail of the sequence's keys; causal: the diagonal, by token (workgroup-uniform condition)
        const int k0 = t * 64;
        if (__builtin_expect(k0 + 64 > lk || (CAUSAL && t >= diag), 0)) {
#pragma unroll
            for (int r = 0; r < 32; r++) {
                const int key = k0 + 32 * (r >> 4) + (r & 3) + 8 * ((r & 15) >> 2) + 4 * hh;
                v16f& sx = (r >> 4) ? s1 : s0;
                sx[r & 15] = key >= kend ? -INFINITY : sx[r & 15];
            }
        }
        sw.softmax_pv(s0, s1, vf0, vf1, two, [&] { return ones; });
    }

    // ---- epilogue (V's one scale per (sequence, head) is applied here)
    const float l_tot = sw.row_sum();
    const float inv = a.sv[(long)i * a.Hkv + kvh] / l_tot;
    store_o_rows<MB>(a.out, a.out_fmt, sw.o, inv, orow, hh, qvalid);
    if (!BYTE && a.lse && hh == 0 && qvalid) a.lse[lrow] = 0.6931471805599453f * (sw.m_run * sw.c - kPShift) + __logf(l_tot);
    if (a.path && hh == 0 && qvalid) a.path[lrow] = (unsigned char)((!BYTE && two) ? QATTN_PATH_TWO_TERM : QATTN_PATH_ONE_TERM);
}

template <int D, int FMT, bool CAUSAL>
static int launch_vfp_attn(const VfpAttn& a, int precision, hipStream_t st) {
    // (total_k: more than any tile can see)
    return fpv_precision_ladder(precision, a.total_k, a.two_term_keys, a.lse != nullptr, [&](auto byte, int two, int sel) {
        return fpv_launch(attn_vfp8_kernel<D, FMT, decltype(byte)::value, CAUSAL>, (unsigned)(a.Hq * a.nblk), fpv_lds_bytes(D), st, a, two, sel);
    });
}

template <int D, int IN_FMT, int OUT_FMT>
static int launch_vfp_d(const VfpQuant& qa, const VfpAttn& a, int numerics, int causal, int precision, const int* window, hipStream_t st) {
    int tmax = qa.total[0] > qa.total[1] ? qa.total[0] : qa.total[1];
    int hmax = qa.H[0] > qa.H[1] ? qa.H[0] : qa.H[1];
    hipLaunchKernelGGL((vfp_amax_kernel<D, IN_FMT>), dim3((unsigned)(qa.B + ceil_div(tmax, kVarlenAmaxRows)), hmax, 3), dim3(256), 0, st, qa);
    hipLaunchKernelGGL((vfp_quant_kernel<D, IN_FMT, OUT_FMT>), dim3((unsigned)(qa.B + ceil_div(tmax, kVarlenQuantRows)), hmax, 3), dim3(256), 0, st, qa,
                       numerics);
    if (window) return launch_varlen_window_fp8_attn(a, D, OUT_FMT, precision, window[0], window[1], st);   // (qattn_varlen_window_fp8.hip)
    return causal ? launch_vfp_attn<D, OUT_FMT, true>(a, precision, st) : launch_vfp_attn<D, OUT_FMT, false>(a, precision, st);
}
template <int D>
static int launch_vfp(const VfpQuant& qa, const VfpAttn& a, int in_fmt, int fp8_fmt, int numerics, int causal, int precision, const int* window,
                      hipStream_t st) {
    if (in_fmt == QATTN_FMT_BF16)
        return fp8_fmt == QATTN_FMT_E4M3 ? launch_vfp_d<D, QATTN_FMT_BF16, QATTN_FMT_E4M3>(qa, a, numerics, causal, precision, window, st)
                                         : launch_vfp_d<D, QATTN_FMT_BF16, QATTN_FMT_E5M2>(qa, a, numerics, causal, precision, window, st);
    return fp8_fmt == QATTN_FMT_E4M3 ? launch_vfp_d<D, QATTN_FMT_FP16, QATTN_FMT_E4M3>(qa, a, numerics, causal, precision, window, st)
                                     : launch_vfp_d<D, QATTN_FMT_FP16, QATTN_FMT_E5M2>(qa, a, numerics, causal, precision, window, st);
}

}  // namespace qattn

using namespace qattn;

namespace {
// the VFRAG images take the room of the KFRAG images: a 64-key chunk is 64 D bytes in both layouts
size_t vfp_v8_bytes(int B, int Hkv, int total_k, int D) { return qattn_varlen_tensor_bytes(QATTN_LAYOUT_KFRAG, B, Hkv, total_k, D); }
bool vfp_dims_ok(int B, int Hq, int Hkv, int total_q, int total_k) { return B >= 1 && Hq > 0 && Hkv > 0 && total_q >= 0 && total_k >= 0; }
}  // namespace

extern "C" size_t qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int D) {
    if (!vfp_dims_ok(B, Hq, Hkv, total_q, total_k) || (D != 64 && D != 128 && D != 256)) return 0;
    // [q8 | k8 | v8 | scale_q, scale_k, scale_v | abs-max words of q, k, v]: the buffers only used where the caller passes none of its own
    return up256(qattn_varlen_tensor_bytes(QATTN_LAYOUT_ROWMAJOR, B, Hq, total_q, D)) + up256(qattn_varlen_tensor_bytes(QATTN_LAYOUT_KFRAG, B, Hkv, total_k, D)) +
           up256(vfp_v8_bytes(B, Hkv, total_k, D)) + 2 * up256(sizeof(float) * (size_t)B * (Hq + 2 * (size_t)Hkv));
}

extern "C" size_t qattn_fp8_quant_attention_varlen_fp8pv_smooth_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int D) {
    const size_t plain = qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes(B, Hq, Hkv, total_q, total_k, D);
    // [the plain workspace | per-block channel sums of the mean pass]
    return plain ? up256(plain) + varlen_smooth_k_workspace_bytes(B, Hkv, D) : 0;
}

int qattn::varlen_fp8pv_forward_impl(const void* q, const void* k, const void* v, const long long* strides, int in_fmt, void* out, float* lse,
                                     const int* cu_seqlens_q, const int* cu_seqlens_k, const int* seqused_k, int B, int Hq, int Hkv, int total_q,
                                     int total_k, int D, int fp8_fmt, int numerics, int is_causal, float sm_scale, int precision, void* q8,
                                     void* k8, void* v8, float* scale_q, float* scale_k, float* scale_v, unsigned char* row_path, float* k_mean,
                                     void* workspace, size_t workspace_bytes, void* stream, const int* window) {
    if (!q || !k || !v || !out || !cu_seqlens_q || !cu_seqlens_k) return QATTN_ERR_INVALID_ARG;
    if (!vfp_dims_ok(B, Hq, Hkv, total_q, total_k)) return QATTN_ERR_INVALID_ARG;
    if ((D != 64 && D != 128 && D != 256) || Hq % Hkv != 0) return QATTN_ERR_UNSUPPORTED_DIM;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (numerics != QATTN_NUMERICS_COMPILED && numerics != QATTN_NUMERICS_EAGER) return QATTN_ERR_INVALID_ARG;
    if (precision != QATTN_PRECISION_FAST && precision != QATTN_PRECISION_ACCURATE) return QATTN_ERR_INVALID_ARG;
    long long st6[6] = {(long long)Hq * D, D, (long long)Hkv * D, D, (long long)Hkv * D, D};   // dense [total, H, D]
    if (strides)
        for (int s = 0; s < 6; s++) {
            if (strides[s] < 0 || strides[s] % 8 != 0) return QATTN_ERR_INVALID_ARG;
            st6[s] = strides[s];
        }
    if (((size_t)q | (size_t)k | (size_t)v | (size_t)out) % 16 != 0) return QATTN_ERR_INVALID_ARG;
    // grids: Hq (B + ceil(total_q / 128)) attention workgroups, B + ceil(total / 64) quantise tiles per head (32-bit dimensions)
    if ((long long)Hq * (B + ceil_div(total_q, kFpvTile)) > 0x7fffffffLL || (long long)B + ceil_div(total_q > total_k ? total_q : total_k, 64) > 0x7fffffffLL)
        return QATTN_ERR_INVALID_ARG;
    const bool smooth = k_mean != nullptr;
    if (smooth && (reinterpret_cast<uintptr_t>(k_mean) & 15u) != 0) return QATTN_ERR_INVALID_ARG;
    const size_t plain_bytes = qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes(B, Hq, Hkv, total_q, total_k, D);
    const size_t need = smooth ? qattn_fp8_quant_attention_varlen_fp8pv_smooth_workspace_bytes(B, Hq, Hkv, total_q, total_k, D) : plain_bytes;
    if (!workspace || workspace_bytes < need) return QATTN_ERR_WORKSPACE;
    if (total_q == 0) return QATTN_OK;   // no query row: nothing to compute or write
    hipStream_t st = (hipStream_t)stream;
    const size_t nq = (size_t)B * Hq, nk = (size_t)B * Hkv;
    unsigned char* w = (unsigned char*)workspace;
    unsigned char* q8w = w;   w += up256(qattn_varlen_tensor_bytes(QATTN_LAYOUT_ROWMAJOR, B, Hq, total_q, D));
    unsigned char* k8w = w;   w += up256(qattn_varlen_tensor_bytes(QATTN_LAYOUT_KFRAG, B, Hkv, total_k, D));
    unsigned char* v8w = w;   w += up256(vfp_v8_bytes(B, Hkv, total_k, D));
    float* sw = (float*)w;    w += up256(sizeof(float) * (nq + 2 * nk));
    unsigned* amax = (unsigned*)w;
    VfpQuant qa;
    qa.x[0] = (const unsigned char*)q; qa.x[1] = (const unsigned char*)k; qa.x[2] = (const unsigned char*)v;
    for (int z = 0; z < 3; z++) { qa.ts[z] = st6[2 * z]; qa.hs[z] = st6[2 * z + 1]; }
    qa.cu[0] = cu_seqlens_q; qa.cu[1] = cu_seqlens_k; qa.cu[2] = cu_seqlens_k; qa.used = seqused_k;
    qa.total[0] = total_q; qa.total[1] = total_k; qa.total[2] = total_k;
    qa.H[0] = Hq; qa.H[1] = Hkv; qa.H[2] = Hkv;
    qa.B = B; qa.skip_k = smooth ? 1 : 0;
    qa.amax[0] = amax; qa.amax[1] = amax + nq; qa.amax[2] = amax + nq + nk;
    qa.x8[0] = q8 ? (unsigned char*)q8 : q8w; qa.x8[1] = k8 ? (unsigned char*)k8 : k8w; qa.x8[2] = v8 ? (unsigned char*)v8 : v8w;
    qa.scale[0] = scale_q ? scale_q : sw; qa.scale[1] = scale_k ? scale_k : sw + nq; qa.scale[2] = scale_v ? scale_v : sw + nq + nk;
    VfpAttn a;
    a.q8 = qa.x8[0]; a.k8 = qa.x8[1]; a.v8 = qa.x8[2];
    a.out = out; a.lse = lse; a.path = row_path;
    a.sq = qa.scale[0]; a.sk = qa.scale[1]; a.sv = qa.scale[2];
    a.cu_q = cu_seqlens_q; a.cu_k = cu_seqlens_k; a.used = seqused_k;
    a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.total_q = total_q; a.total_k = total_k;
    a.nblk = B + ceil_div(total_q, kFpvTile);
    a.out_fmt = in_fmt;
    a.xcd_remap = (Hq % 8 == 0 && xcd_count() == 8) ? 1 : 0;   // (the XCD-contiguous map assumes 8 XCDs; a speed assumption only)
    a.two_term_keys = kTwoTermKeys;
    const float sm = sm_scale > 0.0f ? sm_scale : 1.0f / sqrtf((float)D);
    a.sm_log2e = sm * 1.4426950408889634f;
    if (zero_words(amax, (long)(nq + 2 * nk), st) != hipSuccess) return QATTN_ERR_LAUNCH;
    int rc;
    if (smooth) {   // K first, in launches of its own (mean, abs-max, quantise on k - mean), then q and v through the plain two
        rc = launch_varlen_smooth_k(k, (long)st6[2], (long)st6[3], in_fmt, cu_seqlens_k, seqused_k, B, Hkv, total_k, D, fp8_fmt, numerics, qa.x8[1],
                                    qa.scale[1], k_mean, qa.amax[1], reinterpret_cast<float*>((unsigned char*)workspace + up256(plain_bytes)), st);
        if (rc != QATTN_OK) return rc;
    }
    if (D == 64) rc = launch_vfp<64>(qa, a, in_fmt, fp8_fmt, numerics, is_causal, precision, window, st);
    else if (D == 128) rc = launch_vfp<128>(qa, a, in_fmt, fp8_fmt, numerics, is_causal, precision, window, st);
    else rc = launch_vfp<256>(qa, a, in_fmt, fp8_fmt, numerics, is_causal, precision, window, st);
    if (rc != QATTN_OK) return rc;
    if (hipGetLastError() != hipSuccess) return QATTN_ERR_LAUNCH;
    if (!smooth || !lse) return QATTN_OK;
    // the launch wrote the LSE of the smoothed scores; the true scores of a row lie sm_scale * q.m higher (-inf rows stay -inf)
    return launch_varlen_smooth_lse(q, (long)st6[0], (long)st6[1], in_fmt, cu_seqlens_q, k_mean, lse, B, Hq, Hkv, total_q, D, sm, st);
}

extern "C" int qattn_fp8_quant_attention_varlen_forward_fp8pv(const void* q, const void* k, const void* v, const long long* strides, int in_fmt,
                                                              void* out, float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k,
                                                              const int* seqused_k, int B, int Hq, int Hkv, int total_q, int total_k, int D,
                                                              int fp8_fmt, int numerics, int is_causal, float sm_scale, int precision, void* q8,
                                                              void* k8, void* v8, float* scale_q, float* scale_k, float* scale_v,
                                                              unsigned char* row_path, float* k_mean, void* workspace, size_t workspace_bytes,
                                                              void* stream) {
    return varlen_fp8pv_forward_impl(q, k, v, strides, in_fmt, out, lse, cu_seqlens_q, cu_seqlens_k, seqused_k, B, Hq, Hkv, total_q, total_k, D,
                                     fp8_fmt, numerics, is_causal, sm_scale, precision, q8, k8, v8, scale_q, scale_k, scale_v, row_path, k_mean,
                                     workspace, workspace_bytes, stream, nullptr);
}

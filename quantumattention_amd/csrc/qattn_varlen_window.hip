// qattn_varlen_window.hip -- qattn_fp8_quant_attention_varlen_window_forward (include/qattn_window.h): sliding-window (local) FP8 attention
// on packed sequences.  Query r of a sequence with L_q queries and L_k used keys attends the keys j with
// r + delta - left <= j <= r + delta + right, delta = L_k - L_q (flash-attn's window_size; -1 = unbounded).
//
// The pre-pass (zeroing node, abs-max, quantise, the smoothing launches) is the packed entry's own, launched by its body
// (varlen_forward_impl, qattn_varlen.hip); this unit holds the attention launch: one workgroup per (head, 256-row query block of a
// sequence), found through varlen_tile as there, running pv16_block_pass_at with WINDOW on (qattn_pv16.h) in the loop form of the packed
// kernel (the two-group loop at D = 128).  A block sweeps only the 64-key chunks that hold a key one of its rows attends.
// Built with strided addressing (QATTN_STRIDED16 = 1), as the varlen unit.
#include "qattn_pv16.h"
#include "qattn_varlen_tile.h"
#include "qattn_varlen_attn.h"
#include "../../include/qattn_varlen.h"
#include "../../include/qattn_window.h"

namespace qattn {

static_assert(kStrided16, "the window unit addresses V and the output through strides");

template <int D, int QK_FMT, int V16_FMT, bool PP>
__global__ __launch_bounds__(kThreads, 2) void attn_pv16_varlen_window_kernel(const VarlenAttn a, int left, int right) {
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
    const VarlenTile tq = varlen_tile<kQPerWG>(a.cu_q, nullptr, a.B, a.total_q, j);
    if (tq.tile < 0 || tq.tile * kQPerWG >= tq.len) return;
    const int i = tq.i;
    const int sk0 = clampi(__builtin_amdgcn_readfirstlane(a.cu_k[i]), 0, a.total_k);
    int lk = clampi(__builtin_amdgcn_readfirstlane(a.cu_k[i + 1]), sk0, a.total_k) - sk0;
    if (a.used) lk = clampi(__builtin_amdgcn_readfirstlane(a.used[i]), 0, lk);
    const int lq = tq.len;
    // row r attends the keys j with win_lo <= j - r <= win_hi.  j - r lies in (-lq, lk): an offset clamped to [-lq, lk] masks the same
    // keys as the exact one, and no sum below leaves 32 bits (lq + lk < 2^31: the packed tensors' own extents)
    const long delta = (long)lk - lq;
    auto clampl = [](long x, long lo, long hi) -> int { return (int)(x < lo ? lo : x > hi ? hi : x); };
    const int win_lo = left < 0 ? -lq : clampl(delta - left, -(long)lq, lk);
    const int win_hi = right < 0 ? lk : clampl(delta + right, -(long)lq - 1, lk);
    // the keys any valid row of the block attends
    const int r_first = tq.tile * kQPerWG, r_last = min(r_first + kQPerWG, lq) - 1;
    const int klo = max(r_first + win_lo, 0), khi = min(r_last + win_hi, lk - 1);
    constexpr int RB = 2 * D;   // bytes of a 16-bit row
    const long o_rs = (long)a.Hq * RB;
    unsigned char* out = reinterpret_cast<unsigned char*>(a.out) + (long)tq.start * o_rs;
    if (klo > khi) {   // no key for any row (lk = 0 included): zero rows, LSE -inf, no sweep
        const int row = r_first + (int)threadIdx.x / 2, half = threadIdx.x & 1;
        if (threadIdx.x < 2 * kQPerWG && row < lq) {
            uint4* op = reinterpret_cast<uint4*>(out + (long)row * o_rs + (long)h * RB + half * (RB / 2));
#pragma unroll
            for (int c = 0; c < RB / 32; c++) op[c] = make_uint4(0, 0, 0, 0);
            if (a.lse && half == 0) a.lse[(long)h * a.total_q + tq.start + row] = -INFINITY;
        }
        return;
    }
    AttnParams p;
    __builtin_memset(&p, 0, sizeof(p));
    p.B = 1; p.Hq = a.Hq; p.Hkv = a.Hkv; p.Sq = lq; p.Skv = lk;
    p.nqb = ceil_div(lq, kQPerWG);
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
    pv16_block_pass_at<D, kWaves, QK_FMT, V16_FMT, false, false, false, PP ? 4 : 3, PP, true>(p, smem, (int)threadIdx.x, h, tq.tile, []() { return 0u; },
                                                                                            [](unsigned) {}, win_lo, win_hi);
}

template <int D, int QK_FMT, int V16_FMT>
static int launch_window_attn(const VarlenAttn& a, int left, int right, hipStream_t st) {
    constexpr bool PP = D == 128;
    constexpr int lds = (PP ? 4 : 3) * (64 * D + 64 * D * 2);
    auto kern = attn_pv16_varlen_window_kernel<D, QK_FMT, V16_FMT, PP>;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return QATTN_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3((unsigned)(a.Hq * a.nblk)), dim3(kThreads), lds, st, a, left, right);
    return QATTN_OK;
}
template <int D>
static int launch_window_attn_d(const VarlenAttn& a, int qk_fmt, int v16_fmt, int left, int right, hipStream_t st) {
    if (qk_fmt == QATTN_FMT_E4M3)
        return v16_fmt == QATTN_FMT_BF16 ? launch_window_attn<D, QATTN_FMT_E4M3, QATTN_FMT_BF16>(a, left, right, st)
                                         : launch_window_attn<D, QATTN_FMT_E4M3, QATTN_FMT_FP16>(a, left, right, st);
    return v16_fmt == QATTN_FMT_BF16 ? launch_window_attn<D, QATTN_FMT_E5M2, QATTN_FMT_BF16>(a, left, right, st)
                                     : launch_window_attn<D, QATTN_FMT_E5M2, QATTN_FMT_FP16>(a, left, right, st);
}

int launch_varlen_window_attn(const VarlenAttn& a, int D, int qk_fmt, int v16_fmt, int window_left, int window_right, hipStream_t st) {
    if (D == 64) return launch_window_attn_d<64>(a, qk_fmt, v16_fmt, window_left, window_right, st);
    if (D == 128) return launch_window_attn_d<128>(a, qk_fmt, v16_fmt, window_left, window_right, st);
    return launch_window_attn_d<256>(a, qk_fmt, v16_fmt, window_left, window_right, st);
}

}  // namespace qattn

using namespace qattn;

extern "C" size_t qattn_fp8_quant_attention_varlen_window_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int D) {
    // (the smoothing entry's size holds the plain entry's: one figure serves both forms of the call)
    return qattn_fp8_quant_attention_varlen_smooth_workspace_bytes(B, Hq, Hkv, total_q, total_k, D);
}

extern "C" int qattn_fp8_quant_attention_varlen_window_forward(const void* q, const void* k, const void* v, const long long* strides, int in_fmt,
                                                               void* out, float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k,
                                                               const int* seqused_k, int B, int Hq, int Hkv, int total_q, int total_k, int D,
                                                               int fp8_fmt, int numerics, int window_left, int window_right, float sm_scale,
                                                               void* q8, void* k8, float* scale_q, float* scale_k, void* workspace,
                                                               size_t workspace_bytes, void* stream, float* k_mean) {
    if (window_left < -1 || window_right < -1) return QATTN_ERR_INVALID_ARG;
    const int window[2] = {window_left, window_right};
    return varlen_forward_impl(q, k, v, strides, in_fmt, out, lse, cu_seqlens_q, cu_seqlens_k, seqused_k, B, Hq, Hkv, total_q, total_k, D, fp8_fmt,
                               numerics, 0, sm_scale, q8, k8, scale_q, scale_k, workspace, workspace_bytes, stream, k_mean, window);
}

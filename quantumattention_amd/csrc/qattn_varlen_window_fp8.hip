// qattn_varlen_window_fp8.hip -- qattn_fp8_quant_attention_varlen_window_forward_fp8pv (include/qattn_window.h): sliding-window (local)
// FP8 attention on packed sequences with BOTH products on the FP8 matrix pipe.  Query r of a sequence with L_q queries and L_k used keys
// attends the keys j with r + delta - left <= j <= r + delta + right, delta = L_k - L_q (flash-attn's window_size; -1 = unbounded).
//
// The pre-pass (zeroing node, abs-max, quantise of q / k / v, the smoothing launches) is the packed FP8-PV entry's own, launched by its
// body (varlen_fp8pv_forward_impl, qattn_varlen_fp8.hip); this unit holds the attention launch: the FP8-PV chunk sweep of
// qattn_fp8pv_sweep.h, statement for statement what attn_vfp8_kernel (there) runs, with this kernel's own
//   * the trip range: a 128-row tile sweeps the 64-key chunks klo / 64 .. khi / 64 of [klo, khi], the keys its valid rows attend, and DMAs
//     no other chunk; the one-term rule of FAST is n = khi - klo + 1 >= two_term_keys;
//   * the token mask key - row outside [win_lo, win_hi] (and the ragged tail), applied under a workgroup-uniform condition -- the chunk
//     crosses an edge for some valid row of the tile -- so that barriers and DMA keep one cadence for the four waves;
//   * rows that meet fully masked chunks before their first key, or have no key at all while their neighbours do.  A masked score is
//     -inf: fmaxf(m_run, -inf) keeps m_run (it starts at the finite kNoKeyYet = -1e20), so a rescale another lane triggered gives this lane
//     alpha = 1, lim = -1e20 and a huge finite off8; exp2(fma(-inf, c, mc)) and pknorm(fma(-inf, c8, off8)) are exactly 0 for c > 0 (the
//     scales are >= eps), the row-sum MFMA adds 0, and the first finite score exceeds lim = -1e20 and sets m_run, lim and off8 afresh.
//     The start value is -1e20, not the packed kernel's -1e30: here a row can carry it through whole chunks, where mc = shift + 1e20 c
//     must stay finite (fma(-inf, c, +inf) would be NaN) -- it does for c = sm_scale log2(e) scale_q scale_k < 3e18, while a raw score
//     (a sum of D products of two fp8 values, |s| <= 256 * 57344^2 < 1e12) can never reach it.  A row whose first chunk holds a key is
//     unaffected (alpha multiplies zeros), so the bits of the packed kernel are kept where the masks agree.  A row that
//     ends with l = 0 is scaled by 0 (not by sv / 0) and its LSE is -inf.
//   * registers: the loop carries the row number alone (the output / LSE offsets are formed before and after the sweep, the row's key
//     bounds inside the rare masked branch), and the eight equal words of the row-sum MFMA's A operand are spread from one register where
//     they are used (fpv_spread_ones; the other two kernels carry the v8i) -- the D = 128 byte kernel otherwise kept them in scratch at
//     its 3 waves per SIMD.
#include "qattn_varlen_fp8.h"
#include "qattn_varlen_tile.h"
#include "../../include/qattn_varlen.h"
#include "../../include/qattn_window.h"

namespace qattn {

// BYTE / two / sel: as attn_vfp8_kernel.  left / right: window_left / window_right, >= -1.
template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_vfp8_window_kernel(const VfpAttn a, const int two, const int sel, const int left, const int right) {
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
    // (tiles are handed out front to back.  The packed causal kernel walks them back to front, longest sweep first; under a window the
    // sweep length grows only up to left + right + 128 keys and then stays there, so the order matters for (-1, 0) or a left edge of many
    // thousand keys alone -- speed only, not measured, left as it is)
    const VarlenTile tq = varlen_tile<kFpvTile>(a.cu_q, nullptr, a.B, a.total_q, j);
    if (tq.tile < 0 || tq.tile * kFpvTile >= tq.len) return;   // no tile of any sequence
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
    // [klo, khi]: the keys the tile's valid rows attend (rows without a key can only lead a sequence: r + win_hi < 0).  Workgroup-uniform,
    // as are the rule of the one-term sweep and the trip range derived from it
    const int r_first = tq.tile * kFpvTile, r_last = min(r_first + kFpvTile, lq) - 1;
    const int klo = max(r_first + win_lo, 0), khi = min(r_last + win_hi, lk - 1);
    const int keys = max(khi - klo + 1, 0);
    if (sel == kFpvSelMany && keys < a.two_term_keys) return;
    if (sel == kFpvSelFew && keys >= a.two_term_keys) return;

    const int kvh = h / (a.Hq / a.Hkv);
    const int qrow = r_first + wave * kQPerWave + ql;   // row within the sequence
    const bool qvalid = qrow < lq;
    // (computed where they are used, before and after the sweep: the loop carries qrow alone)
    auto orow_of = [&]() -> long { return ((long)(tq.start + (qvalid ? qrow : 0)) * a.Hq + h) * (2L * D); };   // bytes: rows are a token stride apart
    auto lrow_of = [&]() -> long { return (long)h * a.total_q + tq.start + qrow; };                           // lse / path: [Hq, total_q]
    if (keys == 0) {   // no key for any row of the tile (lk = 0 included): no sweep
        const long lrow = lrow_of();
        fpv_store_empty<D>(a.out, a.out_fmt, orow_of(), a.lse, lrow, a.path, lrow, hh, qvalid);
        return;
    }
    const int c_first = klo >> 6;                   // chunks c_first .. c_first + n_wg - 1 = khi / 64 < nch
    const int n_wg = (khi >> 6) - c_first + 1;
    const int nch = (lk + 63) >> 6;                 // chunks of the sequence's images

    const long img = (long)a.Hkv * D * (sk0 + 64L * i) + (long)kvh * nch * CH + (wave << 10);
    FpvRing<D> ring(smem, wave, lane, a.k8 + img, a.v8 + img);
    ring.dma_chunk(c_first);
    sw.park_q(a.q8 + (long)a.Hq * D * tq.start + ((long)h * tq.len + (qvalid ? qrow : 0)) * D + hh * 32, qvalid);
    constexpr float kNoKeyYet = -1.0e20f;   // below any raw score, and kNoKeyYet * c stays finite (header comment)
    sw.init_state(a.sm_log2e * a.sq[(long)i * a.Hq + h] * a.sk[(long)i * a.Hkv + kvh], kNoKeyYet);
    const int one = fpv_ones_word(lane);   // (spread where it is used: header comment, registers)

    for (int t = 0; t < n_wg; t++) {   // step t sweeps chunk c_first + t
        v8i qf[KS];
        sw.read_q(qf);
        sw.wait_stage();
        if (t + 1 < n_wg) ring.dma_chunk(c_first + t + 1);
        v16f s0, s1;
        v8i vf0, vf1;
        sw.qk(t, qf, s0, s1, vf0, vf1);
        // ---- the window's edges by token, and the ragged tail of the sequence's keys.  The condition is workgroup-uniform: over the
        // chunk's keys k0 .. k0 + 63 and the tile's valid rows, key - row spans [k0 - r_last, k0 + 63 - r_first]
        const int k0 = (c_first + t) * 64;
        if (__builtin_expect(k0 + 64 > lk || k0 - r_last < win_lo || k0 + 63 - r_first > win_hi, 0)) {
            // this lane's row attends the keys with win_lo <= key - qrow <= hi_l (token-exact; hi_l also ends the sequence's keys)
            const int hi_l = min(win_hi, lk - 1 - qrow), base = qrow - 4 * hh;
#pragma unroll
            for (int r = 0; r < 32; r++) {
                const int d = k0 + 32 * (r >> 4) + (r & 3) + 8 * ((r & 15) >> 2) - base;   // key - qrow
                v16f& sx = (r >> 4) ? s1 : s0;
                sx[r & 15] = (d < win_lo || d > hi_l) ? -INFINITY : sx[r & 15];
            }
        }
        sw.softmax_pv(s0, s1, vf0, vf1, two, [&] { return fpv_spread_ones(one); });
    }

    // ---- epilogue (V's one scale per (sequence, head) is applied here)
    const float l_tot = sw.row_sum();
    const long orow = orow_of(), lrow = lrow_of();
    const bool has_key = l_tot > 0.0f;   // (a row without a key inside a tile that sweeps: every P was 0 -- a zero row, LSE -inf)
    const float inv = has_key ? a.sv[(long)i * a.Hkv + kvh] / l_tot : 0.0f;
    store_o_rows<MB>(a.out, a.out_fmt, sw.o, inv, orow, hh, qvalid);
    if (!BYTE && a.lse && hh == 0 && qvalid) a.lse[lrow] = has_key ? 0.6931471805599453f * (sw.m_run * sw.c - kPShift) + __logf(l_tot) : -INFINITY;
    if (a.path && hh == 0 && qvalid) a.path[lrow] = (unsigned char)((!BYTE && two) ? QATTN_PATH_TWO_TERM : QATTN_PATH_ONE_TERM);
}

template <int D, int FMT>
static int launch_wfp_attn(const VfpAttn& a, int precision, int left, int right, hipStream_t st) {
    // (total_k: more than any tile can attend)
    return fpv_precision_ladder(precision, a.total_k, a.two_term_keys, a.lse != nullptr, [&](auto byte, int two, int sel) {
        return fpv_launch(attn_vfp8_window_kernel<D, FMT, decltype(byte)::value>, (unsigned)(a.Hq * a.nblk), fpv_lds_bytes(D), st, a, two, sel, left,
                          right);
    });
}

template <int D>
static int launch_wfp_d(const VfpAttn& a, int fp8_fmt, int precision, int left, int right, hipStream_t st) {
    return fp8_fmt == QATTN_FMT_E4M3 ? launch_wfp_attn<D, QATTN_FMT_E4M3>(a, precision, left, right, st)
                                     : launch_wfp_attn<D, QATTN_FMT_E5M2>(a, precision, left, right, st);
}

int launch_varlen_window_fp8_attn(const VfpAttn& a, int D, int fp8_fmt, int precision, int window_left, int window_right, hipStream_t st) {
    if (D == 64) return launch_wfp_d<64>(a, fp8_fmt, precision, window_left, window_right, st);
    if (D == 128) return launch_wfp_d<128>(a, fp8_fmt, precision, window_left, window_right, st);
    return launch_wfp_d<256>(a, fp8_fmt, precision, window_left, window_right, st);
}

}  // namespace qattn

using namespace qattn;

extern "C" int qattn_fp8_quant_attention_varlen_window_forward_fp8pv(const void* q, const void* k, const void* v, const long long* strides,
                                                                     int in_fmt, void* out, float* lse, const int* cu_seqlens_q,
                                                                     const int* cu_seqlens_k, const int* seqused_k, int B, int Hq, int Hkv,
                                                                     int total_q, int total_k, int D, int fp8_fmt, int numerics, int window_left,
                                                                     int window_right, float sm_scale, int precision, void* q8, void* k8, void* v8,
                                                                     float* scale_q, float* scale_k, float* scale_v, unsigned char* row_path,
                                                                     float* k_mean, void* workspace, size_t workspace_bytes, void* stream) {
    if (window_left < -1 || window_right < -1) return QATTN_ERR_INVALID_ARG;
    const int window[2] = {window_left, window_right};
    return varlen_fp8pv_forward_impl(q, k, v, strides, in_fmt, out, lse, cu_seqlens_q, cu_seqlens_k, seqused_k, B, Hq, Hkv, total_q, total_k, D,
                                     fp8_fmt, numerics, 0, sm_scale, precision, q8, k8, v8, scale_q, scale_k, scale_v, row_path, k_mean, workspace,
                                     workspace_bytes, stream, window);
}

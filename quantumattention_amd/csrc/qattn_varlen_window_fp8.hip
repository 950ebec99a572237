// qattn_varlen_window_fp8.hip -- qattn_fp8_quant_attention_varlen_window_forward_fp8pv (include/qattn_window.h): sliding-window (local)
// FP8 attention on packed sequences with BOTH products on the FP8 matrix pipe.  Query r of a sequence with L_q queries and L_k used keys
// attends the keys j with r + delta - left <= j <= r + delta + right, delta = L_k - L_q (flash-attn's window_size; -1 = unbounded).
//
// The pre-pass (zeroing node, abs-max, quantise of q / k / v, the smoothing launches) is the packed FP8-PV entry's own, launched by its
// body (varlen_fp8pv_forward_impl, qattn_varlen_fp8.hip); this unit holds the attention launch: attn_vfp8_kernel (there) operation for
// operation, with
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
//     they are used -- the D = 128 byte kernel otherwise kept them in scratch at its 3 waves per SIMD.
#include "qattn_varlen_fp8.h"
#include "qattn_varlen_tile.h"
#include "../../include/qattn_varlen.h"
#include "../../include/qattn_window.h"

namespace qattn {

// BYTE / two / sel: as attn_vfp8_kernel.  left / right: window_left / window_right, >= -1.
template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kVfpWaves * 64, (VfpShape<D, BYTE>::WPS))
void attn_vfp8_window_kernel(const VfpAttn a, const int two, const int sel, const int left, const int right) {
    constexpr int NW = kVfpWaves;
    constexpr int CH = 64 * D, STAGE = 2 * CH, MB = D / 32, KS = D / 64;
    constexpr int RK = CH / (NW * 1024);   // 1 KiB DMA pieces per wave for the K (and for the V) part of a stage
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hh = lane >> 5;

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
    const VarlenTile tq = varlen_tile<kVfpTile>(a.cu_q, nullptr, a.B, a.total_q, j);
    if (tq.tile < 0 || tq.tile * kVfpTile >= tq.len) return;   // no tile of any sequence
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
    const int r_first = tq.tile * kVfpTile, r_last = min(r_first + kVfpTile, lq) - 1;
    const int klo = max(r_first + win_lo, 0), khi = min(r_last + win_hi, lk - 1);
    const int keys = max(khi - klo + 1, 0);
    if (sel == kVfpSelMany && keys < a.two_term_keys) return;
    if (sel == kVfpSelFew && keys >= a.two_term_keys) return;

    const int kvh = h / (a.Hq / a.Hkv);
    const int qrow = r_first + wave * kQPerWave + ql;   // row within the sequence
    const bool qvalid = qrow < lq;
    // (computed where they are used, before and after the sweep: the loop carries qrow alone)
    auto orow_of = [&]() -> long { return ((long)(tq.start + (qvalid ? qrow : 0)) * a.Hq + h) * (2L * D); };   // bytes: rows are a token stride apart
    auto lrow_of = [&]() -> long { return (long)h * a.total_q + tq.start + qrow; };                           // lse / path: [Hq, total_q]
    if (keys == 0) {   // no key for any row of the tile (lk = 0 included): zero rows, LSE -inf, path code QATTN_PATH_ONE_TERM, no sweep
        const long orow = orow_of(), lrow = lrow_of();
        v16f z[MB];
#pragma unroll
        for (int m = 0; m < MB; m++)
#pragma unroll
            for (int r = 0; r < 16; r++) z[m][r] = 0.0f;
        store_o_rows<MB>(a.out, a.out_fmt, z, 0.0f, orow, hh, qvalid);
        if (a.lse && hh == 0 && qvalid) a.lse[lrow] = -INFINITY;
        if (a.path && hh == 0 && qvalid) a.path[lrow] = (unsigned char)QATTN_PATH_ONE_TERM;
        return;
    }
    const int c_first = klo >> 6;                   // chunks c_first .. c_first + n_wg - 1 = khi / 64 < nch
    const int n_wg = (khi >> 6) - c_first + 1;
    const int nch = (lk + 63) >> 6;                 // chunks of the sequence's images

    const long img = (long)a.Hkv * D * (sk0 + 64L * i) + (long)kvh * nch * CH + (wave << 10);
    const unsigned char* kg_w = a.k8 + img;
    const unsigned char* vg_w = a.v8 + img;
    // stage(t) = {K chunk c_first + t, V chunk c_first + t} -> slot t & 1; every wave copies 2*RK x 1 KiB of it by LDS-DMA
    const unsigned lane16 = (unsigned)lane << 4;
    unsigned slot_next = 0;
    auto dma_chunk = [&](int chunk) {
        unsigned char* dst = smem + slot_next + (wave << 10);
        const size_t coff = (size_t)chunk * CH + lane16;
#pragma unroll
        for (int r = 0; r < RK; r++) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kg_w + (coff + r * (NW * 1024))),
                                             (__attribute__((address_space(3))) void*)(dst + r * (NW * 1024)), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vg_w + (coff + r * (NW * 1024))),
                                             (__attribute__((address_space(3))) void*)(dst + CH + r * (NW * 1024)), 16, 0, 0);
        }
        slot_next ^= STAGE;
    };
    dma_chunk(c_first);

    // Q^T fragments parked in this lane's own LDS slots
    unsigned char* qbuf = smem + kVfpStages * STAGE + wave * (KS << 11) + (hh << 10) + (ql << 4);
    {
        const unsigned char* qp = a.q8 + (long)a.Hq * D * tq.start + ((long)h * tq.len + (qvalid ? qrow : 0)) * D + hh * 32;
#pragma unroll
        for (int s = 0; s < KS; s++) {
            v4i lo = *reinterpret_cast<const v4i*>(qp + s * 64);
            v4i hi = *reinterpret_cast<const v4i*>(qp + s * 64 + 16);
            if (!qvalid) { lo = v4i{0, 0, 0, 0}; hi = v4i{0, 0, 0, 0}; }
            *reinterpret_cast<v4i*>(qbuf + (s << 11)) = lo;
            *reinterpret_cast<v4i*>(qbuf + (s << 11) + 512) = hi;
        }
    }
    const float c = a.sm_log2e * a.sq[(long)i * a.Hq + h] * a.sk[(long)i * a.Hkv + kvh];

    v16f o[MB];
#pragma unroll
    for (int m = 0; m < MB; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[m][r] = 0.0f;
    v4f lsum = {0.0f, 0.0f, 0.0f, 0.0f};
    int one;  // a word of A of the row-sum MFMA (see WaveState::lsum in qattn_attn_v2.hip): its eight words are equal
    {
        const int row = lane & 15, kg = lane >> 4;
        one = ((row == 0 && !(kg & 1)) || (row == 1 && (kg & 1))) ? 0x38383838 : 0;
    }
    constexpr float kNoKeyYet = -1.0e20f;   // below any raw score, and kNoKeyYet * c stays finite (header comment)
    float m_run = kNoKeyYet, l_run = 0.0f;
    float lim = kNoKeyYet, off8 = 0.0f;   // m_run + thr / c and the byte formula's additive constant (set by the row's first unmasked score)
    constexpr float U16 = 1.0f / 65535.0f;
    const float c8 = (8.0f * U16) * c;
    const int frag_lane_off = (hh << 10) + (ql << 4);

    for (int t = 0; t < n_wg; t++) {
        v8i qf[KS];
#pragma unroll
        for (int s = 0; s < KS; s++) qf[s] = lds_read_frag(qbuf + (s << 11));
        wait_vmcnt<0>();                  // this wave's pieces of stage t have landed
        __builtin_amdgcn_s_barrier();     // ... and everyone's; every wave is also done with stage t-1's slot
        if (t + 1 < n_wg) dma_chunk(c_first + t + 1);
        const unsigned char* kbuf = smem + (t & 1) * STAGE + frag_lane_off;
        const unsigned char* vbuf = kbuf + CH;
        // ---- S^T = K.Q^T
        v16f s0, s1;
#pragma unroll
        for (int r = 0; r < 16; r++) { s0[r] = 0.0f; s1[r] = 0.0f; }
#pragma unroll
        for (int s = 0; s < KS; s++) {
            const v8i ka = lds_read_frag(kbuf + ((0 * KS + s) << 11)), kb = lds_read_frag(kbuf + ((1 * KS + s) << 11));
            s0 = mfma_f8<FMT, FMT>(ka, qf[s], s0);
            s1 = mfma_f8<FMT, FMT>(kb, qf[s], s1);
        }
        const v8i vf0 = lds_read_frag(vbuf), vf1 = lds_read_frag(vbuf + (1 << 11));
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
        // ---- running max; rescale only when a row's max grew past the headroom of the shifted exponent
        float mx = max32_after_mfma(s0, s1);
        {
            auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
            mx = max3_raw(__uint_as_float(sw[0]), __uint_as_float(sw[1]), __uint_as_float(sw[1]));
        }
        if (__builtin_expect(__any(mx > lim) != 0, 0)) {   // (mx - m_run) c > thr: P' could overflow e4m3
            const float m_new = fmaxf(m_run, mx);           // (a row with every score so far masked: mx = -inf, m_new = m_run = kNoKeyYet, alpha = 1)
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
#pragma unroll
            for (int m = 0; m < MB; m++)
#pragma unroll
                for (int r = 0; r < 16; r++) o[m][r] *= alpha;
            if (BYTE) {
                const float alpha16 = __shfl(alpha, (lane & 15) + 16);
                lsum[0] *= alpha;
                lsum[1] *= alpha16;
            } else {
                l_run *= alpha;
            }
            m_run = m_new;
            lim = m_new + kRescaleThrByte / c;
            off8 = __builtin_fmaf((-8.0f * U16) * m_new, c, (8.0f * kPShiftByte + 56.0f + kByteBias) * U16);
        }
        v8i pv, pl;
        if (BYTE) {
#pragma unroll
            for (int w = 0; w < 4; w++) {
                pv[w] = vfp_byte_exp4(s0[4 * w], s0[4 * w + 1], s0[4 * w + 2], s0[4 * w + 3], c8, off8);
                pv[4 + w] = vfp_byte_exp4(s1[4 * w], s1[4 * w + 1], s1[4 * w + 2], s1[4 * w + 3], c8, off8);
            }
        } else {
            const float mc = kPShift - m_run * c;
            float ls = 0.0f;
#pragma unroll
            for (int w = 0; w < 8; w++) {
                const v16f& sx = w < 4 ? s0 : s1;
                const int jj = w & 3;
                float e[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { e[u] = __builtin_amdgcn_exp2f(__builtin_fmaf(sx[4 * jj + u], c, mc)); ls += e[u]; }
                int ph = cvt_pk_fp8<QATTN_FMT_E4M3, false>(e[0], e[1], 0);
                ph = cvt_pk_fp8<QATTN_FMT_E4M3, true>(e[2], e[3], ph);
                pv[w] = ph;
                int plo = 0;
                if (two) plo = lo_terms(e, ph, 0);
                pl[w] = plo;
            }
            l_run += ls;
        }
        // ---- O^T += V^T.P^T, row sums (V's one scale per (sequence, head) is applied in the epilogue; the low term's 2^-5 rides in the scale word)
        o[0] = mfma_f8<FMT, QATTN_FMT_E4M3>(vf0, pv, o[0]);
        o[1] = mfma_f8<FMT, QATTN_FMT_E4M3>(vf1, pv, o[1]);
        if (!BYTE && two) {
            o[0] = mfma_pv_lo<FMT, QATTN_FMT_E4M3>(vf0, pl, o[0], kScaleWordOne);
            o[1] = mfma_pv_lo<FMT, QATTN_FMT_E4M3>(vf1, pl, o[1], kScaleWordOne);
        }
#pragma unroll
        for (int m = 2; m < MB; m += 2) {
            const v8i va = lds_read_frag(vbuf + (m << 11)), vb = lds_read_frag(vbuf + ((m + 1) << 11));
            o[m] = mfma_f8<FMT, QATTN_FMT_E4M3>(va, pv, o[m]);
            o[m + 1] = mfma_f8<FMT, QATTN_FMT_E4M3>(vb, pv, o[m + 1]);
            if (!BYTE && two) {
                o[m] = mfma_pv_lo<FMT, QATTN_FMT_E4M3>(va, pl, o[m], kScaleWordOne);
                o[m + 1] = mfma_pv_lo<FMT, QATTN_FMT_E4M3>(vb, pl, o[m + 1], kScaleWordOne);
            }
        }
        if (BYTE) {
            // the eight equal words are spread where they are used: carried through the loop they cost the D = 128 kernel 7 registers
            // more than its 3 waves per SIMD leave, and the compiler kept them in scratch
            int one_t = one;
            asm volatile("" : "+v"(one_t));
            v8i ones;
#pragma unroll
            for (int w = 0; w < 8; w++) ones[w] = one_t;
            lsum = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ones, pv, lsum, QATTN_FMT_E4M3, QATTN_FMT_E4M3, 0, 0, 0, 0);
        }
    }

    // ---- epilogue
    float l_tot;
    if (BYTE) {
        const float s0l = __shfl(lsum[0], lane & 15), s1l = __shfl(lsum[1], lane & 15);
        l_tot = (lane & 16) ? s1l : s0l;
    } else {
        auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
        l_tot = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    const long orow = orow_of(), lrow = lrow_of();
    const bool has_key = l_tot > 0.0f;   // (a row without a key inside a tile that sweeps: every P was 0 -- a zero row, LSE -inf)
    const float inv = has_key ? a.sv[(long)i * a.Hkv + kvh] / l_tot : 0.0f;
    store_o_rows<MB>(a.out, a.out_fmt, o, inv, orow, hh, qvalid);
    if (!BYTE && a.lse && hh == 0 && qvalid)  // ln sum_j exp(score_j) = ln2 * (m*c - shift) + ln(l')
        a.lse[lrow] = has_key ? 0.6931471805599453f * (m_run * c - kPShift) + __logf(l_tot) : -INFINITY;
    if (a.path && hh == 0 && qvalid) a.path[lrow] = (unsigned char)((!BYTE && two) ? QATTN_PATH_TWO_TERM : QATTN_PATH_ONE_TERM);
}

template <int D, int FMT, bool BYTE>
static int launch_wfp_one(const VfpAttn& a, int two, int sel, int left, int right, hipStream_t st) {
    constexpr int lds = vfp_lds_bytes(D);
    auto kern = attn_vfp8_window_kernel<D, FMT, BYTE>;
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return QATTN_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3((unsigned)(a.Hq * a.nblk)), dim3(kVfpWaves * 64), lds, st, a, two, sel, left, right);
    return QATTN_OK;
}

template <int D, int FMT>
static int launch_wfp_attn(const VfpAttn& a, int precision, int left, int right, hipStream_t st) {
    if (precision == QATTN_PRECISION_ACCURATE || a.total_k < a.two_term_keys)   // (no tile can attend two_term_keys keys: every one is two-term)
        return launch_wfp_one<D, FMT, false>(a, 1, kVfpSelAll, left, right, st);
    // FAST: the tiles that attend many keys on the one-term sweep (an LSE request: exact exponentials), the others two-term
    int rc = a.lse ? launch_wfp_one<D, FMT, false>(a, 0, kVfpSelMany, left, right, st) : launch_wfp_one<D, FMT, true>(a, 0, kVfpSelMany, left, right, st);
    if (rc == QATTN_OK) rc = launch_wfp_one<D, FMT, false>(a, 1, kVfpSelFew, left, right, st);
    return rc;
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

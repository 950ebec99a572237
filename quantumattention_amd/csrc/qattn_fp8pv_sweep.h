// qattn_fp8pv_sweep.h -- the chunk sweep of the kernels that run BOTH attention products on the FP8 matrix pipe, one 4-wave workgroup
// per 128 query rows over a sequence of 64-key chunks: attn_bs_fp8_kernel (qattn_block_sparse_fp8.hip), attn_vfp8_kernel
// (qattn_varlen_fp8.hip) and attn_vfp8_window_kernel (qattn_varlen_window_fp8.hip).  It is the per-wave sequence of attn_fwd_kernel_v4
// (qattn_attn_v4.hip: QK^T -> max / rescale -> exponentials -> PV, two-stage K/V LDS-DMA ring, Q^T fragments parked in LDS) with a
// head-wise FP8 V.  One copy of every step lives here (FpvSweep); a kernel keeps what tells it from the others: the block -> (head, tile)
// map and its launch's `sel` test, which chunk step t sweeps, the mask and its workgroup-uniform guard, the output offsets.  The suite's
// cross-kernel bit equalities (packed = block-sparse under an all-true mask, window = packed where the window masks nothing) hold
// because the three run the same statements below.
//
//   FpvSweep<D, FMT, BYTE> sw(smem);                        lane / wave numbers
//   FpvRing<D> ring(smem, wave, lane, kg_w, vg_w);          K / V images of the head at this wave's 1 KiB piece
//   ring.dma_chunk(first); sw.park_q(row pointer, qvalid); sw.init_state(c, start);
//   for (t = 0; t < n; t++) {
//       sw.read_q(qf); sw.wait_stage(); if (t + 1 < n) ring.dma_chunk(chunk of t + 1);
//       sw.qk(t, qf, s0, s1, vf0, vf1);   -> the kernel's mask on s0 / s1 ->   sw.softmax_pv(s0, s1, vf0, vf1, two, ones);
//   }
//   l = sw.row_sum();   then sw.o, sw.m_run, sw.c and the kernel's own offsets make the rows
// The host side (fpv_launch, fpv_precision_ladder) is at the end.
#pragma once
#include <type_traits>
#include "qattn_attn.h"

namespace qattn {

constexpr int kFpvTile = 128;   // query rows per workgroup
constexpr int kFpvWaves = 4;    // 4 x 32 rows
constexpr int kFpvStages = 2;
static_assert(kFpvTile == kFpvWaves * kQPerWave && kFpvTile == 2 * 64, "a workgroup is one 128-row tile; a 128-key block is two 64-key chunks");

// LIGHT = the byte-exponential kernel (the lean register budget); the exact / two-term variants get one wave per SIMD less
template <int D, bool LIGHT> struct FpvShape {
    static constexpr int WPS = D == 256 ? 2 : (D == 64 ? (LIGHT ? 4 : 3) : (LIGHT ? 3 : 2));
};

// which tiles a launch attends: all / those whose rows see >= two_term_keys keys / fewer (a workgroup of the other launch returns at once)
constexpr int kFpvSelAll = 0, kFpvSelMany = 1, kFpvSelFew = 2;

// LDS: the K / V ring and the parked Q^T fragments (D = 256: 96 KiB); the block-sparse kernel keeps its list behind them
constexpr int fpv_lds_bytes(int D) { return kFpvStages * 2 * 64 * D + kFpvWaves * kQPerWave * D; }
static_assert(fpv_lds_bytes(256) <= 160 * 1024, "the ring and the Q slots fit a CU's LDS");

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }   // workspace sections start 256 bytes apart

// a tile without a key: zero rows, LSE -inf, path code QATTN_PATH_ONE_TERM
template <int D>
__device__ __forceinline__ void fpv_store_empty(void* out, int out_fmt, long orow, float* lse, long lse_at, unsigned char* path, long path_at, int hh,
                                                bool qvalid) {
    constexpr int MB = D / 32;
    v16f z[MB];
#pragma unroll
    for (int m = 0; m < MB; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) z[m][r] = 0.0f;
    store_o_rows<MB>(out, out_fmt, z, 0.0f, orow, hh, qvalid);
    if (lse && hh == 0 && qvalid) lse[lse_at] = -INFINITY;
    if (path && hh == 0 && qvalid) path[path_at] = (unsigned char)QATTN_PATH_ONE_TERM;
}

// A of the row-sum MFMA (see WaveState::lsum in qattn_attn_v2.hip): eight equal words.  softmax_pv asks its `ones` argument for the operand
// at the point of use: a kernel hands back the v8i it carries through the loop (fpv_ones), or -- short of registers -- spreads the one word
// it carries behind an opaque copy that the compiler cannot hoist (fpv_spread_ones)
__device__ __forceinline__ int fpv_ones_word(int lane) {
    const int row = lane & 15, kg = lane >> 4;
    return ((row == 0 && !(kg & 1)) || (row == 1 && (kg & 1))) ? 0x38383838 : 0;
}
__device__ __forceinline__ v8i fpv_ones(int lane) {
    const int one = fpv_ones_word(lane);
    v8i ones;
#pragma unroll
    for (int w = 0; w < 8; w++) ones[w] = one;
    return ones;
}
__device__ __forceinline__ v8i fpv_spread_ones(int one) {
    asm volatile("" : "+v"(one));
    v8i ones;
#pragma unroll
    for (int w = 0; w < 8; w++) ones[w] = one;
    return ones;
}

// The K / V ring.  stage(t) = {K chunk, V chunk} -> slot t & 1; every wave copies 2*RK x 1 KiB of it by LDS-DMA.  kg / vg: the head's
// KFRAG / VFRAG images at this wave's first piece (+ wave << 10)
template <int D>
struct FpvRing {
    static constexpr int NW = kFpvWaves, CH = 64 * D, STAGE = 2 * CH;
    static constexpr int RK = CH / (NW * 1024);   // 1 KiB DMA pieces per wave for the K (and for the V) part of a stage
    unsigned char* dst0;
    const unsigned char *kg_w, *vg_w;
    unsigned lane16, slot_next;
    __device__ __forceinline__ FpvRing(unsigned char* smem, int wave, int lane, const unsigned char* kg, const unsigned char* vg)
        : dst0(smem + (wave << 10)), kg_w(kg), vg_w(vg), lane16((unsigned)lane << 4), slot_next(0) {}
    // (inlined by the compiler's own choice, like the lambda it was: forced, the block-sparse kernels' scalar prologue came out differently)
    __device__ inline void dma_chunk(int chunk) {
        unsigned char* dst = dst0 + slot_next;
        const size_t coff = (size_t)chunk * CH + lane16;
#pragma unroll
        for (int r = 0; r < RK; r++) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kg_w + (coff + r * (NW * 1024))),
                                             (__attribute__((address_space(3))) void*)(dst + r * (NW * 1024)), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vg_w + (coff + r * (NW * 1024))),
                                             (__attribute__((address_space(3))) void*)(dst + CH + r * (NW * 1024)), 16, 0, 0);
        }
        slot_next ^= STAGE;
    }
};

// BYTE: byte-exponential P + matrix-pipe row sums.  !BYTE: exact v_exp_f32, RNE e4m3, fp32 row sums (LSE output) and -- `two` -- the
// hi + lo two-term P.
template <int D, int FMT, bool BYTE>
struct FpvSweep {
    static constexpr int NW = kFpvWaves;
    static constexpr int CH = 64 * D, STAGE = 2 * CH, MB = D / 32, KS = D / 64;

    unsigned char* smem;
    int lane, wave, ql, hh;
    unsigned char* qbuf;                // park_q
    const unsigned char* vbuf;          // qk: the V half of the current stage
    int frag_lane_off;
    // per-wave state: O^T, running max and row sums (BYTE: lsum, by the matrix pipe; else l_run)
    v16f o[MB];
    v4f lsum;
    float c, c8;          // scores -> log2 units, and the byte formula's slope
    float m_run, l_run;
    float lim, off8;      // m_run + thr / c and the byte formula's additive constant (set by the first fix-up)

    __device__ __forceinline__ explicit FpvSweep(unsigned char* smem_) : smem(smem_) {
        const int tid = threadIdx.x;
        lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        ql = lane & 31;
        hh = lane >> 5;
    }

    // Q^T fragments parked in this lane's own LDS slots.  qp: the lane's quantised row (row 0 of the head when !qvalid) + hh * 32
    __device__ __forceinline__ void park_q(const unsigned char* qp, bool qvalid) {
        qbuf = smem + kFpvStages * STAGE + wave * (KS << 11) + (hh << 10) + (ql << 4);
#pragma unroll
        for (int s = 0; s < KS; s++) {
            v4i lo = *reinterpret_cast<const v4i*>(qp + s * 64);
            v4i hi = *reinterpret_cast<const v4i*>(qp + s * 64 + 16);
            if (!qvalid) { lo = v4i{0, 0, 0, 0}; hi = v4i{0, 0, 0, 0}; }
            *reinterpret_cast<v4i*>(qbuf + (s << 11)) = lo;
            *reinterpret_cast<v4i*>(qbuf + (s << 11) + 512) = hi;
        }
    }

    // c_ = sm_scale log2(e) scale_q scale_k; start: where m_run and lim begin, below any raw score
    __device__ __forceinline__ void init_state(float c_, float start) {
        c = c_;
#pragma unroll
        for (int m = 0; m < MB; m++)
#pragma unroll
            for (int r = 0; r < 16; r++) o[m][r] = 0.0f;
        lsum = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        m_run = start; l_run = 0.0f;
        lim = start; off8 = 0.0f;
        constexpr float U16 = 1.0f / 65535.0f;
        c8 = (8.0f * U16) * c;
        frag_lane_off = (hh << 10) + (ql << 4);
    }

    __device__ __forceinline__ void read_q(v8i (&qf)[KS]) const {
#pragma unroll
        for (int s = 0; s < KS; s++) qf[s] = lds_read_frag(qbuf + (s << 11));
    }
    __device__ __forceinline__ void wait_stage() const {
        wait_vmcnt<0>();                  // this wave's pieces of the stage have landed
        __builtin_amdgcn_s_barrier();     // ... and everyone's; every wave is also done with the previous stage's slot
    }

    // S^T = K.Q^T of step t's stage, and the first two V fragments
    __device__ __forceinline__ void qk(int t, const v8i (&qf)[KS], v16f& s0, v16f& s1, v8i& vf0, v8i& vf1) {
        const unsigned char* kbuf = smem + (t & 1) * STAGE + frag_lane_off;
        vbuf = kbuf + CH;
#pragma unroll
        for (int r = 0; r < 16; r++) { s0[r] = 0.0f; s1[r] = 0.0f; }
#pragma unroll
        for (int s = 0; s < KS; s++) {
            const v8i ka = lds_read_frag(kbuf + ((0 * KS + s) << 11)), kb = lds_read_frag(kbuf + ((1 * KS + s) << 11));
            s0 = mfma_f8<FMT, FMT>(ka, qf[s], s0);
            s1 = mfma_f8<FMT, FMT>(kb, qf[s], s1);
        }
        vf0 = lds_read_frag(vbuf);
        vf1 = lds_read_frag(vbuf + (1 << 11));
    }

    // the masked scores of a chunk (-inf = masked) -> P -> O^T += V^T.P^T and the row sums
    template <typename Ones>
    __device__ __forceinline__ void softmax_pv(const v16f& s0, const v16f& s1, const v8i& vf0, const v8i& vf1, int two, Ones&& ones) {
        constexpr float U16 = 1.0f / 65535.0f;
        // ---- running max; rescale only when a row's max grew past the headroom of the shifted exponent
        float mx = max32_after_mfma(s0, s1);
        {
            auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
            mx = max3_raw(__uint_as_float(sw[0]), __uint_as_float(sw[1]), __uint_as_float(sw[1]));
        }
        if (__builtin_expect(__any(mx > lim) != 0, 0)) {   // (mx - m_run) c > thr: P' could overflow e4m3
            const float m_new = fmaxf(m_run, mx);
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
                pv[w] = byte_exp4(s0[4 * w], s0[4 * w + 1], s0[4 * w + 2], s0[4 * w + 3], c8, off8);
                pv[4 + w] = byte_exp4(s1[4 * w], s1[4 * w + 1], s1[4 * w + 2], s1[4 * w + 3], c8, off8);
            }
        } else {
            const float mc = kPShift - m_run * c;
            float ls = 0.0f;
#pragma unroll
            for (int w = 0; w < 8; w++) {
                const v16f& sx = w < 4 ? s0 : s1;
                const int j = w & 3;
                float e[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { e[u] = __builtin_amdgcn_exp2f(__builtin_fmaf(sx[4 * j + u], c, mc)); ls += e[u]; }
                int ph = cvt_pk_fp8<QATTN_FMT_E4M3, false>(e[0], e[1], 0);
                ph = cvt_pk_fp8<QATTN_FMT_E4M3, true>(e[2], e[3], ph);
                pv[w] = ph;
                int plo = 0;
                if (two) plo = lo_terms(e, ph, 0);
                pl[w] = plo;
            }
            l_run += ls;
        }
        // ---- O^T += V^T.P^T, row sums (V's one scale per head is applied in the epilogue; the low term's 2^-5 rides in the scale word)
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
        if (BYTE) lsum = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ones(), pv, lsum, QATTN_FMT_E4M3, QATTN_FMT_E4M3, 0, 0, 0, 0);
    }

    // the row's sum of P' in every lane that holds a piece of it
    __device__ __forceinline__ float row_sum() const {
        if (BYTE) {
            const float s0l = __shfl(lsum[0], lane & 15), s1l = __shfl(lsum[1], lane & 15);
            return (lane & 16) ? s1l : s0l;
        }
        auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
        return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
};

// ---- host side: one launch of an instance, and the launches of a call
template <typename... KArgs, typename... Args>
inline int fpv_launch(void (*kern)(KArgs...), unsigned grid, size_t lds, hipStream_t st, const Args&... args) {
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return QATTN_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kFpvWaves * 64), lds, st, args...);
    return QATTN_OK;
}

// one(byte, two, sel) launches the kernel instance BYTE = decltype(byte)::value.  ACCURATE, or no tile can reach two_term_keys keys
// (max_keys: the most any tile can see): every tile is two-term, one launch.  Otherwise FAST: the tiles that see many keys on the
// one-term sweep (an LSE request: exact exponentials), then the others two-term.
template <typename Launch>
inline int fpv_precision_ladder(int precision, int max_keys, int two_term_keys, bool want_lse, Launch&& one) {
    if (precision == QATTN_PRECISION_ACCURATE || max_keys < two_term_keys) return one(std::false_type{}, 1, kFpvSelAll);
    int rc = want_lse ? one(std::false_type{}, 0, kFpvSelMany) : one(std::true_type{}, 0, kFpvSelMany);
    if (rc == QATTN_OK) rc = one(std::false_type{}, 1, kFpvSelFew);
    return rc;
}

}  // namespace qattn

// qattn_mla_prefill_fp8.hip -- qattn_fp8_mla_prefill_varlen_forward (include/qattn_mla_prefill.h): the NON-ABSORBED prefill form of multi-head
// latent attention on packed sequences, gfx950.  Scores are 192-channel products (128 nope + 64 rotary channels), values have 128 channels, and
// the rotary slice of K is one row per token that every head attends.  A kernel of its own shape, not an instance of
// FpvSweep<D, FMT, BYTE> (qattn_fp8pv_sweep.h): that sweep has ONE D for both products and takes a head-wise q from a pre-pass.
//
// Launches after a zeroing node, none of which reads a length on the host:
//   amax   256-row tiles (qattn_varlen_tile.h), z = 0 / 1 / 2: k_nope and v per (sequence, head), k_pe per sequence; used keys only; atomicMax
//          on the fp32 bits
//   quant  64-row tiles, z = 0: the 192-channel K image of (sequence, head) -- 16 of a row's 24 16-byte vectors come from k_nope[:, h], 8 from
//          the shared k_pe row, all quantised with scale_k[sequence, h] = f(max(amax k_nope, amax k_pe)) -- staged in LDS in KFRAG order
//          (s over 3 slices) and written out linearly; z = 1: the 128-channel VFRAG image of v.  Rows behind the used length are zero bytes.
//   attn   mla_prefill_kernel: one 4-wave workgroup per (head, 128-row tile of a sequence); a wave owns 32 rows.
//            q      the lane's half row (96 of 192 channels) is loaded through q's strides, its abs-max meets the other half's by one
//                   v_permlane32_swap, and the row is quantised to e4m3 in place: the 3 Q^T fragments (24 registers) stay in registers for
//                   the whole sweep -- no q pre-pass, no q8 slab, no parking in LDS
//            ring   two stages of {12 KiB K chunk | 8 KiB V chunk} filled by LDS-DMA, 3 + 2 one-KiB pieces per wave and stage: 40 KiB of LDS,
//                   so that two workgroups share a CU
//            step   S^T = K.Q^T: 2 key tiles x 3 slices = 6 MFMAs -> the kernel's own tail / bottom-right diagonal mask behind a
//                   workgroup-uniform guard -> running max, exact exponentials, P = hi + lo (lo_terms) -> O^T += V^T.P^T: 4 MFMAs per term into
//                   64 accumulators (32 rows x 128 channels)
//          The chunk loop runs to the tile's diagonal (causal) or the sequence's end; no chunk beyond it is read.
#include "qattn_fp8pv_sweep.h"
#include "qattn_varlen_tile.h"
#include "../../include/qattn_mla_prefill.h"

using namespace qattn;

namespace {

constexpr int kDQK = QATTN_MLA_PREFILL_D_QK, kDN = QATTN_MLA_PREFILL_D_NOPE, kDR = QATTN_MLA_PREFILL_D_ROPE, kDV = QATTN_MLA_PREFILL_D_V;
constexpr int kKS = kDQK / 64, kMB = kDV / 32;             // 3 score slices, 4 value blocks
constexpr int kKCh = 64 * kDQK, kVCh = 64 * kDV;           // bytes of a 64-key chunk: 12 288 / 8 192
constexpr int kStage = kKCh + kVCh, kLds = kFpvStages * kStage;
constexpr int kKPieces = kKCh / (kFpvWaves * 1024), kVPieces = kVCh / (kFpvWaves * 1024);   // 1 KiB DMA pieces per wave: 3 + 2
static_assert(kDN + kDR == kDQK && kDN == kDV, "q = nope | rope; k_nope and v are the halves of one projection");
static_assert(2 * kLds <= 160 * 1024, "two workgroups' rings fit a CU's LDS");
constexpr float kStart = -1.0e30f;   // below any raw score (|q8 . k8| <= 192 x 448 x 57344)

// k_nope (z = 0), v (z = 1) and k_pe (z = 2) of one call
struct PrefillQuant {
    const unsigned char* x[3];   // 16-bit inputs
    long ts[3], hs[3];           // element strides of token and head (k_pe: no head axis)
    const int *cu_k, *used;
    int B, H, total_k;
    unsigned* amax[3];           // [B][H], [B][H], [B] fp32 bits, zeroed before the abs-max pass
    unsigned char *k8, *v8;      // the images
    float *sk, *sv;              // [B][H]
};

struct PrefillAttn {
    const unsigned short* q;
    long q_ts, q_hs;
    const unsigned char *k8, *v8;
    const float *sk, *sv;
    void* out;
    float *lse, *scale_q;
    unsigned char* q8;
    const int *cu_q, *cu_k, *used;
    int B, H, total_q, total_k, nblk, out_fmt, xcd_remap;
    float sm_log2e;
};

template <int IN_FMT>
__global__ __launch_bounds__(256) void prefill_amax_kernel(const PrefillQuant a) {
    const int z = blockIdx.z, h = blockIdx.y;
    if (z == 2 && h != 0) return;
    const int vpr = (z == 2 ? kDR : kDN) / 8;   // 16-byte vectors per row
    const VarlenTile t = varlen_tile<kVarlenAmaxRows>(a.cu_k, a.used, a.B, a.total_k, (int)blockIdx.x);
    if (t.tile < 0 || t.tile * kVarlenAmaxRows >= t.len) return;
    const int row0 = t.tile * kVarlenAmaxRows, rows = min(kVarlenAmaxRows, t.len - row0);
    const unsigned char* xh = a.x[z] + 2 * ((long)(t.start + row0) * a.ts[z] + (long)h * a.hs[z]);
    const int nvec = rows * vpr;
    unsigned m = 0;
    for (int base = threadIdx.x; base < nvec; base += 4 * 256) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int idx = base + u * 256;
            v[u] = make_uint4(0, 0, 0, 0);
            if (idx < nvec) v[u] = load_nt(reinterpret_cast<const uint4*>(xh + 2 * (long)(idx / vpr) * a.ts[z]) + idx % vpr);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const unsigned w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int i = 0; i < 4; i++) m = max(m, max(w[i] & 0x7fffu, (w[i] >> 16) & 0x7fffu));   // 16-bit magnitudes order like their values
        }
    }
    m = wave_allmax_u32(m);
    __shared__ unsigned red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        atomicMax(a.amax[z] + (z == 2 ? (long)t.i : (long)t.i * a.H + h), __float_as_uint(load16f<IN_FMT>((unsigned short)m)));
    }
}

// z = 0: K (24 vectors a row: 16 from k_nope[:, h], 8 from k_pe), z = 1: V (16 vectors a row)
template <int IN_FMT, int OUT_FMT>
__global__ __launch_bounds__(256) void prefill_quant_kernel(const PrefillQuant a) {
    constexpr int KPAD = kKCh + (kKCh / 512) * 16;   // the K image, padded by 16 B per 512 B (as vfp_quant_kernel's)
    constexpr int KIT = 64 * (kDQK / 8) / 256, VIT = 64 * (kDV / 8) / 256;   // 6, 4
    __shared__ __attribute__((aligned(16))) unsigned char img[KPAD];
    const int z = blockIdx.z, h = blockIdx.y, tid = threadIdx.x, H = a.H;
    const VarlenTile t = varlen_tile<kVarlenQuantRows>(a.cu_k, a.used, a.B, a.total_k, (int)blockIdx.x);
    if (t.tile < 0) return;
    const float inv_qmax = (float)(1.0 / (double)(OUT_FMT == QATTN_FMT_E4M3 ? 448.0 : 57344.0));
    unsigned am = a.amax[z][(long)t.i * H + h];
    if (z == 0) am = max(am, a.amax[2][t.i]);   // (non-negative fp32 bits order like their values) the rotary slice shares the head's scale
    const float scale = make_scale(__uint_as_float(am & 0x7fffffffu), inv_qmax, QATTN_NUMERICS_COMPILED, IN_FMT);
    if (t.tile == 0 && tid == 0) (z == 0 ? a.sk : a.sv)[(long)t.i * H + h] = scale;   // (also for an empty sequence: amax 0 -> eps)
    if (t.tile * kVarlenQuantRows >= t.len) return;
    const float rinv = 1.0f / scale;
    const int row0 = t.tile * kVarlenQuantRows;
    const long Lp = (long)((t.len + 63) / 64) * 64;
    if (z == 0) {
        const unsigned char* kn = a.x[0] + 2 * ((long)t.start * a.ts[0] + (long)h * a.hs[0]);
        const unsigned char* kp = a.x[2] + 2 * ((long)t.start * a.ts[2]);
        uint4 held[KIT];
#pragma unroll
        for (int it = 0; it < KIT; it++) {
            const int vec = it * 256 + tid, row = row0 + vec / (kDQK / 8), dv = vec % (kDQK / 8);
            held[it] = make_uint4(0, 0, 0, 0);   // (rows behind the used length: zero bytes)
            if (row < t.len)
                held[it] = dv < kDN / 8 ? load_nt(reinterpret_cast<const uint4*>(kn + 2 * (long)row * a.ts[0]) + dv)
                                        : load_nt(reinterpret_cast<const uint4*>(kp + 2 * (long)row * a.ts[2]) + (dv - kDN / 8));
        }
#pragma unroll
        for (int it = 0; it < KIT; it++) {
            const int vec = it * 256 + tid, r = vec / (kDQK / 8), dv = vec % (kDQK / 8);
            const int2 lohi = quant8<IN_FMT, OUT_FMT>(held[it], scale, rinv);
            const int o = kfrag_offset<kDQK>(r, dv * 8);
            *reinterpret_cast<int2*>(img + o + ((o >> 9) << 4)) = lohi;
        }
        __syncthreads();
        uint4* og = reinterpret_cast<uint4*>(a.k8 + (long)H * kDQK * (t.start + 64L * t.i) + ((long)h * Lp + row0) * kDQK);
        for (int i = tid; i < kKCh / 16; i += 256) og[i] = *reinterpret_cast<const uint4*>(img + i * 16 + ((i >> 5) << 4));
        return;
    }
    // v: 8 consecutive d of one key land 16 bytes apart in the image (vfrag_offset); byte scatter as vfp_quant_kernel (a pre-pass, not hot)
    const unsigned char* vh = a.x[1] + 2 * ((long)t.start * a.ts[1] + (long)h * a.hs[1]);
    uint4 held[VIT];
#pragma unroll
    for (int it = 0; it < VIT; it++) {
        const int vec = it * 256 + tid, row = row0 + vec / (kDV / 8);
        held[it] = make_uint4(0, 0, 0, 0);
        if (row < t.len) held[it] = load_nt(reinterpret_cast<const uint4*>(vh + 2 * (long)row * a.ts[1]) + vec % (kDV / 8));
    }
#pragma unroll
    for (int it = 0; it < VIT; it++) {
        const int vec = it * 256 + tid, r = vec / (kDV / 8), dv = vec % (kDV / 8);
        const int2 lohi = quant8<IN_FMT, OUT_FMT>(held[it], scale, rinv);
        unsigned char b[8];
        __builtin_memcpy(b, &lohi, 8);
#pragma unroll
        for (int j = 0; j < 8; j++) img[vfrag_offset<kDV>(r, dv * 8 + j)] = b[j];
    }
    __syncthreads();
    uint4* og = reinterpret_cast<uint4*>(a.v8 + (long)H * kDV * (t.start + 64L * t.i) + ((long)h * Lp + row0) * kDV);
    for (int i = tid; i < kVCh / 16; i += 256) og[i] = reinterpret_cast<const uint4*>(img)[i];
}

// 8 16-bit values x rinv -> 8 e4m3 bytes, saturating (the q quantiser of qattn_mla_splitkv_fp8.hip)
template <int IN_FMT>
__device__ __forceinline__ int2 quant_q8(const uint4& r, float rinv) {
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
    float f[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        f[2 * i] = load16f<IN_FMT>((unsigned short)(w[i] & 0xffffu)) * rinv;
        f[2 * i + 1] = load16f<IN_FMT>((unsigned short)(w[i] >> 16)) * rinv;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) f[i] = fminf(fmaxf(f[i], -448.0f), 448.0f);
    return make_int2(cvt4_fp8<QATTN_FMT_E4M3>(f[0], f[1], f[2], f[3]), cvt4_fp8<QATTN_FMT_E4M3>(f[4], f[5], f[6], f[7]));
}

// grid = H nblk, block = 256.  Two waves per SIMD = the 256-register budget and two workgroups per CU.
template <int FMT, int IN_FMT, bool CAUSAL>
__global__ __launch_bounds__(kFpvWaves * 64, 2) void mla_prefill_kernel(const PrefillAttn a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hh = lane >> 5;

    const int bid = blockIdx.x;
    int h, j;
    if (a.xcd_remap) {   // (speed only) every XCD takes a contiguous range of heads, all sequences of each: their K / V stay in its L2
        const int idx = bid >> 3, hpx = a.H >> 3;
        h = (bid & 7) * hpx + idx / a.nblk;
        j = idx % a.nblk;
    } else {
        h = bid / a.nblk;
        j = bid % a.nblk;
    }
    if (CAUSAL) j = a.nblk - 1 - j;   // (the last tiles of a sequence see the most keys: roughly longest first)
    const VarlenTile tq = varlen_tile<kFpvTile>(a.cu_q, nullptr, a.B, a.total_q, j);
    if (tq.tile < 0 || tq.tile * kFpvTile >= tq.len) return;   // no tile of any sequence
    const int i = tq.i, lq = tq.len;
    const int sk0 = clampi(__builtin_amdgcn_readfirstlane(a.cu_k[i]), 0, a.total_k);
    int lk = clampi(__builtin_amdgcn_readfirstlane(a.cu_k[i + 1]), sk0, a.total_k) - sk0;
    if (a.used) lk = clampi(__builtin_amdgcn_readfirstlane(a.used[i]), 0, lk);
    // bottom-right: row r attends the keys [0, r + 1 + lk - lq).  The tile's first row sets the guard of the mask, its last row the trip count
    const int row_lo = tq.tile * kFpvTile, row_hi = min(row_lo + kFpvTile, lq) - 1;
    const int kguard = CAUSAL ? clampi(row_lo + 1 + lk - lq, 0, lk) : lk;   // every row of the tile attends the keys below it
    const int keys = CAUSAL ? clampi(row_hi + 1 + lk - lq, 0, lk) : lk;     // ... and no row a key at or behind it
    const int n_wg = (keys + 63) >> 6;        // chunks 0 .. n_wg - 1
    const int nch = (lk + 63) >> 6;           // chunks of the sequence's images

    // ---- the ring: stage t -> slot t & 1; a wave copies 3 + 2 one-KiB pieces of it
    const unsigned char* kg = a.k8 + (long)a.H * kDQK * (sk0 + 64L * i) + (long)h * nch * kKCh + (wave << 10) + ((unsigned)lane << 4);
    const unsigned char* vg = a.v8 + (long)a.H * kDV * (sk0 + 64L * i) + (long)h * nch * kVCh + (wave << 10) + ((unsigned)lane << 4);
    unsigned char* dst0 = smem + (wave << 10);
    auto dma_chunk = [&](int chunk) {
        unsigned char* dst = dst0 + (chunk & 1) * kStage;
#pragma unroll
        for (int r = 0; r < kKPieces; r++)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kg + ((size_t)chunk * kKCh + r * 4096)),
                                             (__attribute__((address_space(3))) void*)(dst + r * 4096), 16, 0, 0);
#pragma unroll
        for (int r = 0; r < kVPieces; r++)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vg + ((size_t)chunk * kVCh + r * 4096)),
                                             (__attribute__((address_space(3))) void*)(dst + kKCh + r * 4096), 16, 0, 0);
    };
    if (n_wg > 0) dma_chunk(0);

    // ---- this lane's query row: channels 64 s + 32 hh .. + 32 of every slice; token-wise scale; e4m3 Q^T fragments in registers
    const int qrow = row_lo + wave * kQPerWave + ql;   // row within the sequence
    const bool qvalid = qrow < lq;
    const long tok = tq.start + (qvalid ? qrow : 0);
    const uint4* qp = reinterpret_cast<const uint4*>(a.q + tok * a.q_ts + (long)h * a.q_hs) + 4 * hh;
    uint4 raw[kKS][4];
    unsigned am = 0u;
#pragma unroll
    for (int s = 0; s < kKS; s++)
#pragma unroll
        for (int u = 0; u < 4; u++) {
            raw[s][u] = qp[8 * s + u];
            const unsigned w[4] = {raw[s][u].x, raw[s][u].y, raw[s][u].z, raw[s][u].w};
#pragma unroll
            for (int e = 0; e < 4; e++) am = max(am, max(w[e] & 0x7fffu, (w[e] >> 16) & 0x7fffu));
        }
    {
        const auto sw = __builtin_amdgcn_permlane32_swap(am, am, false, false);
        am = max(sw[0], sw[1]);
    }
    float scale_q = load16f<IN_FMT>((unsigned short)am) / 448.0f;
    if (!(scale_q >= 1.1920928955078125e-07f)) scale_q = 1.1920928955078125e-07f;
    const float rinv = 1.0f / scale_q;
    v8i qf[kKS];
    unsigned char* q8o = a.q8 + (tok * a.H + h) * kDQK + 32 * hh;
#pragma unroll
    for (int s = 0; s < kKS; s++) {
        int2 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            v[u] = quant_q8<IN_FMT>(raw[s][u], rinv);
            if (!qvalid) v[u] = make_int2(0, 0);
        }
        qf[s] = v8i{v[0].x, v[0].y, v[1].x, v[1].y, v[2].x, v[2].y, v[3].x, v[3].y};
        if (a.q8 && qvalid) {
            *reinterpret_cast<v4i*>(q8o + 64 * s) = v4i{v[0].x, v[0].y, v[1].x, v[1].y};
            *reinterpret_cast<v4i*>(q8o + 64 * s + 16) = v4i{v[2].x, v[2].y, v[3].x, v[3].y};
        }
    }
    if (a.scale_q && qvalid && hh == 0) a.scale_q[tok * a.H + h] = scale_q;

    const long orow = (tok * a.H + h) * (2L * kDV);                // bytes: out is dense [total_q, H, 128]
    const long lrow = (long)h * a.total_q + tq.start + qrow;       // lse: [H, total_q]
    if (n_wg == 0) {   // no row of the tile has a key (no DMA was issued)
        fpv_store_empty<kDV>(a.out, a.out_fmt, orow, a.lse, lrow, nullptr, 0, hh, qvalid);
        return;
    }

    const float c = a.sm_log2e * scale_q * a.sk[(long)i * a.H + h];   // raw scores -> log2 units
    int kend = CAUSAL ? qrow + 1 + lk - lq : lk;                      // this lane's row attends the keys [0, kend)
    kend = kend < 0 ? 0 : kend > lk ? lk : kend;
    v16f o[kMB];
#pragma unroll
    for (int m = 0; m < kMB; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[m][r] = 0.0f;
    float m_run = kStart, lim = kStart, l_run = 0.0f;
    const int flo = (hh << 10) + (ql << 4);

    for (int t = 0; t < n_wg; t++) {   // step t sweeps chunk t
        wait_vmcnt<0>();                  // this wave's pieces of the stage have landed
        __builtin_amdgcn_s_barrier();     // ... and everyone's; every wave is also done with the previous stage's slot
        if (t + 1 < n_wg) dma_chunk(t + 1);
        const unsigned char* kbuf = smem + (t & 1) * kStage + flo;
        const unsigned char* vbuf = kbuf + kKCh;
        // ---- S^T = K.Q^T: key tiles 0..31 and 32..63 of the chunk
        v16f s0, s1;
#pragma unroll
        for (int r = 0; r < 16; r++) { s0[r] = 0.0f; s1[r] = 0.0f; }
#pragma unroll
        for (int s = 0; s < kKS; s++) {
            const v8i ka = lds_read_frag(kbuf + (s << 11)), kb = lds_read_frag(kbuf + ((kKS + s) << 11));
            s0 = mfma_f8<FMT, QATTN_FMT_E4M3>(ka, qf[s], s0);
            s1 = mfma_f8<FMT, QATTN_FMT_E4M3>(kb, qf[s], s1);
        }
        const v8i vf0 = lds_read_frag(vbuf), vf1 = lds_read_frag(vbuf + (1 << 11));
        // ---- the ragged tail of the sequence's keys and the bottom-right diagonal, by token (workgroup-uniform condition)
        const int k0 = t * 64;
        if (__builtin_expect(k0 + 64 > kguard, 0)) {
#pragma unroll
            for (int r = 0; r < 32; r++) {
                const int key = k0 + 32 * (r >> 4) + (r & 3) + 8 * ((r & 15) >> 2) + 4 * hh;
                v16f& sx = (r >> 4) ? s1 : s0;
                sx[r & 15] = key >= kend ? -INFINITY : sx[r & 15];
            }
        }
        // ---- running max; rescale only when a row's max grew past the headroom of the shifted exponent
        float mx = max32_after_mfma(s0, s1);
        {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
            mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        }
        if (__builtin_expect(__any(mx > lim) != 0, 0)) {   // (mx - m_run) c > thr: P' could overflow e4m3
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
#pragma unroll
            for (int m = 0; m < kMB; m++)
#pragma unroll
                for (int r = 0; r < 16; r++) o[m][r] *= alpha;
            l_run *= alpha;
            m_run = m_new;
            lim = m_new + kRescaleThr / c;
        }
        // ---- P' = 2^(s c - m c + 5) = hi + lo, fp32 row sums (a masked score: 2^-inf = 0 in both terms)
        v8i ph, pl;
        {
            const float mc = kPShift - m_run * c;
            float ls = 0.0f;
#pragma unroll
            for (int w = 0; w < 8; w++) {
                const v16f& sx = w < 4 ? s0 : s1;
                const int g = w & 3;
                float e[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { e[u] = __builtin_amdgcn_exp2f(__builtin_fmaf(sx[4 * g + u], c, mc)); ls += e[u]; }
                int hi = cvt_pk_fp8<QATTN_FMT_E4M3, false>(e[0], e[1], 0);
                hi = cvt_pk_fp8<QATTN_FMT_E4M3, true>(e[2], e[3], hi);
                ph[w] = hi;
                pl[w] = lo_terms(e, hi, 0);
            }
            l_run += ls;
        }
        // ---- O^T += V^T.P^T (V's one scale per head is applied in the epilogue; the low term's 2^-5 rides in the scale word)
        o[0] = mfma_f8<FMT, QATTN_FMT_E4M3>(vf0, ph, o[0]);
        o[1] = mfma_f8<FMT, QATTN_FMT_E4M3>(vf1, ph, o[1]);
        o[0] = mfma_pv_lo<FMT, QATTN_FMT_E4M3>(vf0, pl, o[0], kScaleWordOne);
        o[1] = mfma_pv_lo<FMT, QATTN_FMT_E4M3>(vf1, pl, o[1], kScaleWordOne);
        {
            const v8i va = lds_read_frag(vbuf + (2 << 11)), vb = lds_read_frag(vbuf + (3 << 11));
            o[2] = mfma_f8<FMT, QATTN_FMT_E4M3>(va, ph, o[2]);
            o[3] = mfma_f8<FMT, QATTN_FMT_E4M3>(vb, ph, o[3]);
            o[2] = mfma_pv_lo<FMT, QATTN_FMT_E4M3>(va, pl, o[2], kScaleWordOne);
            o[3] = mfma_pv_lo<FMT, QATTN_FMT_E4M3>(vb, pl, o[3], kScaleWordOne);
        }
    }

    // ---- epilogue: a row the diagonal left without a key has l = 0 -> a zero row, LSE -inf
    float l_tot;
    {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
        l_tot = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    const float inv = l_tot > 0.0f ? a.sv[(long)i * a.H + h] / l_tot : 0.0f;
    store_o_rows<kMB>(a.out, a.out_fmt, o, inv, orow, hh, qvalid);
    if (a.lse && hh == 0 && qvalid) a.lse[lrow] = l_tot > 0.0f ? 0.6931471805599453f * (m_run * c - kPShift) + __logf(l_tot) : -INFINITY;
}

template <int IN_FMT, int OUT_FMT>
int launch_prefill(const PrefillQuant& qa, const PrefillAttn& a, int causal, hipStream_t st) {
    hipLaunchKernelGGL((prefill_amax_kernel<IN_FMT>), dim3((unsigned)(qa.B + ceil_div(qa.total_k, kVarlenAmaxRows)), qa.H, 3), dim3(256), 0, st, qa);
    hipLaunchKernelGGL((prefill_quant_kernel<IN_FMT, OUT_FMT>), dim3((unsigned)(qa.B + ceil_div(qa.total_k, kVarlenQuantRows)), qa.H, 2), dim3(256), 0,
                       st, qa);
    const unsigned grid = (unsigned)(a.H * a.nblk);
    return causal ? fpv_launch(mla_prefill_kernel<OUT_FMT, IN_FMT, true>, grid, kLds, st, a)
                  : fpv_launch(mla_prefill_kernel<OUT_FMT, IN_FMT, false>, grid, kLds, st, a);
}

bool prefill_dims_ok(int B, int H, int total_q, int total_k) {
    // 32-bit grids: H (B + ceil(total_q / 128)) attention workgroups, B + ceil(total_k / 64) quantise tiles per head (H on the y axis)
    return B >= 1 && H >= 1 && H <= 65535 && total_q >= 0 && total_k >= 0 && (long long)H * (B + (long long)ceil_div(total_q, kFpvTile)) <= 0x7fffffffLL &&
           (long long)B + ceil_div(total_k, 64) <= 0x7fffffffLL && (long long)total_k + 64LL * B <= 0x7fffffffLL;
}
size_t image_bytes(int B, int H, int total_k, int D) { return (size_t)H * D * ((size_t)total_k + 64 * (size_t)B); }

}  // namespace

extern "C" size_t qattn_fp8_mla_prefill_varlen_workspace_bytes(int B, int H, int total_q, int total_k) {
    if (!prefill_dims_ok(B, H, total_q, total_k)) return 0;
    // [K images | V images | scale_k, scale_v | abs-max words of k_nope, v, k_pe]
    return up256(image_bytes(B, H, total_k, kDQK)) + up256(image_bytes(B, H, total_k, kDV)) + up256(sizeof(float) * 2 * (size_t)B * H) +
           up256(sizeof(unsigned) * ((size_t)B * (2 * H + 1)));
}

extern "C" int qattn_fp8_mla_prefill_varlen_forward(const void* q, const void* k_nope, const void* k_pe, const void* v, const long long* strides7,
                                                    int in_fmt, void* out, float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k,
                                                    const int* seqused_k, int B, int H, int total_q, int total_k, int fp8_fmt, int is_causal,
                                                    float sm_scale, void* q8, float* scale_q, float* scale_k, float* scale_v, void* workspace,
                                                    size_t workspace_bytes, void* stream) {
    if (!q || !k_nope || !k_pe || !v || !out || !cu_seqlens_q || !cu_seqlens_k) return QATTN_ERR_INVALID_ARG;
    if (!prefill_dims_ok(B, H, total_q, total_k)) return QATTN_ERR_INVALID_ARG;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (!(sm_scale > 0.0f) || !(sm_scale < INFINITY)) return QATTN_ERR_INVALID_ARG;
    long long st7[7] = {(long long)H * kDQK, kDQK, (long long)H * kDN, kDN, kDR, (long long)H * kDV, kDV};   // dense
    if (strides7)
        for (int s = 0; s < 7; s++) {
            if (strides7[s] < 0 || strides7[s] % 8 != 0) return QATTN_ERR_INVALID_ARG;
            st7[s] = strides7[s];
        }
    if (((size_t)q | (size_t)k_nope | (size_t)k_pe | (size_t)v | (size_t)out | (size_t)q8) % 16 != 0) return QATTN_ERR_INVALID_ARG;
    const size_t need = qattn_fp8_mla_prefill_varlen_workspace_bytes(B, H, total_q, total_k);
    if (!workspace || workspace_bytes < need || (size_t)workspace % 16 != 0) return QATTN_ERR_WORKSPACE;
    if (total_q == 0) return QATTN_OK;   // no query row: nothing to compute or write
    hipStream_t st = (hipStream_t)stream;
    const size_t nh = (size_t)B * H;
    unsigned char* w = (unsigned char*)workspace;
    unsigned char* k8 = w;    w += up256(image_bytes(B, H, total_k, kDQK));
    unsigned char* v8 = w;    w += up256(image_bytes(B, H, total_k, kDV));
    float* sw = (float*)w;    w += up256(sizeof(float) * 2 * nh);
    unsigned* amax = (unsigned*)w;
    PrefillQuant qa;
    qa.x[0] = (const unsigned char*)k_nope; qa.x[1] = (const unsigned char*)v; qa.x[2] = (const unsigned char*)k_pe;
    qa.ts[0] = st7[2]; qa.hs[0] = st7[3]; qa.ts[1] = st7[5]; qa.hs[1] = st7[6]; qa.ts[2] = st7[4]; qa.hs[2] = 0;
    qa.cu_k = cu_seqlens_k; qa.used = seqused_k;
    qa.B = B; qa.H = H; qa.total_k = total_k;
    qa.amax[0] = amax; qa.amax[1] = amax + nh; qa.amax[2] = amax + 2 * nh;
    qa.k8 = k8; qa.v8 = v8;
    qa.sk = scale_k ? scale_k : sw; qa.sv = scale_v ? scale_v : sw + nh;
    PrefillAttn a;
    a.q = (const unsigned short*)q; a.q_ts = st7[0]; a.q_hs = st7[1];
    a.k8 = k8; a.v8 = v8; a.sk = qa.sk; a.sv = qa.sv;
    a.out = out; a.lse = lse; a.scale_q = scale_q; a.q8 = (unsigned char*)q8;
    a.cu_q = cu_seqlens_q; a.cu_k = cu_seqlens_k; a.used = seqused_k;
    a.B = B; a.H = H; a.total_q = total_q; a.total_k = total_k;
    a.nblk = B + ceil_div(total_q, kFpvTile);
    a.out_fmt = in_fmt;
    a.xcd_remap = (H % 8 == 0 && xcd_count() == 8) ? 1 : 0;   // (the XCD-contiguous map assumes 8 XCDs; a speed assumption only)
    a.sm_log2e = sm_scale * 1.4426950408889634f;
    if (zero_words(amax, (long)(2 * nh + B), st) != hipSuccess) return QATTN_ERR_LAUNCH;
    int rc;
    if (in_fmt == QATTN_FMT_BF16)
        rc = fp8_fmt == QATTN_FMT_E4M3 ? launch_prefill<QATTN_FMT_BF16, QATTN_FMT_E4M3>(qa, a, is_causal, st)
                                       : launch_prefill<QATTN_FMT_BF16, QATTN_FMT_E5M2>(qa, a, is_causal, st);
    else
        rc = fp8_fmt == QATTN_FMT_E4M3 ? launch_prefill<QATTN_FMT_FP16, QATTN_FMT_E4M3>(qa, a, is_causal, st)
                                       : launch_prefill<QATTN_FMT_FP16, QATTN_FMT_E5M2>(qa, a, is_causal, st);
    if (rc != QATTN_OK) return rc;
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

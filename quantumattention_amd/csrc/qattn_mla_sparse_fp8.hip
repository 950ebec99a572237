// qattn_mla_sparse_fp8.hip -- qattn_fp8_mla_paged_sparse_forward (include/qattn_mla_sparse.h): absorbed multi-head latent attention over the
// keys an index list names, on the ROW-MAJOR paged FP8 latent cache, gfx950.
//
// WORK ITEM  (slot b, position i, 64-row tile of the position's Hq heads, split of the list), 4 waves.  A tile never spans two positions:
// their lists differ.  The list is cut into groups of 64 entries; a split owns at most 32 consecutive groups.
// RESOLVE    once, in a prologue: index -> validity -> table entry (clamped) -> physical row number.  The three dependent global loads of
//            an entry happen here, 8 entries per thread in flight, never inside the group loop.  The row numbers (-1: invalid) go to 8 KiB of
//            LDS; a wave's 64 lanes resolve exactly one group, so the group's 64-bit valid mask is one ballot.
// GATHER     the LDS-DMA of the dense kernel's ring with per-lane sources: the instruction that fills block (t, s, hh) of the ring image lets
//            lane (half, key) read the 16 bytes at row(32 t + key) 576 + 64 s + 32 hh + 16 half, and the LDS destination stays lane-linear.
//            A gathered group therefore lands in the chunk image [t:2][s:9][hh:2][half:2][key:32][16 B] that csrc/qattn_mla_splitkv_fp8.hip
//            sweeps -- 36 instructions per group, every byte of a fetched row used.  An invalid entry reads row 0 of the pool.
// SWEEP      phase A, the cooperative transposition, phase B, the epilogue and the combine are the dense kernel's, copied: its unit stays
//            instruction-identical.  The tests on L_b became tests on the group's valid mask; a group whose mask is zero is skipped.
// LDS (bytes)  the dense kernel's 153 088 | row numbers 8 192 | group masks 256 = 161 536.
#include "qattn_fp8pv_sweep.h"
#include "../../include/qattn_mla_sparse.h"

using namespace qattn;

namespace {

constexpr int kD = QATTN_MLA_D, kDV = QATTN_MLA_D_LATENT, kKS = kD / 64, kCH = 64 * kD;
constexpr int kMaxGroups = QATTN_MLA_SPARSE_SPLIT_ENTRIES / 64;
constexpr int kOffVT = 2 * kCH, kOffP = kOffVT + 64 * kDV, kOffMx = kOffP + 8192, kOffAl = kOffMx + 512, kOffLs = kOffAl + 256,
              kOffMf = kOffLs + 512, kOffQ = kOffMf + 256, kOffRow = kOffQ + 64 * kD, kOffMask = kOffRow + 4 * QATTN_MLA_SPARSE_SPLIT_ENTRIES,
              kSparseLds = kOffMask + 8 * kMaxGroups;
static_assert(kSparseLds <= 160 * 1024, "the dense kernel's buffers, a split's row numbers and its masks fit a CU's LDS");
static_assert(kMaxGroups == 32, "the live-group set is one 32-bit word");
constexpr float kMlaStart = -1.0e20f;   // below any raw score (|q8 . k8| <= 576 x 448 x 57344)

struct SparseArgs {
    const unsigned short* q;
    long qsb, qsh, qss;   // element strides of q
    const unsigned char* pool;
    const int* table;
    long tstride;
    const float* scale;
    const int* seqused;
    const int* indices;
    long isb, iss;        // element strides of the index lists
    void* out;
    float *lse, *po, *plse, *scale_q;
    unsigned char* q8;
    int B, Hq, Sq, topk, ns, ht, causal, out_fmt, num_pages, page_size, capacity;
    float c0;   // sm_scale log2(e)
};

template <int IN_FMT>
__device__ __forceinline__ unsigned amax_bits16(const uint4& r, unsigned m) {
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; i++) m = max(m, max(w[i] & 0x7fffu, (w[i] >> 16) & 0x7fffu));   // 16-bit magnitudes order like their values
    return m;
}

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

// four bits -> four byte masks: bit k of nib keeps byte k
__device__ __forceinline__ unsigned nibble_bytes(unsigned nib) {
    return ((nib | (nib << 7) | (nib << 14) | (nib << 21)) & 0x01010101u) * 0xffu;
}

// grid = B ns Sq ht, block = 256.  blockIdx.x = ((b ns + split) Sq + i) ht + head tile: the head tiles of a (slot, split, position) gather the
// same rows side by side.  amdgpu_waves_per_eu(2, 2) states the register budget (at most 256 VGPRs, no AGPRs), as in the dense kernel.
template <int FMT, int IN_FMT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void mla_sparse_sweep_kernel(const SparseArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hh = lane >> 5, rh = wave & 1, kh = wave >> 1;
    const int tiles = a.Sq * a.ht;
    const int tile = (int)(blockIdx.x % (unsigned)tiles), bs = (int)(blockIdx.x / (unsigned)tiles);
    const int pos = tile / a.ht, htile = tile % a.ht;
    const int split = bs % a.ns, b = bs / a.ns;
    const int HS = a.Hq * a.Sq;
    int L = a.seqused[b];
    L = L < 0 ? 0 : L > a.capacity ? a.capacity : L;
    int kend = a.causal ? L - a.Sq + pos + 1 : L;   // the positions [0, kend) are valid for this tile's rows
    kend = kend < 0 ? 0 : kend;
    const int ngr = (a.topk + 63) >> 6, per = (ngr + a.ns - 1) / a.ns;   // per <= 32: the launcher's ns >= ceil(topk / 2048)
    const int g_lo = split * per, g_hi = min(ngr, g_lo + per), n = g_hi - g_lo;

    // ---- resolve: this split's entries -> physical rows (-1: invalid) and one valid mask per group.  Entry 64 (4 k + wave) + lane: a wave's
    // ballot is a group's mask.  Every LDS word of the n groups is written, the tail behind topk included.
    int* rows = reinterpret_cast<int*>(smem + kOffRow);
    unsigned* masks = reinterpret_cast<unsigned*>(smem + kOffMask);
    {
        const int* irow = a.indices + (long)b * a.isb + (long)pos * a.iss;
        const int* trow = a.table + (long)b * a.tstride;
        int j[kMaxGroups / 4];
#pragma unroll
        for (int k = 0; k < kMaxGroups / 4; k++) {
            const int e = (g_lo + 4 * k + wave) * 64 + lane;
            j[k] = (4 * k + wave < n && e < a.topk) ? irow[e] : -1;
        }
#pragma unroll
        for (int k = 0; k < kMaxGroups / 4; k++) {
            if (4 * k + wave >= n) break;   // (wave-uniform)
            const bool valid = j[k] >= 0 && j[k] < kend;
            int row = -1;
            if (valid) {   // j < kend <= capacity: an entry of the table's row
                int page = trow[j[k] / a.page_size];
                page = page < 0 ? 0 : page > a.num_pages - 1 ? a.num_pages - 1 : page;
                row = page * a.page_size + j[k] % a.page_size;   // <= num_pages page_size - 1 <= 2^31 - 2
            }
            rows[(4 * k + wave) * 64 + lane] = row;
            const unsigned long long m = __ballot(valid);
            if (lane == 0) { masks[2 * (4 * k + wave)] = (unsigned)m; masks[2 * (4 * k + wave) + 1] = (unsigned)(m >> 32); }
        }
    }
    lds_barrier();
    unsigned live;   // bit g: group g_lo + g has a valid entry
    {
        const bool nz = lane < n && (masks[2 * lane] | masks[2 * lane + 1]) != 0u;
        live = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)__ballot(nz));
    }

    // ---- the gather: every wave fills 9 x 1 KiB blocks of the ring image; block wave + 4 r is (t, s, hh), lane (half, key)
    auto dma_group = [&](int g, int slot) {
        const int r0 = rows[g * 64 + ql], r1 = rows[g * 64 + 32 + ql];
        const unsigned char* s0 = a.pool + (size_t)(r0 < 0 ? 0 : r0) * kD + 16 * hh;
        const unsigned char* s1 = a.pool + (size_t)(r1 < 0 ? 0 : r1) * kD + 16 * hh;
        unsigned char* dst = smem + slot * kCH + (wave << 10);
#pragma unroll
        for (int r = 0; r < kCH / 4096; r++) {
            const int blk = wave + 4 * r, ts = blk >> 1;   // ts = 9 t + s
            const unsigned char* src = (ts >= kKS ? s1 + 64 * (ts - kKS) : s0 + 64 * ts) + 32 * (blk & 1);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(dst + r * 4096), 16, 0, 0);
        }
    };
    if (live) dma_group(__builtin_ctz(live), 0);

    // ---- this lane's query row: token-wise scale from the row's abs-max, e4m3 Q^T fragments parked in LDS
    const int h = htile * 64 + rh * 32 + ql;
    const bool qvalid = h < a.Hq;
    const int R = (qvalid ? h : 0) * a.Sq + pos;   // the row of [Hq, Sq]
    const uint4* qrow = reinterpret_cast<const uint4*>(a.q + (long)b * a.qsb + (long)(qvalid ? h : 0) * a.qsh + (long)pos * a.qss) + 4 * hh;
    unsigned am = 0u;
#pragma unroll
    for (int s = 0; s < kKS; s++)
#pragma unroll
        for (int i = 0; i < 4; i++) am = amax_bits16<IN_FMT>(qrow[8 * s + i], am);
    {
        const auto sw = __builtin_amdgcn_permlane32_swap(am, am, false, false);
        am = max(sw[0], sw[1]);
    }
    float scale_q = load16f<IN_FMT>((unsigned short)am) / 448.0f;
    if (!(scale_q >= 1.1920928955078125e-07f)) scale_q = 1.1920928955078125e-07f;
    const float rinv = 1.0f / scale_q;
    const int flo = (hh << 10) + (ql << 4);
    const unsigned char* qpark = smem + kOffQ + ((rh * kKS) << 11) + flo;   // [rh][s:9][hh][half][q:32][16 B]: the B operands of phase A
    if (kh == 0) {   // (the two waves of a row half would park the same bytes)
        const bool q8_out = split == 0 && qvalid && a.q8;
        unsigned char* qo = a.q8 + ((long)b * HS + R) * kD + 32 * hh;
#pragma unroll
        for (int s = 0; s < kKS; s++) {
            int2 v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                v[i] = quant_q8<IN_FMT>(qrow[8 * s + i], rinv);
                if (!qvalid) v[i] = make_int2(0, 0);
            }
            const v4i lo = v4i{v[0].x, v[0].y, v[1].x, v[1].y}, hi = v4i{v[2].x, v[2].y, v[3].x, v[3].y};
            *reinterpret_cast<v4i*>(const_cast<unsigned char*>(qpark) + (s << 11)) = lo;
            *reinterpret_cast<v4i*>(const_cast<unsigned char*>(qpark) + (s << 11) + 512) = hi;
            if (q8_out) {
                *reinterpret_cast<v4i*>(qo + 64 * s) = lo;
                *reinterpret_cast<v4i*>(qo + 64 * s + 16) = hi;
            }
        }
        if (split == 0 && qvalid && a.scale_q && hh == 0) a.scale_q[(long)b * HS + R] = scale_q;
    }
    lds_barrier();
    const float scale_kv = a.scale[b];
    const float c = a.c0 * scale_q * scale_kv;

    v16f o[2][4];
#pragma unroll
    for (int r2 = 0; r2 < 2; r2++)
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
            for (int r = 0; r < 16; r++) o[r2][m][r] = 0.0f;
    float m_run = kMlaStart, lim = kMlaStart, l_run = 0.0f;

    float* xm = reinterpret_cast<float*>(smem + kOffMx);   // [rh][kh][32]
    float* al = reinterpret_cast<float*>(smem + kOffAl);   // [rh][32]
    unsigned char* pw = smem + kOffP + rh * 2048 + (hh << 10) + (kh << 9) + (ql << 4);   // this lane's 16 bytes of P^T: [term][rh][hh][half][q]

    for (int slot = 0; live != 0u; slot ^= 1) {
        const int g = __builtin_ctz(live);
        live &= live - 1u;
        wait_vmcnt<0>();                  // this wave's pieces of the group have landed
        __builtin_amdgcn_s_barrier();     // ... and everyone's; every wave is done with phase B of the group before and with the other slot
        if (live) dma_group(__builtin_ctz(live), slot ^ 1);
        const unsigned char* ring = smem + slot * kCH;
        const unsigned mlo = (unsigned)__builtin_amdgcn_readfirstlane((int)masks[2 * g]);
        const unsigned mhi = (unsigned)__builtin_amdgcn_readfirstlane((int)masks[2 * g + 1]);

        // ---- phase A: 32 keys x 32 rows of scores
        v16f s;
#pragma unroll
        for (int r = 0; r < 16; r++) s[r] = 0.0f;
        {
            const unsigned char* kbuf = ring + ((kh * kKS) << 11) + flo;
#pragma unroll
            for (int sl = 0; sl < kKS; sl++) s = mfma_f8<FMT, QATTN_FMT_E4M3>(lds_read_frag(kbuf + (sl << 11)), lds_read_frag(qpark + (sl << 11)), s);
        }
        const unsigned mb = qvalid ? (kh ? mhi : mlo) >> (4 * hh) : 0u;   // register r: entry 32 kh + 4 hh + 8 (r >> 2) + (r & 3) of the group
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            if (((mb >> (8 * (r >> 2) + (r & 3))) & 1u) == 0u) s[r] = -INFINITY;
            mx = fmaxf(mx, s[r]);
        }
        {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
            mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        }
        if (hh == 0) xm[(rh * 2 + kh) * 32 + ql] = mx;

        // ---- the group's first 512 channels, transposed into VFRAG order; a thread: 16 keys (one (half, hh) of the key index) x 4 channels
#pragma unroll
        for (int it = 0; it < 2; it++) {
            const int u = it * 256 + tid;
            const int dq = u & 3, khh = (u >> 2) & 1, piece = (u >> 3) & 31, half = u >> 8;   // (it = half)
            const int d0 = 16 * piece + 4 * dq;
            const unsigned char* src = ring + ((half * kKS + (d0 >> 6)) << 11) + (((d0 >> 5) & 1) << 10) + (((d0 >> 4) & 1) << 9) + (d0 & 15);
            unsigned ov[4][4];
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const unsigned char* sk = src + ((8 * w + 4 * khh) << 4);
                const unsigned r0 = *reinterpret_cast<const unsigned*>(sk), r1 = *reinterpret_cast<const unsigned*>(sk + 16);
                const unsigned r2 = *reinterpret_cast<const unsigned*>(sk + 32), r3 = *reinterpret_cast<const unsigned*>(sk + 48);
                const unsigned t0 = __builtin_amdgcn_perm(r1, r0, 0x05010400u), t1 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);
                const unsigned t2 = __builtin_amdgcn_perm(r3, r2, 0x05010400u), t3 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
                ov[w][0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u);
                ov[w][1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
                ov[w][2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
                ov[w][3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
            }
            if ((mlo & mhi) != 0xffffffffu) {   // (workgroup-uniform) a group with invalid entries: their value bytes count as zero
                const unsigned mh = (half ? mhi : mlo) >> (4 * khh);
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    const unsigned keep = nibble_bytes((mh >> (8 * w)) & 0xfu);   // the entries 32 half + 8 w + 4 khh .. + 3
#pragma unroll
                    for (int j = 0; j < 4; j++) ov[w][j] &= keep;
                }
            }
            unsigned char* dst = smem + kOffVT + ((d0 >> 5) << 11) + (khh << 10) + (half << 9) + ((d0 & 31) << 4);
#pragma unroll
            for (int j = 0; j < 4; j++) *reinterpret_cast<v4i*>(dst + 16 * j) = v4i{(int)ov[0][j], (int)ov[1][j], (int)ov[2][j], (int)ov[3][j]};
        }
        lds_barrier();

        // ---- the row maxima of both key halves; rescale only when a row's maximum outgrew the headroom of the shifted exponent
        mx = fmaxf(mx, xm[(rh * 2 + (kh ^ 1)) * 32 + ql]);
        float alpha = 1.0f;
        if (__any(mx > lim) != 0) {   // (the same vote in both waves of a row half: same maxima, same history)
            const float m_new = fmaxf(m_run, mx);
            alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
            l_run *= alpha;
            m_run = m_new;
            lim = m_new + kRescaleThr / c;
        }
        if (kh == 0 && hh == 0) al[rh * 32 + ql] = alpha;
        {
            const float mc = kPShift - m_run * c;
            float ls = 0.0f;
            v4i ph, pl;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                float e[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { e[u] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[4 * w + u], c, mc)); ls += e[u]; }
                int hi = cvt_pk_fp8<QATTN_FMT_E4M3, false>(e[0], e[1], 0);
                hi = cvt_pk_fp8<QATTN_FMT_E4M3, true>(e[2], e[3], hi);
                ph[w] = hi;
                pl[w] = lo_terms(e, hi, 0);
            }
            l_run += ls;
            *reinterpret_cast<v4i*>(pw) = ph;
            *reinterpret_cast<v4i*>(pw + 4096) = pl;
        }
        lds_barrier();

        // ---- phase B: this wave's 128 value channels of all 64 rows
        {
            const float a0 = al[ql], a1 = al[32 + ql];
            if (__any(a0 != 1.0f || a1 != 1.0f) != 0) {
#pragma unroll
                for (int m = 0; m < 4; m++)
#pragma unroll
                    for (int r = 0; r < 16; r++) { o[0][m][r] *= a0; o[1][m][r] *= a1; }
            }
        }
        const unsigned char* vbase = smem + kOffVT + ((4 * wave) << 11) + flo;
#pragma unroll
        for (int r2 = 0; r2 < 2; r2++) {
            const v8i ph = lds_read_frag(smem + kOffP + r2 * 2048 + flo), pl = lds_read_frag(smem + kOffP + 4096 + r2 * 2048 + flo);
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const v8i vf = lds_read_frag(vbase + (m << 11));
                o[r2][m] = mfma_f8<FMT, QATTN_FMT_E4M3>(vf, ph, o[r2][m]);
                o[r2][m] = mfma_pv_lo<FMT, QATTN_FMT_E4M3>(vf, pl, o[r2][m], kScaleWordOne);
            }
        }
    }

    // ---- epilogue: the row sums of both key halves, the rows
    float* lsx = reinterpret_cast<float*>(smem + kOffLs);   // [rh][kh][32]
    float* mfx = reinterpret_cast<float*>(smem + kOffMf);   // [rh][32]
    {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
        l_run = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    if (hh == 0) lsx[(rh * 2 + kh) * 32 + ql] = l_run;
    if (kh == 0 && hh == 0) mfx[rh * 32 + ql] = m_run;
    lds_barrier();
    const long slab = ((long)split * a.B + b) * HS;   // this split's rows of the partial buffers
#pragma unroll
    for (int r2 = 0; r2 < 2; r2++) {
        const float l_tot = lsx[(r2 * 2) * 32 + ql] + lsx[(r2 * 2 + 1) * 32 + ql];
        const float inv = l_tot > 0.0f ? scale_kv / l_tot : 0.0f;
        const int ho = htile * 64 + r2 * 32 + ql;
        const bool valid = ho < a.Hq;
        const long Ro = (long)(valid ? ho : 0) * a.Sq + pos;
        if (a.ns == 1) {
            store_o_rows<4>(a.out, a.out_fmt, o[r2], inv, (((long)b * HS + Ro) * kDV + 128 * wave) * 2, hh, valid);
        } else if (valid) {
            float* dst = a.po + (slab + Ro) * kDV + 128 * wave + 4 * hh;
#pragma unroll
            for (int m = 0; m < 4; m++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    *reinterpret_cast<float4*>(dst + 32 * m + 8 * j) =
                        make_float4(o[r2][m][4 * j] * inv, o[r2][m][4 * j + 1] * inv, o[r2][m][4 * j + 2] * inv, o[r2][m][4 * j + 3] * inv);
        }
    }
    if (kh == 0 && hh == 0 && qvalid) {
        const float l_tot = lsx[(rh * 2) * 32 + ql] + lsx[(rh * 2 + 1) * 32 + ql];
        const float v = l_tot > 0.0f ? 0.6931471805599453f * (mfx[rh * 32 + ql] * c - kPShift) + __logf(l_tot) : -INFINITY;
        if (a.ns == 1) { if (a.lse) a.lse[(long)b * HS + R] = v; }
        else a.plse[slab + R] = v;
    }
}

// One launch merges all ns partials of a row (the dense unit's combine, copied: that unit stays as it is): grid = B Hq Sq rows, block = 128,
// a thread owns 4 channels.  L = log sum_i exp(lse_i), O = sum_i exp(lse_i - L) O_i in fp32 in the order of i, one rounding.
__global__ __launch_bounds__(128) void mla_sparse_combine_kernel(const float* po, const float* plse, void* out, float* lse, long rows, int ns,
                                                                 int out_fmt) {
    const long row = blockIdx.x;
    float mx = -INFINITY;
    for (int i = 0; i < ns; i++) mx = fmaxf(mx, plse[i * rows + row]);
    float sum = 0.0f;
    if (mx > -INFINITY)
        for (int i = 0; i < ns; i++) sum += __expf(plse[i * rows + row] - mx);
    const float Lr = mx > -INFINITY ? mx + __logf(sum) : -INFINITY;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (mx > -INFINITY)
        for (int i = 0; i < ns; i++) {
            const float li = plse[i * rows + row];
            if (!(li > -INFINITY)) continue;   // (an empty split's rows)
            const float w = __expf(li - Lr);
            const float4 x = *reinterpret_cast<const float4*>(po + (i * rows + row) * kDV + 4 * threadIdx.x);
            acc.x += w * x.x; acc.y += w * x.y; acc.z += w * x.z; acc.w += w * x.w;
        }
    const bool bf = out_fmt == QATTN_FMT_BF16;
    uint2 pk;
    pk.x = bf ? pack2_bf16(acc.x, acc.y) : pack2_f16(acc.x, acc.y);
    pk.y = bf ? pack2_bf16(acc.z, acc.w) : pack2_f16(acc.z, acc.w);
    *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(out) + (row * kDV + 4 * threadIdx.x) * 2) = pk;
    if (lse && threadIdx.x == 0) lse[row] = Lr;
}

int min_splits(int topk) { return (topk + QATTN_MLA_SPARSE_SPLIT_ENTRIES - 1) / QATTN_MLA_SPARSE_SPLIT_ENTRIES; }

constexpr int kAutoEntries = 128;   // the fewest list entries the auto rule gives a split: two groups (measured)

}  // namespace

extern "C" int qattn_mla_sparse_auto_splits(int B, int Hq, int Sq, int topk, int num_cus) {
    if (B <= 0 || Hq <= 0 || Sq <= 0 || topk <= 0 || num_cus <= 0) return 1;
    const long long base = (long long)B * Sq * ((Hq + 63) / 64);
    long long ns = num_cus / base;
    if (ns > topk / kAutoEntries) ns = topk / kAutoEntries;
    if (ns > QATTN_MLA_MAX_SPLITS) ns = QATTN_MLA_MAX_SPLITS;
    if (ns < min_splits(topk)) ns = min_splits(topk);   // (<= 64 for every topk the forward call accepts)
    return ns < 1 ? 1 : (int)ns;
}

extern "C" size_t qattn_fp8_mla_paged_sparse_workspace_bytes(int B, int Hq, int Sq, int num_splits) {
    if (B <= 0 || Hq <= 0 || Sq <= 0 || num_splits <= 1) return 0;
    const size_t rows = (size_t)num_splits * B * Hq * Sq;
    return up256(rows * kDV * sizeof(float)) + up256(rows * sizeof(float));
}

extern "C" int qattn_fp8_mla_paged_sparse_forward(const void* q16, int in_fmt, const long long* q_strides3, const void* pool,
                                                  const int* block_table, long long table_stride, int num_pages, int page_size, int max_pages,
                                                  const float* scale, const int* indices, const long long* idx_strides2, int topk, void* out,
                                                  float* lse, const int* seqused_k, int B, int Hq, int Sq, int fp8_fmt, int is_causal,
                                                  float sm_scale, int num_splits, void* q8, float* scale_q, float* partial_o,
                                                  float* partial_lse, void* workspace, size_t workspace_bytes, void* stream) {
    if (!q16 || !pool || !block_table || !scale || !indices || !out || !seqused_k) return QATTN_ERR_INVALID_ARG;
    if (((size_t)block_table | (size_t)indices) % 4 != 0 || ((size_t)pool | (size_t)q16 | (size_t)out | (size_t)q8 | (size_t)workspace) % 16 != 0)
        return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || Hq <= 0 || Sq <= 0 || topk <= 0 || topk > QATTN_MLA_SPARSE_MAX_TOPK || (long long)Hq * Sq > (1 << 20)) return QATTN_ERR_INVALID_ARG;
    if (num_pages <= 0 || max_pages <= 0 || page_size <= 0 || table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    if ((long long)num_pages * page_size > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (a physical row number is an int)
    const long long capacity = (long long)max_pages * page_size;
    if (capacity > 0x7fffffffLL - 64) return QATTN_ERR_INVALID_ARG;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (!(sm_scale > 0.0f) || !(sm_scale < INFINITY)) return QATTN_ERR_INVALID_ARG;
    if (num_splits < 0 || num_splits > QATTN_MLA_MAX_SPLITS || (num_splits > 0 && num_splits < min_splits(topk))) return QATTN_ERR_INVALID_ARG;
    if (q_strides3)
        for (int i = 0; i < 3; i++)
            if (q_strides3[i] < 0 || q_strides3[i] % 8 != 0) return QATTN_ERR_INVALID_ARG;
    if (idx_strides2 && (idx_strides2[0] < 0 || idx_strides2[1] < 0)) return QATTN_ERR_INVALID_ARG;
    const int ns = num_splits ? num_splits : qattn_mla_sparse_auto_splits(B, Hq, Sq, topk, cu_count());
    const int ht = (Hq + 63) / 64;
    if ((long long)B * ns * Sq * ht > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;
    if ((long long)B * Hq * Sq > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (the combine launches one block per row: a 32-bit grid)
    const size_t rows = (size_t)B * Hq * Sq;
    float *po = partial_o, *pl = partial_lse;
    if (ns > 1 && (!po || !pl)) {
        if (!workspace || workspace_bytes < qattn_fp8_mla_paged_sparse_workspace_bytes(B, Hq, Sq, ns)) return QATTN_ERR_INVALID_ARG;
        if (!po) po = reinterpret_cast<float*>(workspace);
        if (!pl) pl = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(workspace) + up256(rows * ns * kDV * sizeof(float)));
    }
    SparseArgs a;
    a.q = (const unsigned short*)q16;
    a.qsb = q_strides3 ? (long)q_strides3[0] : (long)Hq * Sq * kD;
    a.qsh = q_strides3 ? (long)q_strides3[1] : (long)Sq * kD;
    a.qss = q_strides3 ? (long)q_strides3[2] : (long)kD;
    a.pool = (const unsigned char*)pool; a.table = block_table; a.tstride = (long)table_stride; a.scale = scale; a.seqused = seqused_k;
    a.indices = indices;
    a.isb = idx_strides2 ? (long)idx_strides2[0] : (long)Sq * topk;
    a.iss = idx_strides2 ? (long)idx_strides2[1] : (long)topk;
    a.out = out; a.lse = lse; a.po = po; a.plse = pl; a.scale_q = scale_q; a.q8 = (unsigned char*)q8;
    a.B = B; a.Hq = Hq; a.Sq = Sq; a.topk = topk; a.ns = ns; a.ht = ht; a.causal = is_causal ? 1 : 0; a.out_fmt = in_fmt;
    a.num_pages = num_pages; a.page_size = page_size; a.capacity = (int)capacity;
    a.c0 = sm_scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(B * ns * Sq * ht);
    int rc;
    if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E4M3) rc = fpv_launch(mla_sparse_sweep_kernel<QATTN_FMT_E4M3, QATTN_FMT_BF16>, grid, kSparseLds, st, a);
    else if (in_fmt == QATTN_FMT_BF16) rc = fpv_launch(mla_sparse_sweep_kernel<QATTN_FMT_E5M2, QATTN_FMT_BF16>, grid, kSparseLds, st, a);
    else if (fp8_fmt == QATTN_FMT_E4M3) rc = fpv_launch(mla_sparse_sweep_kernel<QATTN_FMT_E4M3, QATTN_FMT_FP16>, grid, kSparseLds, st, a);
    else rc = fpv_launch(mla_sparse_sweep_kernel<QATTN_FMT_E5M2, QATTN_FMT_FP16>, grid, kSparseLds, st, a);
    if (rc != QATTN_OK) return rc;
    if (ns > 1) hipLaunchKernelGGL(mla_sparse_combine_kernel, dim3((unsigned)rows), dim3(128), 0, st, po, pl, out, lse, (long)rows, ns, in_fmt);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

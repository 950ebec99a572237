// qattn_mla_sparse_prefill_fp8.hip -- qattn_fp8_mla_paged_sparse_varlen_forward (include/qattn_mla_sparse_prefill.h): sparse absorbed
// multi-head latent attention for PACKED variable-length queries on the row-major paged FP8 latent cache, gfx950.
//
// WORK ITEM  (packed token t, 128-row tile of the token's Hq heads), 8 waves, no key splits.  Slot b of t: a binary search on cu_seqlens_q.
// LIVE SET   a prologue scans the token's list once (wave w: the groups w, w + 8, ...) and ORs one bit per group with a valid entry into 64
//            LDS words; lane l of every wave then keeps word l in a register, and the next live group is a v_readlane and a ctz.
// RESOLVE    in registers, as a pipeline over the LIVE groups: a lane needs only the entries 64 g + ql and 64 g + 32 + ql of a group.  While
//            group g is swept, the index entries of the live group after next are in flight, the (clamped) table entries of the next one
//            are in flight, and its physical rows are formed right before its gather is issued.  A group's valid mask is two ballots.
// GATHER     section 4.31's mapping (per-lane sources, lane-linear LDS destination, an invalid entry reads row 0 of the pool) into ONE ring
//            slot: the gather of the next live group is issued right after the barrier that ends the transposition, and runs under the
//            softmax and phase B.  Every LDS access between that point and the next loop head is raw asm: in front of an LDS access of its
//            own the compiler would wait for the gather (it cannot tell the access from the LDS-DMA's destination).
// SWEEP      the arithmetic of every (row, key) and (row, channel) is csrc/qattn_mla_sparse_fp8.hip's, operation for operation, copied:
//            phase A  wave (rq = w & 3, kh = w >> 2): 32 keys x 32 rows of S^T, nine MFMAs; the maxima of the key halves meet through LDS;
//            phase B  wave w: the value channels [64 w, 64 w + 64) of all 128 rows, o[4 row blocks][2 tiles]; the two V^T fragments of a
//                     group are read once and stay in registers across the row blocks.
//            A row block wholly at or above Hq skips its MFMAs and exponentials and keeps the barriers.
// LDS (bytes)  ring 36 864 | V^T 32 768 | P 16 384 | Q^T 73 728 | maxima 1 024 | factors 512 | sums 1 024 | final maxima 512 | live 256
//            = 163 072.
#include "qattn_fp8pv_sweep.h"
#include "../../include/qattn_mla_sparse_prefill.h"

using namespace qattn;

namespace {

constexpr int kD = QATTN_MLA_D, kDV = QATTN_MLA_D_LATENT, kKS = kD / 64, kCH = 64 * kD;
constexpr int kRows = QATTN_MLA_SPARSE_PREFILL_ROWS, kWaves = 8, kBlocks = kRows / 32;
constexpr int kLiveWords = QATTN_MLA_SPARSE_MAX_TOPK / 64 / 32;
constexpr int kOffVT = kCH, kOffP = kOffVT + 64 * kDV, kOffQ = kOffP + 2 * kBlocks * 2048, kOffMx = kOffQ + kRows * kD,
              kOffAl = kOffMx + kBlocks * 2 * 32 * 4, kOffLs = kOffAl + kBlocks * 32 * 4, kOffMf = kOffLs + kBlocks * 2 * 32 * 4,
              kOffLive = kOffMf + kBlocks * 32 * 4, kPrefillLds = kOffLive + 4 * kLiveWords;
static_assert(kPrefillLds <= 160 * 1024, "one ring slot, V^T, P, the Q^T fragments of 128 rows and the exchange words fit a CU's LDS");
static_assert(kLiveWords == 64, "the live-group set is one 32-bit word per lane of a wave");
static_assert(kBlocks == 4 && kCH % 1024 == 0, "four 32-row blocks; the ring image is whole 1 KiB pieces");
constexpr float kMlaStart = -1.0e20f;   // below any raw score (|q8 . k8| <= 576 x 448 x 57344)

struct PrefillArgs {
    const unsigned short* q;
    long qst, qsh;        // element strides of q: token, head
    const unsigned char* pool;
    const int* table;
    long tstride;
    const float* scale;
    const int* seqused;
    const int* indices;
    long ist;             // element stride of a token's list
    const int* cu;
    void* out;
    float *lse, *scale_q;
    unsigned char* q8;
    int B, total, Hq, topk, ht, causal, out_fmt, num_pages, page_size, capacity;
    float c0;   // sm_scale log2(e)
};

__device__ __forceinline__ int pf_clampi(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }

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

// ---- LDS accesses the compiler does not see (used while a gather is in flight; each read waits for its own data)
__device__ __forceinline__ float lds_read_f32_raw(const void* p) {
    float v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(lds_addr(p)) : "memory");
    return v;
}
__device__ __forceinline__ void lds_write_f32_raw(void* p, float v) { asm volatile("ds_write_b32 %0, %1" ::"v"(lds_addr(p)), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_write16_raw(void* p, v4i v) { asm volatile("ds_write_b128 %0, %1" ::"v"(lds_addr(p)), "v"(v) : "memory"); }
__device__ __forceinline__ v8i join8(const v4i& lo, const v4i& hi) { return v8i{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}; }
// the fragments at p and p + gap (pieces [half = 0] and [half = 1] of each are 512 bytes apart, as lds_read_frag reads them)
template <int GAP>
__device__ __forceinline__ void lds_read_2frags_raw(const unsigned char* p, v8i& x, v8i& y) {
    v4i a, b, c, d;
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:512\n\tds_read_b128 %2, %4 offset:%5\n\tds_read_b128 %3, %4 offset:%6\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d)
                 : "v"(lds_addr(p)), "n"(GAP), "n"(GAP + 512)
                 : "memory");
    x = join8(a, b);
    y = join8(c, d);
}

// the smallest live group >= from, or -1; livev: lane l holds the bits of the groups 32 l .. 32 l + 31 (all arguments wave-uniform)
__device__ __forceinline__ int next_live(unsigned livev, int from, int ngr) {
    const int words = (ngr + 31) >> 5;
    for (int wi = from >> 5; wi < words; wi++) {
        unsigned w = (unsigned)__builtin_amdgcn_readlane((int)livev, wi);
        if (wi == (from >> 5)) w &= ~0u << (from & 31);
        if (w) return wi * 32 + __builtin_ctz(w);
    }
    return -1;
}

// grid = total_q ht, block = 512.  blockIdx.x = t ht + head tile.  amdgpu_waves_per_eu(2, 2): two waves per SIMD, at most 256 registers each.
template <int FMT, int IN_FMT>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void mla_sparse_prefill_kernel(const PrefillArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hh = lane >> 5, rq = wave & 3, kh = wave >> 2;
    const int t = (int)(blockIdx.x / (unsigned)a.ht), htile = (int)(blockIdx.x % (unsigned)a.ht);
    const int nrows = min(kRows, a.Hq - htile * kRows), nblk = (nrows + 31) >> 5;   // this tile's heads; its live 32-row blocks

    // ---- token -> (slot b, position i): the largest b in 0 .. B with cu[b] <= t; b = B (or a token behind its slot's end) is padding
    int b = 0;
    {
        int hi = a.B;
        while (b < hi) {   // (workgroup-uniform)
            const int mid = (b + hi + 1) >> 1;
            if (pf_clampi(__builtin_amdgcn_readfirstlane(a.cu[mid]), 0, a.total) <= t) b = mid;
            else hi = mid - 1;
        }
    }
    const int start = pf_clampi(__builtin_amdgcn_readfirstlane(a.cu[b]), 0, a.total);
    const int end = b == a.B ? start : pf_clampi(__builtin_amdgcn_readfirstlane(a.cu[b + 1]), start, a.total);
    if (t >= end) {   // a padded token: neither q nor its list is read; zero rows, LSE -inf, q8 / scale_q zero
        const long row0 = (long)t * a.Hq + htile * kRows;
        for (int u = tid; u < nrows * (kDV / 8); u += 512)
            *reinterpret_cast<v4i*>(reinterpret_cast<unsigned char*>(a.out) + (row0 + u / (kDV / 8)) * (kDV * 2) + (u % (kDV / 8)) * 16) = v4i{0, 0, 0, 0};
        if (a.q8)
            for (int u = tid; u < nrows * (kD / 16); u += 512)
                *reinterpret_cast<v4i*>(a.q8 + (row0 + u / (kD / 16)) * kD + (u % (kD / 16)) * 16) = v4i{0, 0, 0, 0};
        if (tid < nrows) {
            if (a.lse) a.lse[(long)(htile * kRows + tid) * a.total + t] = -INFINITY;
            if (a.scale_q) a.scale_q[row0 + tid] = 0.0f;
        }
        return;
    }
    const int pos = t - start, n_b = end - start;
    int L = a.seqused[b];
    L = L < 0 ? 0 : L > a.capacity ? a.capacity : L;
    int kend = a.causal ? L - n_b + pos + 1 : L;   // the positions [0, kend) are valid for this token's rows
    kend = kend < 0 ? 0 : kend;
    const int ngr = (a.topk + 63) >> 6;
    const int* irow = a.indices + (long)t * a.ist;
    const int* trow = a.table + (long)b * a.tstride;

    // ---- the live set: one bit per group with a valid entry (validity needs the list and kend only)
    unsigned* livew = reinterpret_cast<unsigned*>(smem + kOffLive);
    if (tid < kLiveWords) livew[tid] = 0u;
    lds_barrier();
    if (kend > 0)
        for (int g0 = wave; g0 < ngr; g0 += 4 * kWaves) {   // (wave-uniform) four groups of this wave in flight
            int j[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int g = g0 + kWaves * k, e = g * 64 + lane;
                j[k] = (g < ngr && e < a.topk) ? irow[e] : -1;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int g = g0 + kWaves * k;
                if (__ballot(j[k] >= 0 && j[k] < kend) != 0ull && lane == 0) atomicOr(&livew[g >> 5], 1u << (g & 31));
            }
        }

    // ---- this lane's query row: token-wise scale from the row's abs-max, e4m3 Q^T fragments parked in LDS
    const bool blk_live = rq < nblk;   // (wave-uniform)
    const int h = htile * kRows + rq * 32 + ql;
    const bool qvalid = h < a.Hq;
    const long R = (long)t * a.Hq + (qvalid ? h : 0);   // the row of [total_q, Hq]
    const int flo = (hh << 10) + (ql << 4);
    const unsigned char* qpark = smem + kOffQ + ((rq * kKS) << 11) + flo;   // [rq][s:9][hh][half][q:32][16 B]: the B operands of phase A
    float scale_q = 1.0f;
    if (blk_live) {
        const uint4* qrow = reinterpret_cast<const uint4*>(a.q + (long)t * a.qst + (long)(qvalid ? h : 0) * a.qsh) + 4 * hh;
        unsigned am = 0u;
#pragma unroll
        for (int s = 0; s < kKS; s++)
#pragma unroll
            for (int i = 0; i < 4; i++) am = amax_bits16<IN_FMT>(qrow[8 * s + i], am);
        {
            const auto sw = __builtin_amdgcn_permlane32_swap(am, am, false, false);
            am = max(sw[0], sw[1]);
        }
        scale_q = load16f<IN_FMT>((unsigned short)am) / 448.0f;
        if (!(scale_q >= 1.1920928955078125e-07f)) scale_q = 1.1920928955078125e-07f;
        const float rinv = 1.0f / scale_q;
        if (kh == 0) {   // (the two waves of a row block would park the same bytes)
            const bool q8_out = qvalid && a.q8;
            unsigned char* qo = a.q8 + R * kD + 32 * hh;
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
            if (qvalid && a.scale_q && hh == 0) a.scale_q[R] = scale_q;
        }
    }
    lds_barrier();
    const unsigned livev = livew[lane];
    const float scale_kv = a.scale[b];
    const float c = a.c0 * scale_q * scale_kv;

    // ---- the resolve pipeline: index entries -> (validity, table entries) -> physical rows, two entries per lane and group
    auto load_idx = [&](int g, int& ja, int& jb) {
        const int e = g * 64 + ql;
        ja = e < a.topk ? irow[e] : -1;
        jb = e + 32 < a.topk ? irow[e + 32] : -1;
    };
    // j -> its position inside the page (-1: invalid); returns the table entry (0 for an invalid entry, whose load is not made)
    auto load_page = [&](int& j) {
        int page = 0;
        if (j >= 0 && j < kend) {   // j < kend <= capacity: an entry of the table's row
            const int pi = j / a.page_size;
            page = trow[pi];
            j -= pi * a.page_size;
        } else {
            j = -1;
        }
        return page;
    };
    // the gather: the ring image is 36 pieces of 1 KiB; wave w fills the pieces w, w + 8, ...; piece (t, s, hh), lane (half, key)
    auto dma_rows = [&](int rem0, int page0, int rem1, int page1) {
        page0 = page0 < 0 ? 0 : page0 > a.num_pages - 1 ? a.num_pages - 1 : page0;
        page1 = page1 < 0 ? 0 : page1 > a.num_pages - 1 ? a.num_pages - 1 : page1;
        const int r0 = rem0 < 0 ? 0 : page0 * a.page_size + rem0, r1 = rem1 < 0 ? 0 : page1 * a.page_size + rem1;   // <= num_pages page_size - 1
        const unsigned char* s0 = a.pool + (size_t)r0 * kD + 16 * hh;
        const unsigned char* s1 = a.pool + (size_t)r1 * kD + 16 * hh;
#pragma unroll
        for (int r = 0; r < (kCH / 1024 + kWaves - 1) / kWaves; r++) {
            const int blk = wave + kWaves * r, ts = blk >> 1;   // ts = 9 t + s
            if (blk < kCH / 1024) {   // (wave-uniform)
                const unsigned char* src = (ts >= kKS ? s1 + 64 * (ts - kKS) : s0 + 64 * ts) + 32 * (blk & 1);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(smem + (blk << 10)), 16, 0, 0);
            }
        }
    };
    int g = next_live(livev, 0, ngr), g1 = -1, g2 = -1;
    int j1a = -1, j1b = -1, p1a = 0, p1b = 0, j2a = -1, j2b = -1;
    unsigned mlo = 0u, mhi = 0u;   // the valid mask of group g
    if (g >= 0) {
        int ja, jb;
        load_idx(g, ja, jb);
        g1 = next_live(livev, g + 1, ngr);
        if (g1 >= 0) {
            load_idx(g1, j1a, j1b);
            g2 = next_live(livev, g1 + 1, ngr);
            if (g2 >= 0) load_idx(g2, j2a, j2b);
        }
        const int pa = load_page(ja), pb = load_page(jb);
        if (g1 >= 0) { p1a = load_page(j1a); p1b = load_page(j1b); }
        mlo = (unsigned)__ballot(ja >= 0);
        mhi = (unsigned)__ballot(jb >= 0);
        dma_rows(ja, pa, jb, pb);
    }

    v16f o[kBlocks][2];
#pragma unroll
    for (int r2 = 0; r2 < kBlocks; r2++)
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int r = 0; r < 16; r++) o[r2][m][r] = 0.0f;
    float m_run = kMlaStart, lim = kMlaStart, l_run = 0.0f;

    float* xm = reinterpret_cast<float*>(smem + kOffMx);   // [rq][kh][32]
    float* al = reinterpret_cast<float*>(smem + kOffAl);   // [rq][32]
    unsigned char* pw = smem + kOffP + rq * 2048 + (hh << 10) + (kh << 9) + (ql << 4);   // this lane's 16 bytes of P^T: [term][rq][hh][half][q]
    constexpr int kPTerm = kBlocks * 2048;

    while (g >= 0) {
        wait_vmcnt<0>();                  // this wave's pieces of the group have landed
        __builtin_amdgcn_s_barrier();     // ... and everyone's; every wave is done with phase B of the group before

        // ---- phase A: 32 keys x 32 rows of scores
        v16f s;
        float mx = -INFINITY;
        if (blk_live) {
#pragma unroll
            for (int r = 0; r < 16; r++) s[r] = 0.0f;
            {
                const unsigned char* kbuf = smem + ((kh * kKS) << 11) + flo;
#pragma unroll
                for (int sl = 0; sl < kKS; sl++) s = mfma_f8<FMT, QATTN_FMT_E4M3>(lds_read_frag(kbuf + (sl << 11)), lds_read_frag(qpark + (sl << 11)), s);
            }
            const unsigned mb = qvalid ? (kh ? mhi : mlo) >> (4 * hh) : 0u;   // register r: entry 32 kh + 4 hh + 8 (r >> 2) + (r & 3) of the group
#pragma unroll
            for (int r = 0; r < 16; r++) {
                if (((mb >> (8 * (r >> 2) + (r & 3))) & 1u) == 0u) s[r] = -INFINITY;
                mx = fmaxf(mx, s[r]);
            }
            {
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
                mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
            }
            if (hh == 0) xm[(rq * 2 + kh) * 32 + ql] = mx;
        }

        // ---- the group's first 512 channels, transposed into VFRAG order; a thread: 16 keys (one (half, hh) of the key index) x 4 channels
        {
            const int dq = tid & 3, khh = (tid >> 2) & 1, piece = (tid >> 3) & 31, half = kh;   // (half = tid >> 8)
            const int d0 = 16 * piece + 4 * dq;
            const unsigned char* src = smem + ((half * kKS + (d0 >> 6)) << 11) + (((d0 >> 5) & 1) << 10) + (((d0 >> 4) & 1) << 9) + (d0 & 15);
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
        lds_barrier();   // the ring slot is free

        // ---- the next live group's gather, and the pipeline one step on.  No compiler-visible LDS access from here to the loop head.
        // The pipeline's loads go FIRST: the vector-memory counter is in order, and a wait for a load issued behind the gather would wait
        // for the gather.
        const int gn = g1, na = j1a, npa = p1a, nb = j1b, npb = p1b;
        g1 = g2; j1a = j2a; j1b = j2b;
        g2 = -1;
        if (g1 >= 0) {   // (workgroup-uniform)
            p1a = load_page(j1a);
            p1b = load_page(j1b);
            g2 = next_live(livev, g1 + 1, ngr);
            if (g2 >= 0) load_idx(g2, j2a, j2b);
        }
        unsigned nlo = 0u, nhi = 0u;
        if (gn >= 0) {
            nlo = (unsigned)__ballot(na >= 0);
            nhi = (unsigned)__ballot(nb >= 0);
            dma_rows(na, npa, nb, npb);
        }

        // ---- the row maxima of both key halves; rescale only when a row's maximum outgrew the headroom of the shifted exponent
        if (blk_live) {
            mx = fmaxf(mx, lds_read_f32_raw(&xm[(rq * 2 + (kh ^ 1)) * 32 + ql]));
            float alpha = 1.0f;
            if (__any(mx > lim) != 0) {   // (the same vote in both waves of a row block: same maxima, same history)
                const float m_new = fmaxf(m_run, mx);
                alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
                l_run *= alpha;
                m_run = m_new;
                lim = m_new + kRescaleThr / c;
            }
            if (kh == 0 && hh == 0) lds_write_f32_raw(&al[rq * 32 + ql], alpha);
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
            lds_write16_raw(pw, ph);
            lds_write16_raw(pw + kPTerm, pl);
        }
        lds_barrier();

        // ---- phase B: this wave's 64 value channels of all 128 rows.  The rescale votes are per 64 rows, as in the 64-row kernel.
        {
            float av[kBlocks];
#pragma unroll
            for (int r2 = 0; r2 < kBlocks; r2++) av[r2] = r2 < nblk ? lds_read_f32_raw(&al[r2 * 32 + ql]) : 1.0f;
#pragma unroll
            for (int p2 = 0; p2 < kBlocks; p2 += 2)
                if (__any(av[p2] != 1.0f || av[p2 + 1] != 1.0f) != 0) {
#pragma unroll
                    for (int m = 0; m < 2; m++)
#pragma unroll
                        for (int r = 0; r < 16; r++) { o[p2][m][r] *= av[p2]; o[p2 + 1][m][r] *= av[p2 + 1]; }
                }
        }
        v8i vf[2];
        lds_read_2frags_raw<2048>(smem + kOffVT + ((2 * wave) << 11) + flo, vf[0], vf[1]);
#pragma unroll
        for (int r2 = 0; r2 < kBlocks; r2++) {
            if (r2 < nblk) {   // (workgroup-uniform)
                v8i ph, pl;
                lds_read_2frags_raw<kPTerm>(smem + kOffP + r2 * 2048 + flo, ph, pl);
#pragma unroll
                for (int m = 0; m < 2; m++) {
                    o[r2][m] = mfma_f8<FMT, QATTN_FMT_E4M3>(vf[m], ph, o[r2][m]);
                    o[r2][m] = mfma_pv_lo<FMT, QATTN_FMT_E4M3>(vf[m], pl, o[r2][m], kScaleWordOne);
                }
            }
        }
        g = gn; mlo = nlo; mhi = nhi;
    }

    // ---- epilogue: the row sums of both key halves, the rows
    float* lsx = reinterpret_cast<float*>(smem + kOffLs);   // [rq][kh][32]
    float* mfx = reinterpret_cast<float*>(smem + kOffMf);   // [rq][32]
    {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
        l_run = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    if (blk_live && hh == 0) lsx[(rq * 2 + kh) * 32 + ql] = l_run;
    if (blk_live && kh == 0 && hh == 0) mfx[rq * 32 + ql] = m_run;
    lds_barrier();
#pragma unroll
    for (int r2 = 0; r2 < kBlocks; r2++) {
        if (r2 < nblk) {
            const float l_tot = lsx[(r2 * 2) * 32 + ql] + lsx[(r2 * 2 + 1) * 32 + ql];
            const float inv = l_tot > 0.0f ? scale_kv / l_tot : 0.0f;
            const int ho = htile * kRows + r2 * 32 + ql;
            const bool valid = ho < a.Hq;
            store_o_rows<2>(a.out, a.out_fmt, o[r2], inv, (((long)t * a.Hq + (valid ? ho : 0)) * kDV + 64 * wave) * 2, hh, valid);
        }
    }
    if (blk_live && kh == 0 && hh == 0 && qvalid && a.lse) {
        const float l_tot = lsx[(rq * 2) * 32 + ql] + lsx[(rq * 2 + 1) * 32 + ql];
        a.lse[(long)h * a.total + t] = l_tot > 0.0f ? 0.6931471805599453f * (mfx[rq * 32 + ql] * c - kPShift) + __logf(l_tot) : -INFINITY;
    }
}

template <typename... KArgs>
int launch512(void (*kern)(KArgs...), unsigned grid, hipStream_t st, const PrefillArgs& a) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kPrefillLds) != hipSuccess) return QATTN_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kWaves * 64), kPrefillLds, st, a);
    return QATTN_OK;
}

}  // namespace

extern "C" int qattn_fp8_mla_paged_sparse_varlen_forward(const void* q16, int in_fmt, const long long* q_strides2, const void* pool,
                                                         const int* block_table, long long table_stride, int num_pages, int page_size,
                                                         int max_pages, const float* scale, const int* indices, long long idx_stride, int topk,
                                                         const int* cu_seqlens_q, void* out, float* lse, const int* seqused_k, int B,
                                                         int total_q, int Hq, int fp8_fmt, int is_causal, float sm_scale, void* q8,
                                                         float* scale_q, void* stream) {
    if (!q16 || !pool || !block_table || !scale || !indices || !cu_seqlens_q || !out || !seqused_k) return QATTN_ERR_INVALID_ARG;
    if (((size_t)block_table | (size_t)indices | (size_t)cu_seqlens_q) % 4 != 0 || ((size_t)pool | (size_t)q16 | (size_t)out | (size_t)q8) % 16 != 0)
        return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || total_q <= 0 || Hq <= 0 || Hq > (1 << 20) || topk <= 0 || topk > QATTN_MLA_SPARSE_MAX_TOPK) return QATTN_ERR_INVALID_ARG;
    if (num_pages <= 0 || max_pages <= 0 || page_size <= 0 || table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    if ((long long)num_pages * page_size > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (a physical row number is an int)
    const long long capacity = (long long)max_pages * page_size;
    if (capacity > 0x7fffffffLL - 64) return QATTN_ERR_INVALID_ARG;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (!(sm_scale > 0.0f) || !(sm_scale < INFINITY)) return QATTN_ERR_INVALID_ARG;
    if (q_strides2)
        for (int i = 0; i < 2; i++)
            if (q_strides2[i] < 0 || q_strides2[i] % 8 != 0) return QATTN_ERR_INVALID_ARG;
    if (idx_stride < 0) return QATTN_ERR_INVALID_ARG;
    const int ht = (Hq + kRows - 1) / kRows;
    if ((long long)total_q * ht > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;
    PrefillArgs a;
    a.q = (const unsigned short*)q16;
    a.qst = q_strides2 ? (long)q_strides2[0] : (long)Hq * kD;
    a.qsh = q_strides2 ? (long)q_strides2[1] : (long)kD;
    a.pool = (const unsigned char*)pool; a.table = block_table; a.tstride = (long)table_stride; a.scale = scale; a.seqused = seqused_k;
    a.indices = indices; a.ist = (long)idx_stride; a.cu = cu_seqlens_q;
    a.out = out; a.lse = lse; a.scale_q = scale_q; a.q8 = (unsigned char*)q8;
    a.B = B; a.total = total_q; a.Hq = Hq; a.topk = topk; a.ht = ht; a.causal = is_causal ? 1 : 0; a.out_fmt = in_fmt;
    a.num_pages = num_pages; a.page_size = page_size; a.capacity = (int)capacity;
    a.c0 = sm_scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(total_q * ht);
    int rc;
    if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E4M3) rc = launch512(mla_sparse_prefill_kernel<QATTN_FMT_E4M3, QATTN_FMT_BF16>, grid, st, a);
    else if (in_fmt == QATTN_FMT_BF16) rc = launch512(mla_sparse_prefill_kernel<QATTN_FMT_E5M2, QATTN_FMT_BF16>, grid, st, a);
    else if (fp8_fmt == QATTN_FMT_E4M3) rc = launch512(mla_sparse_prefill_kernel<QATTN_FMT_E4M3, QATTN_FMT_FP16>, grid, st, a);
    else rc = launch512(mla_sparse_prefill_kernel<QATTN_FMT_E5M2, QATTN_FMT_FP16>, grid, st, a);
    if (rc != QATTN_OK) return rc;
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

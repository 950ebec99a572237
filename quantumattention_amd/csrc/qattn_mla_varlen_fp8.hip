// qattn_mla_varlen_fp8.hip -- qattn_fp8_mla_paged_varlen_forward (include/qattn_mla_varlen.h): absorbed multi-head latent attention for PACKED
// variable-length queries over the one-image paged FP8 latent cache, gfx950.
//
// WORK ITEM  (tile slot, key split), 8 waves; a tile is 128 rows of ONE slot.  Inside slot b (n_b tokens) row R = h n_b + i, head-major: the
//            dense kernel's h = R / Sq, pos = R % Sq with Sq = n_b, so a 32-row block R / 32 holds the rows it holds in
//            qattn_fp8_mla_paged_forward called on the slot alone -- the rescale vote is per block, and with it every bit of a row.
// TILE MAP   slot b's tiles start at tile slot floor(cu[b] Hq / 128) + b; the slot of a tile slot is a binary search on cu_seqlens_q.  The
//            rows behind cu[B] (a padded bucket) form a last pseudo-slot whose tiles only store zeros.  A tile slot without rows exits.
// CHUNKS     the dense kernel's linear LDS-DMA through the clamped block table, spread over 8 waves, into ONE ring slot: the next chunk's
//            copy is issued right after the barrier that ends the transposition and runs under the softmax and phase B.  Every LDS access
//            between that point and the next loop head is raw asm: in front of an LDS access of its own the compiler would wait for the
//            copy (it cannot tell the access from the LDS-DMA's destination).
// SWEEP      the arithmetic of every (row, key) and (row, channel) is csrc/qattn_mla_splitkv_fp8.hip's, operation for operation, copied:
//            phase A  wave (rq = w & 3, kh = w >> 2): 32 keys x 32 rows of S^T, nine MFMAs; the maxima of the key halves meet through LDS;
//            phase B  wave w: the value channels [64 w, 64 w + 64) of all 128 rows, o[4 row blocks][2 tiles]; the two V^T fragments of a
//                     chunk are read once and stay in registers across the row blocks.
//            A row block wholly behind the slot's rows skips its MFMAs and exponentials and keeps the barriers.  Under a causal mask a tile
//            stops at the last chunk one of its rows attends: a chunk masked for a whole block adds exp2(-inf) = 0 and casts no vote.
// LDS (bytes)  ring 36 864 | V^T 32 768 | P 16 384 | Q^T 73 728 | maxima 1 024 | factors 512 | sums 1 024 | final maxima 512 = 162 816.
#include "qattn_fp8pv_sweep.h"
#include "../../include/qattn_mla_varlen.h"

using namespace qattn;

namespace {

constexpr int kD = QATTN_MLA_D, kDV = QATTN_MLA_D_LATENT, kKS = kD / 64, kCH = 64 * kD;
constexpr int kRows = QATTN_MLA_VARLEN_ROWS, kWaves = 8, kBlocks = kRows / 32;
constexpr int kOffVT = kCH, kOffP = kOffVT + 64 * kDV, kOffQ = kOffP + 2 * kBlocks * 2048, kOffMx = kOffQ + kRows * kD,
              kOffAl = kOffMx + kBlocks * 2 * 32 * 4, kOffLs = kOffAl + kBlocks * 32 * 4, kOffMf = kOffLs + kBlocks * 2 * 32 * 4,
              kVarlenLds = kOffMf + kBlocks * 32 * 4;
static_assert(kVarlenLds <= 160 * 1024, "one ring slot, V^T, P, the Q^T fragments of 128 rows and the exchange words fit a CU's LDS");
static_assert(kBlocks == 4 && kCH % 1024 == 0, "four 32-row blocks; the ring image is whole 1 KiB pieces");
constexpr float kMlaStart = -1.0e20f;   // below any raw score (|q8 . k8| <= 576 x 448 x 57344)

struct VarlenArgs {
    const unsigned short* q;
    long qst, qsh;        // element strides of q: token, head
    const unsigned char* pool;
    const int* table;
    long tstride;
    const float* scale;
    const int* seqused;
    const int* cu;
    void* out;
    float *lse, *po, *plse, *scale_q;
    unsigned char* q8;
    long rows;            // total_q Hq: the rows of a split's slab of the partials
    int B, total, Hq, Skv, ns, slots, causal, out_fmt, num_pages, pc;
    float c0;   // sm_scale log2(e)
};

__device__ __forceinline__ int vl_clampi(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }

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

// ---- LDS accesses the compiler does not see (used while a chunk's copy is in flight; each read waits for its own data)
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

// grid = slots ns, block = 512.  blockIdx.x = split slots + tile slot: the tiles of a (slot, split) sweep the same chunks side by side.
// amdgpu_waves_per_eu(2, 2): two waves per SIMD, at most 256 registers each.
template <int FMT, int IN_FMT>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void mla_varlen_sweep_kernel(const VarlenArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hh = lane >> 5, rq = wave & 3, kh = wave >> 2;
    const int ts = (int)(blockIdx.x % (unsigned)a.slots), split = (int)(blockIdx.x / (unsigned)a.slots);

    // ---- tile slot -> (slot b, tile): the largest b in 0 .. B whose first tile slot floor(cu[b] Hq / 128) + b is <= ts; b = B is the padding
    auto cu_at = [&](int i) { return vl_clampi(__builtin_amdgcn_readfirstlane(a.cu[i]), 0, a.total); };
    int b = 0;
    {
        int hi = a.B;
        while (b < hi) {   // (workgroup-uniform)
            const int mid = (b + hi + 1) >> 1;
            if ((long)cu_at(mid) * a.Hq / kRows + mid <= ts) b = mid;
            else hi = mid - 1;
        }
    }
    const int start = cu_at(b);
    const long tile0 = ts - ((long)start * a.Hq / kRows + b);   // (negative only where cu[0] > 0: rows no slot owns)
    if (tile0 < 0) return;
    if (b == a.B) {   // a padded bucket: q is not read; zero rows, LSE -inf, q8 / scale_q zero, and the same in every split's partials
        const long row0 = (long)start * a.Hq + tile0 * kRows;
        const int nrows = (int)min((long)kRows, a.rows - row0);
        if (nrows <= 0) return;
        if (a.ns == 1) {
            for (int u = tid; u < nrows * (kDV / 8); u += 512)
                *reinterpret_cast<v4i*>(reinterpret_cast<unsigned char*>(a.out) + (row0 + u / (kDV / 8)) * (kDV * 2) + (u % (kDV / 8)) * 16) = v4i{0, 0, 0, 0};
            if (tid < nrows && a.lse) a.lse[((row0 + tid) % a.Hq) * a.total + (row0 + tid) / a.Hq] = -INFINITY;
        } else {
            for (int u = tid; u < nrows * (kDV / 4); u += 512)
                *reinterpret_cast<v4i*>(a.po + (split * a.rows + row0 + u / (kDV / 4)) * kDV + (u % (kDV / 4)) * 4) = v4i{0, 0, 0, 0};
            if (tid < nrows) a.plse[split * a.rows + row0 + tid] = -INFINITY;
        }
        if (split == 0) {
            if (a.q8)
                for (int u = tid; u < nrows * (kD / 16); u += 512)
                    *reinterpret_cast<v4i*>(a.q8 + (row0 + u / (kD / 16)) * kD + (u % (kD / 16)) * 16) = v4i{0, 0, 0, 0};
            if (tid < nrows && a.scale_q) a.scale_q[row0 + tid] = 0.0f;
        }
        return;
    }
    const int n_b = vl_clampi(__builtin_amdgcn_readfirstlane(a.cu[b + 1]), start, a.total) - start;
    const int HS = a.Hq * n_b;   // (<= total_q Hq < 2^31, checked on the host)
    if (tile0 * kRows >= HS) return;
    const int R0 = (int)tile0 * kRows;
    const int nblk = (min(kRows, HS - R0) + 31) >> 5;   // this tile's live 32-row blocks

    int L = a.seqused[b];
    L = L < 0 ? 0 : L > a.Skv ? a.Skv : L;
    const int nch = (L + 63) >> 6, per = (nch + a.ns - 1) / a.ns;
    const int c_lo = split * per;
    int c_hi = min(nch, c_lo + per);
    if (a.causal) {   // the last key one of the tile's rows attends: its largest position is n_b - 1 once the tile reaches the next head
        const int R1 = min(R0 + kRows, HS) - 1;
        const int pmax = R1 / n_b > R0 / n_b ? n_b - 1 : R1 % n_b;
        const int kmax = L - n_b + pmax + 1;
        c_hi = min(c_hi, kmax <= 0 ? 0 : (kmax + 63) >> 6);
    }
    const int n = c_hi - c_lo;

    // ---- the chunk copy: the ring image is 36 pieces of 1 KiB; wave w copies the pieces w, w + 8, ...
    const unsigned lane16 = (unsigned)lane << 4;
    const int* trow = a.table + (long)b * a.tstride;
    auto load_page = [&](int chunk) { return trow[chunk / a.pc]; };   // chunk < ceil(L_b / 64): an entry below ceil(L_b / page_size)
    auto dma_chunk = [&](int chunk, int page) {
        page = __builtin_amdgcn_readfirstlane(page);
        page = page < 0 ? 0 : page > a.num_pages - 1 ? a.num_pages - 1 : page;
        const unsigned char* src = a.pool + ((size_t)page * a.pc + chunk % a.pc) * (size_t)kCH + lane16;
#pragma unroll
        for (int r = 0; r < (kCH / 1024 + kWaves - 1) / kWaves; r++) {
            const int piece = wave + kWaves * r;
            if (piece < kCH / 1024)   // (wave-uniform)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (piece << 10)),
                                                 (__attribute__((address_space(3))) void*)(smem + (piece << 10)), 16, 0, 0);
        }
    };
    if (n > 0) dma_chunk(c_lo, load_page(c_lo));

    // ---- this lane's query row: token-wise scale from the row's abs-max, e4m3 Q^T fragments parked in LDS
    const bool blk_live = rq < nblk;   // (wave-uniform)
    const int R = R0 + rq * 32 + ql;
    const bool qvalid = R < HS;
    const int h = qvalid ? R / n_b : 0, pos = qvalid ? R % n_b : 0;
    const long Rout = (long)(start + pos) * a.Hq + h;   // the row of [total_q, Hq]
    const int flo = (hh << 10) + (ql << 4);
    const unsigned char* qpark = smem + kOffQ + ((rq * kKS) << 11) + flo;   // [rq][s:9][hh][half][q:32][16 B]: the B operands of phase A
    float scale_q = 1.0f;
    if (blk_live) {
        const uint4* qrow = reinterpret_cast<const uint4*>(a.q + (long)(start + pos) * a.qst + (long)h * a.qsh) + 4 * hh;
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
            const bool q8_out = split == 0 && qvalid && a.q8;
            unsigned char* qo = a.q8 + Rout * kD + 32 * hh;
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
            if (split == 0 && qvalid && a.scale_q && hh == 0) a.scale_q[Rout] = scale_q;
        }
    }
    lds_barrier();
    const float scale_kv = a.scale[b];
    const float c = a.c0 * scale_q * scale_kv;
    int kend = a.causal ? L - n_b + pos + 1 : L;   // the keys [0, kend) are this row's
    kend = !qvalid || kend < 0 ? 0 : kend;

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

    for (int t = 0; t < n; t++) {
        const int chunk = c_lo + t;
        wait_vmcnt<0>();                  // this wave's pieces of the chunk have landed
        __builtin_amdgcn_s_barrier();     // ... and everyone's; every wave is done with phase B of the chunk before
        // the next chunk's table entry arrives under phase A, not in front of the copy.  Loaded and consumed on EVERY pass (the last one
        // re-reads its own entry): a load that one path leaves unconsumed makes the compiler wait for it -- and for the copy -- further down
        const int page_load = load_page(min(chunk + 1, c_hi - 1));

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
            const int key0 = chunk * 64 + 32 * kh + 4 * hh;   // register r: key key0 + 8 (r >> 2) + (r & 3)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                if (key0 + 8 * (r >> 2) + (r & 3) >= kend) s[r] = -INFINITY;
                mx = fmaxf(mx, s[r]);
            }
            {
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
                mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
            }
            if (hh == 0) xm[(rq * 2 + kh) * 32 + ql] = mx;
        }

        const int page_next = __builtin_amdgcn_readfirstlane(page_load);

        // ---- the chunk's first 512 channels, transposed into VFRAG order; a thread: 16 keys (one (half, hh) of the key index) x 4 channels
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
            if (chunk * 64 + 64 > L) {   // (workgroup-uniform) the chunk that holds key L_b: the value bytes at or behind it count as zero
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    const int nv = L - (chunk * 64 + 32 * half + 8 * w + 4 * khh);
                    const unsigned keep = nv >= 4 ? 0xffffffffu : nv <= 0 ? 0u : (1u << (8 * nv)) - 1u;
#pragma unroll
                    for (int j = 0; j < 4; j++) ov[w][j] &= keep;
                }
            }
            unsigned char* dst = smem + kOffVT + ((d0 >> 5) << 11) + (khh << 10) + (half << 9) + ((d0 & 31) << 4);
#pragma unroll
            for (int j = 0; j < 4; j++) *reinterpret_cast<v4i*>(dst + 16 * j) = v4i{(int)ov[0][j], (int)ov[1][j], (int)ov[2][j], (int)ov[3][j]};
        }
        lds_barrier();   // the ring slot is free

        // ---- the next chunk's copy.  No compiler-visible LDS access from here to the loop head.
        if (t + 1 < n) dma_chunk(chunk + 1, page_next);

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
    const long slab = split * a.rows;   // this split's rows of the partial buffers
#pragma unroll
    for (int r2 = 0; r2 < kBlocks; r2++) {
        if (r2 < nblk) {
            const float l_tot = lsx[(r2 * 2) * 32 + ql] + lsx[(r2 * 2 + 1) * 32 + ql];
            const float inv = l_tot > 0.0f ? scale_kv / l_tot : 0.0f;
            const int Ro = R0 + r2 * 32 + ql;
            const bool valid = Ro < HS;
            const long orow = valid ? (long)(start + Ro % n_b) * a.Hq + Ro / n_b : 0;
            if (a.ns == 1) {
                store_o_rows<2>(a.out, a.out_fmt, o[r2], inv, (orow * kDV + 64 * wave) * 2, hh, valid);
            } else if (valid) {
                float* dst = a.po + (slab + orow) * kDV + 64 * wave + 4 * hh;
#pragma unroll
                for (int m = 0; m < 2; m++)
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        *reinterpret_cast<float4*>(dst + 32 * m + 8 * j) =
                            make_float4(o[r2][m][4 * j] * inv, o[r2][m][4 * j + 1] * inv, o[r2][m][4 * j + 2] * inv, o[r2][m][4 * j + 3] * inv);
            }
        }
    }
    if (blk_live && kh == 0 && hh == 0 && qvalid) {
        const float l_tot = lsx[(rq * 2) * 32 + ql] + lsx[(rq * 2 + 1) * 32 + ql];
        const float v = l_tot > 0.0f ? 0.6931471805599453f * (mfx[rq * 32 + ql] * c - kPShift) + __logf(l_tot) : -INFINITY;
        if (a.ns == 1) { if (a.lse) a.lse[(long)h * a.total + start + pos] = v; }
        else a.plse[slab + Rout] = v;
    }
}

// One launch merges all ns partials of an output row (token Hq + h): grid = total_q Hq rows, block = 128, a thread owns 4 channels.
// mla_combine_kernel's arithmetic (csrc/qattn_mla_splitkv_fp8.hip), copied: L = log sum_i exp(lse_i), O = sum_i exp(lse_i - L) O_i in fp32 in
// the order of i, one rounding.  lse is written as [Hq, total_q]; a row behind cu[B] is a zero row with LSE -inf whatever its partials hold.
__global__ __launch_bounds__(128) void mla_varlen_combine_kernel(const float* po, const float* plse, void* out, float* lse, const int* cu, int B,
                                                                 int total, int Hq, long rows, int ns, int out_fmt) {
    const long row = blockIdx.x;
    const int token = (int)(row / Hq), h = (int)(row % Hq);
    const bool live = token < vl_clampi(cu[B], 0, total);
    float mx = -INFINITY;
    if (live)
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
    if (lse && threadIdx.x == 0) lse[(long)h * total + token] = Lr;
}

template <typename... KArgs>
int launch512(void (*kern)(KArgs...), unsigned grid, hipStream_t st, const VarlenArgs& a) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kVarlenLds) != hipSuccess) return QATTN_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kWaves * 64), kVarlenLds, st, a);
    return QATTN_OK;
}

long long varlen_tile_slots(int B, int total_q, int Hq) { return ((long long)total_q * Hq + kRows - 1) / kRows + B; }

}  // namespace

extern "C" int qattn_mla_varlen_auto_splits(int tile_slots, int Skv, int num_cus) {
    if (tile_slots <= 0 || Skv <= 0 || num_cus <= 0) return 1;
    int ns = num_cus / tile_slots;
    if (ns > Skv / 1024) ns = Skv / 1024;
    return ns < 1 ? 1 : ns > QATTN_MLA_MAX_SPLITS ? QATTN_MLA_MAX_SPLITS : ns;
}

extern "C" size_t qattn_fp8_mla_paged_varlen_workspace_bytes(int total_q, int Hq, int num_splits) {
    if (total_q <= 0 || Hq <= 0 || num_splits <= 1) return 0;
    const size_t rows = (size_t)num_splits * total_q * Hq;
    return up256(rows * kDV * sizeof(float)) + up256(rows * sizeof(float));
}

extern "C" int qattn_fp8_mla_paged_varlen_forward(const void* q16, int in_fmt, const long long* q_strides2, const void* pool,
                                                  const int* block_table, long long table_stride, int num_pages, int page_size, int max_pages,
                                                  const float* scale, const int* cu_seqlens_q, int max_seqlen_q, void* out, float* lse,
                                                  const int* seqused_k, int B, int total_q, int Hq, int Skv, int fp8_fmt, int is_causal,
                                                  float sm_scale, int num_splits, void* q8, float* scale_q, float* partial_o,
                                                  float* partial_lse, void* workspace, size_t workspace_bytes, void* stream) {
    if (!q16 || !pool || !block_table || !scale || !cu_seqlens_q || !out || !seqused_k) return QATTN_ERR_INVALID_ARG;
    if (((size_t)block_table | (size_t)cu_seqlens_q) % 4 != 0 || ((size_t)pool | (size_t)q16 | (size_t)out | (size_t)q8 | (size_t)workspace) % 16 != 0)
        return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || total_q <= 0 || Hq <= 0 || Hq > (1 << 20) || Skv <= 0 || max_seqlen_q <= 0 || max_seqlen_q > total_q) return QATTN_ERR_INVALID_ARG;
    if (num_pages <= 0 || max_pages <= 0 || page_size < 64 || page_size % 64 != 0 || table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    const int pc = page_size / 64;
    if ((long long)num_pages * pc > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;
    const long long capacity = (long long)max_pages * page_size;
    if (capacity > 0x7fffffffLL - 64 || Skv > capacity) return QATTN_ERR_INVALID_ARG;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (!(sm_scale > 0.0f) || !(sm_scale < INFINITY)) return QATTN_ERR_INVALID_ARG;
    if (num_splits < 0 || num_splits > QATTN_MLA_MAX_SPLITS) return QATTN_ERR_INVALID_ARG;
    if (q_strides2)
        for (int i = 0; i < 2; i++)
            if (q_strides2[i] < 0 || q_strides2[i] % 8 != 0) return QATTN_ERR_INVALID_ARG;
    const long long rows = (long long)total_q * Hq;
    if (rows + (long long)kRows * (B + 1LL) > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (row numbers are ints; the combine: one block per row)
    const long long slots = varlen_tile_slots(B, total_q, Hq);
    const int ns = num_splits ? num_splits : qattn_mla_varlen_auto_splits((int)slots, Skv, cu_count());
    if (slots * ns > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;
    float *po = partial_o, *pl = partial_lse;
    if (ns > 1 && (!po || !pl)) {
        if (!workspace || workspace_bytes < qattn_fp8_mla_paged_varlen_workspace_bytes(total_q, Hq, ns)) return QATTN_ERR_INVALID_ARG;
        if (!po) po = reinterpret_cast<float*>(workspace);
        if (!pl) pl = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(workspace) + up256((size_t)rows * ns * kDV * sizeof(float)));
    }
    VarlenArgs a;
    a.q = (const unsigned short*)q16;
    a.qst = q_strides2 ? (long)q_strides2[0] : (long)Hq * kD;
    a.qsh = q_strides2 ? (long)q_strides2[1] : (long)kD;
    a.pool = (const unsigned char*)pool; a.table = block_table; a.tstride = (long)table_stride; a.scale = scale; a.seqused = seqused_k;
    a.cu = cu_seqlens_q;
    a.out = out; a.lse = lse; a.po = po; a.plse = pl; a.scale_q = scale_q; a.q8 = (unsigned char*)q8;
    a.rows = (long)rows;
    a.B = B; a.total = total_q; a.Hq = Hq; a.Skv = Skv; a.ns = ns; a.slots = (int)slots; a.causal = is_causal ? 1 : 0; a.out_fmt = in_fmt;
    a.num_pages = num_pages; a.pc = pc;
    a.c0 = sm_scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(slots * ns);
    int rc;
    if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E4M3) rc = launch512(mla_varlen_sweep_kernel<QATTN_FMT_E4M3, QATTN_FMT_BF16>, grid, st, a);
    else if (in_fmt == QATTN_FMT_BF16) rc = launch512(mla_varlen_sweep_kernel<QATTN_FMT_E5M2, QATTN_FMT_BF16>, grid, st, a);
    else if (fp8_fmt == QATTN_FMT_E4M3) rc = launch512(mla_varlen_sweep_kernel<QATTN_FMT_E4M3, QATTN_FMT_FP16>, grid, st, a);
    else rc = launch512(mla_varlen_sweep_kernel<QATTN_FMT_E5M2, QATTN_FMT_FP16>, grid, st, a);
    if (rc != QATTN_OK) return rc;
    if (ns > 1)
        hipLaunchKernelGGL(mla_varlen_combine_kernel, dim3((unsigned)rows), dim3(128), 0, st, po, pl, out, lse, cu_seqlens_q, B, total_q, Hq,
                           (long)rows, ns, in_fmt);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

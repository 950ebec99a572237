// qattn_mla_splitkv_fp8.hip -- qattn_fp8_mla_paged_forward (include/qattn_mla.h): absorbed multi-head latent attention over the one-image
// paged FP8 latent cache, gfx950.  A kernel of its own shape, not a switch of qattn_splitkv_body.h: scores are
// 576-channel products, values the first 512 channels of the SAME bytes, and all Hq heads of a slot share them.
//
// WORK ITEM  (slot b, 64-row tile of the slot's Hq Sq (head, position) rows, key split), 4 waves.  O for 32 rows x 512 channels would fill a
// wave's 256 accumulator registers, so the VALUE axis is cut across the waves, not the rows:
//   phase A  wave w: S^T = K.Q^T for the rows 32 (w & 1) .. +32 and the keys 32 (w >> 1) .. +32 of the chunk: 9 MFMAs on the e4m3 Q^T fragments
//            the kernel quantised itself and parked in LDS (in registers they are 72 of a wave's 256 beside the 128 accumulators of phase B,
//            and the compiler spilled 54 of them to scratch, which no kernel here may use).  The row maxima of the two key halves meet
//            through 512 bytes of LDS; P = hi + lo (two-term e4m3, lo_terms) goes to LDS as the B operand of phase B.
//   phase B  wave w: O^T[128 w .. +128][64 rows] += V^T.P^T: 4 x 2 tiles = 128 accumulator registers, 8 MFMAs per P term.
// TRANSPOSITION  A chunk arrives once, by linear LDS-DMA, in K-operand order (a lane of the A operand holds 32 CHANNELS of one key).  Phase B
// needs the other orientation (32 KEYS of one channel).  One cooperative pass per chunk -- ds_read_b32 of 4 channels x 16 keys, 4x4 byte
// transposes with v_perm_b32 (the butterflies of vfrag_copy_out, csrc/qattn_common.h), four ds_write_b128 -- fills a 32 KiB VFRAG-order
// buffer that phase B reads with ds_read_b128; the bytes of keys at or behind L_b are zeroed on the way.
// LDS (bytes)  ring 2 x 36 864 | V^T 32 768 | P 8 192 | row maxima 512 | rescale factors 256 | row sums 512 | final maxima 256 | Q^T 36 864 = 153 088.
#include "qattn_fp8pv_sweep.h"
#include "../../include/qattn_mla.h"

using namespace qattn;

namespace {

constexpr int kD = QATTN_MLA_D, kDV = QATTN_MLA_D_LATENT, kKS = kD / 64, kCH = 64 * kD;
constexpr int kOffVT = 2 * kCH, kOffP = kOffVT + 64 * kDV, kOffMx = kOffP + 8192, kOffAl = kOffMx + 512, kOffLs = kOffAl + 256,
              kOffMf = kOffLs + 512, kOffQ = kOffMf + 256, kMlaLds = kOffQ + 64 * kD;
static_assert(kMlaLds <= 160 * 1024, "the ring, the transposed values and P fit a CU's LDS");
constexpr float kMlaStart = -1.0e20f;   // below any raw score (|q8 . k8| <= 576 x 448 x 57344)

struct MlaArgs {
    const unsigned short* q;
    long qsb, qsh, qss;   // element strides of q
    const unsigned char* pool;
    const int* table;
    long tstride;
    const float* scale;
    const int* seqused;
    void* out;
    float *lse, *po, *plse, *scale_q;
    unsigned char* q8;
    int B, Hq, Sq, Skv, ns, tiles, causal, out_fmt, num_pages, pc;
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

// grid = B ns tiles, block = 256.  blockIdx.x = (b ns + split) tiles + tile: the tiles of a (slot, split) sweep the same chunks side by side
// amdgpu_waves_per_eu(2, 2) is NOT an occupancy plan -- 256 threads and 153 088 bytes of LDS give one workgroup per CU, one wave per SIMD -- it
// states the register budget: at most 256 VGPRs and no AGPRs, the ceiling tests/test_kernel_resources.py holds every kernel of the library to
// (with launch_bounds alone the compiler may take up to 512).
template <int FMT, int IN_FMT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void mla_sweep_kernel(const MlaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hh = lane >> 5, rh = wave & 1, kh = wave >> 1;
    const int tile = (int)(blockIdx.x % (unsigned)a.tiles), bs = (int)(blockIdx.x / (unsigned)a.tiles);
    const int split = bs % a.ns, b = bs / a.ns;
    const int HS = a.Hq * a.Sq;
    int L = a.seqused[b];
    L = L < 0 ? 0 : L > a.Skv ? a.Skv : L;
    const int nch = (L + 63) >> 6, per = (nch + a.ns - 1) / a.ns;
    const int c_lo = split * per, c_hi = min(nch, c_lo + per), n = c_hi - c_lo;

    // ---- the K ring: every wave copies 9 x 1 KiB of a chunk
    const unsigned lane16 = (unsigned)lane << 4;
    const int* trow = a.table + (long)b * a.tstride;
    auto dma_chunk = [&](int chunk, int slot) {
        int page = trow[chunk / a.pc];   // chunk < ceil(L_b / 64): an entry below ceil(L_b / page_size)
        page = page < 0 ? 0 : page > a.num_pages - 1 ? a.num_pages - 1 : page;
        const unsigned char* src = a.pool + ((size_t)page * a.pc + chunk % a.pc) * (size_t)kCH + (wave << 10) + lane16;
        unsigned char* dst = smem + slot * kCH + (wave << 10);
#pragma unroll
        for (int r = 0; r < kCH / 4096; r++)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + r * 4096),
                                             (__attribute__((address_space(3))) void*)(dst + r * 4096), 16, 0, 0);
    };
    if (n > 0) dma_chunk(c_lo, 0);

    // ---- this lane's query row: token-wise scale from the row's abs-max, e4m3 Q^T fragments in registers
    const int R = tile * 64 + rh * 32 + ql;
    const bool qvalid = R < HS;
    const int h = qvalid ? R / a.Sq : 0, pos = qvalid ? R % a.Sq : 0;
    const uint4* qrow = reinterpret_cast<const uint4*>(a.q + (long)b * a.qsb + (long)h * a.qsh + (long)pos * a.qss) + 4 * hh;
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
    int kend = a.causal ? L - a.Sq + pos + 1 : L;   // the keys [0, kend) are this row's
    kend = !qvalid || kend < 0 ? 0 : kend;

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

    for (int t = 0; t < n; t++) {
        const int chunk = c_lo + t, slot = t & 1;
        wait_vmcnt<0>();                  // this wave's pieces of the chunk have landed
        __builtin_amdgcn_s_barrier();     // ... and everyone's; every wave is done with phase B of the chunk before and with the other slot
        if (t + 1 < n) dma_chunk(chunk + 1, slot ^ 1);
        const unsigned char* ring = smem + slot * kCH;

        // ---- phase A: 32 keys x 32 rows of scores
        v16f s;
#pragma unroll
        for (int r = 0; r < 16; r++) s[r] = 0.0f;
        {
            const unsigned char* kbuf = ring + ((kh * kKS) << 11) + flo;
#pragma unroll
            for (int sl = 0; sl < kKS; sl++) s = mfma_f8<FMT, QATTN_FMT_E4M3>(lds_read_frag(kbuf + (sl << 11)), lds_read_frag(qpark + (sl << 11)), s);
        }
        const int key0 = chunk * 64 + 32 * kh + 4 * hh;   // register r: key key0 + 8 (r >> 2) + (r & 3)
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            if (key0 + 8 * (r >> 2) + (r & 3) >= kend) s[r] = -INFINITY;
            mx = fmaxf(mx, s[r]);
        }
        {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
            mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        }
        if (hh == 0) xm[(rh * 2 + kh) * 32 + ql] = mx;

        // ---- the chunk's first 512 channels, transposed into VFRAG order; a thread: 16 keys (one (half, hh) of the key index) x 4 channels
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
        const int Ro = tile * 64 + r2 * 32 + ql;
        const bool valid = Ro < HS;
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

// One launch merges all ns partials of a row: grid = B Hq Sq rows, block = 128, a thread owns 4 channels.
// L = log sum_i exp(lse_i), O = sum_i exp(lse_i - L) O_i in fp32 in the order of i, one rounding.
__global__ __launch_bounds__(128) void mla_combine_kernel(const float* po, const float* plse, void* out, float* lse, long rows, int ns, int out_fmt) {
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

int mla_tiles(int Hq, int Sq) { return (Hq * Sq + 63) / 64; }

}  // namespace

extern "C" int qattn_mla_auto_splits(int B, int Hq, int Sq, int Skv, int num_cus) {
    if (B <= 0 || Hq <= 0 || Sq <= 0 || Skv <= 0 || num_cus <= 0) return 1;
    const long long base = (long long)B * (((long long)Hq * Sq + 63) / 64);
    long long ns = num_cus / base;
    if (ns > Skv / 1024) ns = Skv / 1024;
    return ns < 1 ? 1 : ns > QATTN_MLA_MAX_SPLITS ? QATTN_MLA_MAX_SPLITS : (int)ns;
}

extern "C" size_t qattn_fp8_mla_paged_workspace_bytes(int B, int Hq, int Sq, int num_splits) {
    if (B <= 0 || Hq <= 0 || Sq <= 0 || num_splits <= 1) return 0;
    const size_t rows = (size_t)num_splits * B * Hq * Sq;
    return up256(rows * kDV * sizeof(float)) + up256(rows * sizeof(float));
}

extern "C" int qattn_fp8_mla_paged_forward(const void* q16, int in_fmt, const long long* q_strides3, const void* pool, const int* block_table,
                                           long long table_stride, int num_pages, int page_size, int max_pages, const float* scale, void* out,
                                           float* lse, const int* seqused_k, int B, int Hq, int Sq, int Skv, int fp8_fmt, int is_causal,
                                           float sm_scale, int num_splits, void* q8, float* scale_q, float* partial_o, float* partial_lse,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!q16 || !pool || !block_table || !scale || !out || !seqused_k) return QATTN_ERR_INVALID_ARG;
    if ((size_t)block_table % 4 != 0 || ((size_t)pool | (size_t)q16 | (size_t)out | (size_t)q8 | (size_t)workspace) % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || Hq <= 0 || Sq <= 0 || Skv <= 0 || (long long)Hq * Sq > (1 << 20)) return QATTN_ERR_INVALID_ARG;
    if (num_pages <= 0 || max_pages <= 0 || page_size < 64 || page_size % 64 != 0 || table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    const int pc = page_size / 64;
    if ((long long)num_pages * pc > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;
    const long long capacity = (long long)max_pages * page_size;
    if (capacity > 0x7fffffffLL - 64 || Skv > capacity) return QATTN_ERR_INVALID_ARG;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (!(sm_scale > 0.0f) || !(sm_scale < INFINITY)) return QATTN_ERR_INVALID_ARG;
    if (num_splits < 0 || num_splits > QATTN_MLA_MAX_SPLITS) return QATTN_ERR_INVALID_ARG;
    if (q_strides3)
        for (int i = 0; i < 3; i++)
            if (q_strides3[i] < 0 || q_strides3[i] % 8 != 0) return QATTN_ERR_INVALID_ARG;
    const int ns = num_splits ? num_splits : qattn_mla_auto_splits(B, Hq, Sq, Skv, cu_count());
    const int tiles = mla_tiles(Hq, Sq);
    if ((long long)B * ns * tiles > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;
    if ((long long)B * Hq * Sq > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (the combine launches one block per row: a 32-bit grid)
    const size_t rows = (size_t)B * Hq * Sq;
    float *po = partial_o, *pl = partial_lse;
    if (ns > 1 && (!po || !pl)) {
        if (!workspace || workspace_bytes < qattn_fp8_mla_paged_workspace_bytes(B, Hq, Sq, ns)) return QATTN_ERR_INVALID_ARG;
        if (!po) po = reinterpret_cast<float*>(workspace);
        if (!pl) pl = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(workspace) + up256(rows * ns * kDV * sizeof(float)));
    }
    MlaArgs a;
    a.q = (const unsigned short*)q16;
    a.qsb = q_strides3 ? (long)q_strides3[0] : (long)Hq * Sq * kD;
    a.qsh = q_strides3 ? (long)q_strides3[1] : (long)Sq * kD;
    a.qss = q_strides3 ? (long)q_strides3[2] : (long)kD;
    a.pool = (const unsigned char*)pool; a.table = block_table; a.tstride = (long)table_stride; a.scale = scale; a.seqused = seqused_k;
    a.out = out; a.lse = lse; a.po = po; a.plse = pl; a.scale_q = scale_q; a.q8 = (unsigned char*)q8;
    a.B = B; a.Hq = Hq; a.Sq = Sq; a.Skv = Skv; a.ns = ns; a.tiles = tiles; a.causal = is_causal ? 1 : 0; a.out_fmt = in_fmt;
    a.num_pages = num_pages; a.pc = pc;
    a.c0 = sm_scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(B * ns * tiles);
    int rc;
    if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E4M3) rc = fpv_launch(mla_sweep_kernel<QATTN_FMT_E4M3, QATTN_FMT_BF16>, grid, kMlaLds, st, a);
    else if (in_fmt == QATTN_FMT_BF16) rc = fpv_launch(mla_sweep_kernel<QATTN_FMT_E5M2, QATTN_FMT_BF16>, grid, kMlaLds, st, a);
    else if (fp8_fmt == QATTN_FMT_E4M3) rc = fpv_launch(mla_sweep_kernel<QATTN_FMT_E4M3, QATTN_FMT_FP16>, grid, kMlaLds, st, a);
    else rc = fpv_launch(mla_sweep_kernel<QATTN_FMT_E5M2, QATTN_FMT_FP16>, grid, kMlaLds, st, a);
    if (rc != QATTN_OK) return rc;
    if (ns > 1) hipLaunchKernelGGL(mla_combine_kernel, dim3((unsigned)rows), dim3(128), 0, st, po, pl, out, lse, (long)rows, ns, in_fmt);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

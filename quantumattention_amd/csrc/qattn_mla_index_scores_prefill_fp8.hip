// qattn_mla_index_scores_prefill_fp8.hip -- qattn_fp8_mla_index_scores_varlen and qattn_fp8_mla_index_topk_varlen
// (include/qattn_mla_index_prefill.h): the index scores of the lightning indexer for PACKED variable-length queries -- a prompt, a prompt
// chunk over its cached prefix, several of them -- over the row-major paged FP8 index-key cache, gfx950.
//
//   logit[r, j] = scale[b] sum_h (w[r, h] scale_q[r, h]) max(q8[r, h, :] . k8[b, j, :], 0)
//
// WORK ITEM  (slot b, tile of kTQ = 8 consecutive tokens of the slot, range of kWG keys), 4 waves; wave w owns the tokens 2 w and 2 w + 1 of
//            the tile and sweeps EVERY key of the range for them.  blockIdx.x / nranges is a tile slot, resolved by a binary search on cu_seqlens_q
//            (qattn_varlen_tile.h's map, with the rows behind cu[B] as one more "slot" of length 0 keys); spare tile slots exit.
// K          a key tile is kKT = 128 keys x 128 bytes.  The workgroup brings it into LDS ONCE -- 8 lanes fetch one 128-byte row, a lane
//            holds four 16-byte pieces -- and all four waves read the whole tile from there: the key bytes a workgroup pulls from L2 serve
//            8 tokens instead of one.  Two LDS images: the pieces of tile t + 1 are loaded into registers before the MFMAs of tile t and
//            stored behind them, one barrier per tile; the physical rows of tile t + 2 (one clamped table load per piece, page and offset
//            stepped by 128 keys with an add and a compare) are looked up at the same time, so no load waits on a load inside the sweep.
// LDS IMAGE  piece c = 4 s + 2 hh + i of key k (bytes 16 c .. 16 c + 15 of its row) of the 32-key group g lies at
//            4096 g + 512 c + 16 (k ^ c): the FRAGMENT order [group][piece][key][16 B] with the key slot XORed by the piece number.  A
//            ds_read_b128 of the sweep has one c per half wave and the keys ql = 0 .. 31: 32 lanes read one contiguous 512-byte run (the
//            XOR permutes within aligned runs of 8 slots), every bank once -- no conflict.  A ds_write_b128 of the fetch has c = lane & 7
//            and keys 8 (lane >> 3 & 3) + 2 u + (lane >> 5): 16 consecutive lanes hold 2 keys 8 apart x 8 pieces, whose slots k ^ c are
//            all 16 residues mod 16 -- 256 contiguous-equivalent bytes, every bank once.  (With plain 128-byte rows the 32 lanes of a read
//            would be 128 bytes apart: all on the same 4 banks.)
// Q, REDUCTION, OPERANDS  csrc/qattn_mla_index_scores_fp8.hip's, operation for operation, twice: the heads are the M operand, the keys the N
//            operand of v_mfma_f32_32x32x64_f8f6f4; a wave quantises the Hi x 128 bytes of each of its two tokens in its prologue and keeps
//            them and the 32 weights w scale_q in registers; ReLU and the weighted head sum are 16 fused multiply-adds per head tile in
//            accumulator-row order, one add over the head tiles, one add of lanes l and l + 32, last the slot's scale.
// CAUSAL     kend is per token.  The sweep ends at kend of the tile's LAST token (tiles behind it are not fetched); inside it a wave skips
//            the 32-key groups at or behind kend of both its tokens, and a lane writes a logit only below its token's kend.
// VGPRs      Q 64 | weights 64 | accumulators 32 | K operands 16 | pieces in flight 16 | rows, pages, offsets 12.  LDS 32 768 bytes.
#include "qattn_fp8pv_sweep.h"
#include "qattn_varlen_tile.h"
#include "../../include/qattn_mla_index_prefill.h"

using namespace qattn;

namespace {

constexpr int kDI = QATTN_MLA_INDEX_D, kTQ = QATTN_MLA_INDEX_PREFILL_TOKENS, kKT = QATTN_MLA_INDEX_PREFILL_KEYS;
constexpr int kWG = QATTN_MLA_INDEX_PREFILL_WG_KEYS, kSelRows = 65535;
static_assert(kDI == 128 && kTQ == 8 && kKT == 128, "4 waves x 2 tokens; a wave fetches one 32-key group of the 128-key tile");
static_assert(kWG % kKT == 0 && kWG >= kKT, "a range is whole key tiles");

struct PrefillScoreArgs {
    const unsigned short* q;
    long qst, qsh;        // element strides of q: token, head
    const float* w;
    long wst;             // elements between the weights of two tokens
    const unsigned char* pool;
    const int* table;
    long tstride;
    const float* scale;
    const int* cu;
    const int* seqused;
    float* logits;
    long lst;             // elements between two logits rows
    int* kend;
    unsigned char* q8;
    float* scale_q;
    int B, Hi, total, N, causal, fill, num_pages, page_size, nranges;
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

// The query rows of packed row r: head 32 t + ql, this lane's channels 64 s + 32 hh .. + 31, quantised by the dense kernel's rule; the
// weights w scale_q in the order of the accumulator rows.  `on` (wave-uniform): the row has a query -- else nothing is read, the operands and
// weights are 0.  `emit`: the row's q8 / scale_q are written (zeros for a row without a query).
template <int IN_FMT>
__device__ __forceinline__ void load_token(const PrefillScoreArgs& a, long r, bool on, bool emit, int ql, int hh, v8i (&qf)[2][2], float (&wq)[2][16]) {
    float wown[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int h = 32 * t + ql;
        const bool valid = h < a.Hi;
        uint4 x[2][4];
        unsigned am = 0u;
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int i = 0; i < 4; i++) x[s][i] = make_uint4(0u, 0u, 0u, 0u);
        if (on) {
            const uint4* qrow = reinterpret_cast<const uint4*>(a.q + r * a.qst + (long)(valid ? h : 0) * a.qsh) + 4 * hh;
#pragma unroll
            for (int s = 0; s < 2; s++)
#pragma unroll
                for (int i = 0; i < 4; i++) { x[s][i] = qrow[8 * s + i]; am = amax_bits16<IN_FMT>(x[s][i], am); }
        }
        {
            const auto sw = __builtin_amdgcn_permlane32_swap(am, am, false, false);
            am = max(sw[0], sw[1]);
        }
        float scale_q = load16f<IN_FMT>((unsigned short)am) / 448.0f;
        if (!(scale_q >= 1.1920928955078125e-07f)) scale_q = 1.1920928955078125e-07f;
        const float rinv = 1.0f / scale_q;
        const long R = r * a.Hi + h;   // the row of [total_q, Hi]
#pragma unroll
        for (int s = 0; s < 2; s++) {
            int2 v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                v[i] = quant_q8<IN_FMT>(x[s][i], rinv);
                if (!valid) v[i] = make_int2(0, 0);
            }
            qf[t][s] = v8i{v[0].x, v[0].y, v[1].x, v[1].y, v[2].x, v[2].y, v[3].x, v[3].y};
            if (emit && valid) {
                unsigned char* qo = a.q8 + R * kDI + 64 * s + 32 * hh;
                *reinterpret_cast<v4i*>(qo) = v4i{v[0].x, v[0].y, v[1].x, v[1].y};
                *reinterpret_cast<v4i*>(qo + 16) = v4i{v[2].x, v[2].y, v[3].x, v[3].y};
            }
        }
        if (emit && valid && hh == 0 && a.scale_q) a.scale_q[R] = on ? scale_q : 0.0f;
        wown[t] = 0.0f;
        if (on && valid) wown[t] = a.w[r * a.wst + h] * scale_q;
    }
    // register r of tile t is head 32 t + 8 (r >> 2) + 4 hh + (r & 3)
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int r16 = 0; r16 < 16; r16++) wq[t][r16] = __shfl(wown[t], 8 * (r16 >> 2) + 4 * hh + (r16 & 3));
}

// grid = (B + ceil(total / kTQ) tile slots) x (nranges = ceil(N / kWG) key ranges, the fast index), block = 256
template <int FMT, int IN_FMT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void mla_index_scores_prefill_kernel(const PrefillScoreArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char kt[2][kKT * kDI];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hh = lane >> 5;
    const int slot = (int)(blockIdx.x / (unsigned)a.nranges), range = (int)(blockIdx.x % (unsigned)a.nranges);

    // ---- tile slot -> (slot b, tile): the largest b in 0 .. B with b + floor(start_b / kTQ) <= slot; b = B is the rows behind cu[B]
    int b = 0;
    {
        int hi = a.B;
        const int j = slot;
        while (b < hi) {   // (workgroup-uniform)
            const int mid = (b + hi + 1) >> 1;
            const int s = clampi(__builtin_amdgcn_readfirstlane(a.cu[mid]), 0, a.total);
            if (mid + s / kTQ <= j) b = mid;
            else hi = mid - 1;
        }
    }
    const bool pad = b == a.B;
    const int start = clampi(__builtin_amdgcn_readfirstlane(a.cu[b]), 0, a.total);
    const int n = (pad ? a.total : clampi(__builtin_amdgcn_readfirstlane(a.cu[b + 1]), start, a.total)) - start;
    const int t0 = (slot - (b + start / kTQ)) * kTQ;   // the tile's first token of the slot
    if (t0 < 0 || t0 >= n) return;
    int L = 0;
    if (!pad) {
        L = __builtin_amdgcn_readfirstlane(a.seqused[b]);
        L = L < 0 ? 0 : L > a.N ? a.N : L;
    }
    // kend of token i of the slot; non-decreasing in i, so the tile's last token bounds the sweep
    auto kend_of = [&](int i) { const int k = a.causal ? L - n + i + 1 : L; return k < 0 ? 0 : k; };
    const int kmax = kend_of((t0 + kTQ < n ? t0 + kTQ : n) - 1);
    const int lo = range * kWG;
    const bool live = lo < kmax, first = range == 0;
    const int ntiles = live ? ((kmax - lo < kWG ? kmax - lo : kWG) + kKT - 1) / kKT : 0;   // key tiles this workgroup sweeps

    // ---- this wave's two tokens
    bool have[2];
    int kend[2];
    long row[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const int i = t0 + 2 * wave + e;
        have[e] = i < n;
        kend[e] = have[e] ? kend_of(i) : 0;
        row[e] = (long)start + (have[e] ? i : 0);
        if (first && have[e] && lane == 0) a.kend[row[e]] = kend[e];
    }
    const int kwave = kend[0] > kend[1] ? kend[0] : kend[1];
    const bool emit_q8 = first && a.q8 != nullptr;

    if (live || emit_q8) {
        v8i qf[2][2][2];
        float wq[2][2][16];
#pragma unroll
        for (int e = 0; e < 2; e++) load_token<IN_FMT>(a, row[e], have[e] && !pad, emit_q8 && have[e], ql, hh, qf[e], wq[e]);

        if (live) {
            const bool two_tiles = a.Hi > 32;   // (workgroup-uniform)
            const float scale_k = a.scale[pad ? 0 : b];
            // ---- the fetch: piece c of the keys lo + 128 t + 32 wave + kl[u]
            const int c = lane & 7, klb = 8 * ((lane >> 3) & 3) + (lane >> 5);
            const int* trow = a.table + (long)(pad ? 0 : b) * a.tstride;
            const int ps = a.page_size, dq = kKT / ps, dr = kKT % ps;
            int pi[4], po[4], jn[4], st[4];   // page index, offset and key of the NEXT tile to look up; LDS byte of the piece
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int kl = klb + 2 * u;
                jn[u] = lo + 32 * wave + kl;
                pi[u] = jn[u] / ps; po[u] = jn[u] % ps;
                st[u] = 4096 * wave + 512 * c + 16 * (kl ^ c);
            }
            auto lookup = [&](int (&r)[4]) {   // the physical rows of the next tile; a key at or behind kmax reads row 0 of the pool
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    r[u] = 0;
                    if (jn[u] < kmax) {   // below kend <= max_seqlen_k <= capacity: an entry of the table's row
                        int page = trow[pi[u]];
                        page = page < 0 ? 0 : page > a.num_pages - 1 ? a.num_pages - 1 : page;
                        r[u] = page * ps + po[u];   // <= num_pages page_size - 1
                    }
                    jn[u] += kKT; pi[u] += dq; po[u] += dr;
                    if (po[u] >= ps) { po[u] -= ps; pi[u]++; }
                }
            };
            auto fetch = [&](const int (&r)[4], v4i (&p)[4]) {
#pragma unroll
                for (int u = 0; u < 4; u++) p[u] = *reinterpret_cast<const v4i*>(a.pool + (size_t)r[u] * kDI + 16 * c);
            };
            auto stash = [&](unsigned char* img, const v4i (&p)[4]) {
#pragma unroll
                for (int u = 0; u < 4; u++) *reinterpret_cast<v4i*>(img + st[u]) = p[u];
            };
            // ---- the sweep's LDS reads: piece 4 s + 2 hh + i of key ql
            int rd[2][2];
#pragma unroll
            for (int s = 0; s < 2; s++)
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const int cc = 4 * s + 2 * hh + i;
                    rd[s][i] = 512 * cc + 16 * (ql ^ cc);
                }

            int rows[4];
            v4i piece[4];
            lookup(rows);
            fetch(rows, piece);
            if (ntiles > 1) lookup(rows);
            stash(kt[0], piece);
            __syncthreads();
            for (int t = 0; t < ntiles; t++) {
                if (t + 1 < ntiles) fetch(rows, piece);
                if (t + 2 < ntiles) lookup(rows);
                const unsigned char* img = kt[t & 1];
                const int base0 = lo + kKT * t;
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const int base = base0 + 32 * g, j = base + ql;
                    if (base < kwave) {   // (wave-uniform)
                        v8i kc[2];
#pragma unroll
                        for (int s = 0; s < 2; s++) {
                            const v4i k0 = *reinterpret_cast<const v4i*>(img + 4096 * g + rd[s][0]);
                            const v4i k1 = *reinterpret_cast<const v4i*>(img + 4096 * g + rd[s][1]);
                            kc[s] = v8i{k0[0], k0[1], k0[2], k0[3], k1[0], k1[1], k1[2], k1[3]};
                        }
#pragma unroll
                        for (int e = 0; e < 2; e++) {
                            float* lrow = a.logits + row[e] * a.lst;
                            if (base < kend[e]) {
                                v16f s0, s1;
#pragma unroll
                                for (int r = 0; r < 16; r++) s0[r] = s1[r] = 0.0f;
                                s0 = mfma_f8<QATTN_FMT_E4M3, FMT>(qf[e][0][0], kc[0], s0);
                                s0 = mfma_f8<QATTN_FMT_E4M3, FMT>(qf[e][0][1], kc[1], s0);
                                float acc = 0.0f;
#pragma unroll
                                for (int r = 0; r < 16; r++) acc = __builtin_fmaf(wq[e][0][r], fmaxf(s0[r], 0.0f), acc);
                                if (two_tiles) {
                                    s1 = mfma_f8<QATTN_FMT_E4M3, FMT>(qf[e][1][0], kc[0], s1);
                                    s1 = mfma_f8<QATTN_FMT_E4M3, FMT>(qf[e][1][1], kc[1], s1);
                                    float acc1 = 0.0f;
#pragma unroll
                                    for (int r = 0; r < 16; r++) acc1 = __builtin_fmaf(wq[e][1][r], fmaxf(s1[r], 0.0f), acc1);
                                    acc += acc1;
                                }
                                {
                                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc), __float_as_uint(acc), false, false);
                                    acc = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
                                }
                                if (hh == 0 && j < kend[e]) lrow[j] = acc * scale_k;
                                else if (hh == 0 && a.fill && j < a.N) lrow[j] = -INFINITY;
                            } else if (a.fill && have[e]) {
                                if (hh == 0 && j < a.N) lrow[j] = -INFINITY;
                            }
                        }
                    } else if (a.fill) {
#pragma unroll
                        for (int e = 0; e < 2; e++)
                            if (have[e] && hh == 0 && j < a.N) a.logits[row[e] * a.lst + j] = -INFINITY;
                    }
                }
                if (t + 1 < ntiles) stash(kt[(t + 1) & 1], piece);
                __syncthreads();
            }
        }
    }
    // ---- the rest of the range, behind the last swept tile: -inf when asked to
    if (a.fill) {
        const long end = (long)lo + kWG < a.N ? (long)lo + kWG : a.N;
#pragma unroll
        for (int e = 0; e < 2; e++)
            if (have[e])
                for (long j = (long)lo + (long)kKT * ntiles + lane; j < end; j += 64) a.logits[row[e] * a.lst + j] = -INFINITY;
    }
}

}  // namespace

extern "C" size_t qattn_fp8_mla_index_varlen_workspace_bytes(int total_q, int max_seqlen_k) {
    if (total_q <= 0 || max_seqlen_k <= 0) return 0;
    return up256((size_t)total_q * sizeof(int)) + up256((size_t)total_q * (size_t)max_seqlen_k * sizeof(float));
}

extern "C" int qattn_fp8_mla_index_scores_varlen(const void* q16, int in_fmt, const long long* q_strides2, const float* weights,
                                                 long long w_stride, const void* pool, const int* block_table, long long table_stride,
                                                 int num_pages, int page_size, int max_pages, const float* scale, const int* cu_seqlens_q,
                                                 const int* seqused_k, int B, int Hi, int total_q, int max_seqlen_k, int fp8_fmt, int is_causal,
                                                 float* logits, long long logits_stride, int fill_tail, int* kend, void* q8, float* scale_q,
                                                 void* stream) {
    if (!q16 || !weights || !pool || !block_table || !scale || !cu_seqlens_q || !seqused_k || !logits || !kend) return QATTN_ERR_INVALID_ARG;
    if (((size_t)block_table | (size_t)weights | (size_t)logits | (size_t)cu_seqlens_q | (size_t)seqused_k | (size_t)kend | (size_t)scale_q) % 4 != 0 ||
        ((size_t)pool | (size_t)q16 | (size_t)q8) % 16 != 0)
        return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || B > 65535 || total_q <= 0 || total_q > 0x7fffffff - 65535 || Hi <= 0 || Hi > QATTN_MLA_INDEX_MAX_HEADS) return QATTN_ERR_INVALID_ARG;
    if (num_pages <= 0 || max_pages <= 0 || page_size <= 0 || table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    if ((long long)num_pages * page_size > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (a physical row number is an int)
    const long long capacity = (long long)max_pages * page_size;
    if (capacity > 0x7fffffffLL - 64) return QATTN_ERR_INVALID_ARG;
    if (max_seqlen_k <= 0 || max_seqlen_k > capacity || max_seqlen_k > (1 << 30)) return QATTN_ERR_INVALID_ARG;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (q_strides2)
        for (int i = 0; i < 2; i++)
            if (q_strides2[i] < 0 || q_strides2[i] % 8 != 0) return QATTN_ERR_INVALID_ARG;
    if (w_stride < 0 || logits_stride < 0) return QATTN_ERR_INVALID_ARG;
    PrefillScoreArgs a;
    a.q = (const unsigned short*)q16;
    a.qst = q_strides2 ? (long)q_strides2[0] : (long)Hi * kDI;
    a.qsh = q_strides2 ? (long)q_strides2[1] : (long)kDI;
    a.w = weights; a.wst = w_stride ? (long)w_stride : (long)Hi;
    a.pool = (const unsigned char*)pool; a.table = block_table; a.tstride = (long)table_stride; a.scale = scale;
    a.cu = cu_seqlens_q; a.seqused = seqused_k;
    a.logits = logits; a.lst = logits_stride ? (long)logits_stride : (long)max_seqlen_k;
    a.kend = kend; a.q8 = (unsigned char*)q8; a.scale_q = scale_q;
    a.B = B; a.Hi = Hi; a.total = total_q; a.N = max_seqlen_k; a.causal = is_causal ? 1 : 0; a.fill = fill_tail ? 1 : 0;
    a.num_pages = num_pages; a.page_size = page_size; a.nranges = (max_seqlen_k + kWG - 1) / kWG;
    const long long nwg = (long long)(B + (total_q + kTQ - 1) / kTQ) * a.nranges;
    if (nwg > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (the grid: 2^34 logits or more)
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nwg), block(256);
    if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E4M3) hipLaunchKernelGGL((mla_index_scores_prefill_kernel<QATTN_FMT_E4M3, QATTN_FMT_BF16>), grid, block, 0, st, a);
    else if (in_fmt == QATTN_FMT_BF16) hipLaunchKernelGGL((mla_index_scores_prefill_kernel<QATTN_FMT_E5M2, QATTN_FMT_BF16>), grid, block, 0, st, a);
    else if (fp8_fmt == QATTN_FMT_E4M3) hipLaunchKernelGGL((mla_index_scores_prefill_kernel<QATTN_FMT_E4M3, QATTN_FMT_FP16>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((mla_index_scores_prefill_kernel<QATTN_FMT_E5M2, QATTN_FMT_FP16>), grid, block, 0, st, a);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

extern "C" int qattn_fp8_mla_index_topk_varlen(const void* q16, int in_fmt, const long long* q_strides2, const float* weights,
                                               long long w_stride, const void* pool, const int* block_table, long long table_stride,
                                               int num_pages, int page_size, int max_pages, const float* scale, const int* cu_seqlens_q,
                                               const int* seqused_k, int B, int Hi, int total_q, int max_seqlen_k, int topk, int fp8_fmt,
                                               int is_causal, int* indices, float* logits, void* q8, float* scale_q, void* workspace,
                                               size_t workspace_bytes, void* stream) {
    if (!indices || (size_t)indices % 4 != 0 || !workspace || (size_t)workspace % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if (topk <= 0 || topk > QATTN_MLA_SPARSE_MAX_TOPK || total_q <= 0 || max_seqlen_k <= 0) return QATTN_ERR_INVALID_ARG;
    const size_t kend_bytes = up256((size_t)total_q * sizeof(int));
    if (workspace_bytes < (logits ? kend_bytes : qattn_fp8_mla_index_varlen_workspace_bytes(total_q, max_seqlen_k))) return QATTN_ERR_INVALID_ARG;
    int* kend = reinterpret_cast<int*>(workspace);
    float* rows = logits ? logits : reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(workspace) + kend_bytes);
    const int rc = qattn_fp8_mla_index_scores_varlen(q16, in_fmt, q_strides2, weights, w_stride, pool, block_table, table_stride, num_pages,
                                                     page_size, max_pages, scale, cu_seqlens_q, seqused_k, B, Hi, total_q, max_seqlen_k, fp8_fmt,
                                                     is_causal, rows, 0, logits != nullptr, kend, q8, scale_q, stream);
    if (rc != QATTN_OK) return rc;
    // the packed rows as B = rows, Sq = 1 of the dense selection, non-causal with seqused_k = kend; its grid limit per launch
    for (long r0 = 0; r0 < total_q; r0 += kSelRows) {
        const int nr = total_q - r0 < kSelRows ? (int)(total_q - r0) : kSelRows;
        const int rs = qattn_mla_index_select(rows + r0 * max_seqlen_k, nullptr, kend + r0, nr, 1, max_seqlen_k, topk, 0,
                                              indices + r0 * topk, stream);
        if (rs != QATTN_OK) return rs;
    }
    return QATTN_OK;
}

// qattn_mla_index_scores_fp8.hip -- qattn_fp8_mla_index_scores and qattn_fp8_mla_index_topk (include/qattn_mla_index.h): the index scores of
// the lightning indexer over the row-major paged FP8 index-key cache, gfx950.
//
//   logit[b, i, j] = scale[b] sum_h (w[b, i, h] scale_q[b, h, i]) max(q8[b, h, i, :] . k8[b, j, :], 0)
//
// WORK ITEM  (slot b, position i, range of kWG keys), 4 waves; wave w owns the 32-key groups w, w + 4, ... of the range.  A range at or
//            behind kend(b, i) only fills its logits with -inf (when asked to) and exits.
// OPERANDS   v_mfma_f32_32x32x64_f8f6f4 with the HEADS as the M operand and the KEYS as the N operand: in the 32 x 32 accumulator lane
//            (ql, hh) holds the 16 head rows 8 (r >> 2) + 4 hh + (r & 3) of the ONE key column ql.  K = 128 is two instructions per head tile.
// Q          Hi x 128 bytes = 2 head tiles x 2 k-steps x 8 VGPRs per lane, quantised by every wave for itself in the prologue (two 64-byte
//            pieces of a row per lane pair, the row's abs-max through one permlane32 swap) and kept in registers for the whole sweep; no LDS.
//            Heads >= Hi are zero rows with weight 0; the second head tile is skipped when Hi <= 32.
// K          the k-slot order inside the instruction is irrelevant as long as A and B agree, so lane (ql, hh) takes the 32 CONTIGUOUS bytes
//            64 s + 32 hh .. + 31 of its key's row straight from global memory into the B operand of k-step s (two 16-byte loads), and Q's
//            A operand holds the same channels.  No LDS staging, no transposition.  The physical rows of a lane's keys come from one
//            (clamped) table load per group, all issued in the prologue; the page of group g + 1 follows from group g's by an add and a
//            compare (128 keys further), so no division by page_size sits in the sweep.  The loads of group g + 1 are issued before the
//            MFMAs of group g.
// REDUCTION  ReLU and the weighted head sum are 16 fused multiply-adds per head tile on weights w scale_q held in registers in the order of
//            the accumulator rows, one add over the two head tiles, one cross-lane add of lanes l and l + 32.  No LDS.
// VGPRs      Q 32 | weights 32 | accumulators 32 | K now and next 32 | rows kWG / 128.  LDS 0.
#include "qattn_fp8pv_sweep.h"
#include "../../include/qattn_mla_index.h"

using namespace qattn;

namespace {

constexpr int kDI = QATTN_MLA_INDEX_D, kWG = QATTN_MLA_INDEX_WG_KEYS, kNG = kWG / 128;   // kNG: 32-key groups per wave
static_assert(kWG % 128 == 0 && kNG >= 1 && kNG <= 32, "a range is whole rounds of the 4 waves' 32-key groups");

struct IndexScoreArgs {
    const unsigned short* q;
    long qsb, qsh, qss;   // element strides of q
    const float* w;
    long wsb, wss;        // element strides of the weights
    const unsigned char* pool;
    const int* table;
    long tstride;
    const float* scale;
    const int* seqused;
    float* logits;
    long lsb, lss;        // element strides of the logits rows
    unsigned char* q8;
    float* scale_q;
    int Hi, Sq, N, causal, fill, num_pages, page_size;
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

// the 64 bytes of a key row this lane feeds to the two k-steps: bytes 32 hh .. + 31 and 64 + 32 hh .. + 31
__device__ __forceinline__ void load_key(const unsigned char* pool, int row, int hh, v8i (&k)[2]) {
    const v4i* p = reinterpret_cast<const v4i*>(pool + (size_t)row * kDI + 32 * hh);
    const v4i a0 = p[0], a1 = p[1], b0 = p[4], b1 = p[5];
    k[0] = v8i{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    k[1] = v8i{b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
}

// grid = (ceil(N / kWG), Sq, B), block = 256
template <int FMT, int IN_FMT>
__global__ __launch_bounds__(256) void mla_index_scores_kernel(const IndexScoreArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hh = lane >> 5;
    const int b = blockIdx.z, pos = blockIdx.y, lo = (int)blockIdx.x * kWG;
    int L = a.seqused[b];
    L = L < 0 ? 0 : L > a.N ? a.N : L;
    int kend = a.causal ? L - a.Sq + pos + 1 : L;   // the keys [0, kend) are scored for this position
    kend = kend < 0 ? 0 : kend;
    float* lrow = a.logits + (long)b * a.lsb + (long)pos * a.lss;
    const bool live = lo < kend, emit_q8 = blockIdx.x == 0 && a.q8 != nullptr;
    if (!live && a.fill)
        for (int j = lo + tid; j < lo + kWG && j < a.N; j += 256) lrow[j] = -INFINITY;
    if (!live && !emit_q8) return;

    // ---- the query rows of this position: head 32 t + ql, this lane's channels 64 s + 32 hh .. + 31; a row's scale from its abs-max
    v8i qf[2][2];
    float wown[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int h = 32 * t + ql;
        const bool valid = h < a.Hi;
        const uint4* qrow = reinterpret_cast<const uint4*>(a.q + (long)b * a.qsb + (long)(valid ? h : 0) * a.qsh + (long)pos * a.qss) + 4 * hh;
        uint4 x[2][4];
        unsigned am = 0u;
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int i = 0; i < 4; i++) { x[s][i] = qrow[8 * s + i]; am = amax_bits16<IN_FMT>(x[s][i], am); }
        {
            const auto sw = __builtin_amdgcn_permlane32_swap(am, am, false, false);
            am = max(sw[0], sw[1]);
        }
        float scale_q = load16f<IN_FMT>((unsigned short)am) / 448.0f;
        if (!(scale_q >= 1.1920928955078125e-07f)) scale_q = 1.1920928955078125e-07f;
        const float rinv = 1.0f / scale_q;
        const long R = ((long)b * a.Hi + h) * a.Sq + pos;   // the row of [B, Hi, Sq]
#pragma unroll
        for (int s = 0; s < 2; s++) {
            int2 v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                v[i] = quant_q8<IN_FMT>(x[s][i], rinv);
                if (!valid) v[i] = make_int2(0, 0);
            }
            qf[t][s] = v8i{v[0].x, v[0].y, v[1].x, v[1].y, v[2].x, v[2].y, v[3].x, v[3].y};
            if (emit_q8 && wave == 0 && valid) {
                unsigned char* qo = a.q8 + R * kDI + 64 * s + 32 * hh;
                *reinterpret_cast<v4i*>(qo) = v4i{v[0].x, v[0].y, v[1].x, v[1].y};
                *reinterpret_cast<v4i*>(qo + 16) = v4i{v[2].x, v[2].y, v[3].x, v[3].y};
            }
        }
        if (emit_q8 && wave == 0 && valid && hh == 0 && a.scale_q) a.scale_q[R] = scale_q;
        wown[t] = valid ? a.w[(long)b * a.wsb + (long)pos * a.wss + h] * scale_q : 0.0f;
    }
    if (!live) return;

    // ---- the weights in the order of the accumulator rows: register r of tile t is head 32 t + 8 (r >> 2) + 4 hh + (r & 3)
    const bool two_tiles = a.Hi > 32;   // (workgroup-uniform)
    float wq[2][16];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) wq[t][r] = __shfl(wown[t], 8 * (r >> 2) + 4 * hh + (r & 3));

    // ---- the physical rows of this lane's keys lo + 32 wave + ql + 128 g: one division here, then 128 keys further per group
    int row[kNG];
    {
        const int* trow = a.table + (long)b * a.tstride;
        const int ps = a.page_size, dq = 128 / ps, dr = 128 % ps;
        const int j0 = lo + 32 * wave + ql;
        int pi = j0 / ps, po = j0 % ps;
#pragma unroll
        for (int g = 0; g < kNG; g++) {
            int page = 0;
            if (j0 + 128 * g < kend) {   // a key below kend <= max_seqlen_k <= capacity: an entry of the table's row
                page = trow[pi];
                page = page < 0 ? 0 : page > a.num_pages - 1 ? a.num_pages - 1 : page;
                row[g] = page * ps + po;   // <= num_pages page_size - 1
            } else {
                row[g] = 0;                // (a masked lane reads row 0 of the pool)
            }
            pi += dq; po += dr;
            if (po >= ps) { po -= ps; pi++; }
        }
    }
    const float scale_k = a.scale[b];

    // ---- the sweep
    const int base0 = lo + 32 * wave;   // (wave-uniform) the first key of this wave's group g is base0 + 128 g
    v8i kc[2], kn[2];
#pragma unroll
    for (int s = 0; s < 2; s++) kc[s] = kn[s] = v8i{0, 0, 0, 0, 0, 0, 0, 0};
    if (base0 < kend) load_key(a.pool, row[0], hh, kc);
#pragma unroll
    for (int g = 0; g < kNG; g++) {
        const int base = base0 + 128 * g;
        if (g + 1 < kNG && base + 128 < kend) load_key(a.pool, row[g + 1 < kNG ? g + 1 : g], hh, kn);
        const int j = base + ql;
        if (base < kend) {
            v16f s0, s1;
#pragma unroll
            for (int r = 0; r < 16; r++) s0[r] = s1[r] = 0.0f;
            s0 = mfma_f8<QATTN_FMT_E4M3, FMT>(qf[0][0], kc[0], s0);
            s0 = mfma_f8<QATTN_FMT_E4M3, FMT>(qf[0][1], kc[1], s0);
            float acc = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; r++) acc = __builtin_fmaf(wq[0][r], fmaxf(s0[r], 0.0f), acc);
            if (two_tiles) {
                s1 = mfma_f8<QATTN_FMT_E4M3, FMT>(qf[1][0], kc[0], s1);
                s1 = mfma_f8<QATTN_FMT_E4M3, FMT>(qf[1][1], kc[1], s1);
                float acc1 = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; r++) acc1 = __builtin_fmaf(wq[1][r], fmaxf(s1[r], 0.0f), acc1);
                acc += acc1;
            }
            {
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc), __float_as_uint(acc), false, false);
                acc = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
            }
            if (hh == 0 && j < kend) lrow[j] = acc * scale_k;   // (kend <= N)
            else if (hh == 0 && a.fill && j < a.N) lrow[j] = -INFINITY;   // the group that kend cuts: its tail is the caller's unless asked for
        } else if (a.fill) {
            if (hh == 0 && j < a.N) lrow[j] = -INFINITY;
        }
#pragma unroll
        for (int s = 0; s < 2; s++) kc[s] = kn[s];
    }
}

}  // namespace

extern "C" size_t qattn_fp8_mla_index_workspace_bytes(int B, int Sq, int max_seqlen_k) {
    if (B <= 0 || Sq <= 0 || max_seqlen_k <= 0) return 0;
    return up256((size_t)B * Sq * (size_t)max_seqlen_k * sizeof(float));
}

extern "C" int qattn_fp8_mla_index_scores(const void* q16, int in_fmt, const long long* q_strides3, const float* weights,
                                          const long long* w_strides2, const void* pool, const int* block_table, long long table_stride,
                                          int num_pages, int page_size, int max_pages, const float* scale, const int* seqused_k, int B, int Hi,
                                          int Sq, int max_seqlen_k, int fp8_fmt, int is_causal, float* logits, const long long* logits_strides2,
                                          int fill_tail, void* q8, float* scale_q, void* stream) {
    if (!q16 || !weights || !pool || !block_table || !scale || !seqused_k || !logits) return QATTN_ERR_INVALID_ARG;
    if (((size_t)block_table | (size_t)weights | (size_t)logits) % 4 != 0 || ((size_t)pool | (size_t)q16 | (size_t)q8) % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || Sq <= 0 || B > 65535 || Sq > 65535 || Hi <= 0 || Hi > QATTN_MLA_INDEX_MAX_HEADS) return QATTN_ERR_INVALID_ARG;
    if (num_pages <= 0 || max_pages <= 0 || page_size <= 0 || table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    if ((long long)num_pages * page_size > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (a physical row number is an int)
    const long long capacity = (long long)max_pages * page_size;
    if (capacity > 0x7fffffffLL - 64) return QATTN_ERR_INVALID_ARG;
    if (max_seqlen_k <= 0 || max_seqlen_k > capacity || max_seqlen_k > (1 << 30)) return QATTN_ERR_INVALID_ARG;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (q_strides3)
        for (int i = 0; i < 3; i++)
            if (q_strides3[i] < 0 || q_strides3[i] % 8 != 0) return QATTN_ERR_INVALID_ARG;
    if (w_strides2 && (w_strides2[0] < 0 || w_strides2[1] < 0)) return QATTN_ERR_INVALID_ARG;
    if (logits_strides2 && (logits_strides2[0] < 0 || logits_strides2[1] < 0)) return QATTN_ERR_INVALID_ARG;
    IndexScoreArgs a;
    a.q = (const unsigned short*)q16;
    a.qsb = q_strides3 ? (long)q_strides3[0] : (long)Hi * Sq * kDI;
    a.qsh = q_strides3 ? (long)q_strides3[1] : (long)Sq * kDI;
    a.qss = q_strides3 ? (long)q_strides3[2] : (long)kDI;
    a.w = weights;
    a.wsb = w_strides2 ? (long)w_strides2[0] : (long)Sq * Hi;
    a.wss = w_strides2 ? (long)w_strides2[1] : (long)Hi;
    a.pool = (const unsigned char*)pool; a.table = block_table; a.tstride = (long)table_stride; a.scale = scale; a.seqused = seqused_k;
    a.logits = logits;
    a.lsb = logits_strides2 ? (long)logits_strides2[0] : (long)Sq * max_seqlen_k;
    a.lss = logits_strides2 ? (long)logits_strides2[1] : (long)max_seqlen_k;
    a.q8 = (unsigned char*)q8; a.scale_q = scale_q;
    a.Hi = Hi; a.Sq = Sq; a.N = max_seqlen_k; a.causal = is_causal ? 1 : 0; a.fill = fill_tail ? 1 : 0;
    a.num_pages = num_pages; a.page_size = page_size;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((max_seqlen_k + kWG - 1) / kWG), (unsigned)Sq, (unsigned)B), block(256);
    if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E4M3) hipLaunchKernelGGL((mla_index_scores_kernel<QATTN_FMT_E4M3, QATTN_FMT_BF16>), grid, block, 0, st, a);
    else if (in_fmt == QATTN_FMT_BF16) hipLaunchKernelGGL((mla_index_scores_kernel<QATTN_FMT_E5M2, QATTN_FMT_BF16>), grid, block, 0, st, a);
    else if (fp8_fmt == QATTN_FMT_E4M3) hipLaunchKernelGGL((mla_index_scores_kernel<QATTN_FMT_E4M3, QATTN_FMT_FP16>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((mla_index_scores_kernel<QATTN_FMT_E5M2, QATTN_FMT_FP16>), grid, block, 0, st, a);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

extern "C" int qattn_fp8_mla_index_topk(const void* q16, int in_fmt, const long long* q_strides3, const float* weights,
                                        const long long* w_strides2, const void* pool, const int* block_table, long long table_stride,
                                        int num_pages, int page_size, int max_pages, const float* scale, const int* seqused_k, int B, int Hi,
                                        int Sq, int max_seqlen_k, int topk, int fp8_fmt, int is_causal, int* indices, float* logits, void* q8,
                                        float* scale_q, void* workspace, size_t workspace_bytes, void* stream) {
    if (!indices || (size_t)indices % 4 != 0 || (size_t)workspace % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if (topk <= 0 || topk > QATTN_MLA_SPARSE_MAX_TOPK) return QATTN_ERR_INVALID_ARG;
    float* rows = logits;
    if (!rows) {
        const size_t need = qattn_fp8_mla_index_workspace_bytes(B, Sq, max_seqlen_k);
        if (!workspace || need == 0 || workspace_bytes < need) return QATTN_ERR_INVALID_ARG;
        rows = reinterpret_cast<float*>(workspace);
    }
    const int rc = qattn_fp8_mla_index_scores(q16, in_fmt, q_strides3, weights, w_strides2, pool, block_table, table_stride, num_pages, page_size,
                                              max_pages, scale, seqused_k, B, Hi, Sq, max_seqlen_k, fp8_fmt, is_causal, rows, nullptr,
                                              logits != nullptr, q8, scale_q, stream);
    if (rc != QATTN_OK) return rc;
    return qattn_mla_index_select(rows, nullptr, seqused_k, B, Sq, max_seqlen_k, topk, is_causal, indices, stream);
}

// qattn_block_sparse_fp8.hip -- qattn_fp8_block_sparse_attention_forward_fp8pv (include/qattn_block_sparse.h): block-sparse FP8 attention
// with BOTH products on the FP8 matrix pipe -- Q K^T as the 16-bit-PV entry, P.V as e4m3 P on a head-wise FP8 V.
//
// Launches, none of which reads the mask on the host:
//   quant  qattn_quant_fp8 of q (row-major), k (KFRAG; with smoothing launch_smooth_k) and v (VFRAG): head-wise over the WHOLE tensors
//   lists  block_mask_to_list128_kernel, one wave per (b, h, 128-row query block): {n, keys listed, j_0 < j_1 < ... < j_n-1}
//          (ballot + prefix popcount: no atomics, no scan)
//   attn   attn_bs_fp8_kernel, one 4-wave workgroup per (b, h, 128-row query block) at every head dimension: the FP8-PV chunk sweep of
//          qattn_fp8pv_sweep.h (shared with the packed and the sliding-window kernels) over the 64-key chunks of the block's OWN list,
//          which sits in LDS behind the ring.  This unit keeps the block map, the list and the ragged-tail mask.  A workgroup is exactly
//          one mask row, so nothing is swept for a neighbour (the 256-row workgroups of the 16-bit-PV entry sweep the union of two lists).
//          ACCURATE: one launch, exact exponentials and two-term (hi + lo) e4m3 P.  FAST: two launches -- the byte-exponential one-term
//          sweep (exact exponentials when an LSE is asked for) for the blocks that list >= kTwoTermKeys keys, the two-term sweep for the
//          rest; a workgroup whose block belongs to the other launch returns at once.
#include "qattn_fp8pv_sweep.h"
#include "../../include/qattn_block_sparse.h"

namespace qattn {

constexpr int kBsfBlock = QATTN_BLOCK_SPARSE_BLOCK;
static_assert(kBsfBlock == kFpvTile, "a workgroup is one mask block; a key block is two 64-key chunks");

struct BsfMask {
    const unsigned char* m;   // one byte per tile, 0 = off
    long s[4];                // element (= byte) strides of b, h, query block, key block (0: broadcast)
    int Hq, nqb, nkb, Skv;    // heads; 128-row query blocks and key blocks per head; keys per head
    long rows;                // B Hq nqb list rows
    int* lists;               // [rows][2 + nkb]: {n, keys, j_0 .. j_n-1}
};

// list row r = (b Hq + h) nqb + i: the key blocks j that query block i lists, ascending; keys = sum over them of min(128, Skv - 128 j)
__global__ __launch_bounds__(256) void block_mask_to_list128_kernel(const BsfMask a) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const int i = (int)(row % a.nqb);
    const long bh = row / a.nqb, b = bh / a.Hq, h = bh % a.Hq;
    const unsigned char* m0 = a.m + b * a.s[0] + h * a.s[1] + (long)i * a.s[2];
    int* out = a.lists + row * (2 + a.nkb);
    int n = 0, keys = 0;
    for (int j0 = 0; j0 < a.nkb; j0 += 64) {
        const int j = j0 + lane;
        const bool on_l = j < a.nkb && m0[(long)j * a.s[3]] != 0;
        const unsigned long long on = __ballot(on_l);
        if (on_l) out[2 + n + __popcll(on & ((1ull << lane) - 1))] = j;
        n += __popcll(on);
        keys += kBsfBlock * __popcll(on);
        if (__ballot(on_l && j == a.nkb - 1) != 0ull) keys -= a.nkb * kBsfBlock - a.Skv;   // the ragged last block
    }
    if (lane == 0) { out[0] = n; out[1] = keys; }
}

// BYTE / two: FpvSweep (qattn_fp8pv_sweep.h).  sel: the launch (kFpvSel*).  p.nqb: 128-row blocks per head; p.v / p.sv: the head-wise
// FP8 V (VFRAG) and its scales.
template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_bs_fp8_kernel(const AttnParams p, const int* lists, const int list_stride, const int two, const int sel) {
    constexpr int CH = 64 * D, MB = D / 32, KS = D / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    FpvSweep<D, FMT, BYTE> sw(smem);
    const int lane = sw.lane, wave = sw.wave, ql = sw.ql, hh = sw.hh;

    int head, qb;
    map_block(p, (int)blockIdx.x, p.nqb, false, head, qb);
    const int b = head / p.Hq, h = head % p.Hq;
    const long kv_head = (long)b * p.Hkv + h / (p.Hq / p.Hkv);
    const long bh = head;
    const int q0 = qb * kBsfBlock + wave * kQPerWave, qrow = q0 + ql;
    const int* lrow = lists + ((long)head * p.nqb + qb) * list_stride;
    const int n = __builtin_amdgcn_readfirstlane(lrow[0]);
    {   // workgroup-uniform: the launch this block belongs to
        const int keys = __builtin_amdgcn_readfirstlane(lrow[1]);
        if (sel == kFpvSelMany && keys < p.two_term_keys) return;
        if (sel == kFpvSelFew && keys >= p.two_term_keys) return;
    }
    if (n == 0) {   // a query block that lists nothing
        fpv_store_empty<D>(p.out, p.out_fmt, out_row_offset(p, bh, qrow, MB * 64), p.lse, bh * p.lse_stride + qrow, p.path, bh * p.Sq + qrow, hh, qrow < p.Sq);
        return;
    }
    // 64-key chunks to sweep: two per listed block, one for a last key block of at most 64 keys (ascending: it can only be the last entry)
    const int nkb = (p.nchunks + 1) >> 1;
    const int last = __builtin_amdgcn_readfirstlane(lrow[1 + n]);
    const int n_wg = 2 * n - ((last == nkb - 1 && (p.nchunks & 1)) ? 1 : 0);

    FpvRing<D> ring(smem, wave, lane, p.k + kv_head * (long)p.nchunks * CH + (wave << 10), p.v + kv_head * (long)p.nchunks * CH + (wave << 10));
    // the block's list, behind the ring and the Q slots (requested before the first DMA: the wait for these loads does not wait for it)
    int* lst = reinterpret_cast<int*>(smem + fpv_lds_bytes(D));
    for (int i = (int)threadIdx.x; i < n; i += kFpvWaves * 64) lst[i] = lrow[2 + i];
    int cur = 2 * __builtin_amdgcn_readfirstlane(lrow[2]);   // chunk of step 0
    ring.dma_chunk(cur);
    {
        const bool qvalid = qrow < p.Sq;
        sw.park_q(p.q + (bh * p.Sq + (qvalid ? qrow : 0)) * D + hh * 32, qvalid);
    }
    lds_barrier();   // the list is in LDS
    sw.init_state(p.sm_log2e * p.sq[bh] * p.sk[kv_head], -1.0e30f);
    const v8i ones = fpv_ones(lane);

    for (int t = 0; t < n_wg; t++) {
        v8i qf[KS];
        sw.read_q(qf);
        int nxt = 0;   // chunk of step t + 1 (workgroup-uniform)
        if (t + 1 < n_wg) nxt = __builtin_amdgcn_readfirstlane(2 * lst[(t + 1) >> 1] + ((t + 1) & 1));
        sw.wait_stage();
        if (t + 1 < n_wg) ring.dma_chunk(nxt);
        v16f s0, s1;
        v8i vf0, vf1;
        sw.qk(t, qf, s0, s1, vf0, vf1);
        // ---- ragged tail of the key sequence
        const int k0 = cur * 64;
        cur = nxt;
        if (__builtin_expect(k0 + 64 > p.Skv, 0)) {
#pragma unroll
            for (int r = 0; r < 32; r++) {
                const int key = k0 + 32 * (r >> 4) + (r & 3) + 8 * ((r & 15) >> 2) + 4 * hh;
                v16f& sx = (r >> 4) ? s1 : s0;
                sx[r & 15] = key >= p.Skv ? -INFINITY : sx[r & 15];
            }
        }
        sw.softmax_pv(s0, s1, vf0, vf1, two, [&] { return ones; });
    }

    // ---- epilogue (V's one scale per head is applied here)
    const float l_tot = sw.row_sum();
    const float inv = p.sv[kv_head] / l_tot;
    store_o_rows<MB>(p.out, p.out_fmt, sw.o, inv, out_row_offset(p, bh, qrow, MB * 64), hh, qrow < p.Sq);
    if (!BYTE && p.lse && hh == 0 && qrow < p.Sq) p.lse[bh * p.lse_stride + qrow] = 0.6931471805599453f * (sw.m_run * sw.c - kPShift) + __logf(l_tot);
    if (p.path && hh == 0 && qrow < p.Sq) p.path[bh * p.Sq + qrow] = (unsigned char)((!BYTE && two) ? QATTN_PATH_TWO_TERM : QATTN_PATH_ONE_TERM);
}

// LDS of the attention kernel: the K / V ring, the parked Q^T fragments, then the block's list
inline size_t bsf_lds_bytes(int D, int nkb) { return (size_t)fpv_lds_bytes(D) + ((size_t)4 * nkb + 15) / 16 * 16; }
constexpr size_t kBsfMaxLds = 160 * 1024;

template <int D, int FMT>
static int launch_bsf_fmt(const AttnParams& p, const int* lists, int list_stride, int nkb, int precision, hipStream_t st) {
    // (Skv: the most keys a block can list)
    return fpv_precision_ladder(precision, p.Skv, p.two_term_keys, p.lse != nullptr, [&](auto byte, int two, int sel) {
        return fpv_launch(attn_bs_fp8_kernel<D, FMT, decltype(byte)::value>, (unsigned)(p.B * p.Hq * p.nqb), bsf_lds_bytes(D, nkb), st, p, lists,
                          list_stride, two, sel);
    });
}

template <int D>
static int launch_bsf_d(const AttnParams& p, const int* lists, int list_stride, int nkb, int fp8_fmt, int precision, hipStream_t st) {
    return fp8_fmt == QATTN_FMT_E4M3 ? launch_bsf_fmt<D, QATTN_FMT_E4M3>(p, lists, list_stride, nkb, precision, st)
                                     : launch_bsf_fmt<D, QATTN_FMT_E5M2>(p, lists, list_stride, nkb, precision, st);
}

}  // namespace qattn

using namespace qattn;

namespace {
bool bsf_dims_ok(int B, int Hq, int Hkv, int Sq, int Skv) { return B > 0 && Hq > 0 && Hkv > 0 && Sq > 0 && Skv > 0; }
size_t bsf_quant_ws_bytes(int B, int Hq, int Hkv, int Sq, int Skv, int D) {
    const size_t a = qattn_quant_workspace_bytes(B, Hq, Sq, D, QATTN_SCALE_HEAD), b = qattn_quant_workspace_bytes(B, Hkv, Skv, D, QATTN_SCALE_HEAD);
    return a > b ? a : b;   // (the pre-pass calls run one after the other on the stream)
}
size_t bsf_list_bytes(int B, int Hq, int Sq, int Skv) {
    return sizeof(int) * (size_t)B * Hq * ceil_div(Sq, kBsfBlock) * (2 + (size_t)ceil_div(Skv, kBsfBlock));
}
}  // namespace

extern "C" size_t qattn_fp8_block_sparse_attention_fp8pv_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Skv, int D) {
    if (!bsf_dims_ok(B, Hq, Hkv, Sq, Skv) || (D != 64 && D != 128 && D != 256)) return 0;
    // [q8 (unless the caller passes one) | k8 KFRAG | v8 VFRAG | scale_q | scale_k | scale_v | pre-pass words | key-block lists]
    return up256(qattn_fp8_tensor_bytes(QATTN_LAYOUT_ROWMAJOR, B, Hq, Sq, D)) + up256(qattn_fp8_tensor_bytes(QATTN_LAYOUT_KFRAG, B, Hkv, Skv, D)) +
           up256(qattn_fp8_tensor_bytes(QATTN_LAYOUT_VFRAG, B, Hkv, Skv, D)) + up256(sizeof(float) * (size_t)B * Hq) +
           2 * up256(sizeof(float) * (size_t)B * Hkv) + up256(bsf_quant_ws_bytes(B, Hq, Hkv, Sq, Skv, D)) + up256(bsf_list_bytes(B, Hq, Sq, Skv));
}

extern "C" size_t qattn_fp8_block_sparse_attention_fp8pv_smooth_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Skv, int D) {
    const size_t plain = qattn_fp8_block_sparse_attention_fp8pv_workspace_bytes(B, Hq, Hkv, Sq, Skv, D);
    // [the plain workspace | per-block channel sums of the mean pass]
    return plain ? up256(plain) + smooth_k_workspace_bytes(B, Hkv, D) : 0;
}

extern "C" int qattn_fp8_block_sparse_attention_forward_fp8pv(const void* q, const void* k, const void* v, int in_fmt, void* out, float* lse,
                                                              const void* block_mask, const long long* mask_strides, int B, int Hq, int Hkv,
                                                              int Sq, int Skv, int D, int fp8_fmt, int numerics, float sm_scale, int precision,
                                                              void* q8, void* k8, void* v8, float* scale_q, float* scale_k, float* scale_v,
                                                              unsigned char* row_path, float* k_mean, void* workspace, size_t workspace_bytes,
                                                              void* stream) {
    if (!q || !k || !v || !out || !block_mask) return QATTN_ERR_INVALID_ARG;
    if (!bsf_dims_ok(B, Hq, Hkv, Sq, Skv)) return QATTN_ERR_INVALID_ARG;
    if ((D != 64 && D != 128 && D != 256) || Hq % Hkv != 0) return QATTN_ERR_UNSUPPORTED_DIM;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (numerics != QATTN_NUMERICS_COMPILED && numerics != QATTN_NUMERICS_EAGER) return QATTN_ERR_INVALID_ARG;
    if (precision != QATTN_PRECISION_FAST && precision != QATTN_PRECISION_ACCURATE) return QATTN_ERR_INVALID_ARG;
    const int nqb = ceil_div(Sq, kBsfBlock), nkb = ceil_div(Skv, kBsfBlock);
    long long ms[4] = {(long long)Hq * nqb * nkb, (long long)nqb * nkb, nkb, 1};   // dense [B, Hq, nqb, nkb]
    if (mask_strides)
        for (int s = 0; s < 4; s++) {
            if (mask_strides[s] < 0) return QATTN_ERR_INVALID_ARG;
            ms[s] = mask_strides[s];
        }
    if (((size_t)q | (size_t)k | (size_t)v | (size_t)out) % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if ((long long)B * Hq * nqb > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (one workgroup per list row: a 32-bit grid)
    if (bsf_lds_bytes(D, nkb) > kBsfMaxLds) return QATTN_ERR_UNSUPPORTED_DIM;      // (the list lives behind the ring and the Q slots in LDS)
    const bool smooth = k_mean != nullptr;
    if (smooth && (reinterpret_cast<uintptr_t>(k_mean) & 15u) != 0) return QATTN_ERR_INVALID_ARG;
    const size_t plain_bytes = qattn_fp8_block_sparse_attention_fp8pv_workspace_bytes(B, Hq, Hkv, Sq, Skv, D);
    if (!workspace || workspace_bytes < (smooth ? qattn_fp8_block_sparse_attention_fp8pv_smooth_workspace_bytes(B, Hq, Hkv, Sq, Skv, D) : plain_bytes))
        return QATTN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)workspace;
    unsigned char* q8w = w;   w += up256(qattn_fp8_tensor_bytes(QATTN_LAYOUT_ROWMAJOR, B, Hq, Sq, D));
    unsigned char* kfrag = w; w += up256(qattn_fp8_tensor_bytes(QATTN_LAYOUT_KFRAG, B, Hkv, Skv, D));
    unsigned char* vfrag = w; w += up256(qattn_fp8_tensor_bytes(QATTN_LAYOUT_VFRAG, B, Hkv, Skv, D));
    float* sqw = (float*)w;   w += up256(sizeof(float) * (size_t)B * Hq);
    float* skw = (float*)w;   w += up256(sizeof(float) * (size_t)B * Hkv);
    float* svw = (float*)w;   w += up256(sizeof(float) * (size_t)B * Hkv);
    void* qws = w;            const size_t qws_bytes = bsf_quant_ws_bytes(B, Hq, Hkv, Sq, Skv, D);
    w += up256(qws_bytes);
    int* lists = (int*)w;
    unsigned char* q8p = q8 ? (unsigned char*)q8 : q8w;
    float* sq = scale_q ? scale_q : sqw;
    float* sk = scale_k ? scale_k : skw;
    float* sv = scale_v ? scale_v : svw;
    int rc = qattn_quant_fp8(q, in_fmt, q8p, sq, B, Hq, Sq, D, fp8_fmt, QATTN_SCALE_HEAD, numerics, QATTN_LAYOUT_ROWMAJOR, qws, qws_bytes, stream);
    if (rc != QATTN_OK) return rc;
    if (smooth) {   // mean over the whole Skv, then K's abs-max words (where the pre-pass would leave them) and quantise pass on k - mean
        if (k8) kfrag = (unsigned char*)k8;
        rc = launch_smooth_k(k, in_fmt, kfrag, sk, k_mean, B, Hkv, Skv, D, fp8_fmt, QATTN_SCALE_HEAD, numerics, (unsigned*)qws, nullptr,
                             amax_splits(Skv, Skv, D), reinterpret_cast<float*>((unsigned char*)workspace + up256(plain_bytes)), st, nullptr);
    } else {
        rc = qattn_quant_fp8(k, in_fmt, kfrag, sk, B, Hkv, Skv, D, fp8_fmt, QATTN_SCALE_HEAD, numerics, QATTN_LAYOUT_KFRAG, qws, qws_bytes, stream);
    }
    if (rc != QATTN_OK) return rc;
    if (k8 && !smooth) {   // (the row-major k8 on request: the same bytes, in the other order)
        rc = qattn_quant_fp8(k, in_fmt, k8, sk, B, Hkv, Skv, D, fp8_fmt, QATTN_SCALE_HEAD, numerics, QATTN_LAYOUT_ROWMAJOR, qws, qws_bytes, stream);
        if (rc != QATTN_OK) return rc;
    }
    rc = qattn_quant_fp8(v, in_fmt, vfrag, sv, B, Hkv, Skv, D, fp8_fmt, QATTN_SCALE_HEAD, numerics, QATTN_LAYOUT_VFRAG, qws, qws_bytes, stream);
    if (rc != QATTN_OK) return rc;
    if (v8) {   // (row-major on request, as k8)
        rc = qattn_quant_fp8(v, in_fmt, v8, sv, B, Hkv, Skv, D, fp8_fmt, QATTN_SCALE_HEAD, numerics, QATTN_LAYOUT_ROWMAJOR, qws, qws_bytes, stream);
        if (rc != QATTN_OK) return rc;
    }
    BsfMask bm;
    bm.m = (const unsigned char*)block_mask;
    for (int s = 0; s < 4; s++) bm.s[s] = (long)ms[s];
    bm.Hq = Hq; bm.nqb = nqb; bm.nkb = nkb; bm.Skv = Skv;
    bm.rows = (long)B * Hq * nqb;
    bm.lists = lists;
    hipLaunchKernelGGL(block_mask_to_list128_kernel, dim3((unsigned)((bm.rows + 3) / 4)), dim3(256), 0, st, bm);
    AttnParams p;
    __builtin_memset(&p, 0, sizeof(p));
    p.q = q8p; p.k = kfrag; p.v = vfrag; p.sq = sq; p.sk = sk; p.sv = sv;
    p.B = B; p.Hq = Hq; p.Hkv = Hkv; p.Sq = Sq; p.Skv = Skv;
    p.nqb = nqb;
    p.nchunks = ceil_div(Skv, 64);
    p.out = out; p.out_fmt = in_fmt;
    p.xcd_remap = ((B * Hq) % 8 == 0 && xcd_count() == 8) ? 1 : 0;   // (as attention_impl: the maps of qattn_attn.h are written for 8 XCDs)
    p.causal_group = 1;
    const float sm = sm_scale > 0.0f ? sm_scale : 1.0f / sqrtf((float)D);
    p.sm_log2e = sm * 1.4426950408889634f;
    p.precision = precision;
    p.two_term_keys = kTwoTermKeys;
    p.lse = lse; p.lse_stride = Sq; p.lse_mul = 1.0f;
    p.path = row_path;
    p.o_rs = 2L * D; p.o_hs = p.o_rs * Sq; p.o_bs = p.o_hs * Hq;
    const int list_stride = 2 + nkb;
    if (D == 64) rc = launch_bsf_d<64>(p, lists, list_stride, nkb, fp8_fmt, precision, st);
    else if (D == 128) rc = launch_bsf_d<128>(p, lists, list_stride, nkb, fp8_fmt, precision, st);
    else rc = launch_bsf_d<256>(p, lists, list_stride, nkb, fp8_fmt, precision, st);
    if (rc != QATTN_OK) return rc;
    if (hipGetLastError() != hipSuccess) return QATTN_ERR_LAUNCH;
    if (!smooth || !lse) return QATTN_OK;
    // the launch wrote the LSE of the smoothed scores; the true scores of row i lie sm_scale * q_i.m higher (-inf rows stay -inf)
    return launch_smooth_lse(q, in_fmt, k_mean, lse, (long)Sq, B, Hq, Hkv, Sq, D, sm, st, nullptr);
}

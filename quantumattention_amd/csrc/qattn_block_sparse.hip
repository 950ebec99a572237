// qattn_block_sparse.hip -- qattn_fp8_block_sparse_attention_forward (include/qattn_block_sparse.h): FP8 attention over the 128 x 128 tiles
// that a boolean block mask turns on, with the reference kernel's own P.V numerics (16-bit P on the original 16-bit V).
//
// Four launches, none of which reads the mask on the host:
//   quant  qattn_quant_fp8 of q (row-major) and of k (KFRAG): the head-wise pre-pass over the WHOLE tensors (the bytes and scales of
//          dynamically_quantize_fp8(x, reduction_dim=[2, 3]))
//   lists  block_mask_to_list_kernel, one wave per (b, h, 256-row query block): the ascending list of the key blocks that either of the
//          block's two 128-row halves lists, each entry tagged with the halves that list it (ballot + prefix popcount: no atomics, no scan)
//   attn   one workgroup per (b, h, 256-row query block): pv16_block_pass (qattn_pv16.h) with SPARSE on, in the loop form of the whole-
//          tensor launch (launch_one, qattn_attn_pv16.hip: the two-group loop at D = 128) -- each wave's bits are those of the dense pass
//          on its own listed keys, gathered
// Built with strided addressing (QATTN_STRIDED16 = 1), as the varlen unit; the strides passed are the dense ones.
#include "qattn_pv16.h"
#include "../../include/qattn_block_sparse.h"

namespace qattn {

static_assert(kStrided16, "the block-sparse unit is built like the varlen unit: V and the output through strides");

constexpr int kBsBlock = QATTN_BLOCK_SPARSE_BLOCK;
static_assert(2 * kBsBlock == kQPerWG && kBsBlock == 4 * kQPerWave, "a workgroup's 256 rows are two mask blocks of four waves each");

struct BsMask {
    const unsigned char* m;   // one byte per tile, 0 = off
    long s[4];                // element (= byte) strides of b, h, query block, key block (0: broadcast)
    int Hq, nqb, nkb, nwg;    // heads; 128-row query blocks, key blocks and 256-row query blocks per head
    long rows;                // B Hq nwg list rows
    int* lists;               // [rows][1 + nkb]: {n, e_0 .. e_n-1}
};

// list row r = (b Hq + h) nwg + w: the key blocks j that query block 2 w or 2 w + 1 lists, ascending, entry (j << 2) | bit 0 (2 w lists j)
// | bit 1 (2 w + 1 lists j; never set beyond the last query block)
__global__ __launch_bounds__(256) void block_mask_to_list_kernel(const BsMask a) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const int w = (int)(row % a.nwg);
    const long bh = row / a.nwg, b = bh / a.Hq, h = bh % a.Hq;
    const unsigned char* m0 = a.m + b * a.s[0] + h * a.s[1] + (long)(2 * w) * a.s[2];
    const bool has1 = 2 * w + 1 < a.nqb;
    int* out = a.lists + row * (1 + a.nkb);
    int n = 0;
    for (int j0 = 0; j0 < a.nkb; j0 += 64) {
        const int j = j0 + lane;
        int bits = 0;
        if (j < a.nkb) {
            const unsigned char* mj = m0 + (long)j * a.s[3];
            bits = (mj[0] != 0 ? 1 : 0) | (has1 && mj[a.s[2]] != 0 ? 2 : 0);
        }
        const unsigned long long on = __ballot(bits != 0);
        if (bits) out[1 + n + __popcll(on & ((1ull << lane) - 1))] = (j << 2) | bits;
        n += __popcll(on);
    }
    if (lane == 0) out[0] = n;
}

// PP: the two-group loop, as launch_one picks it for a whole-tensor launch (D = 128); else the one-group loop with three stages
template <int D, int QK_FMT, int V16_FMT, bool PP>
__global__ __launch_bounds__(kThreads, 2) void attn_pv16_block_sparse_kernel(const AttnParams p, const int* lists, int list_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int head, qb;
    map_block(p, (int)blockIdx.x, p.nqb, false, head, qb);   // (the dense launch's order: every XCD a contiguous range of heads)
    pv16_block_pass<D, kWaves, QK_FMT, V16_FMT, false, false, false, PP ? 4 : 3, PP, true, true>(
        p, smem, (int)threadIdx.x, head, []() { return 0u; }, [](unsigned) {}, qb, lists + ((long)head * p.nqb + qb) * list_stride);
}

// LDS of the attention kernel: the K / V ring, then the workgroup's list (nkb entries and one word of slack)
constexpr int bs_ring_bytes(int D) { return (D == 128 ? 4 : 3) * (64 * D + 64 * D * 2); }
inline size_t bs_lds_bytes(int D, int nkb) { return (size_t)bs_ring_bytes(D) + ((size_t)4 * (nkb + 1) + 15) / 16 * 16; }
constexpr size_t kBsMaxLds = 160 * 1024;

template <int D, int QK_FMT, int V16_FMT>
static int launch_bs_attn(const AttnParams& p, const int* lists, int list_stride, int nkb, hipStream_t st) {
    constexpr bool PP = D == 128;   // (ring: NS = 4 stages with the two-group loop, else 3 -- bs_ring_bytes)
    const int lds = (int)bs_lds_bytes(D, nkb);
    auto kern = attn_pv16_block_sparse_kernel<D, QK_FMT, V16_FMT, PP>;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return QATTN_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3((unsigned)(p.B * p.Hq * p.nqb)), dim3(kThreads), lds, st, p, lists, list_stride);
    return QATTN_OK;
}
template <int D>
static int launch_bs_d(const AttnParams& p, const int* lists, int list_stride, int nkb, int qk_fmt, int v16_fmt, hipStream_t st) {
    if (qk_fmt == QATTN_FMT_E4M3)
        return v16_fmt == QATTN_FMT_BF16 ? launch_bs_attn<D, QATTN_FMT_E4M3, QATTN_FMT_BF16>(p, lists, list_stride, nkb, st)
                                         : launch_bs_attn<D, QATTN_FMT_E4M3, QATTN_FMT_FP16>(p, lists, list_stride, nkb, st);
    return v16_fmt == QATTN_FMT_BF16 ? launch_bs_attn<D, QATTN_FMT_E5M2, QATTN_FMT_BF16>(p, lists, list_stride, nkb, st)
                                     : launch_bs_attn<D, QATTN_FMT_E5M2, QATTN_FMT_FP16>(p, lists, list_stride, nkb, st);
}

}  // namespace qattn

using namespace qattn;

namespace {
size_t up256(size_t x) { return (x + 255) / 256 * 256; }
bool bs_dims_ok(int B, int Hq, int Hkv, int Sq, int Skv) { return B > 0 && Hq > 0 && Hkv > 0 && Sq > 0 && Skv > 0; }
size_t bs_quant_ws_bytes(int B, int Hq, int Hkv, int Sq, int Skv, int D) {
    const size_t a = qattn_quant_workspace_bytes(B, Hq, Sq, D, QATTN_SCALE_HEAD), b = qattn_quant_workspace_bytes(B, Hkv, Skv, D, QATTN_SCALE_HEAD);
    return a > b ? a : b;   // (the two pre-pass calls run one after the other on the stream)
}
size_t bs_list_bytes(int B, int Hq, int Sq, int Skv) {
    return sizeof(int) * (size_t)B * Hq * ceil_div(Sq, kQPerWG) * (1 + (size_t)ceil_div(Skv, kBsBlock));
}
}  // namespace

extern "C" size_t qattn_fp8_block_sparse_attention_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Skv, int D) {
    if (!bs_dims_ok(B, Hq, Hkv, Sq, Skv) || (D != 64 && D != 128 && D != 256)) return 0;
    // [q8 (unless the caller passes one) | k8 KFRAG | scale_q | scale_k | pre-pass words | key-block lists]
    return up256(qattn_fp8_tensor_bytes(QATTN_LAYOUT_ROWMAJOR, B, Hq, Sq, D)) + up256(qattn_fp8_tensor_bytes(QATTN_LAYOUT_KFRAG, B, Hkv, Skv, D)) +
           up256(sizeof(float) * (size_t)B * Hq) + up256(sizeof(float) * (size_t)B * Hkv) + up256(bs_quant_ws_bytes(B, Hq, Hkv, Sq, Skv, D)) +
           up256(bs_list_bytes(B, Hq, Sq, Skv));
}

extern "C" size_t qattn_fp8_block_sparse_attention_smooth_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Skv, int D) {
    const size_t plain = qattn_fp8_block_sparse_attention_workspace_bytes(B, Hq, Hkv, Sq, Skv, D);
    // [the plain entry's workspace | per-block channel sums of the mean pass]
    return plain ? up256(plain) + smooth_k_workspace_bytes(B, Hkv, D) : 0;
}

// k_mean != nullptr: key smoothing (include/qattn_smooth.h) -- K goes through launch_smooth_k instead of its share of the pre-pass, and k8
// (when asked for) is the KFRAG image the attention kernel reads
static int block_sparse_forward_impl(const void* q, const void* k, const void* v, int in_fmt, void* out, float* lse, const void* block_mask,
                                     const long long* mask_strides, int B, int Hq, int Hkv, int Sq, int Skv, int D, int fp8_fmt, int numerics,
                                     float sm_scale, void* q8, void* k8, float* scale_q, float* scale_k, void* workspace, size_t workspace_bytes,
                                     void* stream, float* k_mean) {
    if (!q || !k || !v || !out || !block_mask) return QATTN_ERR_INVALID_ARG;
    if (!bs_dims_ok(B, Hq, Hkv, Sq, Skv)) return QATTN_ERR_INVALID_ARG;
    if ((D != 64 && D != 128 && D != 256) || Hq % Hkv != 0) return QATTN_ERR_UNSUPPORTED_DIM;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (numerics != QATTN_NUMERICS_COMPILED && numerics != QATTN_NUMERICS_EAGER) return QATTN_ERR_INVALID_ARG;
    const int nqb = ceil_div(Sq, kBsBlock), nkb = ceil_div(Skv, kBsBlock), nwg = ceil_div(Sq, kQPerWG);
    long long ms[4] = {(long long)Hq * nqb * nkb, (long long)nqb * nkb, nkb, 1};   // dense [B, Hq, nqb, nkb]
    if (mask_strides)
        for (int s = 0; s < 4; s++) {
            if (mask_strides[s] < 0) return QATTN_ERR_INVALID_ARG;
            ms[s] = mask_strides[s];
        }
    if (((size_t)q | (size_t)k | (size_t)v | (size_t)out) % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if ((long long)B * Hq * nwg > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (one workgroup per list row: a 32-bit grid)
    if (bs_lds_bytes(D, nkb) > kBsMaxLds) return QATTN_ERR_UNSUPPORTED_DIM;        // (the list lives behind the ring in LDS)
    const bool smooth = k_mean != nullptr;
    if (smooth && (reinterpret_cast<uintptr_t>(k_mean) & 15u) != 0) return QATTN_ERR_INVALID_ARG;
    const size_t plain_bytes = qattn_fp8_block_sparse_attention_workspace_bytes(B, Hq, Hkv, Sq, Skv, D);
    if (!workspace || workspace_bytes < (smooth ? qattn_fp8_block_sparse_attention_smooth_workspace_bytes(B, Hq, Hkv, Sq, Skv, D) : plain_bytes))
        return QATTN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)workspace;
    unsigned char* q8w = w;   w += up256(qattn_fp8_tensor_bytes(QATTN_LAYOUT_ROWMAJOR, B, Hq, Sq, D));
    unsigned char* kfrag = w; w += up256(qattn_fp8_tensor_bytes(QATTN_LAYOUT_KFRAG, B, Hkv, Skv, D));
    float* sqw = (float*)w;   w += up256(sizeof(float) * (size_t)B * Hq);
    float* skw = (float*)w;   w += up256(sizeof(float) * (size_t)B * Hkv);
    void* qws = w;            const size_t qws_bytes = bs_quant_ws_bytes(B, Hq, Hkv, Sq, Skv, D);
    w += up256(qws_bytes);
    int* lists = (int*)w;
    unsigned char* q8p = q8 ? (unsigned char*)q8 : q8w;
    float* sq = scale_q ? scale_q : sqw;
    float* sk = scale_k ? scale_k : skw;
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
    BsMask bm;
    bm.m = (const unsigned char*)block_mask;
    for (int s = 0; s < 4; s++) bm.s[s] = (long)ms[s];
    bm.Hq = Hq; bm.nqb = nqb; bm.nkb = nkb; bm.nwg = nwg;
    bm.rows = (long)B * Hq * nwg;
    bm.lists = lists;
    hipLaunchKernelGGL(block_mask_to_list_kernel, dim3((unsigned)((bm.rows + 3) / 4)), dim3(256), 0, st, bm);
    AttnParams p;
    __builtin_memset(&p, 0, sizeof(p));
    p.q = q8p; p.k = kfrag; p.sq = sq; p.sk = sk;
    p.B = B; p.Hq = Hq; p.Hkv = Hkv; p.Sq = Sq; p.Skv = Skv;
    p.nqb = nwg;
    p.nchunks = ceil_div(Skv, 64);
    p.out = out; p.out_fmt = in_fmt;
    p.xcd_remap = ((B * Hq) % 8 == 0 && xcd_count() == 8) ? 1 : 0;   // (as attention_impl: the maps of qattn_attn.h are written for 8 XCDs)
    p.causal_group = 1;
    const float sm = sm_scale > 0.0f ? sm_scale : 1.0f / sqrtf((float)D);
    p.sm_log2e = sm * 1.4426950408889634f;
    p.lse = lse; p.lse_stride = Sq; p.lse_mul = 1.0f;
    p.v16 = (const unsigned char*)v;
    p.v16_rs = 2L * D; p.v16_hs = p.v16_rs * Skv; p.v16_bs = p.v16_hs * Hkv;
    p.o_rs = 2L * D; p.o_hs = p.o_rs * Sq; p.o_bs = p.o_hs * Hq;
    const int list_stride = 1 + nkb;
    if (D == 64) rc = launch_bs_d<64>(p, lists, list_stride, nkb, fp8_fmt, in_fmt, st);
    else if (D == 128) rc = launch_bs_d<128>(p, lists, list_stride, nkb, fp8_fmt, in_fmt, st);
    else rc = launch_bs_d<256>(p, lists, list_stride, nkb, fp8_fmt, in_fmt, st);
    if (rc != QATTN_OK) return rc;
    if (hipGetLastError() != hipSuccess) return QATTN_ERR_LAUNCH;
    if (!smooth || !lse) return QATTN_OK;
    // the launch wrote the LSE of the smoothed scores; the true scores of row i lie sm_scale * q_i.m higher (-inf rows stay -inf)
    return launch_smooth_lse(q, in_fmt, k_mean, lse, (long)Sq, B, Hq, Hkv, Sq, D, sm, st, nullptr);
}

extern "C" int qattn_fp8_block_sparse_attention_forward(const void* q, const void* k, const void* v, int in_fmt, void* out, float* lse,
                                                        const void* block_mask, const long long* mask_strides, int B, int Hq, int Hkv, int Sq,
                                                        int Skv, int D, int fp8_fmt, int numerics, float sm_scale, void* q8, void* k8,
                                                        float* scale_q, float* scale_k, void* workspace, size_t workspace_bytes, void* stream) {
    return block_sparse_forward_impl(q, k, v, in_fmt, out, lse, block_mask, mask_strides, B, Hq, Hkv, Sq, Skv, D, fp8_fmt, numerics, sm_scale, q8, k8,
                                     scale_q, scale_k, workspace, workspace_bytes, stream, nullptr);
}

// The block-sparse entry with key smoothing (include/qattn_block_sparse.h; the idea: include/qattn_smooth.h): K is quantised as fp32(k) - its channel mean over the WHOLE Skv.
extern "C" int qattn_fp8_block_sparse_attention_forward_smooth(const void* q, const void* k, const void* v, int in_fmt, void* out, float* lse,
                                                               const void* block_mask, const long long* mask_strides, int B, int Hq, int Hkv,
                                                               int Sq, int Skv, int D, int fp8_fmt, int numerics, float sm_scale, void* q8, void* k8,
                                                               float* scale_q, float* scale_k, void* workspace, size_t workspace_bytes, void* stream,
                                                               float* k_mean) {
    if (!k_mean) return QATTN_ERR_INVALID_ARG;
    return block_sparse_forward_impl(q, k, v, in_fmt, out, lse, block_mask, mask_strides, B, Hq, Hkv, Sq, Skv, D, fp8_fmt, numerics, sm_scale, q8, k8,
                                     scale_q, scale_k, workspace, workspace_bytes, stream, k_mean);
}

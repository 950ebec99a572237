// qattn_paged_varlen_attn.h -- the host driver of the packed paged split-KV entries (include/qattn_paged_varlen.h): the workspace plan, the
// argument checks, the packed q pre-pass, the launch ladder, the merge chain and the path launch.  Shared by
// qattn_fp8_attention_paged_varlen_forward (qattn_paged_varlen_splitkv_fp8.hip) and its sibling under a sliding window,
// qattn_fp8_attention_paged_varlen_window_forward (qattn_paged_varlen_splitkv_window_fp8.hip, include/qattn_splitkv_window.h); each unit
// instantiates its own kernels only.
#pragma once
#include "qattn_splitkv_attn.h"
#include "qattn_varlen_attn.h"
#include "../../include/qattn_paged_varlen.h"

namespace qattn {

// the sections of the workspace, in order (each up256)
struct PvqWs {
    size_t q8, sq, amax, po, plse, ppath, acc, acc_lse;
    size_t total() const { return q8 + sq + amax + po + plse + ppath + acc + acc_lse; }
};
inline PvqWs pvq_ws(int B, int Hq, int total_q, int D, int ns) {
    const size_t rows = (size_t)Hq * total_q;
    PvqWs w = {};
    w.q8 = up256(rows * D);
    w.sq = up256(sizeof(float) * (size_t)B * Hq);
    w.amax = up256(sizeof(unsigned) * (size_t)B * Hq);
    if (ns > 1) {
        w.po = up256(sizeof(float) * ns * rows * D);
        w.plse = up256(sizeof(float) * ns * rows);
        w.ppath = up256((size_t)ns * rows);
    }
    if (ns > QATTN_MERGE_MAX_PARTIALS) {
        w.acc = up256(sizeof(float) * rows * D);
        w.acc_lse = up256(sizeof(float) * rows);
    }
    return w;
}

inline bool pvq_dims_ok(int B, int Hq, int Hkv, int total_q, int Skv, int D) {
    return B > 0 && Hq > 0 && Hkv > 0 && total_q >= 0 && Skv > 0 && skv_d_ok(D) && Hq % Hkv == 0 && (long long)(Hq / Hkv) * total_q <= 0x7fffffffLL;
}
// (0: the auto rule never picks more splits than key blocks)
inline int pvq_most_splits(int Skv, int num_splits) {
    const int nkb = ceil_div(Skv, 128);
    return num_splits > 0 ? num_splits : (nkb < QATTN_SPLITKV_MAX_SPLITS ? nkb : QATTN_SPLITKV_MAX_SPLITS);
}


// WINDOW: the window kernel under (window_left, window_right) in is_causal's place -- also for (-1, 0) and (-1, -1).
// SINK (with WINDOW; include/qattn_sinks.h): the sink kernel with `sinks` fp32 [Hq], as skv_forward.
// TREE (without WINDOW; include/qattn_paged_varlen_tree.h): the tree kernel under `tree_mask`, one 64-bit word per packed token on the
// device; the call is causal whatever is_causal says.
// TREE with WINDOW, and with SINK (include/qattn_paged_varlen_tree_window.h): the tree over the window kernel, for windows (left, 0) with
// left = -1 or left >= 63; the split plan, the num_splits = 0 rule and the merge chain are the window / sink entry's.
// SOFTCAP (with WINDOW, without SINK and TREE; include/qattn_softcap.h): the soft-cap kernel under the host float `softcap`, as skv_forward.
template <bool WINDOW, bool SINK = false, bool TREE = false, bool SOFTCAP = false>
int pvq_forward(const void* q16, const long long* q_strides2, int in_fmt, const void* k_pool, const void* v_pool, const int* block_table,
                long long table_stride, int num_pages, int page_size, int max_pages, const float* scale_k, const float* scale_v, void* out,
                float* lse, const int* cu_seqlens_q, const int* seqused_k, int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int Skv, int D,
                int fp8_fmt, int numerics, int is_causal, int window_left, int window_right, float sm_scale, int precision, int num_splits,
                void* q8, float* scale_q, unsigned char* row_path, float* partial_o, float* partial_lse, unsigned char* partial_path,
                void* workspace, size_t workspace_bytes, void* stream, const float* sinks = nullptr,
                const unsigned long long* tree_mask = nullptr, float softcap = 0.0f) {
    static_assert(WINDOW || !SINK, "the sink kernel is a window kernel");
    static_assert(!SOFTCAP || (WINDOW && !SINK && !TREE), "the soft-cap kernel is the window kernel without a sink or a tree");
    if (SOFTCAP && !skv_softcap_ok(softcap)) return QATTN_ERR_INVALID_ARG;
    if (TREE && (!tree_mask || (size_t)tree_mask % 8 != 0)) return QATTN_ERR_INVALID_ARG;
    // a tree under a window (include/qattn_paged_varlen_tree_window.h): causal, and a window that holds every ancestor of a draft token
    if (TREE && WINDOW && (window_right != 0 || (window_left != -1 && window_left < 63))) return QATTN_ERR_INVALID_ARG;
    if (WINDOW && (window_left < -1 || window_right < -1)) return QATTN_ERR_INVALID_ARG;
    if (SINK && (!sinks || (size_t)sinks % 4 != 0)) return QATTN_ERR_INVALID_ARG;
    // ---- the paging arguments, as qattn_fp8_attention_paged_splitkv_forward
    if (!block_table || !seqused_k || (size_t)block_table % 4 != 0) return QATTN_ERR_INVALID_ARG;
    if (num_pages <= 0 || max_pages <= 0 || Hkv <= 0 || page_size < 64 || page_size % 64 != 0) return QATTN_ERR_INVALID_ARG;
    if (table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    const int pc = page_size / 64;
    if ((long long)num_pages * Hkv * pc > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (the physical chunk index is an int)
    if ((long long)Skv > (long long)max_pages * page_size) return QATTN_ERR_INVALID_ARG;
    // ---- the packed queries
    if (!cu_seqlens_q || (size_t)cu_seqlens_q % 4 != 0) return QATTN_ERR_INVALID_ARG;
    if (total_q < 0 || max_seqlen_q < 1) return QATTN_ERR_INVALID_ARG;
    // ---- what skv_forward checks, on this entry's shapes
    if (!q16 || !k_pool || !v_pool || !scale_k || !scale_v || !out) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || Hq <= 0 || Skv <= 0) return QATTN_ERR_INVALID_ARG;
    if (!skv_d_ok(D) || Hq % Hkv != 0) return QATTN_ERR_UNSUPPORTED_DIM;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (numerics != QATTN_NUMERICS_COMPILED && numerics != QATTN_NUMERICS_EAGER) return QATTN_ERR_INVALID_ARG;
    if (precision != QATTN_PRECISION_FAST && precision != QATTN_PRECISION_ACCURATE) return QATTN_ERR_INVALID_ARG;
    if (num_splits < 0 || num_splits > QATTN_SPLITKV_MAX_SPLITS) return QATTN_ERR_INVALID_ARG;
    if (Hq > 65535) return QATTN_ERR_INVALID_ARG;   // (the y dimension of the pre-pass's and the merge's grids; B enters their x dimension only)
    if (Skv > 0x7fffffff - (1 << 15)) return QATTN_ERR_INVALID_ARG;   // (the split plan's key numbers stay in 32 bits)
    if (((size_t)q16 | (size_t)k_pool | (size_t)v_pool | (size_t)out | (size_t)q8 | (size_t)partial_o | (size_t)workspace) % 16 != 0)
        return QATTN_ERR_INVALID_ARG;
    long long ts = (long long)Hq * D, hs = D;   // dense [total_q, Hq, D]
    if (q_strides2) {
        if (q_strides2[0] < 0 || q_strides2[0] % 8 != 0 || q_strides2[1] < 0 || q_strides2[1] % 8 != 0) return QATTN_ERR_INVALID_ARG;
        ts = q_strides2[0]; hs = q_strides2[1];
    }
    const int G = Hq / Hkv;
    if ((long long)G * total_q > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;
    const long long nt = (long long)B + ((long long)G * total_q + kFpvTile - 1) / kFpvTile;   // tile slots per kv head
    if (num_splits == 0 && (partial_o || partial_lse || partial_path)) return QATTN_ERR_INVALID_ARG;   // (their shape would not be known)
    const int ns_most = pvq_most_splits(Skv, num_splits);
    if ((long long)Hkv * nt * ns_most > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (one workgroup per work item: a 32-bit grid)
    // the pre-pass's grids: B + ceil(total_q / rows per tile) in x.  The quantise pass has the smaller tiles, so its grid bounds the abs-max pass's
    static_assert(kVarlenQuantRows <= kVarlenAmaxRows, "the quantise grid is the larger of the two");
    if ((long long)B + ceil_div(total_q, kVarlenQuantRows) > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;
    if (total_q == 0) return QATTN_OK;   // no query row: nothing to compute or write, no workspace needed
    if (!workspace || workspace_bytes < pvq_ws(B, Hq, total_q, D, ns_most).total()) return QATTN_ERR_WORKSPACE;
    const int ns = num_splits > 0 ? num_splits
                                  : qattn_paged_varlen_auto_splits(B, Hq, Hkv, total_q, max_seqlen_q,
                                                                   WINDOW ? skv_window_keys(Skv, max_seqlen_q, window_left) : Skv, D, cu_count());
    const PvqWs ws = pvq_ws(B, Hq, total_q, D, ns);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)workspace;
    unsigned char* q8w = w;         w += ws.q8;
    float* sqw = (float*)w;         w += ws.sq;
    unsigned* amax = (unsigned*)w;  w += ws.amax;
    float* pow_ = (float*)w;        w += ws.po;
    float* plsew = (float*)w;       w += ws.plse;
    unsigned char* ppathw = w;      w += ws.ppath;
    float* acc = (float*)w;         w += ws.acc;
    float* acc_lse = (float*)w;
    unsigned char* q8p = q8 ? (unsigned char*)q8 : q8w;
    float* sq = scale_q ? scale_q : sqw;
    float* po = partial_o ? partial_o : pow_;
    float* plse = partial_lse ? partial_lse : plsew;
    unsigned char* ppath = partial_path ? partial_path : ((row_path && ns > 1) ? ppathw : nullptr);

    int rc = varlen_quant_q(q16, (long)ts, (long)hs, in_fmt, cu_seqlens_q, B, Hq, total_q, D, fp8_fmt, numerics, amax, q8p, sq, st);
    if (rc != QATTN_OK) return rc;

    const long rows = (long)Hq * total_q;
    SkvAttn a;
    __builtin_memset(&a, 0, sizeof(a));
    a.q8 = q8p; a.k8 = (const unsigned char*)k_pool; a.v8 = (const unsigned char*)v_pool;
    a.sq = sq; a.sk = scale_k; a.sv = scale_v;
    a.used = seqused_k;
    a.out = out; a.lse = lse; a.path = row_path;
    a.po = po; a.plse = plse; a.ppath = ppath;
    a.part_rows = rows;
    a.out_fmt = in_fmt; a.Hkv = Hkv; a.G = G; a.Skv = Skv;
    a.ntile = (int)nt;   // (Sq and rows are per sequence: read from cu_seqlens_q on the device)
    a.ns = ns; a.nchunks = ceil_div(Skv, 64);
    a.causal = (TREE || is_causal) ? 1 : 0;
    a.two_term_keys = kTwoTermKeys;
    a.sm_log2e = (sm_scale > 0.0f ? sm_scale : 1.0f / sqrtf((float)D)) * 1.4426950408889634f;
    SkvPages pg;
    pg.table = block_table; pg.stride = (long)table_stride; pg.num_pages = num_pages; pg.pc = pc;
    SkvVarq vq;
    vq.cu = cu_seqlens_q; vq.B = B; vq.total_q = total_q; vq.Hq = Hq;
    // the most keys a split can own; the sweep asks for the LSE whenever it feeds the merge (both as skv_forward).  Under a window the
    // bound takes total_q for a sequence's query count: cu_seqlens_q is not read on the host, and no sequence holds more (the extents are
    // clamped), whatever max_seqlen_q says
    const int max_keys = skv_max_keys(Skv, total_q, WINDOW ? window_left : -1, ns);
    const bool want_lse = SINK || SOFTCAP || lse != nullptr || ns > 1;
    rc = launch_skv<(SOFTCAP ? kSkvSoftcap : 0) + (TREE ? kSkvTree : 0) + (SINK ? kSkvSink : 0) + (WINDOW ? kSkvWindow : 0) + kSkvPagedVarq>(
        a, pg, vq, SkvWindow{window_left, window_right}, (unsigned)((long long)Hkv * nt * ns), max_keys, D, fp8_fmt, precision, want_lse, st,
        SkvSink{sinks}, SkvTree{tree_mask}, SOFTCAP ? skv_softcap_arg(softcap, a.sm_log2e) : SkvSoftcap{});
    if (rc != QATTN_OK) return rc;
    if (hipGetLastError() != hipSuccess) return QATTN_ERR_LAUNCH;
    if (ns == 1) return QATTN_OK;

    // ---- the merge on the packed conventions of include/qattn_merge.h: B = 1, S = total_q
    const long long os3[3] = {0, D, (long long)Hq * D}, ls3[3] = {0, total_q, 1};
    rc = skv_merge_chain_sink(po, plse, ns, rows, os3, ls3, 1, Hq, total_q, D, out, in_fmt, lse, acc, acc_lse, stream, SINK ? sinks : nullptr);
    if (rc != QATTN_OK) return rc;
    if (row_path) return skv_launch_path(plse, ppath, row_path, rows, ns, st);
    return QATTN_OK;
}

// pvq_forward<true, true, true> behind a function of its own (qattn_paged_varlen_splitkv_tree_sink_fp8.hip), so that the sink kernels are
// compiled in their own unit: qattn_fp8_attention_paged_varlen_tree_window_forward calls it when `sinks` is given.  The arguments are that
// entry's, in its order.
int pvq_tree_window_sink_forward(const void* q16, const long long* q_strides2, int in_fmt, const void* k_pool, const void* v_pool,
                                 const int* block_table, long long table_stride, int num_pages, int page_size, int max_pages,
                                 const float* scale_k, const float* scale_v, void* out, float* lse, const int* cu_seqlens_q,
                                 const int* seqused_k, int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int Skv, int D, int fp8_fmt,
                                 int numerics, const unsigned long long* tree_mask, int window_left, int window_right, const float* sinks,
                                 float sm_scale, int precision, int num_splits, void* q8, float* scale_q, unsigned char* row_path,
                                 float* partial_o, float* partial_lse, unsigned char* partial_path, void* workspace, size_t workspace_bytes,
                                 void* stream);

}  // namespace qattn

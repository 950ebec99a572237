// qattn_splitkv_attn.h -- the split-KV sweep kernel and its host driver, shared by the two entries that differ only in WHERE a head's 64-key
// chunks live: qattn_fp8_attention_splitkv_forward (qattn_splitkv_fp8.hip: contiguous KFRAG / VFRAG images, include/qattn_splitkv.h) and
// qattn_fp8_attention_paged_splitkv_forward (qattn_paged_splitkv_fp8.hip: a pool of pages behind a block table, include/qattn_paged.h).
// The kernel body is qattn_splitkv_body.h, compiled once per chunk addressing; each unit instantiates its own kernels only, and the
// contiguous kernel is, statement for statement, the kernel qattn_splitkv_fp8.hip held before the paged entry existed.
// A third compilation of the body, paged K / V under PACKED queries of a different count per sequence, belongs to
// qattn_fp8_attention_paged_varlen_forward (qattn_paged_varlen_splitkv_fp8.hip, include/qattn_paged_varlen.h); that entry has a driver of
// its own and shares the launch ladder, the merge chain (skv_merge_chain) and the path launch with skv_forward.
// Three more compilations put a sliding window where `causal` stands (QATTN_SKV_WINDOW; include/qattn_splitkv_window.h): the kernels of
// qattn_splitkv_window_fp8.hip, qattn_paged_splitkv_window_fp8.hip and qattn_paged_varlen_splitkv_window_fp8.hip, launched through the same
// ladder and the same drivers.  The window travels as a kernel argument of its own (SkvWindow): SkvAttn is what it was, field for field.
// And three more add a learned attention sink per query head to the window kernels (QATTN_SKV_SINK; include/qattn_sinks.h): the kernels of
// qattn_splitkv_sink_fp8.hip, qattn_paged_splitkv_sink_fp8.hip and qattn_paged_varlen_splitkv_sink_fp8.hip, the sink again an argument of
// its own (SkvSink).
// A tenth puts a draft tree over the packed paged kernel's causal rule (QATTN_SKV_TREE; include/qattn_paged_varlen_tree.h): the kernel of
// qattn_paged_varlen_splitkv_tree_fp8.hip, its mask words an argument of their own (SkvTree).
// And three more cap the window kernels' scaled scores, y = softcap tanh(x / softcap) (QATTN_SKV_SOFTCAP; include/qattn_softcap.h): the kernels
// of qattn_splitkv_softcap_fp8.hip, qattn_paged_splitkv_softcap_fp8.hip and qattn_paged_varlen_splitkv_softcap_fp8.hip, the cap's two
// factors an argument of their own (SkvSoftcap).
#pragma once
#include <limits.h>

#include "qattn_fp8pv_sweep.h"
#include "qattn_varlen_tile.h"
#include "../../include/qattn_merge.h"
#include "../../include/qattn_sinks.h"
#include "../../include/qattn_softcap.h"
#include "../../include/qattn_splitkv.h"

namespace qattn {

struct SkvAttn {
    const unsigned char *q8, *k8, *v8;   // q8 row-major [B, Hq, Sq, D]; the KFRAG / VFRAG images of [B, Hkv, Skv, D] (PAGED: the pools)
    const float *sq, *sk, *sv;           // [B, Hq], [B, Hkv], [B, Hkv]
    const int* used;                     // seqused_k [B] or nullptr
    void* out;                           // ns = 1: the call's outputs
    float* lse;
    unsigned char* path;
    float* po;                           // ns > 1: [ns][B Hq Sq][D], [ns][B Hq Sq], [ns][B Hq Sq] (ppath may be nullptr)
    float* plse;
    unsigned char* ppath;
    long part_rows;                      // B Hq Sq
    int out_fmt, Hkv, G, Sq, Skv;
    int rows, ntile;                     // packed rows G Sq of a kv head, and their 128-row tiles
    int ns, nchunks;                     // splits; 64-key chunks of a head's images
    int causal, two_term_keys;
    float sm_log2e;
};

// PAGED: the block table (include/qattn_paged.h).  Logical chunk c of (b, hkv) is chunk c % pc of page clamp(table[b][c / pc]): physical
// chunk (page Hkv + hkv) pc + c % pc of the pool.
struct SkvPages {
    const int* table;   // [B][stride]
    long stride;
    int num_pages, pc;  // pages of the pool; 64-key chunks per page
};

// VARQ: packed queries (include/qattn_paged_varlen.h).  q8 / out / the partials are [total_q, Hq, D]-shaped and the LSE-like outputs
// [Hq, total_q]; sequence i owns the tokens [clamp(cu[i]), clamp(cu[i + 1])).  SkvAttn then carries ntile = B + ceil(G total_q / 128) (tile
// slots per kv head) and part_rows = total_q Hq; its Sq and rows are not read.
struct SkvVarq {
    const int* cu;   // cu_seqlens_q [B + 1]
    int B, total_q, Hq;
};

// WINDOW: window_size = (left, right) of include/qattn_window.h, each >= -1 (-1: unbounded on that side).  A kernel argument of its own,
// so that SkvAttn -- and with it every kernarg offset of the kernels without a window -- stays what it was.
struct SkvWindow {
    int left, right;
};

// SINK: learned attention sinks (include/qattn_sinks.h): one logit per QUERY head, fp32 [Hq], in natural-log units of the scaled scores.
// A kernel argument of its own, as the window: the kernels without a sink keep their kernarg layout.
struct SkvSink {
    const float* sink;
};

// TREE: the draft tree of a speculative step (include/qattn_paged_varlen_tree.h): one 64-bit word per packed token, [total_q] on the
// device; bit i of token (b, p)'s word lets position p attend draft token i of its slot.  A kernel argument of its own, as the window.
struct SkvTree {
    const unsigned long long* mask;
};

// SOFTCAP: logit soft-capping (include/qattn_softcap.h), y = softcap tanh(x / softcap) on the scaled scores x.  Two host floats, a kernel
// argument of their own as the window: c = softcap log2e (the sweep's scores -> log2 units factor, the sweep seeing tanh(x / softcap)) and
// kin2 = 2 log2e sm_scale / softcap (times the row's scale_q scale_k: raw score -> the exponent of the tanh formula).
struct SkvSoftcap {
    float c, kin2;
};

// Physical chunk of chunk `ch` of kv head hkv of the page a RAW table entry names. The clamp is what keeps every address inside the
// pool, whatever the table holds; it is applied here, where the entry forms an address, so that the entry's load can be issued a step
// ahead of its use without its wait following it.  (Everything is workgroup-uniform.)
__device__ __forceinline__ int skv_phys(const SkvPages& pg, int entry, int Hkv, int hkv, int ch) {
    const int page = __builtin_amdgcn_readfirstlane(clampi(entry, 0, pg.num_pages - 1));
    return (page * Hkv + hkv) * pg.pc + ch;
}

// this lane's piece of an fp32 row: o[m][4 j + i] is column 32 m + 8 j + 4 hh + i (the map of store_o_rows), four floats at a time
template <int MB>
__device__ __forceinline__ void store_o_rows_f32(float* row, const v16f (&o)[MB], float inv, int hh, bool valid) {
    float* op = row + 4 * hh;
#pragma unroll
    for (int m = 0; m < MB; m++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const v4f x = {o[m][4 * j] * inv, o[m][4 * j + 1] * inv, o[m][4 * j + 2] * inv, o[m][4 * j + 3] * inv};
            if (valid) *reinterpret_cast<v4f*>(op + 32 * m + 8 * j) = x;
        }
}

// The V chunk of a stage, in LDS, with the bytes of its keys >= nvalid set to zero; all four waves call it (workgroup-uniform), after the
// stage has landed and before anyone reads it.  Only the chunk that holds key L_b needs it: a prepared image holds ALL Skv keys, so behind
// the used ones sit bytes the caller does not vouch for (a cache slot not yet filled: NaN patterns included).  Their P is exactly 0 -- the
// masked scores are -inf -- but 0 x NaN is NaN in the matrix pipe.  (K needs nothing: a NaN score is replaced by -inf, not multiplied.)
// VFRAG: the 16-byte piece at offset o holds, for one channel, the keys 32 half + 8 w + 4 hh + i at byte 4 w + i, half = bit 9, hh = bit 10.
template <int D>
__device__ __forceinline__ void skv_zero_v_tail(unsigned char* vst, int nvalid) {
    constexpr int CH = 64 * D;
    for (int o = (int)threadIdx.x * 16; o < CH; o += kFpvWaves * 64 * 16) {
        v4i x = *reinterpret_cast<v4i*>(vst + o);
        const int key0 = 32 * ((o >> 9) & 1) + 4 * ((o >> 10) & 1);
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int left = nvalid - (key0 + 8 * w);   // keys of this word that are valid: bytes 0 .. left - 1
            const unsigned keep = left >= 4 ? 0xffffffffu : left <= 0 ? 0u : (1u << (8 * left)) - 1u;
            x[w] = (int)((unsigned)x[w] & keep);
        }
        *reinterpret_cast<v4i*>(vst + o) = x;
    }
    lds_barrier();
}

// The mirror of skv_zero_v_tail for the chunk that holds the first key of a sliding window's interval: the bytes of its keys < nfirst
// (0 < nfirst < 64) set to zero.  Same callers' duties: all four waves, after the stage has landed, before anyone reads it.
template <int D>
__device__ __forceinline__ void skv_zero_v_head(unsigned char* vst, int nfirst) {
    constexpr int CH = 64 * D;
    for (int o = (int)threadIdx.x * 16; o < CH; o += kFpvWaves * 64 * 16) {
        v4i x = *reinterpret_cast<v4i*>(vst + o);
        const int key0 = 32 * ((o >> 9) & 1) + 4 * ((o >> 10) & 1);
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int dead = nfirst - (key0 + 8 * w);   // keys of this word below the interval: bytes 0 .. dead - 1
            const unsigned keep = dead >= 4 ? 0u : dead <= 0 ? 0xffffffffu : ~((1u << (8 * dead)) - 1u);
            x[w] = (int)((unsigned)x[w] & keep);
        }
        *reinterpret_cast<v4i*>(vst + o) = x;
    }
    lds_barrier();
}

// The two kernels: one body (qattn_splitkv_body.h), compiled once per chunk addressing.  BYTE / two / sel: as attn_vfp8_window_kernel.
template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_splitkv_fp8_kernel(const SkvAttn a, const int two, const int sel) {
#define QATTN_SKV_PAGED 0
#define QATTN_SKV_VARQ 0
#define QATTN_SKV_WINDOW 0
#define QATTN_SKV_SINK 0
#define QATTN_SKV_TREE 0
#define QATTN_SKV_SOFTCAP 0
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_paged_splitkv_fp8_kernel(const SkvAttn a, const SkvPages pg, const int two, const int sel) {
#define QATTN_SKV_PAGED 1
#define QATTN_SKV_VARQ 0
#define QATTN_SKV_WINDOW 0
#define QATTN_SKV_SINK 0
#define QATTN_SKV_TREE 0
#define QATTN_SKV_SOFTCAP 0
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_paged_varlen_splitkv_fp8_kernel(const SkvAttn a, const SkvPages pg, const SkvVarq vq, const int two, const int sel) {
#define QATTN_SKV_PAGED 1
#define QATTN_SKV_VARQ 1
#define QATTN_SKV_WINDOW 0
#define QATTN_SKV_SINK 0
#define QATTN_SKV_TREE 0
#define QATTN_SKV_SOFTCAP 0
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

// ... and the same three under a sliding window `wn` in a.causal's place (QATTN_SKV_WINDOW)
template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_splitkv_window_fp8_kernel(const SkvAttn a, const SkvWindow wn, const int two, const int sel) {
#define QATTN_SKV_PAGED 0
#define QATTN_SKV_VARQ 0
#define QATTN_SKV_WINDOW 1
#define QATTN_SKV_SINK 0
#define QATTN_SKV_TREE 0
#define QATTN_SKV_SOFTCAP 0
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_paged_splitkv_window_fp8_kernel(const SkvAttn a, const SkvPages pg, const SkvWindow wn, const int two, const int sel) {
#define QATTN_SKV_PAGED 1
#define QATTN_SKV_VARQ 0
#define QATTN_SKV_WINDOW 1
#define QATTN_SKV_SINK 0
#define QATTN_SKV_TREE 0
#define QATTN_SKV_SOFTCAP 0
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_paged_varlen_splitkv_window_fp8_kernel(const SkvAttn a, const SkvPages pg, const SkvVarq vq, const SkvWindow wn, const int two,
                                                 const int sel) {
#define QATTN_SKV_PAGED 1
#define QATTN_SKV_VARQ 1
#define QATTN_SKV_WINDOW 1
#define QATTN_SKV_SINK 0
#define QATTN_SKV_TREE 0
#define QATTN_SKV_SOFTCAP 0
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

// ... and the three window kernels with a learned sink per query head `sn` (QATTN_SKV_SINK; include/qattn_sinks.h).  Only the exact
// instances (BYTE = false) are ever launched: the sink entries ask the ladder for the exact one-term sweep under FAST.
template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_splitkv_window_sink_fp8_kernel(const SkvAttn a, const SkvWindow wn, const SkvSink sn, const int two, const int sel) {
#define QATTN_SKV_PAGED 0
#define QATTN_SKV_VARQ 0
#define QATTN_SKV_WINDOW 1
#define QATTN_SKV_SINK 1
#define QATTN_SKV_TREE 0
#define QATTN_SKV_SOFTCAP 0
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_paged_splitkv_window_sink_fp8_kernel(const SkvAttn a, const SkvPages pg, const SkvWindow wn, const SkvSink sn, const int two,
                                               const int sel) {
#define QATTN_SKV_PAGED 1
#define QATTN_SKV_VARQ 0
#define QATTN_SKV_WINDOW 1
#define QATTN_SKV_SINK 1
#define QATTN_SKV_TREE 0
#define QATTN_SKV_SOFTCAP 0
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_paged_varlen_splitkv_window_sink_fp8_kernel(const SkvAttn a, const SkvPages pg, const SkvVarq vq, const SkvWindow wn,
                                                      const SkvSink sn, const int two, const int sel) {
#define QATTN_SKV_PAGED 1
#define QATTN_SKV_VARQ 1
#define QATTN_SKV_WINDOW 1
#define QATTN_SKV_SINK 1
#define QATTN_SKV_TREE 0
#define QATTN_SKV_SOFTCAP 0
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

// ... and the packed paged kernel under a draft tree `tr` (QATTN_SKV_TREE; include/qattn_paged_varlen_tree.h), both sweeps
template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_paged_varlen_splitkv_tree_fp8_kernel(const SkvAttn a, const SkvPages pg, const SkvVarq vq, const SkvTree tr, const int two,
                                               const int sel) {
#define QATTN_SKV_PAGED 1
#define QATTN_SKV_VARQ 1
#define QATTN_SKV_WINDOW 0
#define QATTN_SKV_SINK 0
#define QATTN_SKV_TREE 1
#define QATTN_SKV_SOFTCAP 0
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

// ... and the draft tree over the packed paged WINDOW kernel, without and with a sink (QATTN_SKV_TREE with QATTN_SKV_WINDOW;
// include/qattn_paged_varlen_tree_window.h): the kernels of qattn_paged_varlen_splitkv_tree_window_fp8.hip (both sweeps) and
// qattn_paged_varlen_splitkv_tree_sink_fp8.hip (the exact instances only, as the sink kernels above)
template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_paged_varlen_splitkv_tree_window_fp8_kernel(const SkvAttn a, const SkvPages pg, const SkvVarq vq, const SkvWindow wn,
                                                      const SkvTree tr, const int two, const int sel) {
#define QATTN_SKV_PAGED 1
#define QATTN_SKV_VARQ 1
#define QATTN_SKV_WINDOW 1
#define QATTN_SKV_SINK 0
#define QATTN_SKV_TREE 1
#define QATTN_SKV_SOFTCAP 0
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_paged_varlen_splitkv_tree_window_sink_fp8_kernel(const SkvAttn a, const SkvPages pg, const SkvVarq vq, const SkvWindow wn,
                                                           const SkvSink sn, const SkvTree tr, const int two, const int sel) {
#define QATTN_SKV_PAGED 1
#define QATTN_SKV_VARQ 1
#define QATTN_SKV_WINDOW 1
#define QATTN_SKV_SINK 1
#define QATTN_SKV_TREE 1
#define QATTN_SKV_SOFTCAP 0
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

// ... and the three window kernels with the scaled scores soft-capped under `sc` (QATTN_SKV_SOFTCAP; include/qattn_softcap.h).  As with
// the sink kernels only the exact instances (BYTE = false) are ever launched: the byte-exponential formula is fitted to raw scores.
template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_splitkv_window_softcap_fp8_kernel(const SkvAttn a, const SkvWindow wn, const SkvSoftcap sc, const int two, const int sel) {
#define QATTN_SKV_PAGED 0
#define QATTN_SKV_VARQ 0
#define QATTN_SKV_WINDOW 1
#define QATTN_SKV_SINK 0
#define QATTN_SKV_TREE 0
#define QATTN_SKV_SOFTCAP 1
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_paged_splitkv_window_softcap_fp8_kernel(const SkvAttn a, const SkvPages pg, const SkvWindow wn, const SkvSoftcap sc, const int two,
                                                  const int sel) {
#define QATTN_SKV_PAGED 1
#define QATTN_SKV_VARQ 0
#define QATTN_SKV_WINDOW 1
#define QATTN_SKV_SINK 0
#define QATTN_SKV_TREE 0
#define QATTN_SKV_SOFTCAP 1
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_paged_varlen_splitkv_window_softcap_fp8_kernel(const SkvAttn a, const SkvPages pg, const SkvVarq vq, const SkvWindow wn,
                                                         const SkvSoftcap sc, const int two, const int sel) {
#define QATTN_SKV_PAGED 1
#define QATTN_SKV_VARQ 1
#define QATTN_SKV_WINDOW 1
#define QATTN_SKV_SINK 0
#define QATTN_SKV_TREE 0
#define QATTN_SKV_SOFTCAP 1
#include "qattn_splitkv_body.h"
#undef QATTN_SKV_SOFTCAP
#undef QATTN_SKV_TREE
#undef QATTN_SKV_SINK
#undef QATTN_SKV_WINDOW
#undef QATTN_SKV_VARQ
#undef QATTN_SKV_PAGED
}

// which of the fifteen kernels a launch runs (kSkvWindow + one of the first three: that kernel under a window; + kSkvSink: with a sink;
// kSkvTree + kSkvPagedVarq: the packed paged kernel under a draft tree; + kSkvWindow: the tree over its window kernel; + kSkvSink: with a sink;
// kSkvSoftcap + kSkvWindow + one of the first three: that window kernel with soft-capped scores)
constexpr int kSkvContig = 0, kSkvPaged = 1, kSkvPagedVarq = 2, kSkvWindow = 4, kSkvSink = 8, kSkvTree = 16, kSkvSoftcap = 32;

template <int D, int FMT, int MODE>
static int launch_skv_fmt(const SkvAttn& a, const SkvPages& pg, const SkvVarq& vq, const SkvWindow& wn, unsigned grid, int max_keys,
                          int precision, bool want_lse, hipStream_t st, const SkvSink& sn = SkvSink{}, const SkvTree& tr = SkvTree{},
                          const SkvSoftcap& sc = SkvSoftcap{}) {
    return fpv_precision_ladder(precision, max_keys, a.two_term_keys, want_lse, [&](auto byte, int two, int sel) {
        if constexpr ((MODE & kSkvSoftcap) != 0) {
            // (the byte-exponential instances are not compiled for the soft-cap kernels: their callers pass want_lse = true)
            static_assert((MODE & (kSkvSink | kSkvTree)) == 0 && (MODE & kSkvWindow) != 0, "soft-capping sits on the plain window kernels");
            if constexpr (decltype(byte)::value) return (int)QATTN_ERR_LAUNCH;
            else if constexpr (MODE == kSkvSoftcap + kSkvWindow + kSkvPagedVarq)
                return fpv_launch(attn_paged_varlen_splitkv_window_softcap_fp8_kernel<D, FMT, false>, grid, fpv_lds_bytes(D), st, a, pg, vq, wn, sc,
                                  two, sel);
            else if constexpr (MODE == kSkvSoftcap + kSkvWindow + kSkvPaged)
                return fpv_launch(attn_paged_splitkv_window_softcap_fp8_kernel<D, FMT, false>, grid, fpv_lds_bytes(D), st, a, pg, wn, sc, two, sel);
            else return fpv_launch(attn_splitkv_window_softcap_fp8_kernel<D, FMT, false>, grid, fpv_lds_bytes(D), st, a, wn, sc, two, sel);
        } else if constexpr (MODE == kSkvTree + kSkvSink + kSkvWindow + kSkvPagedVarq) {
            if constexpr (decltype(byte)::value) return (int)QATTN_ERR_LAUNCH;   // (as the sink kernels below: want_lse = true)
            else
                return fpv_launch(attn_paged_varlen_splitkv_tree_window_sink_fp8_kernel<D, FMT, false>, grid, fpv_lds_bytes(D), st, a, pg, vq, wn,
                                  sn, tr, two, sel);
        } else if constexpr (MODE == kSkvTree + kSkvWindow + kSkvPagedVarq)
            return fpv_launch(attn_paged_varlen_splitkv_tree_window_fp8_kernel<D, FMT, decltype(byte)::value>, grid, fpv_lds_bytes(D), st, a, pg,
                              vq, wn, tr, two, sel);
        else if constexpr (MODE == kSkvTree + kSkvPagedVarq)
            return fpv_launch(attn_paged_varlen_splitkv_tree_fp8_kernel<D, FMT, decltype(byte)::value>, grid, fpv_lds_bytes(D), st, a, pg, vq, tr,
                              two, sel);
        else if constexpr ((MODE & kSkvSink) != 0) {
            // (the byte-exponential instances are not compiled for the sink kernels: their callers pass want_lse = true)
            if constexpr (decltype(byte)::value) return (int)QATTN_ERR_LAUNCH;
            else if constexpr (MODE == kSkvSink + kSkvWindow + kSkvPagedVarq)
                return fpv_launch(attn_paged_varlen_splitkv_window_sink_fp8_kernel<D, FMT, false>, grid, fpv_lds_bytes(D), st, a, pg, vq, wn, sn, two,
                                  sel);
            else if constexpr (MODE == kSkvSink + kSkvWindow + kSkvPaged)
                return fpv_launch(attn_paged_splitkv_window_sink_fp8_kernel<D, FMT, false>, grid, fpv_lds_bytes(D), st, a, pg, wn, sn, two, sel);
            else return fpv_launch(attn_splitkv_window_sink_fp8_kernel<D, FMT, false>, grid, fpv_lds_bytes(D), st, a, wn, sn, two, sel);
        } else if constexpr (MODE == kSkvWindow + kSkvPagedVarq)
            return fpv_launch(attn_paged_varlen_splitkv_window_fp8_kernel<D, FMT, decltype(byte)::value>, grid, fpv_lds_bytes(D), st, a, pg, vq, wn,
                              two, sel);
        else if constexpr (MODE == kSkvWindow + kSkvPaged)
            return fpv_launch(attn_paged_splitkv_window_fp8_kernel<D, FMT, decltype(byte)::value>, grid, fpv_lds_bytes(D), st, a, pg, wn, two, sel);
        else if constexpr (MODE == kSkvWindow + kSkvContig)
            return fpv_launch(attn_splitkv_window_fp8_kernel<D, FMT, decltype(byte)::value>, grid, fpv_lds_bytes(D), st, a, wn, two, sel);
        else if constexpr (MODE == kSkvPagedVarq)
            return fpv_launch(attn_paged_varlen_splitkv_fp8_kernel<D, FMT, decltype(byte)::value>, grid, fpv_lds_bytes(D), st, a, pg, vq, two, sel);
        else if constexpr (MODE == kSkvPaged)
            return fpv_launch(attn_paged_splitkv_fp8_kernel<D, FMT, decltype(byte)::value>, grid, fpv_lds_bytes(D), st, a, pg, two, sel);
        else return fpv_launch(attn_splitkv_fp8_kernel<D, FMT, decltype(byte)::value>, grid, fpv_lds_bytes(D), st, a, two, sel);
    });
}

template <int D, int MODE>
static int launch_skv_d(const SkvAttn& a, const SkvPages& pg, const SkvVarq& vq, const SkvWindow& wn, unsigned grid, int max_keys, int fp8_fmt,
                        int precision, bool want_lse, hipStream_t st, const SkvSink& sn = SkvSink{}, const SkvTree& tr = SkvTree{},
                        const SkvSoftcap& sc = SkvSoftcap{}) {
    return fp8_fmt == QATTN_FMT_E4M3 ? launch_skv_fmt<D, QATTN_FMT_E4M3, MODE>(a, pg, vq, wn, grid, max_keys, precision, want_lse, st, sn, tr, sc)
                                     : launch_skv_fmt<D, QATTN_FMT_E5M2, MODE>(a, pg, vq, wn, grid, max_keys, precision, want_lse, st, sn, tr, sc);
}

// every head dimension of one entry
template <int MODE>
static int launch_skv(const SkvAttn& a, const SkvPages& pg, const SkvVarq& vq, const SkvWindow& wn, unsigned grid, int max_keys, int D,
                      int fp8_fmt, int precision, bool want_lse, hipStream_t st, const SkvSink& sn = SkvSink{}, const SkvTree& tr = SkvTree{},
                      const SkvSoftcap& sc = SkvSoftcap{}) {
    if (D == 64) return launch_skv_d<64, MODE>(a, pg, vq, wn, grid, max_keys, fp8_fmt, precision, want_lse, st, sn, tr, sc);
    if (D == 128) return launch_skv_d<128, MODE>(a, pg, vq, wn, grid, max_keys, fp8_fmt, precision, want_lse, st, sn, tr, sc);
    return launch_skv_d<256, MODE>(a, pg, vq, wn, grid, max_keys, fp8_fmt, precision, want_lse, st, sn, tr, sc);
}

// Host side of a soft cap (include/qattn_softcap.h): finite and > 0 ...
inline bool skv_softcap_ok(float softcap) { return softcap > 0.0f && softcap <= 3.402823466e38f; }
// ... and the kernel's two factors from it and the call's sm_scale log2e (a.sm_log2e)
inline SkvSoftcap skv_softcap_arg(float softcap, float sm_log2e) { return SkvSoftcap{softcap * 1.4426950408889634f, 2.0f * sm_log2e / softcap}; }

// Host side of a window (include/qattn_splitkv_window.h).  Under left >= 0 a sequence's interval [lo_i, L) holds at most left + Sq keys,
// which touch at most ceil((left + Sq) / 128) + 1 key blocks.
// skv_window_keys: the key count the num_splits = 0 rule sees, min(Skv, left + Sq + 127).
inline int skv_window_keys(int Skv, int Sq, int left) {
    const long long k = (long long)left + Sq + 127;
    return (left < 0 || k >= Skv) ? Skv : (int)k;
}
// skv_max_keys: an upper bound on the keys any workgroup sweeps with ns splits -- what fpv_precision_ladder needs to launch the one-term
// kernel whenever a workgroup can reach two_term_keys.  Sq: the most queries of a sequence.  left = -1: the most keys a split can own.
inline int skv_max_keys(int Skv, int Sq, int left, int ns) {
    long long nkb = ceil_div(Skv, 128);
    if (left >= 0) {
        const long long in_window = ((long long)left + Sq + 127) / 128 + 1;
        if (in_window < nkb) nkb = in_window;
    }
    const long long span = 128 * ((nkb + ns - 1) / ns);
    return span < Skv ? (int)span : Skv;
}

inline bool skv_dims_ok(int B, int Hq, int Hkv, int Sq, int Skv) { return B > 0 && Hq > 0 && Hkv > 0 && Sq > 0 && Skv > 0; }
inline bool skv_d_ok(int D) { return D == 64 || D == 128 || D == 256; }

// the sections of the workspace, in order (each up256)
struct SkvWs {
    size_t q8, sq, qws, po, plse, ppath, acc, acc_lse;
    size_t total() const { return q8 + sq + qws + po + plse + ppath + acc + acc_lse; }
};
inline SkvWs skv_ws(int B, int Hq, int Sq, int D, int ns) {
    const size_t rows = (size_t)B * Hq * Sq;
    SkvWs w = {};
    w.q8 = up256(qattn_fp8_tensor_bytes(QATTN_LAYOUT_ROWMAJOR, B, Hq, Sq, D));
    w.sq = up256(sizeof(float) * (size_t)B * Hq);
    w.qws = up256(qattn_quant_workspace_bytes(B, Hq, Sq, D, QATTN_SCALE_HEAD));
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

// splitkv_path_kernel's launch (qattn_splitkv_fp8.hip): row_path of a merged row from the per-split path bytes
int skv_launch_path(const float* plse, const unsigned char* ppath, unsigned char* path, long rows, int ns, hipStream_t st);

// the num_splits = 0 rule from the count of (kv head, tile) work items on (qattn_splitkv_fp8.hip): residency, the key-block cap, the
// fewest splits with the same blocks per split.  Both auto_splits functions are this on their own tile count.
int skv_auto_splits_of_tiles(long long tiles, int Skv, int D, int num_cus);

// The merge of ns > 1 fp32 partials po [ns][rows][D] / plse [ns][rows] into out / lse: partials 0 .. 7 (into the accumulator when more
// follow), then 7 more per launch in place, the last one into out.  os3 / ls3: the element strides (batch, head, query) every partial,
// the accumulator and the destination share -- dense [B, Hq, Sq, D] / [B, Hq, Sq], or the packed conventions of include/qattn_merge.h with
// B = 1, Sq = total_q.  acc / acc_lse are read only with ns > QATTN_MERGE_MAX_PARTIALS.
// skv_merge_chain_sink: the chain with a learned sink per head (include/qattn_sinks.h; nullptr: none, the chain as it always was).  The
// sink is one more state of the row and may be counted once: it enters the LAST launch only (qattn_attention_state_merge_sink), the
// launches before it are the plain merge.
inline int skv_merge_chain_sink(const float* po, const float* plse, int ns, long rows, const long long (&os3)[3], const long long (&ls3)[3],
                                int B, int Hq, int Sq, int D, void* out, int out_fmt, float* lse, float* acc, float* acc_lse, void* stream,
                                const float* sink) {
    constexpr int top = QATTN_MERGE_MAX_PARTIALS;
    auto merge = [&](const float* o0, const float* l0, int first, int n_more, void* dst, int dst_fmt, float* dst_lse, bool last) -> int {
        const void* o[top];
        const float* l[top];
        int fmt[top];
        long long ostr[3 * top], lstr[3 * top];
        int n = 0;
        if (o0) { o[n] = o0; l[n] = l0; n++; }
        for (int i = 0; i < n_more; i++, n++) { o[n] = po + (size_t)(first + i) * rows * D; l[n] = plse + (size_t)(first + i) * rows; }
        for (int i = 0; i < n; i++) {
            fmt[i] = QATTN_FMT_FP32;
            for (int j = 0; j < 3; j++) { ostr[3 * i + j] = os3[j]; lstr[3 * i + j] = ls3[j]; }
        }
        if (last && sink) return qattn_attention_state_merge_sink(n, o, fmt, ostr, l, lstr, dst, dst_fmt, os3, dst_lse, ls3, B, Hq, Sq, D, stream, sink);
        return qattn_attention_state_merge(n, o, fmt, ostr, l, lstr, dst, dst_fmt, os3, dst_lse, ls3, B, Hq, Sq, D, stream);
    };
    if (ns <= top) return merge(nullptr, nullptr, 0, ns, out, out_fmt, lse, true);
    int rc = merge(nullptr, nullptr, 0, top, acc, QATTN_FMT_FP32, acc_lse, false);
    int done = top;
    while (rc == QATTN_OK && ns - done > top - 1) {
        rc = merge(acc, acc_lse, done, top - 1, acc, QATTN_FMT_FP32, acc_lse, false);
        done += top - 1;
    }
    if (rc == QATTN_OK) rc = merge(acc, acc_lse, done, ns - done, out, out_fmt, lse, true);
    return rc;
}

inline int skv_merge_chain(const float* po, const float* plse, int ns, long rows, const long long (&os3)[3], const long long (&ls3)[3], int B,
                           int Hq, int Sq, int D, void* out, int out_fmt, float* lse, float* acc, float* acc_lse, void* stream) {
    return skv_merge_chain_sink(po, plse, ns, rows, os3, ls3, B, Hq, Sq, D, out, out_fmt, lse, acc, acc_lse, stream, nullptr);
}

// Both entries, from their common arguments on: k8 / v8 are the contiguous images of [B, Hkv, Skv, D] or -- PAGED, with pg filled in and
// checked by the caller -- the pools.
// WINDOW: the window kernels under (window_left, window_right) in is_causal's place -- also for (-1, 0) and (-1, -1).
// SINK (with WINDOW; include/qattn_sinks.h): the sink kernels with `sinks` fp32 [Hq] on the device -- folded into the sweep's epilogue with
// one split, into the last launch of the merge chain with more.  Under FAST they take the exact one-term sweep, never the byte one.
// SOFTCAP (with WINDOW, without SINK; include/qattn_softcap.h): the soft-cap kernels under the host float `softcap`, finite and > 0 -- a
// kernel argument, so a captured graph keeps the value it was captured with.  The partials are ordinary states over the capped scores: the
// merge chain is the window entry's.  Under FAST the exact one-term sweep, as SINK.
template <bool PAGED, bool WINDOW = false, bool SINK = false, bool SOFTCAP = false>
int skv_forward(const void* q16, int in_fmt, const void* k8, const void* v8, const SkvPages& pg, const float* scale_k, const float* scale_v,
                void* out, float* lse, const int* seqused_k, int B, int Hq, int Hkv, int Sq, int Skv, int D, int fp8_fmt, int numerics,
                int is_causal, float sm_scale, int precision, int num_splits, void* q8, float* scale_q, unsigned char* row_path,
                float* partial_o, float* partial_lse, unsigned char* partial_path, void* workspace, size_t workspace_bytes, void* stream,
                int window_left = -1, int window_right = -1, const float* sinks = nullptr, float softcap = 0.0f) {
    static_assert(WINDOW || !SINK, "the sink kernels are window kernels");
    static_assert(!SOFTCAP || (WINDOW && !SINK), "the soft-cap kernels are window kernels without a sink");
    if (SOFTCAP && !skv_softcap_ok(softcap)) return QATTN_ERR_INVALID_ARG;
    if (WINDOW && (window_left < -1 || window_right < -1)) return QATTN_ERR_INVALID_ARG;
    if (SINK && (!sinks || (size_t)sinks % 4 != 0)) return QATTN_ERR_INVALID_ARG;
    if (!q16 || !k8 || !v8 || !scale_k || !scale_v || !out) return QATTN_ERR_INVALID_ARG;
    if (!skv_dims_ok(B, Hq, Hkv, Sq, Skv)) return QATTN_ERR_INVALID_ARG;
    if (!skv_d_ok(D) || Hq % Hkv != 0) return QATTN_ERR_UNSUPPORTED_DIM;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (numerics != QATTN_NUMERICS_COMPILED && numerics != QATTN_NUMERICS_EAGER) return QATTN_ERR_INVALID_ARG;
    if (precision != QATTN_PRECISION_FAST && precision != QATTN_PRECISION_ACCURATE) return QATTN_ERR_INVALID_ARG;
    if (num_splits < 0 || num_splits > QATTN_SPLITKV_MAX_SPLITS) return QATTN_ERR_INVALID_ARG;
    if (B > 65535 || Hq > 65535) return QATTN_ERR_INVALID_ARG;   // (the merge's grid)
    if (Skv > 0x7fffffff - (1 << 15)) return QATTN_ERR_INVALID_ARG;   // (the split plan's key numbers stay in 32 bits)
    if (((size_t)q16 | (size_t)k8 | (size_t)v8 | (size_t)out | (size_t)q8 | (size_t)partial_o | (size_t)workspace) % 16 != 0)
        return QATTN_ERR_INVALID_ARG;
    const int G = Hq / Hkv;
    if ((long long)G * Sq > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;
    const int ntile = ceil_div(G * Sq, kFpvTile);
    // num_splits = 0: the grid and the workspace are checked for the most splits the rule can pick -- qattn_..._workspace_bytes(..., 0) --
    // so that every check is done before the device is asked for its CU count; the partial buffers' shape would not be known to the caller
    if (num_splits == 0 && (partial_o || partial_lse || partial_path)) return QATTN_ERR_INVALID_ARG;
    const int nkb_all = ceil_div(Skv, 128);
    const int ns_most = num_splits > 0 ? num_splits : (nkb_all < QATTN_SPLITKV_MAX_SPLITS ? nkb_all : QATTN_SPLITKV_MAX_SPLITS);
    if ((long long)B * Hkv * ntile * ns_most > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (one workgroup per work item: a 32-bit grid)
    if (!workspace || workspace_bytes < skv_ws(B, Hq, Sq, D, ns_most).total()) return QATTN_ERR_WORKSPACE;
    const int ns = num_splits > 0 ? num_splits
                                  : qattn_splitkv_auto_splits(B, Hq, Hkv, Sq, WINDOW ? skv_window_keys(Skv, Sq, window_left) : Skv, D, cu_count());
    const SkvWs ws = skv_ws(B, Hq, Sq, D, ns);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)workspace;
    unsigned char* q8w = w;         w += ws.q8;
    float* sqw = (float*)w;         w += ws.sq;
    void* qws = w;                  w += ws.qws;
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

    int rc = qattn_quant_fp8(q16, in_fmt, q8p, sq, B, Hq, Sq, D, fp8_fmt, QATTN_SCALE_HEAD, numerics, QATTN_LAYOUT_ROWMAJOR, qws,
                             qattn_quant_workspace_bytes(B, Hq, Sq, D, QATTN_SCALE_HEAD), stream);
    if (rc != QATTN_OK) return rc;

    const long rows = (long)B * Hq * Sq;
    SkvAttn a;
    __builtin_memset(&a, 0, sizeof(a));
    a.q8 = q8p; a.k8 = (const unsigned char*)k8; a.v8 = (const unsigned char*)v8;
    a.sq = sq; a.sk = scale_k; a.sv = scale_v;
    a.used = seqused_k;
    a.out = out; a.lse = lse; a.path = row_path;
    a.po = po; a.plse = plse; a.ppath = ppath;
    a.part_rows = rows;
    a.out_fmt = in_fmt; a.Hkv = Hkv; a.G = G; a.Sq = Sq; a.Skv = Skv;
    a.rows = G * Sq; a.ntile = ntile;
    a.ns = ns; a.nchunks = ceil_div(Skv, 64);
    a.causal = is_causal ? 1 : 0;
    a.two_term_keys = kTwoTermKeys;
    a.sm_log2e = (sm_scale > 0.0f ? sm_scale : 1.0f / sqrtf((float)D)) * 1.4426950408889634f;
    // the most keys a split can own; the sweep asks for the LSE whenever it feeds the merge
    const int max_keys = skv_max_keys(Skv, Sq, WINDOW ? window_left : -1, ns);
    const bool want_lse = SINK || SOFTCAP || lse != nullptr || ns > 1;
    const unsigned grid = (unsigned)((long long)B * Hkv * ntile * ns);
    rc = launch_skv<(SOFTCAP ? kSkvSoftcap : 0) + (SINK ? kSkvSink : 0) + (WINDOW ? kSkvWindow : 0) + (PAGED ? kSkvPaged : kSkvContig)>(
        a, pg, SkvVarq{}, SkvWindow{window_left, window_right}, grid, max_keys, D, fp8_fmt, precision, want_lse, st, SkvSink{sinks}, SkvTree{},
        SOFTCAP ? skv_softcap_arg(softcap, a.sm_log2e) : SkvSoftcap{});
    if (rc != QATTN_OK) return rc;
    if (hipGetLastError() != hipSuccess) return QATTN_ERR_LAUNCH;
    if (ns == 1) return QATTN_OK;

    const long long os3[3] = {(long long)Hq * Sq * D, (long long)Sq * D, D}, ls3[3] = {(long long)Hq * Sq, Sq, 1};
    rc = skv_merge_chain_sink(po, plse, ns, rows, os3, ls3, B, Hq, Sq, D, out, in_fmt, lse, acc, acc_lse, stream, SINK ? sinks : nullptr);
    if (rc != QATTN_OK) return rc;
    if (row_path) return skv_launch_path(plse, ppath, row_path, rows, ns, st);
    return QATTN_OK;
}

}  // namespace qattn

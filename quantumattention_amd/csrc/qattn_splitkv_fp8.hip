// qattn_splitkv_fp8.hip -- qattn_fp8_attention_splitkv_forward (include/qattn_splitkv.h): FP8 attention of few queries over many PREPARED
// keys, the key axis of a head cut across workgroups.
//
// Launches, none of which reads seqused_k on the host:
//   quant  qattn_quant_fp8 of q (row-major, head-wise): q8 and scale_q
//   attn   attn_splitkv_fp8_kernel, one 4-wave workgroup per (b, kv head, 128-row tile of the head group's packed rows, split): the fourth
//          client of the FP8-PV chunk sweep (qattn_fp8pv_sweep.h), statement for statement what attn_vfp8_window_kernel runs, with this
//          kernel's own
//            * row map: packed row r of kv head (b, hkv) is query head hkv G + r / Sq at position r % Sq -- in q8 / out / lse simply row r
//              of the [B, Hkv, G Sq, D] view; K and V are read once per group.  scale_q is per query head, so the sweep's `c` is this
//              lane's own product (a VGPR here, uniform in the other three kernels);
//            * trip range: the 64-key chunks of the split's key blocks [s per, (s + 1) per), cut at L_b and -- causal -- at the largest key a
//              valid row of the tile attends; FAST's one-term rule counts exactly those keys;
//            * masks: the ragged tail at L_b and the causal edge by token, under a workgroup-uniform guard; rows that meet no key in a chunk
//              or in the whole split follow the window kernel's rules (start value -1e20, has_key; its header comment has the argument).
//              Padding rows (r >= G Sq) attend every key below L_b with zero scores, as the window and block-sparse kernels' do: the
//              rescale decision of softmax_pv is wave-wide, so the bit equalities with those kernels need the same wave-mates;
//            * the chunk that holds key L_b: the V bytes of the keys behind L_b are zeroed in LDS before the step (skv_zero_v_tail) -- a
//              prepared image holds all Skv keys, and 0 x NaN would be NaN;
//            * stores: num_splits = 1 -> out / lse / row_path; else the fp32 row o (scale_v / l), the natural LSE and the path byte of the
//              split into the partial buffers [ns, B, Hq, Sq, ...];
//            * registers: as the window kernel -- the ones word of the row-sum MFMA is spread where it is used.
//   merge  num_splits > 1: qattn_attention_state_merge over the fp32 partials, 8 at a time (through an fp32 accumulator for more than 8)
//   path   row_path with num_splits > 1: splitkv_path_kernel combines the per-split bytes
#include <limits.h>

#include "qattn_fp8pv_sweep.h"
#include "qattn_varlen_tile.h"
#include "../../include/qattn_merge.h"
#include "../../include/qattn_splitkv.h"

namespace qattn {

struct SkvAttn {
    const unsigned char *q8, *k8, *v8;   // q8 row-major [B, Hq, Sq, D]; the KFRAG / VFRAG images of [B, Hkv, Skv, D]
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

// BYTE / two / sel: as attn_vfp8_window_kernel
template <int D, int FMT, bool BYTE>
__global__ __launch_bounds__(kFpvWaves * 64, (FpvShape<D, BYTE>::WPS))
void attn_splitkv_fp8_kernel(const SkvAttn a, const int two, const int sel) {
    constexpr int CH = 64 * D, MB = D / 32, KS = D / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    FpvSweep<D, FMT, BYTE> sw(smem);
    const int lane = sw.lane, wave = sw.wave, ql = sw.ql, hh = sw.hh;

    // block -> (kv head b Hkv + hkv, tile, split): the splits of a tile are neighbours, the tiles of a kv head follow each other.
    // (Handing each XCD a contiguous range of kv heads, as the other launchers do, was measured and moved no time: not kept.)
    const int bid = blockIdx.x, per_head = a.ntile * a.ns;
    const int kvh = bid / per_head, rest = bid % per_head;
    const int s = rest % a.ns, tile = rest / a.ns;
    int L = a.Skv;
    if (a.used) L = clampi(__builtin_amdgcn_readfirstlane(a.used[kvh / a.Hkv]), 0, a.Skv);
    // the split plan (workgroup-uniform, as everything down to the row numbers)
    const int nkb = (L + 127) >> 7, per = (nkb + a.ns - 1) / a.ns;
    const int k_begin = 128 * s * per, k_end = min(128 * (s + 1) * per, L);
    const int r_first = tile * kFpvTile, r_last = min(r_first + kFpvTile, a.rows) - 1;
    // positions of the tile's valid rows: [smin, smax] (a tile that crosses a head boundary holds a last and a first position)
    const int g_first = r_first / a.Sq, g_last = r_last / a.Sq;
    const int smin = g_first != g_last ? 0 : r_first - g_first * a.Sq, smax = g_first != g_last ? a.Sq - 1 : r_last - g_first * a.Sq;
    const int delta = L - a.Sq;   // causal: position p attends the keys j <= p + delta
    const int khi = a.causal ? min(k_end - 1, smax + delta) : k_end - 1;
    const int keys = max(khi - k_begin + 1, 0);   // the keys this workgroup sweeps
    if (sel == kFpvSelMany && keys < a.two_term_keys) return;
    if (sel == kFpvSelFew && keys >= a.two_term_keys) return;

    const int r = r_first + wave * kQPerWave + ql;   // packed row
    const bool rvalid = r < a.rows;
    const int g = min(r / a.Sq, a.G - 1);            // (padding rows: the last head's scale)
    const long grow = (long)kvh * a.rows + r;        // row of the dense [B Hq Sq] index space
    if (keys == 0) {   // no key for any row of the tile in this split (L = 0, a split past the last block, a split above the causal edge)
        if (a.ns == 1) {
            fpv_store_empty<D>(a.out, a.out_fmt, (rvalid ? grow : 0L) * (2L * D), a.lse, grow, a.path, grow, hh, rvalid);
        } else {
            const long prow = (long)s * a.part_rows + (rvalid ? grow : 0L);
            v16f z[MB];
#pragma unroll
            for (int m = 0; m < MB; m++)
#pragma unroll
                for (int e = 0; e < 16; e++) z[m][e] = 0.0f;
            store_o_rows_f32<MB>(a.po + prow * D, z, 0.0f, hh, rvalid);
            if (hh == 0 && rvalid) a.plse[prow] = -INFINITY;
            if (a.ppath && hh == 0 && rvalid) a.ppath[prow] = (unsigned char)QATTN_PATH_ONE_TERM;
        }
        return;
    }
    const int c_first = k_begin >> 6;               // chunks c_first .. khi / 64 <= (L - 1) / 64 < nchunks
    const int n_wg = (khi >> 6) - c_first + 1;

    const long img = (long)kvh * a.nchunks * CH + (wave << 10);
    FpvRing<D> ring(smem, wave, lane, a.k8 + img, a.v8 + img);
    ring.dma_chunk(c_first);
    sw.park_q(a.q8 + (rvalid ? grow : (long)kvh * a.rows) * D + hh * 32, rvalid);
    constexpr float kNoKeyYet = -1.0e20f;   // (attn_vfp8_window_kernel's header comment)
    sw.init_state(a.sm_log2e * a.sq[(long)kvh * a.G + g] * a.sk[kvh], kNoKeyYet);
    const int one = fpv_ones_word(lane);
    // the last key this lane's row attends, and the first chunk end that crosses the causal edge of some valid row
    const int hi_l = (a.causal && rvalid) ? min(L - 1, r - g * a.Sq + delta) : L - 1;
    const int edge = a.causal ? smin + delta : INT_MAX;

    for (int t = 0; t < n_wg; t++) {   // step t sweeps chunk c_first + t
        const int k0 = (c_first + t) * 64;
        if (__builtin_expect(k0 + 64 > L, 0)) {   // the chunk that holds key L: its stage is waited for here, ahead of the step's own (then idle) wait
            sw.wait_stage();
            skv_zero_v_tail<D>(smem + (t & 1) * (2 * CH) + CH, L - k0);
        }
        v8i qf[KS];
        sw.read_q(qf);
        sw.wait_stage();
        if (t + 1 < n_wg) ring.dma_chunk(c_first + t + 1);
        v16f s0, s1;
        v8i vf0, vf1;
        sw.qk(t, qf, s0, s1, vf0, vf1);
        // ---- the ragged tail at L and the causal edge by token, under a workgroup-uniform condition
        if (__builtin_expect(k0 + 64 > L || k0 + 63 > edge, 0)) {
            const int base = k0 + 4 * hh;
#pragma unroll
            for (int e = 0; e < 32; e++) {
                const int key = base + 32 * (e >> 4) + (e & 3) + 8 * ((e & 15) >> 2);
                v16f& sx = (e >> 4) ? s1 : s0;
                sx[e & 15] = key > hi_l ? -INFINITY : sx[e & 15];
            }
        }
        sw.softmax_pv(s0, s1, vf0, vf1, two, [&] { return fpv_spread_ones(one); });
    }

    // ---- epilogue (V's one scale per kv head is applied here)
    const float l_tot = sw.row_sum();
    const bool has_key = l_tot > 0.0f;   // (a row without a key inside a workgroup that sweeps: every P was 0 -- a zero row, LSE -inf)
    const float inv = has_key ? a.sv[kvh] / l_tot : 0.0f;
    const float lse_row = has_key ? 0.6931471805599453f * (sw.m_run * sw.c - kPShift) + __logf(l_tot) : -INFINITY;
    const unsigned char code = (unsigned char)((!BYTE && two) ? QATTN_PATH_TWO_TERM : QATTN_PATH_ONE_TERM);
    if (a.ns == 1) {
        store_o_rows<MB>(a.out, a.out_fmt, sw.o, inv, (rvalid ? grow : 0L) * (2L * D), hh, rvalid);
        if (!BYTE && a.lse && hh == 0 && rvalid) a.lse[grow] = lse_row;
        if (a.path && hh == 0 && rvalid) a.path[grow] = code;
    } else {
        const long prow = (long)s * a.part_rows + (rvalid ? grow : 0L);
        store_o_rows_f32<MB>(a.po + prow * D, sw.o, inv, hh, rvalid);
        if (!BYTE && hh == 0 && rvalid) a.plse[prow] = lse_row;
        if (a.ppath && hh == 0 && rvalid) a.ppath[prow] = code;
    }
}

// row_path of a merged row: ONE_TERM if a split that gave it a key ran one-term, else TWO_TERM; a row without a key: ONE_TERM
__global__ __launch_bounds__(256) void splitkv_path_kernel(const float* plse, const unsigned char* ppath, unsigned char* path, const long rows,
                                                           const int ns) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    bool any = false, one = false;
    for (int s = 0; s < ns; s++) {
        const bool live = plse[s * rows + i] > -INFINITY;
        any = any || live;
        one = one || (live && ppath[s * rows + i] == (unsigned char)QATTN_PATH_ONE_TERM);
    }
    path[i] = (unsigned char)((!any || one) ? QATTN_PATH_ONE_TERM : QATTN_PATH_TWO_TERM);
}

template <int D, int FMT>
static int launch_skv_fmt(const SkvAttn& a, unsigned grid, int max_keys, int precision, bool want_lse, hipStream_t st) {
    return fpv_precision_ladder(precision, max_keys, a.two_term_keys, want_lse, [&](auto byte, int two, int sel) {
        return fpv_launch(attn_splitkv_fp8_kernel<D, FMT, decltype(byte)::value>, grid, fpv_lds_bytes(D), st, a, two, sel);
    });
}

template <int D>
static int launch_skv_d(const SkvAttn& a, unsigned grid, int max_keys, int fp8_fmt, int precision, bool want_lse, hipStream_t st) {
    return fp8_fmt == QATTN_FMT_E4M3 ? launch_skv_fmt<D, QATTN_FMT_E4M3>(a, grid, max_keys, precision, want_lse, st)
                                     : launch_skv_fmt<D, QATTN_FMT_E5M2>(a, grid, max_keys, precision, want_lse, st);
}

}  // namespace qattn

using namespace qattn;

namespace {
bool skv_dims_ok(int B, int Hq, int Hkv, int Sq, int Skv) { return B > 0 && Hq > 0 && Hkv > 0 && Sq > 0 && Skv > 0; }
bool skv_d_ok(int D) { return D == 64 || D == 128 || D == 256; }

// the sections of the workspace, in order (each up256)
struct SkvWs {
    size_t q8, sq, qws, po, plse, ppath, acc, acc_lse;
    size_t total() const { return q8 + sq + qws + po + plse + ppath + acc + acc_lse; }
};
SkvWs skv_ws(int B, int Hq, int Sq, int D, int ns) {
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
}  // namespace

extern "C" size_t qattn_fp8_attention_splitkv_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Skv, int D, int num_splits) {
    if (!skv_dims_ok(B, Hq, Hkv, Sq, Skv) || !skv_d_ok(D) || Hq % Hkv != 0 || num_splits < 0 || num_splits > QATTN_SPLITKV_MAX_SPLITS) return 0;
    // (0: the auto rule never picks more splits than key blocks)
    const int nkb = ceil_div(Skv, 128);
    const int ns = num_splits > 0 ? num_splits : (nkb < QATTN_SPLITKV_MAX_SPLITS ? nkb : QATTN_SPLITKV_MAX_SPLITS);
    return skv_ws(B, Hq, Sq, D, ns).total();
}

// The num_splits = 0 rule (profiles/splitkv/: the table the two constants came from).  The sweep keeps ONE 16 KiB chunk in flight per
// workgroup, so a workgroup streams at the rate its load latency allows and the chip's bandwidth is reached only with every resident slot
// taken; a grid that exceeds the resident slots by a little runs a second, nearly empty round (13 splits of 40 tiles = 520 workgroups on
// 512 slots measured 13 % slower than 16 splits).  Every split also costs its share of a merge launch (8 states per launch, chained: about
// 6 us each) and 1024 keys are what FAST needs for its one-term sweep.  Hence: the LARGEST count whose grid still fits the resident slots
// -- kSkvResident workgroups per CU -- with at least kSkvMinBlocks key blocks per split, at most 64; then the fewest splits with the same
// blocks per split (none is empty when every key is used).
// What the constants rest on: D = 128, bf16, ACCURATE measurements only.  On both decode shapes of that table the binding term was the
// kSkvMinBlocks cap, not residency; residency bound the Sq = 64 shape alone.  The residency figures of D = 64 and D = 256 come from those
// kernels' launch bounds and LDS use, not from a measurement.
constexpr int kSkvMinBlocks = 8;   // key blocks (of 128 keys) a split keeps at least
// 4-wave workgroups a CU holds at once: one wave per SIMD each, by the exact kernels' register budget and by the CU's 160 KiB of LDS
template <int D> constexpr int skv_resident() {
    return FpvShape<D, false>::WPS < 160 * 1024 / fpv_lds_bytes(D) ? FpvShape<D, false>::WPS : 160 * 1024 / fpv_lds_bytes(D);
}
static_assert(skv_resident<64>() == 3 && skv_resident<128>() == 2 && skv_resident<256>() == 1, "include/qattn_splitkv.h states these");

extern "C" int qattn_splitkv_auto_splits(int B, int Hq, int Hkv, int Sq, int Skv, int D, int num_cus) {
    if (!skv_dims_ok(B, Hq, Hkv, Sq, Skv) || !skv_d_ok(D) || Hq % Hkv != 0 || num_cus <= 0) return 1;
    const long long tiles = (long long)B * Hkv * (((long long)(Hq / Hkv) * Sq + kFpvTile - 1) / kFpvTile);
    const long long slots = (long long)num_cus * (D == 64 ? skv_resident<64>() : D == 128 ? skv_resident<128>() : skv_resident<256>());
    long long ns = slots / tiles;
    const int nkb = ceil_div(Skv, 128);
    if (ns > nkb / kSkvMinBlocks) ns = nkb / kSkvMinBlocks;
    if (ns > QATTN_SPLITKV_MAX_SPLITS) ns = QATTN_SPLITKV_MAX_SPLITS;
    if (ns <= 1) return 1;
    const int per = ceil_div(nkb, (int)ns);
    return ceil_div(nkb, per);
}

extern "C" int qattn_fp8_attention_splitkv_forward(const void* q16, int in_fmt, const void* k8_kfrag, const void* v8_vfrag, const float* scale_k,
                                                   const float* scale_v, void* out, float* lse, const int* seqused_k, int B, int Hq, int Hkv,
                                                   int Sq, int Skv, int D, int fp8_fmt, int numerics, int is_causal, float sm_scale,
                                                   int precision, int num_splits, void* q8, float* scale_q, unsigned char* row_path,
                                                   float* partial_o, float* partial_lse, unsigned char* partial_path, void* workspace,
                                                   size_t workspace_bytes, void* stream) {
    if (!q16 || !k8_kfrag || !v8_vfrag || !scale_k || !scale_v || !out) return QATTN_ERR_INVALID_ARG;
    if (!skv_dims_ok(B, Hq, Hkv, Sq, Skv)) return QATTN_ERR_INVALID_ARG;
    if (!skv_d_ok(D) || Hq % Hkv != 0) return QATTN_ERR_UNSUPPORTED_DIM;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (numerics != QATTN_NUMERICS_COMPILED && numerics != QATTN_NUMERICS_EAGER) return QATTN_ERR_INVALID_ARG;
    if (precision != QATTN_PRECISION_FAST && precision != QATTN_PRECISION_ACCURATE) return QATTN_ERR_INVALID_ARG;
    if (num_splits < 0 || num_splits > QATTN_SPLITKV_MAX_SPLITS) return QATTN_ERR_INVALID_ARG;
    if (B > 65535 || Hq > 65535) return QATTN_ERR_INVALID_ARG;   // (the merge's grid)
    if (Skv > 0x7fffffff - (1 << 15)) return QATTN_ERR_INVALID_ARG;   // (the split plan's key numbers stay in 32 bits)
    if (((size_t)q16 | (size_t)k8_kfrag | (size_t)v8_vfrag | (size_t)out | (size_t)q8 | (size_t)partial_o | (size_t)workspace) % 16 != 0)
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
    const int ns = num_splits > 0 ? num_splits : qattn_splitkv_auto_splits(B, Hq, Hkv, Sq, Skv, D, cu_count());
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
    a.q8 = q8p; a.k8 = (const unsigned char*)k8_kfrag; a.v8 = (const unsigned char*)v8_vfrag;
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
    const int nkb = ceil_div(Skv, 128);
    const long long span = 128LL * ceil_div(nkb, ns);
    const int max_keys = span < Skv ? (int)span : Skv;
    const bool want_lse = lse != nullptr || ns > 1;
    const unsigned grid = (unsigned)((long long)B * Hkv * ntile * ns);
    if (D == 64) rc = launch_skv_d<64>(a, grid, max_keys, fp8_fmt, precision, want_lse, st);
    else if (D == 128) rc = launch_skv_d<128>(a, grid, max_keys, fp8_fmt, precision, want_lse, st);
    else rc = launch_skv_d<256>(a, grid, max_keys, fp8_fmt, precision, want_lse, st);
    if (rc != QATTN_OK) return rc;
    if (hipGetLastError() != hipSuccess) return QATTN_ERR_LAUNCH;
    if (ns == 1) return QATTN_OK;

    // ---- the merge: partials 0 .. 7 (into the accumulator when more follow), then 7 more per launch in place, the last one into out
    constexpr int top = QATTN_MERGE_MAX_PARTIALS;
    const long long os3[3] = {(long long)Hq * Sq * D, (long long)Sq * D, D}, ls3[3] = {(long long)Hq * Sq, Sq, 1};
    auto merge = [&](const float* o0, const float* l0, int first, int n_more, void* dst, int dst_fmt, float* dst_lse) -> int {
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
        return qattn_attention_state_merge(n, o, fmt, ostr, l, lstr, dst, dst_fmt, os3, dst_lse, ls3, B, Hq, Sq, D, stream);
    };
    if (ns <= top) {
        rc = merge(nullptr, nullptr, 0, ns, out, in_fmt, lse);
    } else {
        rc = merge(nullptr, nullptr, 0, top, acc, QATTN_FMT_FP32, acc_lse);
        int done = top;
        while (rc == QATTN_OK && ns - done > top - 1) {
            rc = merge(acc, acc_lse, done, top - 1, acc, QATTN_FMT_FP32, acc_lse);
            done += top - 1;
        }
        if (rc == QATTN_OK) rc = merge(acc, acc_lse, done, ns - done, out, in_fmt, lse);
    }
    if (rc != QATTN_OK) return rc;
    if (row_path) {
        hipLaunchKernelGGL(splitkv_path_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, plse, ppath, row_path, rows, ns);
        if (hipGetLastError() != hipSuccess) return QATTN_ERR_LAUNCH;
    }
    return QATTN_OK;
}

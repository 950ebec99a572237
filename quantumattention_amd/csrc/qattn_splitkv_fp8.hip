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
// The kernel and the host driver are qattn_splitkv_attn.h's (shared with the paged entry, qattn_paged_splitkv_fp8.hip); this unit
// instantiates the contiguous kernels and holds what both entries call: the workspace plan's size function, the num_splits = 0 rule and
// the path launch.
#include "qattn_splitkv_attn.h"

namespace qattn {

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

int skv_launch_path(const float* plse, const unsigned char* ppath, unsigned char* path, long rows, int ns, hipStream_t st) {
    hipLaunchKernelGGL(splitkv_path_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, plse, ppath, path, rows, ns);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

}  // namespace qattn

using namespace qattn;

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
    return skv_auto_splits_of_tiles((long long)B * Hkv * (((long long)(Hq / Hkv) * Sq + kFpvTile - 1) / kFpvTile), Skv, D, num_cus);
}

// (tiles >= 1, Skv >= 1, D supported, num_cus >= 1: checked by the callers)
int qattn::skv_auto_splits_of_tiles(long long tiles, int Skv, int D, int num_cus) {
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
    return skv_forward<false>(q16, in_fmt, k8_kfrag, v8_vfrag, SkvPages{}, scale_k, scale_v, out, lse, seqused_k, B, Hq, Hkv, Sq, Skv, D, fp8_fmt,
                              numerics, is_causal, sm_scale, precision, num_splits, q8, scale_q, row_path, partial_o, partial_lse, partial_path,
                              workspace, workspace_bytes, stream);
}

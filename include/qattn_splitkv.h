/*
 * qattn_splitkv.h -- split-KV FP8 attention for FEW queries over MANY keys, on K / V that are already in the kernels' format (ABI 8
 * addition; the names are found by symbol, include/qattn.h and QATTN_ABI_VERSION unchanged).
 *
 * Every other attention entry gives one workgroup one 128-row query tile of one head and lets it sweep all of that head's keys: right when
 * B Hq ceil(Sq/128) is a few hundred, wrong for decode (Sq = 1 .. 16), a prompt suffix over a cached prefix, a few latent queries over a
 * long sequence.  This entry cuts the key axis of a head across `num_splits` workgroups, packs the G = Hq / Hkv query heads of a kv head
 * into the same tiles (K and V are read once per group), and merges the partial states with qattn_attention_state_merge
 * (include/qattn_merge.h).  K and V arrive PREPARED: the KFRAG image of k and the VFRAG image of v with their head-wise scales, exactly
 * what two qattn_quant_fp8(..., QATTN_SCALE_HEAD, ..., QATTN_LAYOUT_KFRAG / _VFRAG) calls leave -- quantise once, attend many times.
 *
 * Semantics.  q16 [B, Hq, Sq, D] bf16 / fp16 (in_fmt), dense; k8_kfrag / v8_vfrag: qattn_fp8_tensor_bytes(QATTN_LAYOUT_KFRAG / _VFRAG, B, Hkv,
 * Skv, D) bytes each in fp8_fmt, scale_k / scale_v fp32 [B, Hkv].  V must have been finite everywhere.
 *   seqused_k    NULL, or int32 [B] on the device: batch element b uses its first L_b = clamp(seqused_k[b], 0, Skv) keys.  Keys beyond L_b
 *                influence no output bit (they DID count toward the prepared scales).  Read on the device: a captured call follows the
 *                table's later contents.
 *   is_causal    bottom-right (flash-attn's kv-cache entry; window (-1, 0) of include/qattn_window.h): query s attends keys j <= s + L_b - Sq.
 *   empty rows   a row without a key is a zero row with an LSE of -inf.
 *   precision    QATTN_PRECISION_ACCURATE: two-term (hi + lo) e4m3 P, exact exponentials, everywhere.  QATTN_PRECISION_FAST: a workgroup runs
 *                the one-term sweep iff the keys it sweeps -- its split's keys, cut at L_b and at the causal edge of the last of its valid
 *                rows -- number >= 1024; byte exponentials only when num_splits = 1 and lse = NULL, exact exponentials otherwise.
 *   num_splits   1 .. 64, or 0 = qattn_splitkv_auto_splits on the current device's CU count.  With 0 the workspace must hold
 *                qattn_fp8_attention_splitkv_workspace_bytes(..., 0) bytes (the most splits the rule can pick; checked before the CU count is
 *                asked for) and the three partial_* pointers must be NULL (their shape would not be known to the caller).
 *
 * Work item = (b, kv head, 128-row tile of the head group's PACKED rows, split s); the grid is B Hkv ceil(G Sq / 128) num_splits workgroups
 * of 4 waves.  Packed row r < G Sq is query head g = r / Sq at position r % Sq: in q8 / out / lse these are consecutive rows
 * ([B, Hq, Sq, D] viewed as [B, Hkv, G Sq, D]).  Split plan, evaluated on the device: nkb = ceil(L_b / 128), per = ceil(nkb / num_splits);
 * split s owns the key blocks [s per, min((s + 1) per, nkb)), i.e. the keys [128 s per, min(128 (s + 1) per, L_b)).  Under is_causal a
 * workgroup sweeps only the chunks up to the largest key any of its valid rows attends.  A workgroup that sweeps no key writes zero rows,
 * LSE -inf and QATTN_PATH_ONE_TERM.
 *
 * Launches of one call, all on `stream`, none reading a table on the host:
 *   1  qattn_quant_fp8 of q (head-wise, row-major): q8 and scale_q [B, Hq], the bits of that entry            (2 launches: abs-max, quantise)
 *   2  the split sweep attn_splitkv_fp8_kernel: 1 launch for ACCURATE, 2 for FAST (when a split can reach 1024 keys)
 *   3  num_splits > 1: qattn_attention_state_merge on the fp32 partials, 8 at a time in the order merge_attn_states chains them (the first
 *      8 into an fp32 accumulator in the workspace, then 7 more per launch in place; the last launch rounds once into out):
 *      1 + ceil((num_splits - 8) / 7) launches for num_splits > 8.  The partial buffers are left intact.
 *   4  row_path != NULL and num_splits > 1: one small launch that combines the per-split path bytes.
 *
 * Contract (tests/test_gpu_splitkv.py):
 *   (a) num_splits > 1: out, lse = merge_attn_states(partial_o[0..], partial_lse[0..], out_dtype = in_fmt) bit for bit.
 *   (b) Hq = Hkv, seqused_k = NULL, not causal: partial s, rounded to in_fmt, its LSE and its path bytes are, bit for bit, what
 *       qattn_fp8_block_sparse_attention_forward_fp8pv gives under the mask that turns on exactly split s's key blocks; with
 *       num_splits = 1 out is the all-true-mask call's.
 *   (c) Hq = Hkv, seqused_k = NULL, causal, num_splits = 1: out, lse, row_path are qattn_fp8_quant_attention_varlen_window_forward_fp8pv's
 *       with window (-1, 0) bit for bit.
 *   (d) a (k, v) pair prepared inside the Python call and prepare_kv_fp8(k, v) give the same bits.
 *   (e) a batched call equals its per-batch-element calls (same num_splits) bit for bit.
 *   (f) graph replay equals the eager call, also after seqused_k's contents are rewritten.
 *   (g) Hq > Hkv, seqused_k, causal with num_splits > 1: no bit equality with another entry (the rescale decision of the shared sweep is
 *       wave-wide, so a row's bits depend on its wave-mates; the packed entries scale V over the used keys only) -- the fp64 oracle's bound.
 *
 * Buffers (sizes, alignment, written bytes: include/qattn_buffers.h).  Optional outputs -- NULL: kept in the workspace or not produced:
 *   q8           fp8 [B, Hq, Sq, D] row-major;   scale_q fp32 [B, Hq];   row_path uint8 [B, Hq, Sq] (QATTN_PATH_*: ONE_TERM if any split that gave
 *                the row a key ran one-term, else TWO_TERM; with num_splits = 1 the workgroup's own code; rows without a key in any split of
 *                a num_splits > 1 call: ONE_TERM)
 *   partial_o    fp32 [num_splits, B, Hq, Sq, D]: o scale_v / l of the split, one multiplication, no other rounding (num_splits > 1 only)
 *   partial_lse  fp32 [num_splits, B, Hq, Sq] natural log-sum-exp;   partial_path uint8 [num_splits, B, Hq, Sq]
 *   lse          NULL or fp32 [B, Hq, Sq].
 *
 * Errors (negative QATTN_ERR_* before any device call, the codes of the block-sparse FP8-PV entry): QATTN_ERR_INVALID_ARG for a NULL or
 * misaligned (16 bytes: q16, k8_kfrag, v8_vfrag, out, q8, partial_o, workspace) pointer, a non-positive dimension, B or Hq above 65535, an
 * unknown numerics / precision, num_splits outside 0 .. 64, a partial_* pointer with num_splits = 0, a grid beyond 2^31 - 1 workgroups; QATTN_ERR_UNSUPPORTED_DIM for D outside
 * {64, 128, 256} or Hq % Hkv != 0; QATTN_ERR_UNSUPPORTED_FMT; QATTN_ERR_WORKSPACE.  No host synchronisation, no allocation, graph-capture safe.
 *
 * The same entry over a PAGED cache (a pool of fixed-size pages behind a block table): qattn_fp8_attention_paged_splitkv_forward,
 * include/qattn_paged.h -- the bits of this entry on the images gathered through the table.
 */
#ifndef QATTN_SPLITKV_H_
#define QATTN_SPLITKV_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QATTN_SPLITKV_MAX_SPLITS 64

/* bytes of workspace a call with this num_splits needs (0: enough for whatever the auto rule picks); 0 for unsupported arguments */
size_t qattn_fp8_attention_splitkv_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Skv, int D, int num_splits);

/* The num_splits = 0 rule: a pure host function of the shape and the CU count (it never reads seqused_k).  The largest count whose grid
 * B Hkv ceil(G Sq / 128) num_splits still fits the workgroups the chip holds at once (per CU: 3 at D = 64, 2 at D = 128, 1 at D = 256, whose ring fills most of a CU's LDS), capped so
 * that every split keeps >= 8 key blocks of 128 keys and at 64, then lowered to the fewest splits with the same blocks per split (no split
 * is empty at L_b = Skv); 1 when that leaves nothing to split -- a grid that already fills the chip, or fewer than 16 key blocks.  Measured
 * table: DESIGN.md section 4.17, profiles/splitkv/ -- D = 128, bf16, ACCURATE only: there the 8-block cap, not residency, bound both decode
 * shapes, and the residency figures of D = 64 and 256 come from those kernels' launch bounds and LDS use, not from a measurement.
 * Invalid arguments: 1. */
int qattn_splitkv_auto_splits(int B, int Hq, int Hkv, int Sq, int Skv, int D, int num_cus);

int qattn_fp8_attention_splitkv_forward(const void* q16, int in_fmt, const void* k8_kfrag, const void* v8_vfrag, const float* scale_k,
                                        const float* scale_v, void* out, float* lse, const int* seqused_k, int B, int Hq, int Hkv, int Sq,
                                        int Skv, int D, int fp8_fmt, int numerics, int is_causal, float sm_scale, int precision,
                                        int num_splits, void* q8, float* scale_q, unsigned char* row_path, float* partial_o,
                                        float* partial_lse, unsigned char* partial_path, void* workspace, size_t workspace_bytes,
                                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_SPLITKV_H_ */

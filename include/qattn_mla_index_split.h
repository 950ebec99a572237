/*
 * qattn_mla_index_split.h -- the MULTI-WORKGROUP exact top-k selection of the lightning indexer (include/qattn_mla_index.h): the selection of
 * one row of logits cut across up to QATTN_MLA_INDEX_MAX_SELECT_SPLITS workgroups, for few rows over many keys (decode at a long context),
 * where qattn_mla_index_select leaves all compute units but one per row idle.  The names are found by symbol; include/qattn.h,
 * QATTN_ABI_VERSION and every entry of include/qattn_mla_index.h are unchanged.
 *
 * CONTRACT.  "SELECTION" of include/qattn_mla_index.h word for word: indices[b, i] = the positions of the min(topk, kend) largest logits among
 * j < kend(b, i), ascending, then -1; a larger logit wins, equal logits go to the lower position, -0.0 equals +0.0, a NaN ranks as -inf;
 * kend <= topk writes 0 .. kend - 1, -1 .. without reading a logit.  The output is a pure function of the logits below kend for ANY
 * distribution (all-equal rows, a threshold bin that holds the whole row): it equals qattn_mla_index_select's bit for bit, for every
 * num_splits.  No atomics on the output, no sort, nothing read on the host; the launches depend on (B, Sq, N, topk, num_splits) only, so a
 * call is graph-capture safe and a replayed graph follows the later contents of the logits and seqused_k.
 *
 * GEOMETRY.  num_splits = s, 1 <= s <= QATTN_MLA_INDEX_MAX_SELECT_SPLITS.  SEG = ceil(N / s) rounded up to a multiple of 64; split k of a row
 * owns the positions [k SEG, min((k + 1) SEG, kend)); a split whose segment starts at or behind kend does nothing.  s = 1 is
 * qattn_mla_index_select itself (no workspace).
 *
 * METHOD (s >= 2).  Radix select on the order-preserving 32-bit keys ACROSS LAUNCHES, digits of 11, 11 and 10 bits:
 * six launches over work items (row, split) -- clear, three histogram passes, count, place -- ordered by the stream alone.  NO workgroup
 * waits for another inside a kernel: no cooperative launch, no grid barrier, no flag.  A pass adds its segment's LDS histogram to the row's
 * histogram in the workspace with integer atomics (order-independent sums: deterministic); the next launch finds the chosen digit there.
 * After the three passes the threshold key T and need_eq, the number of keys equal to T still admitted, are exact for any distribution: no
 * candidate buffer, no fallback path.  The count launch stores, per (split, wave), how many keys lie above T and equal T; the place launch
 * sums what lies in front of it and runs the ordered compaction of the one-workgroup kernel inside its segment.
 *
 * WORKSPACE.  qattn_mla_index_select_split_workspace_bytes(B, Sq, N, num_splits) bytes, 16-byte aligned (0 for num_splits = 1): the rows'
 * histograms, the digits found so far and the counts.  The call clears what it accumulates into, inside itself: the result does not depend
 * on what the workspace held before.  Calls that share a workspace must be ordered by their stream.  COST: the histograms are 20 KiB a row
 * and the call clears those of EVERY row of B Sq, the rows with kend <= topk included -- at most 640 KiB under the auto rule (which splits 32
 * rows at the most on 256 compute units), but 20 KiB B Sq under an explicit num_splits: with B Sq in the thousands that is a clear of tens of
 * megabytes a call.  An explicit num_splits >= 2 is meant for few rows.
 *
 * qattn_fp8_mla_index_topk_split = qattn_fp8_mla_index_scores and then this selection; its workspace holds the logits rows (when logits is
 * NULL) followed by the selection's workspace: qattn_fp8_mla_index_topk_split_workspace_bytes(B, Sq, max_seqlen_k, select_splits,
 * own_logits) bytes, own_logits != 0 when the caller passes logits.
 *
 * qattn_mla_index_select_auto_splits(rows = B Sq, N, topk, num_cus): the rule behind num_splits = 0 of the Python interface, a pure function
 * of the shape.  The library's entries themselves take 1 .. QATTN_MLA_INDEX_MAX_SELECT_SPLITS and reject 0: the caller resolves the rule
 * first (the Python interface does, in ONE place: _native.mla_index_resolve_splits).  The rule: s = the largest count
 * <= QATTN_MLA_INDEX_MAX_SELECT_SPLITS with rows s <= num_cus and ceil(N / s) >= QATTN_MLA_INDEX_AUTO_MIN_SEG; it answers s only where the split
 * path was measured faster than one workgroup a row and 1 everywhere else: for N < QATTN_MLA_INDEX_AUTO_MIN_KEYS, for
 * N <= topk, and for s < QATTN_MLA_INDEX_AUTO_MIN_SPLITS, that is for rows > num_cus / QATTN_MLA_INDEX_AUTO_MIN_SPLITS (2 splits were measured
 * 25 % slower than one workgroup at 16 384 keys and 4 no faster; at 64 and 128 rows of 16 384 keys no count was faster).
 *
 * Argument checks, before any device call (QATTN_ERR_INVALID_ARG): those of qattn_mla_index_select / qattn_fp8_mla_index_topk; num_splits in
 * 1 .. QATTN_MLA_INDEX_MAX_SELECT_SPLITS; for num_splits >= 2: B, Sq <= 65535 (grid axes), the workspace non-NULL, 16-byte aligned and
 * workspace_bytes large enough.
 *
 * Not offered: fusing the first histogram into the score sweep; per-key index scales; packed variable-length q.
 */
#ifndef QATTN_MLA_INDEX_SPLIT_H_
#define QATTN_MLA_INDEX_SPLIT_H_

#include "qattn_mla_index.h"

#define QATTN_MLA_INDEX_MAX_SELECT_SPLITS 256   /* the CU count of an MI355X */
#ifndef QATTN_MLA_INDEX_AUTO_MIN_SEG
#define QATTN_MLA_INDEX_AUTO_MIN_SEG 2048       /* the shortest segment the auto rule gives a split (measured) */
#endif
#ifndef QATTN_MLA_INDEX_AUTO_MIN_KEYS
#define QATTN_MLA_INDEX_AUTO_MIN_KEYS 16384     /* rows shorter than this stay on one workgroup under the auto rule (measured, ibid.) */
#endif
#ifndef QATTN_MLA_INDEX_AUTO_MIN_SPLITS
#define QATTN_MLA_INDEX_AUTO_MIN_SPLITS 8       /* the auto rule answers 1 where it could give a row fewer splits than this (measured, ibid.) */
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* 0 for num_splits = 1 or when a limit is broken */
size_t qattn_mla_index_select_split_workspace_bytes(int B, int Sq, int N, int num_splits);

int qattn_mla_index_select_auto_splits(int rows, int N, int topk, int num_cus);

int qattn_mla_index_select_split(const float* logits, const long long* logits_strides2, const int* seqused_k, int B, int Sq, int N, int topk,
                                 int is_causal, int num_splits, int* indices, void* workspace, size_t workspace_bytes, void* stream);

size_t qattn_fp8_mla_index_topk_split_workspace_bytes(int B, int Sq, int max_seqlen_k, int select_splits, int own_logits);

int qattn_fp8_mla_index_topk_split(const void* q16, int in_fmt, const long long* q_strides3, const float* weights, const long long* w_strides2,
                                   const void* pool, const int* block_table, long long table_stride, int num_pages, int page_size,
                                   int max_pages, const float* scale, const int* seqused_k, int B, int Hi, int Sq, int max_seqlen_k, int topk,
                                   int fp8_fmt, int is_causal, int select_splits, int* indices, float* logits, void* q8, float* scale_q,
                                   void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_MLA_INDEX_SPLIT_H_ */

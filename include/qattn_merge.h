/*
 * qattn_merge.h -- merging of attention states: N partial results (O_i, lse_i) of ONE set of queries over DISJOINT key sets become the
 * result over the union (ABI 8 addition; the name is found by symbol, include/qattn.h and QATTN_ABI_VERSION unchanged).
 *
 *     m = max_i lse_i,   e_i = exp(lse_i - m),   out = (sum_i e_i O_i) / sum_i e_i,   lse_out = m + log sum_i e_i
 *
 * lse_i is the NATURAL log-sum-exp every attention entry of this library returns (QATTN_LSE_NATURAL; the packed, sliding-window and
 * block-sparse entries and their FP8-P.V siblings return no other).  One launch for 2 <= n <= QATTN_MERGE_MAX_PARTIALS partials, on `stream`.
 *
 * Index space: rows (b, h, s), 0 <= b < B, 0 <= h < H, 0 <= s < S, each D in {64, 128, 256} elements.  Every tensor is described by its
 * base pointer and three ELEMENT strides {batch, head, row}; nothing is copied and nothing need be dense:
 *   o[i]         partial i's output rows: bf16, fp16 or fp32 (o_fmt[i], QATTN_FMT_BF16 / _FP16 / _FP32 -- each partial its own, a ring
 *                loop merges its fp32 accumulator with a 16-bit partial); D innermost and contiguous; base and every row 16-byte aligned
 *                (strides of the dimensions with more than one index: multiples of 8 elements for 16-bit, of 4 for fp32); strides >= 0, a
 *                stride of 0 broadcasts.  o_strides: 3 n values, partial i's at [3 i].
 *   lse[i]       fp32, one value per row, 4-byte aligned, strides >= 0 (lse_strides: 3 n values).
 *   out          out_fmt (independent of the inputs' formats), rules of o[i]; out_strides: 3 values.
 *   lse_out      NULL (not wanted; lse_out_strides is then not read) or fp32 with its 3 strides.
 *   Dense [B,H,S,D] / [B,H,S] is {H S D, S D, D} / {H S, S, 1}; the packed entries' [total,H,D] / [H,total] is B = 1, S = total with
 *   {0, D, H D} / {0, total, 1}; the views fp8_window_attn_func returns are {S H D, D, H D} / {S, B S, 1}; QATTN_LSE_REFERENCE's padded
 *   rows are {H ld, ld, 1} with ld = qattn_lse_row_stride(S, QATTN_LSE_REFERENCE).
 *   The strides of a dimension with a single index are not read.  B, H <= 65535.
 *   The tables (o, o_fmt, o_strides, lse, lse_strides, *_strides) are HOST arrays, read before the call returns; they travel to the
 *   kernel by value in its arguments: no device allocation, no host synchronisation, graph-capture safe.
 *
 * Arithmetic: fp32 throughout, exp and log accurate to about an ulp, the partials summed in index order (deterministic), ONE rounding to
 * out_fmt at the end (round to nearest even); the quotient is the sum times the correctly rounded reciprocal of sum_i e_i.
 *   lse_i = -inf            the partial attended no key for this row (the zero row / LSE -inf the window and block-sparse entries
 *                           produce): it contributes nothing and NO BYTE of its O row influences the result, NaN and Inf included.  The
 *                           same holds for a partial whose e_i underflows to zero (more than about 87 below the row's maximum).
 *   every lse_i = -inf      a zero row and lse_out = -inf: the library's empty-row convention, so merged states merge again.
 *   lse_i = +inf or NaN     the row of out is NaN and lse_out is NaN.
 *   With a single contributing partial the row is that partial's row converted to out_fmt: exactly that row when the formats agree.
 *
 * Aliasing: out / lse_out may be EXACTLY partial 0's buffers -- out = o[0] with out_fmt = o_fmt[0] and equal strides, lse_out = lse[0]
 * with equal strides: the in-place accumulate of a ring step.  Any other overlap between an output and an input, and any two rows of an
 * output that overlap, are the caller's error; what can be seen from the strides alone is refused: an output stride of 0 over more than
 * one index, an output row stride below D, strides under which one dimension's rows reach into the next index of a wider one.
 *
 * Buffer contract (as include/qattn_buffers.h): of every tensor exactly the described elements are read or written -- the D elements of
 * each row of o[i] / out, one float per row of lse[i] / lse_out; pads between rows and heads are neither read nor written, every described
 * element of out and lse_out is written, and no result depends on a byte outside the described inputs.
 *
 * Errors (negative QATTN_ERR_* of include/qattn.h, before any device call): QATTN_ERR_INVALID_ARG for n outside 2 .. 8, a non-positive B,
 * H or S, B or H above 65535, a NULL table, o[i], lse[i], out or (with lse_out) lse_out_strides, a misaligned base or row, a negative
 * stride, a refused output layout; QATTN_ERR_UNSUPPORTED_DIM for D; QATTN_ERR_UNSUPPORTED_FMT for a format that is not bf16, fp16, fp32.
 */
#ifndef QATTN_MERGE_H_
#define QATTN_MERGE_H_

#include "qattn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QATTN_FMT_FP32 4             /* element format of a partial / of the merged output (this header's entry only) */
#define QATTN_MERGE_MAX_PARTIALS 8

int qattn_attention_state_merge(int n, const void* const* o, const int* o_fmt, const long long* o_strides, const float* const* lse,
                                const long long* lse_strides, void* out, int out_fmt, const long long* out_strides, float* lse_out,
                                const long long* lse_out_strides, int B, int H, int S, int D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QATTN_MERGE_H_ */

// qattn_merge.hip -- merging of attention states (include/qattn_merge.h): out = sum_i exp(lse_i - L) O_i, L = log sum_i exp(lse_i), for the
// partial results of one set of queries over disjoint key sets.  One launch, fp32 arithmetic, bandwidth-bound.
//
// Shape: a lane owns 8 consecutive elements of one row -- 16 bytes of a 16-bit tensor, 32 of an fp32 one -- so a row of D elements is D / 8
// neighbouring lanes of ONE wave (8 / 16 / 32) and a wave's request covers whole rows.  256 threads = 32 / 16 / 8 rows of one (b, h); the
// grid is (row tiles, H, B): no division, the batch and head offsets are scalar.  N is a template argument: the N row pieces are N
// independent 16-byte loads in flight per lane before the first use, and every register array is indexed statically (no scratch).  The
// FORMAT of a partial is a launch-uniform runtime branch (not 3^8 instantiations).  No LDS: the N log-sum-exps of a row are read by the
// row's lanes from one address each (a broadcast within the request) and the weights are computed per lane.
#include "qattn_merge_dev.h"

namespace qattn {

template <int D, int N>
__global__ __launch_bounds__(256) void merge_states_kernel(const MergeParams p) {
#define QATTN_MERGE_SINK 0
#include "qattn_merge_body.h"
#undef QATTN_MERGE_SINK
}

template <int D>
static void launch_merge(int n, const MergeParams& p, dim3 grid, hipStream_t st) {
    switch (n) {
#define QATTN_MERGE_CASE(NN) case NN: hipLaunchKernelGGL((merge_states_kernel<D, NN>), grid, dim3(256), 0, st, p); break
        QATTN_MERGE_CASE(2);
        QATTN_MERGE_CASE(3);
        QATTN_MERGE_CASE(4);
        QATTN_MERGE_CASE(5);
        QATTN_MERGE_CASE(6);
        QATTN_MERGE_CASE(7);
        QATTN_MERGE_CASE(8);
#undef QATTN_MERGE_CASE
    }
}

}  // namespace qattn

using namespace qattn;

extern "C" int qattn_attention_state_merge(int n, const void* const* o, const int* o_fmt, const long long* o_strides, const float* const* lse,
                                           const long long* lse_strides, void* out, int out_fmt, const long long* out_strides,
                                           float* lse_out, const long long* lse_out_strides, int B, int H, int S, int D, void* stream) {
    MergeParams p;
    dim3 grid;
    const int rc = merge_check_and_fill(2, n, o, o_fmt, o_strides, lse, lse_strides, out, out_fmt, out_strides, lse_out, lse_out_strides, B, H, S,
                                        D, p, grid);
    if (rc != QATTN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (D == 64) launch_merge<64>(n, p, grid, st);
    else if (D == 128) launch_merge<128>(n, p, grid, st);
    else launch_merge<256>(n, p, grid, st);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

// qattn_merge_sink.hip -- qattn_attention_state_merge_sink (include/qattn_sinks.h): the state merge of qattn_merge.hip with a learned sink
// per head as one more state of every row -- lse = sink[h], no O row.  The kernel is qattn_merge_body.h with QATTN_MERGE_SINK on, a unit of
// its own so that qattn_merge.hip's kernels keep their device code; N = 1 exists here (one state and the sink).  The sink is a kernel
// argument of its own: MergeParams is what it was.
#include "qattn_merge_dev.h"
#include "../../include/qattn_sinks.h"

namespace qattn {

template <int D, int N>
__global__ __launch_bounds__(256) void merge_states_sink_kernel(const MergeParams p, const float* __restrict__ sink) {
#define QATTN_MERGE_SINK 1
#include "qattn_merge_body.h"
#undef QATTN_MERGE_SINK
}

template <int D>
static void launch_merge_sink(int n, const MergeParams& p, const float* sink, dim3 grid, hipStream_t st) {
    switch (n) {
#define QATTN_MERGE_CASE(NN) case NN: hipLaunchKernelGGL((merge_states_sink_kernel<D, NN>), grid, dim3(256), 0, st, p, sink); break
        QATTN_MERGE_CASE(1);
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

extern "C" int qattn_attention_state_merge_sink(int n, const void* const* o, const int* o_fmt, const long long* o_strides,
                                                const float* const* lse, const long long* lse_strides, void* out, int out_fmt,
                                                const long long* out_strides, float* lse_out, const long long* lse_out_strides, int B, int H,
                                                int S, int D, void* stream, const float* sink) {
    MergeParams p;
    dim3 grid;
    const int rc = merge_check_and_fill(1, n, o, o_fmt, o_strides, lse, lse_strides, out, out_fmt, out_strides, lse_out, lse_out_strides, B, H, S,
                                        D, p, grid);
    if (rc != QATTN_OK) return rc;
    if (!sink || (size_t)sink % 4 != 0) return QATTN_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (D == 64) launch_merge_sink<64>(n, p, sink, grid, st);
    else if (D == 128) launch_merge_sink<128>(n, p, sink, grid, st);
    else launch_merge_sink<256>(n, p, sink, grid, st);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

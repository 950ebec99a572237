// qattn_paged_varlen_rope_pos_append.hip -- the rotary embedding at the CALLER's positions (include/qattn_paged_varlen_rope_pos.h), gfx950:
//   qattn_paged_kv_cache_append_varlen_rope_pos_fp8   the rotating packed append of qattn_paged_varlen_rope_append.hip with the table row of
//                                                     a key taken from positions[token] instead of from the key's index
//   qattn_rope_packed_positions                       packed rows [total, H, D] (q) rotated at positions[row], 16-bit out
//
// The append kernel is a fifth compilation of qattn_kvcache_append_body.h (QATTN_KVA_POS on top of QATTN_KVA_ROPE): one line differs, the
// one that forms a key's table row.  The row kernel is rope_paged_varlen_kernel without its slot search.  Both share qattn_rope_dev.h with
// the units that rotate at the cache's positions, so equal positions give equal bits.
#include "qattn_kvcache_append.h"
#include "qattn_rope_dev.h"
#include "../../include/qattn_paged_varlen_rope_pos.h"

namespace qattn {

// grid = (Hkv NS, 2), block = 256.  blockIdx.y: 0 = K (rotated), 1 = V.  blockIdx.x = h NS + j: chunk slot j of kv head h.
template <int D, int IN_FMT, int OUT_FMT, bool IL>
__global__ __launch_bounds__(256) void kv_paged_varlen_rope_pos_append_kernel(const KvAppendArgs a, const KvPages pg, const KvVarq vq, const KvRope rp,
                                                                              const KvPos ps) {
#define QATTN_KVA_PAGED 1
#define QATTN_KVA_VARQ 1
#define QATTN_KVA_ROPE 1
#define QATTN_KVA_POS 1
#include "qattn_kvcache_append_body.h"
#undef QATTN_KVA_POS
#undef QATTN_KVA_ROPE
#undef QATTN_KVA_VARQ
#undef QATTN_KVA_PAGED
}

struct RopePosArgs {
    const uint4* x;          // [total, H, D] 16-bit through st / sh (16-byte vectors between tokens, heads)
    uint4* out;              // [total, H, D] dense
    const long long* pos;    // [total]
    KvRope rp;
    long st, sh;
    long units;              // total H D/16
    int H;
};

// One unit (row, head, dvh) per thread; grid = ceil(units / 256), block = 256.  Row `row` rotates with table row clamp(pos[row], 0, T - 1).
template <int IN_FMT, bool IL>
__global__ __launch_bounds__(256) void rope_packed_positions_kernel(const RopePosArgs g, int D) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.units) return;
    const int hv = D >> 4;   // units per row
    const long rh = idx / hv;
    const int dvh = (int)(idx - rh * hv);
    const int row = (int)(rh / g.H), h = (int)(rh - (long)row * g.H);
    const long long want = g.pos[row];
    const long pos = want < 0 ? 0 : want < g.rp.T ? (long)want : (long)g.rp.T - 1;
    const uint4* px = g.x + (long)row * g.st + (long)h * g.sh + dvh;
    uint4 A = load_nt(px), Bv = load_nt(px + hv);
    const float4* cg = reinterpret_cast<const float4*>(g.rp.cs) + pos * (g.rp.tr >> 2);
    const float4* sg = reinterpret_cast<const float4*>(g.rp.sn) + pos * (g.rp.tr >> 2);
    const int t0 = IL ? dvh : 2 * dvh, t1 = IL ? dvh + hv : 2 * dvh + 1;
    const float4 c[2] = {cg[t0], cg[t1]}, s[2] = {sg[t0], sg[t1]};
    rope_unit<IN_FMT, IL>(A, Bv, c, s);
    uint4* po = g.out + rh * (2 * hv) + dvh;
    po[0] = A;
    po[hv] = Bv;
}

template <int D, int IN, int OUT>
static void launch_kv_rope_pos_append2(const KvAppendArgs& a, const KvPages& pg, const KvVarq& vq, const KvRope& rp, const KvPos& ps, bool il,
                                       dim3 grid, hipStream_t st) {
    dim3 block(256);
    if (il) hipLaunchKernelGGL((kv_paged_varlen_rope_pos_append_kernel<D, IN, OUT, true>), grid, block, 0, st, a, pg, vq, rp, ps);
    else hipLaunchKernelGGL((kv_paged_varlen_rope_pos_append_kernel<D, IN, OUT, false>), grid, block, 0, st, a, pg, vq, rp, ps);
}

template <int D>
static int launch_kv_rope_pos_append(const KvAppendArgs& a, const KvPages& pg, const KvVarq& vq, const KvRope& rp, const KvPos& ps, int in_fmt,
                                     int fp8_fmt, bool il, dim3 grid, hipStream_t st) {
    if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E4M3) launch_kv_rope_pos_append2<D, QATTN_FMT_BF16, QATTN_FMT_E4M3>(a, pg, vq, rp, ps, il, grid, st);
    else if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E5M2) launch_kv_rope_pos_append2<D, QATTN_FMT_BF16, QATTN_FMT_E5M2>(a, pg, vq, rp, ps, il, grid, st);
    else if (in_fmt == QATTN_FMT_FP16 && fp8_fmt == QATTN_FMT_E4M3) launch_kv_rope_pos_append2<D, QATTN_FMT_FP16, QATTN_FMT_E4M3>(a, pg, vq, rp, ps, il, grid, st);
    else if (in_fmt == QATTN_FMT_FP16 && fp8_fmt == QATTN_FMT_E5M2) launch_kv_rope_pos_append2<D, QATTN_FMT_FP16, QATTN_FMT_E5M2>(a, pg, vq, rp, ps, il, grid, st);
    else return QATTN_ERR_UNSUPPORTED_FMT;
    return QATTN_OK;
}

// one table pair for every token: both bases 16-byte aligned (float4 loads), the row stride a non-negative multiple of 4 floats, T >= 1
static bool rope_pos_table_ok(const float* c, const float* s, long long tr, int T, int interleaved) {
    return c && s && ((uintptr_t)c & 15) == 0 && ((uintptr_t)s & 15) == 0 && tr >= 0 && tr % 4 == 0 && T >= 1 && (interleaved == 0 || interleaved == 1);
}

}  // namespace qattn

using namespace qattn;

extern "C" int qattn_paged_kv_cache_append_varlen_rope_pos_fp8(const void* k16, const void* v16, int in_fmt, const long long* k_strides2,
                                                               const long long* v_strides2, void* k_pool, void* v_pool, const float* scale_k,
                                                               const float* scale_v, const int* block_table, long long table_stride,
                                                               int* seqlens, const int* cu_seqlens, int advance, int B, int Hkv, int total,
                                                               int num_pages, int page_size, int max_pages, int D, int fp8_fmt,
                                                               const float* cos, const float* sin, long long table_row_stride, int T,
                                                               int interleaved, const long long* positions, void* stream) {
    KvAppendArgs a;
    KvPages pg;
    KvVarq vq;
    const int ok = kv_varlen_append_args(k16, v16, in_fmt, k_strides2, v_strides2, k_pool, v_pool, scale_k, scale_v, block_table, table_stride, seqlens,
                                         cu_seqlens, B, Hkv, total, num_pages, page_size, max_pages, D, fp8_fmt, a, pg, vq);
    if (ok != QATTN_OK) return ok;
    if (!rope_pos_table_ok(cos, sin, table_row_stride, T, interleaved)) return QATTN_ERR_INVALID_ARG;
    if (!positions || (size_t)positions % 8 != 0) return QATTN_ERR_INVALID_ARG;
    if (total == 0) return QATTN_OK;   // nothing launched, nothing written
    KvRope rp;
    rp.cs = cos; rp.sn = sin; rp.tr = (long)table_row_stride; rp.T = T;
    KvPos ps;
    ps.pos = positions;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)((long long)vq.NS * Hkv), 2, 1);
    const bool il = interleaved != 0;
    int rc;
    if (D == 64) rc = launch_kv_rope_pos_append<64>(a, pg, vq, rp, ps, in_fmt, fp8_fmt, il, grid, st);
    else if (D == 128) rc = launch_kv_rope_pos_append<128>(a, pg, vq, rp, ps, in_fmt, fp8_fmt, il, grid, st);
    else rc = launch_kv_rope_pos_append<256>(a, pg, vq, rp, ps, in_fmt, fp8_fmt, il, grid, st);
    if (rc != QATTN_OK) return rc;
    if (advance) kv_launch_varlen_advance(seqlens, cu_seqlens, B, total, a.capacity, st);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

extern "C" int qattn_rope_packed_positions(const void* x16, int in_fmt, const long long* x_strides2, void* out16, const long long* positions,
                                           int H, int total, int D, const float* cos, const float* sin, long long table_row_stride, int T,
                                           int interleaved, void* stream) {
    if (!x16 || !x_strides2 || !out16 || !positions) return QATTN_ERR_INVALID_ARG;
    if ((size_t)positions % 8 != 0) return QATTN_ERR_INVALID_ARG;
    if (H <= 0 || total < 0) return QATTN_ERR_INVALID_ARG;
    if (D != 64 && D != 128 && D != 256) return QATTN_ERR_UNSUPPORTED_DIM;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (((size_t)x16 | (size_t)out16) % 16 != 0) return QATTN_ERR_INVALID_ARG;   // rows: 16-byte loads and stores
    for (int i = 0; i < 2; i++)   // (a negative stride would read in front of the base pointer)
        if (x_strides2[i] < 0 || x_strides2[i] % 8 != 0) return QATTN_ERR_INVALID_ARG;
    if (!rope_pos_table_ok(cos, sin, table_row_stride, T, interleaved)) return QATTN_ERR_INVALID_ARG;
    const long long units = (long long)total * H * (D / 16);
    if ((units + 255) / 256 > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (one thread per unit: a 32-bit grid)
    if (total == 0) return QATTN_OK;   // nothing launched, nothing written
    RopePosArgs g;
    g.x = (const uint4*)x16; g.out = (uint4*)out16; g.pos = positions;
    g.rp.cs = cos; g.rp.sn = sin; g.rp.tr = (long)table_row_stride; g.rp.T = T;
    g.st = (long)(x_strides2[0] / 8); g.sh = (long)(x_strides2[1] / 8);
    g.units = (long)units;
    g.H = H;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)((units + 255) / 256)), block(256);
    const bool il = interleaved != 0;
    if (in_fmt == QATTN_FMT_BF16) {
        if (il) hipLaunchKernelGGL((rope_packed_positions_kernel<QATTN_FMT_BF16, true>), grid, block, 0, st, g, D);
        else hipLaunchKernelGGL((rope_packed_positions_kernel<QATTN_FMT_BF16, false>), grid, block, 0, st, g, D);
    } else {
        if (il) hipLaunchKernelGGL((rope_packed_positions_kernel<QATTN_FMT_FP16, true>), grid, block, 0, st, g, D);
        else hipLaunchKernelGGL((rope_packed_positions_kernel<QATTN_FMT_FP16, false>), grid, block, 0, st, g, D);
    }
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

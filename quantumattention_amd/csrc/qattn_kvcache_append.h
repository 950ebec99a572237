// qattn_kvcache_append.h -- the append kernel of an FP8 K/V cache with fixed scales, shared by the two entries that differ only in WHERE a
// touched 64-key chunk is stored: qattn_kv_cache_append_fp8 (qattn_kvcache_append.hip: contiguous images, include/qattn_kvcache.h) and
// qattn_paged_kv_cache_append_fp8 (qattn_paged_append.hip: pages of a pool behind a block table, include/qattn_paged.h).  The kernel
// body is qattn_kvcache_append_body.h, compiled once per chunk address (`og`); each unit instantiates its own kernels only, and the
// contiguous kernel is, statement for statement, the kernel qattn_kvcache_append.hip held before the paged entry existed.
#pragma once
#include <type_traits>

#include "qattn_common.h"

#include "../../include/qattn_kvcache.h"

namespace qattn {

struct KvAppendArgs {
    const uint4* x[2];         // k16, v16
    unsigned char* img[2];     // KFRAG image of K, VFRAG image of V: [B Hkv][Sp / 64][64 D bytes]
    const float* scale[2];     // [B Hkv]
    long sb[2], sh[2], st[2];  // batch / head / token strides of x in 16-byte vectors
    const int* seqlens;        // [B]
    const int* new_lens;       // [B] or nullptr
    int Hkv, T, capacity, nchunk;   // nchunk = ceil(T / 64) + 1: the most chunks T consecutive keys touch
};

// PAGED: the block table (include/qattn_paged.h).  Chunk c of sequence b's kv head h is chunk c % pc of page clamp(table[b][c / pc])
struct KvPages {
    const int* table;   // [B][stride]
    long stride;
    int num_pages, pc;  // pages of the pool; 64-key chunks per page
};

// PACKED tokens (include/qattn_paged_varlen_append.h): sequence i owns the rows clamp(cu[i], 0, total) .. clamp(cu[i + 1], that, total) of
// x [total, Hkv, D]; NS = 2 B + total / 64 chunk slots per kv head (the kernel of qattn_paged_varlen_append.hip)
struct KvVarq {
    const int* cu;   // [B + 1]
    int B, total, NS;
};

// ROTATED keys (include/qattn_paged_varlen_rope.h): key j of every slot rotates with row min(j, T - 1) of cos / sin [T, D/2] fp32
struct KvRope {
    const float* cs;
    const float* sn;
    long tr;   // floats between table rows (a multiple of 4)
    int T;
};

// POSITIONS (include/qattn_paged_varlen_rope_pos.h): the table row of a rotated key from the caller -- one 64-bit position per packed
// token, [total] on the device, clamped into [0, T - 1] where it is read
struct KvPos {
    const long long* pos;
};

__device__ __forceinline__ int kv_clampi(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }

// the appended keys of batch element b: [p, p + n) cut at the capacity
__device__ __forceinline__ void kv_append_range(const int* seqlens, const int* new_lens, int b, int T, int capacity, int& p, int& end) {
    p = seqlens[b];
    p = p < 0 ? 0 : p > capacity ? capacity : p;
    int n = T;
    if (new_lens) { n = new_lens[b]; n = n < 0 ? 0 : n > T ? T : n; }
    end = capacity - p >= n ? p + n : capacity;
}

// an inf or a NaN among the 8 16-bit elements of a vector (all exponent bits set).  The scale here is finite whatever the data hold, so
// quant8 has to be told (force_exact): its bf16 fast path relies on a scale derived from the data's abs-max, which such an element makes NaN
template <int IN_FMT>
__device__ __forceinline__ bool has_nonfinite16(const uint4& raw) {
    constexpr unsigned E = IN_FMT == QATTN_FMT_BF16 ? 0x7f80u : 0x7c00u;
    const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
    bool any = false;
#pragma unroll
    for (int i = 0; i < 4; i++) any = any || ((w[i] & E) == E) || ((w[i] & (E << 16)) == (E << 16));
    return any;
}

// grid = (B Hkv nchunk, 2), block = 256.  blockIdx.y: 0 = K, 1 = V.  blockIdx.x = (b Hkv + h) nchunk + c: the c-th chunk from the one that
// holds key p_b.
template <int D, int IN_FMT, int OUT_FMT>
__global__ __launch_bounds__(256) void kv_append_kernel(const KvAppendArgs a) {
#define QATTN_KVA_PAGED 0
#define QATTN_KVA_VARQ 0
#define QATTN_KVA_ROPE 0
#include "qattn_kvcache_append_body.h"
#undef QATTN_KVA_ROPE
#undef QATTN_KVA_VARQ
#undef QATTN_KVA_PAGED
}

template <int D, int IN_FMT, int OUT_FMT>
__global__ __launch_bounds__(256) void kv_paged_append_kernel(const KvAppendArgs a, const KvPages pg) {
#define QATTN_KVA_PAGED 1
#define QATTN_KVA_VARQ 0
#define QATTN_KVA_ROPE 0
#include "qattn_kvcache_append_body.h"
#undef QATTN_KVA_ROPE
#undef QATTN_KVA_VARQ
#undef QATTN_KVA_PAGED
}

// kv_advance_kernel's launch (qattn_kvcache_append.hip): the second launch of an advancing call
void kv_launch_advance(int* seqlens, const int* new_lens, int B, int T, int capacity, hipStream_t st);

// kv_varlen_advance_kernel's launch (qattn_paged_varlen_append.hip): the second launch of an advancing packed call
void kv_launch_varlen_advance(int* seqlens, const int* cu, int B, int total, int capacity, hipStream_t st);

// The argument checks of the packed append (include/qattn_paged_varlen_append.h) and its argument structs, shared by its entries
// (qattn_paged_varlen_append.hip, qattn_paged_varlen_rope_append.hip).  QATTN_OK with total = 0: nothing is to be launched.
inline int kv_varlen_append_args(const void* k16, const void* v16, int in_fmt, const long long* k_strides2, const long long* v_strides2,
                                 void* k_pool, void* v_pool, const float* scale_k, const float* scale_v, const int* block_table,
                                 long long table_stride, int* seqlens, const int* cu_seqlens, int B, int Hkv, int total, int num_pages,
                                 int page_size, int max_pages, int D, int fp8_fmt, KvAppendArgs& a, KvPages& pg, KvVarq& vq) {
    // the paging arguments, as qattn_paged_kv_cache_append_fp8 checks them
    if (!block_table || (size_t)block_table % 4 != 0) return QATTN_ERR_INVALID_ARG;
    if (num_pages <= 0 || max_pages <= 0 || Hkv <= 0 || page_size < 64 || page_size % 64 != 0) return QATTN_ERR_INVALID_ARG;
    if (table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    const int pc = page_size / 64;
    if ((long long)num_pages * Hkv * pc > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (the physical chunk index is an int)
    const long long capacity = (long long)max_pages * page_size;
    if (capacity > 0x7fffffffLL - 64) return QATTN_ERR_INVALID_ARG;   // (p_i + n_i stays in 32 bits)
    // the packed arguments
    if (!cu_seqlens || (size_t)cu_seqlens % 4 != 0) return QATTN_ERR_INVALID_ARG;
    if (total < 0) return QATTN_ERR_INVALID_ARG;
    // kv_append's checks (qattn_kvcache_append.h), T > 0 excepted
    if (!k16 || !v16 || !k_strides2 || !v_strides2 || !k_pool || !v_pool || !scale_k || !scale_v || !seqlens) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || D <= 0) return QATTN_ERR_INVALID_ARG;
    if (D != 64 && D != 128 && D != 256) return QATTN_ERR_UNSUPPORTED_DIM;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (((size_t)k_pool | (size_t)v_pool) % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if (((size_t)k16 | (size_t)v16) % 16 != 0) return QATTN_ERR_INVALID_ARG;   // rows: 16-byte loads
    for (int i = 0; i < 2; i++)   // (a negative stride would read in front of the base pointer)
        if (k_strides2[i] < 0 || v_strides2[i] < 0 || k_strides2[i] % 8 != 0 || v_strides2[i] % 8 != 0) return QATTN_ERR_INVALID_ARG;
    const long long NS = 2LL * B + total / 64;   // chunk slots per kv head
    if (NS * Hkv > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (one workgroup per (kv head, slot): a 32-bit grid; NS itself an int)
    a.x[0] = (const uint4*)k16; a.x[1] = (const uint4*)v16;
    a.img[0] = (unsigned char*)k_pool; a.img[1] = (unsigned char*)v_pool;
    a.scale[0] = scale_k; a.scale[1] = scale_v;
    a.sb[0] = a.sb[1] = 0;   // (no batch axis: the sequence's rows start at start_i)
    a.st[0] = (long)(k_strides2[0] / 8); a.sh[0] = (long)(k_strides2[1] / 8);
    a.st[1] = (long)(v_strides2[0] / 8); a.sh[1] = (long)(v_strides2[1] / 8);
    a.seqlens = seqlens; a.new_lens = nullptr;
    a.Hkv = Hkv; a.T = total; a.capacity = (int)capacity; a.nchunk = (int)NS;
    pg.table = block_table; pg.stride = (long)table_stride; pg.num_pages = num_pages; pg.pc = pc;
    vq.cu = cu_seqlens; vq.B = B; vq.total = total; vq.NS = (int)NS;
    return QATTN_OK;
}

template <int D, bool PAGED>
static int launch_kv_append(const KvAppendArgs& a, const KvPages& pg, int in_fmt, int fp8_fmt, dim3 grid, hipStream_t st) {
    dim3 block(256);
    auto go = [&](auto in, auto out) {
        if constexpr (PAGED) hipLaunchKernelGGL((kv_paged_append_kernel<D, decltype(in)::value, decltype(out)::value>), grid, block, 0, st, a, pg);
        else hipLaunchKernelGGL((kv_append_kernel<D, decltype(in)::value, decltype(out)::value>), grid, block, 0, st, a);
    };
    using BF16 = std::integral_constant<int, QATTN_FMT_BF16>;
    using FP16 = std::integral_constant<int, QATTN_FMT_FP16>;
    using E4M3 = std::integral_constant<int, QATTN_FMT_E4M3>;
    using E5M2 = std::integral_constant<int, QATTN_FMT_E5M2>;
    if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E4M3) go(BF16{}, E4M3{});
    else if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E5M2) go(BF16{}, E5M2{});
    else if (in_fmt == QATTN_FMT_FP16 && fp8_fmt == QATTN_FMT_E4M3) go(FP16{}, E4M3{});
    else if (in_fmt == QATTN_FMT_FP16 && fp8_fmt == QATTN_FMT_E5M2) go(FP16{}, E5M2{});
    else return QATTN_ERR_UNSUPPORTED_FMT;
    return QATTN_OK;
}

// Both entries, from their common arguments on: the images of [B, Hkv, capacity, D] or -- PAGED, with pg filled in and checked by the
// caller and capacity = max_pages page_size -- the pools.
template <bool PAGED>
int kv_append(const void* k16, const void* v16, int in_fmt, const long long* k_strides3, const long long* v_strides3, void* k8, void* v8,
              const KvPages& pg, const float* scale_k, const float* scale_v, int* seqlens, const int* new_lens, int advance, int B, int Hkv,
              int T, int capacity, int D, int fp8_fmt, void* stream) {
    if (!k16 || !v16 || !k_strides3 || !v_strides3 || !k8 || !v8 || !scale_k || !scale_v || !seqlens) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || Hkv <= 0 || T <= 0 || capacity <= 0 || D <= 0) return QATTN_ERR_INVALID_ARG;
    if (D != 64 && D != 128 && D != 256) return QATTN_ERR_UNSUPPORTED_DIM;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (((size_t)k8 | (size_t)v8) % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if (((size_t)k16 | (size_t)v16) % 16 != 0) return QATTN_ERR_INVALID_ARG;   // rows: 16-byte loads
    for (int i = 0; i < 3; i++)   // (a negative stride would read in front of the base pointer)
        if (k_strides3[i] < 0 || v_strides3[i] < 0 || k_strides3[i] % 8 != 0 || v_strides3[i] % 8 != 0) return QATTN_ERR_INVALID_ARG;
    if (capacity > 0x7fffffff - 64) return QATTN_ERR_INVALID_ARG;   // (p_b + n_b and the padded length stay in 32 bits)
    const int nchunk = (int)(((long long)T + 63) / 64 + 1);
    if ((long long)B * Hkv * nchunk > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (one workgroup per (b, kv head, chunk): a 32-bit grid)
    KvAppendArgs a;
    a.x[0] = (const uint4*)k16; a.x[1] = (const uint4*)v16;
    a.img[0] = (unsigned char*)k8; a.img[1] = (unsigned char*)v8;
    a.scale[0] = scale_k; a.scale[1] = scale_v;
    a.sb[0] = (long)(k_strides3[0] / 8); a.sh[0] = (long)(k_strides3[1] / 8); a.st[0] = (long)(k_strides3[2] / 8);
    a.sb[1] = (long)(v_strides3[0] / 8); a.sh[1] = (long)(v_strides3[1] / 8); a.st[1] = (long)(v_strides3[2] / 8);
    a.seqlens = seqlens; a.new_lens = new_lens;
    a.Hkv = Hkv; a.T = T; a.capacity = capacity; a.nchunk = nchunk;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)(B * Hkv * nchunk), 2, 1);
    int rc;
    if (D == 64) rc = launch_kv_append<64, PAGED>(a, pg, in_fmt, fp8_fmt, grid, st);
    else if (D == 128) rc = launch_kv_append<128, PAGED>(a, pg, in_fmt, fp8_fmt, grid, st);
    else rc = launch_kv_append<256, PAGED>(a, pg, in_fmt, fp8_fmt, grid, st);
    if (rc != QATTN_OK) return rc;
    if (advance) kv_launch_advance(seqlens, new_lens, B, T, capacity, st);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

}  // namespace qattn

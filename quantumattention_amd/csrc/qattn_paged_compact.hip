// qattn_paged_compact.hip -- qattn_paged_kv_cache_compact_fp8 (include/qattn_paged_varlen_tree.h): after a tree-shaped speculative step,
// the accepted root-to-leaf path of every slot becomes the contiguous tail of its keys in the paged FP8 K/V cache, gfx950.
//
// A slot's draft tokens are its last Sq_b <= 64 keys: they lie in at most two 64-key chunks, which may lie in two pages.  One workgroup
// per (slot, kv head, K or V) stages those chunks in LDS, waits at a barrier, and then stores the destination keys from LDS: every read
// of the pool precedes every write, so any index list is well defined.  The scales are fixed per (slot, head): bytes move unchanged.
// K moves as the 16-byte pieces of a key (KFRAG), V as the bytes of a key -- whole words where all four keys of a word are destinations
// (VFRAG); the layouts are stated in qattn_common.h and qattn_kvcache_append_body.h.  seqlens is written by a launch of its own behind
// the move (stream order), as the append's advance is, so that no workgroup reads a rewritten length.
#include "qattn_kvcache_append.h"
#include "../../include/qattn_paged_varlen_tree.h"

namespace qattn {

struct KvCompactArgs {
    unsigned char* img[2];    // the K pool (KFRAG chunks) and the V pool (VFRAG chunks)
    const int* seqlens;       // [B]
    const int* cu;            // cu_seqlens [B + 1]
    const int* accept_index;  // [total]
    const int* accept_lens;   // [B]
    int Hkv, total, capacity;
};

// The slot's draft region: true iff it is compactable (1 <= Sq_b <= 64 and L_b >= Sq_b); then its tokens start at `start`, its first
// draft key is `base` and n of the Sq drafts are kept.  (Workgroup-uniform; every value is clamped, so nothing leaves the tensors.)
__device__ __forceinline__ bool kv_compact_slot(const int* seqlens, const int* cu, const int* accept_lens, int b, int total, int capacity,
                                                int& start, int& Sq, int& base, int& n) {
    start = kv_clampi(cu[b], 0, total);
    Sq = kv_clampi(cu[b + 1], start, total) - start;
    const int L = kv_clampi(seqlens[b], 0, capacity);
    if (Sq < 1 || Sq > 64 || L < Sq) return false;
    base = L - Sq;
    n = kv_clampi(accept_lens[b], 0, Sq);
    return true;
}

// grid = (B Hkv, 2), block = 256.  blockIdx.y: 0 = K, 1 = V.  blockIdx.x = b Hkv + h.
template <int D>
__global__ __launch_bounds__(256) void kv_paged_compact_kernel(const KvCompactArgs a, const KvPages pg) {
    constexpr int CH = 64 * D;   // bytes of a chunk
    __shared__ __attribute__((aligned(16))) unsigned char img[2 * CH];
    __shared__ int sidx[64];
    const int tid = threadIdx.x, z = blockIdx.y;
    const int b = (int)(blockIdx.x / (unsigned)a.Hkv), h = (int)(blockIdx.x % (unsigned)a.Hkv);
    int start, Sq, base, n;
    if (!kv_compact_slot(a.seqlens, a.cu, a.accept_lens, b, a.total, a.capacity, start, Sq, base, n)) return;
    if (n == 0) return;   // nothing is kept: only the length changes
    // the drafts are the keys [base, base + Sq) of the chunks c0 and c1 <= c0 + 1, both below ceil(L / 64) <= max_pages pc
    const int c0 = base >> 6, nc = ((base + Sq - 1) >> 6) - c0 + 1;
    // token start + i < start + Sq <= total
    if (tid < n) sidx[tid] = kv_clampi(a.accept_index[start + tid], 0, Sq - 1);
    unsigned char* og[2];
#pragma unroll
    for (int cc = 0; cc < 2; cc++) {
        const int c = c0 + (cc < nc ? cc : 0);
        int page = pg.table[(long)b * pg.stride + c / pg.pc];
        page = page < 0 ? 0 : page > pg.num_pages - 1 ? pg.num_pages - 1 : page;   // (the append's clamp: the chunk stays inside the pool)
        og[cc] = a.img[z] + (((long)page * a.Hkv + h) * pg.pc + c % pg.pc) * (long)CH;
        if (cc < nc)
            for (int i = tid; i < CH / 16; i += 256) reinterpret_cast<uint4*>(img + cc * CH)[i] = reinterpret_cast<const uint4*>(og[cc])[i];
    }
    __syncthreads();
    if (z == 0) {
        // key base + i takes the D / 16 pieces of key base + idx_i
        for (int u = tid; u < n * (D / 16); u += 256) {
            const int i = u / (D / 16), d0 = 16 * (u % (D / 16));
            const int dk = base + i, sk = base + sidx[i];
            const int dc = (dk >> 6) - c0, sc = (sk >> 6) - c0;   // 0 or 1, below nc
            *reinterpret_cast<uint4*>((dc ? og[1] : og[0]) + kfrag_offset<D>(dk & 63, d0)) =
                *reinterpret_cast<const uint4*>(img + sc * CH + kfrag_offset<D>(sk & 63, d0));
        }
    } else {
        // word wd of a VFRAG chunk = [m:D/32][hh:2][half:2][d:32][w:4] holds channel 32 m + d of the 4 keys 32 half + 8 w + 4 hh + (0..3):
        // a word store where all four are destinations, byte stores of the destinations otherwise -- the others' bytes are not written
        for (int x = tid; x < nc * (CH / 4); x += 256) {
            const int cc = x / (CH / 4), wd = x % (CH / 4);
            const int w = wd & 3, dl = (wd >> 2) & 31, half = (wd >> 7) & 1, hh = (wd >> 8) & 1, m = wd >> 9;
            const int di0 = 64 * (c0 + cc) + 32 * half + 8 * w + 4 * hh - base;   // the word's first key as a draft index
            if (di0 + 4 <= 0 || di0 >= n) continue;
            unsigned bytes[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                bytes[i] = 0;
                if (di0 + i >= 0 && di0 + i < n) {
                    const int sk = base + sidx[di0 + i];
                    bytes[i] = img[((sk >> 6) - c0) * CH + vfrag_offset<D>(sk & 63, 32 * m + dl)];
                }
            }
            unsigned char* dst = (cc ? og[1] : og[0]) + 4 * wd;
            if (di0 >= 0 && di0 + 4 <= n) {
                *reinterpret_cast<unsigned*>(dst) = bytes[0] | (bytes[1] << 8) | (bytes[2] << 16) | (bytes[3] << 24);
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (di0 + i >= 0 && di0 + i < n) dst[i] = (unsigned char)bytes[i];
            }
        }
    }
}

// the second launch (stream order puts it behind every workgroup that had to read the old lengths): one thread per slot
__global__ __launch_bounds__(256) void kv_compact_lens_kernel(int* seqlens, const int* cu, const int* accept_lens, int B, int total,
                                                              int capacity) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int start, Sq, base, n;
    if (kv_compact_slot(seqlens, cu, accept_lens, b, total, capacity, start, Sq, base, n)) seqlens[b] = base + n;
}

}  // namespace qattn

using namespace qattn;

extern "C" int qattn_paged_kv_cache_compact_fp8(void* k_pool, void* v_pool, const int* block_table, long long table_stride, int* seqlens,
                                                const int* cu_seqlens, const int* accept_index, const int* accept_lens, int B, int Hkv,
                                                int total, int num_pages, int page_size, int max_pages, int D, void* stream) {
    // the paging arguments, as qattn_paged_kv_cache_append_varlen_fp8 checks them
    if (!block_table || (size_t)block_table % 4 != 0) return QATTN_ERR_INVALID_ARG;
    if (num_pages <= 0 || max_pages <= 0 || Hkv <= 0 || page_size < 64 || page_size % 64 != 0) return QATTN_ERR_INVALID_ARG;
    if (table_stride < max_pages) return QATTN_ERR_INVALID_ARG;
    const int pc = page_size / 64;
    if ((long long)num_pages * Hkv * pc > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (the physical chunk index is an int)
    const long long capacity = (long long)max_pages * page_size;
    if (capacity > 0x7fffffffLL - 64) return QATTN_ERR_INVALID_ARG;
    if (!cu_seqlens || !accept_index || !accept_lens || !seqlens) return QATTN_ERR_INVALID_ARG;
    if (((size_t)cu_seqlens | (size_t)accept_index | (size_t)accept_lens | (size_t)seqlens) % 4 != 0) return QATTN_ERR_INVALID_ARG;
    if (total < 0 || B <= 0) return QATTN_ERR_INVALID_ARG;
    if (!k_pool || !v_pool || ((size_t)k_pool | (size_t)v_pool) % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if (D != 64 && D != 128 && D != 256) return QATTN_ERR_UNSUPPORTED_DIM;
    if ((long long)B * Hkv > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (one workgroup per (slot, kv head): a 32-bit grid)
    if (total == 0) return QATTN_OK;   // no draft token: nothing launched, nothing written
    KvCompactArgs a;
    a.img[0] = (unsigned char*)k_pool; a.img[1] = (unsigned char*)v_pool;
    a.seqlens = seqlens; a.cu = cu_seqlens; a.accept_index = accept_index; a.accept_lens = accept_lens;
    a.Hkv = Hkv; a.total = total; a.capacity = (int)capacity;
    KvPages pg;
    pg.table = block_table; pg.stride = (long)table_stride; pg.num_pages = num_pages; pg.pc = pc;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)(B * Hkv), 2, 1), block(256);
    if (D == 64) hipLaunchKernelGGL(kv_paged_compact_kernel<64>, grid, block, 0, st, a, pg);
    else if (D == 128) hipLaunchKernelGGL(kv_paged_compact_kernel<128>, grid, block, 0, st, a, pg);
    else hipLaunchKernelGGL(kv_paged_compact_kernel<256>, grid, block, 0, st, a, pg);
    hipLaunchKernelGGL(kv_compact_lens_kernel, dim3((unsigned)((B + 255) / 256)), block, 0, st, seqlens, cu_seqlens, accept_lens, B, total,
                       (int)capacity);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

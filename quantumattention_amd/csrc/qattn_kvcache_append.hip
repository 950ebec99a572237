// qattn_kvcache_append.hip -- appending tokens to an FP8 K/V cache with fixed scales (include/qattn_kvcache.h), gfx950.
//
// quant_multi_kernel's tile (qattn_quant.hip) with three differences: the scale is the cache's, not the tensor's abs-max; the first key is
// read from seqlens on the device, so the tokens of a call do not start at a chunk boundary; and a chunk that the call covers only in
// part is stored key by key, because the bytes of the keys that are already there must not change.  quant8, the LDS staging images and the
// copy-out of a whole chunk (vfrag_copy_out) are qattn_common.h's.
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
    constexpr int VPR = D / 8;             // 16-byte input vectors per row
    constexpr int ITERS = 64 * VPR / 256;  // vectors per thread
    constexpr int KPAD = 64 * D + (64 * D / 512) * 16;  // KFRAG image + 16 B per 512 B     (the staging images of quant_multi_kernel)
    constexpr int VSTRIDE = D + 4;                      // VFRAG staging: fp8 row-major
    constexpr int LDS_BYTES = KPAD > 64 * VSTRIDE ? KPAD : 64 * VSTRIDE;
    __shared__ __attribute__((aligned(16))) unsigned char img[LDS_BYTES];
    const int tid = threadIdx.x, z = blockIdx.y;
    const int g = (int)(blockIdx.x / (unsigned)a.nchunk), ci = (int)(blockIdx.x % (unsigned)a.nchunk);
    const int b = g / a.Hkv, h = g % a.Hkv;
    int p, end;
    kv_append_range(a.seqlens, a.new_lens, b, a.T, a.capacity, p, end);
    const long key0 = 64L * (p / 64 + ci);   // first key of this workgroup's chunk
    if (p >= end || key0 >= end) return;     // (workgroup-uniform: nothing is appended -- new_lens 0, a full cache -- or nothing of this chunk)
    // the chunk's keys [lo, hi) are the tokens [key0 + lo - p, key0 + hi - p) of the call
    const int lo = p > key0 ? (int)(p - key0) : 0, hi = end - key0 < 64 ? (int)(end - key0) : 64;
    const float scale = a.scale[z][g];
    const float rinv = 1.0f / scale;
    const uint4* xg = a.x[z] + (long)b * a.sb[z] + (long)h * a.sh[z] + (key0 - p) * a.st[z];   // row of chunk key 0 (not touched below lo)
    const long st = a.st[z];
    uint4 held[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int vec = it * 256 + tid;
        const int r = vec / VPR;
        held[it] = make_uint4(0, 0, 0, 0);
        if (r >= lo && r < hi) held[it] = load_nt(xg + (long)r * st + vec % VPR);
    }
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const int vec = it * 256 + tid;
        const int r = vec / VPR, d0 = (vec % VPR) * 8;
        const int2 lohi = quant8<IN_FMT, OUT_FMT>(held[it], scale, rinv, has_nonfinite16<IN_FMT>(held[it]));   // NaN stays NaN, +-inf clamps to +-qmax
        if (z == 0) {
            const int o = kfrag_offset<D>(r, d0);
            *reinterpret_cast<int2*>(img + o + ((o >> 9) << 4)) = lohi;
        } else {
            *reinterpret_cast<int*>(img + r * VSTRIDE + d0) = lohi.x;
            *reinterpret_cast<int*>(img + r * VSTRIDE + d0 + 4) = lohi.y;
        }
    }
    __syncthreads();
    const long Sp = ((long)a.capacity + 63) / 64 * 64;
    unsigned char* og = a.img[z] + ((long)g * Sp + key0) * D;   // the chunk in the image
    const bool whole = lo == 0 && hi == 64;
    if (z == 0) {
        // piece i of a KFRAG chunk = [t:2][s:D/64][hh:2][half:2][key:32] holds 16 channels of ONE key, 32 t + key
        for (int i = tid; i < 64 * D / 16; i += 256) {
            const int r = 32 * (i / (2 * D)) + (i & 31);
            if (whole || (r >= lo && r < hi)) reinterpret_cast<uint4*>(og)[i] = *reinterpret_cast<const uint4*>(img + i * 16 + ((i >> 5) << 4));
        }
    } else if (whole) {
        vfrag_copy_out<D, VSTRIDE>(img, og, tid);
    } else {
        // word wd of a VFRAG chunk = [m:D/32][hh:2][half:2][d:32][w:4] holds channel 32 m + d of the 4 keys 32 half + 8 w + 4 hh + (0..3):
        // a word store where all four are appended, byte stores of the appended ones otherwise -- the others' bytes are neither read nor written
        for (int wd = tid; wd < 64 * D / 4; wd += 256) {
            const int w = wd & 3, dl = (wd >> 2) & 31, half = (wd >> 7) & 1, hh = (wd >> 8) & 1, m = wd >> 9;
            const int kb = 32 * half + 8 * w + 4 * hh;
            if (kb + 4 <= lo || kb >= hi) continue;
            const unsigned char* src = img + kb * VSTRIDE + 32 * m + dl;
            const unsigned b0 = src[0], b1 = src[VSTRIDE], b2 = src[2 * VSTRIDE], b3 = src[3 * VSTRIDE];
            if (kb >= lo && kb + 4 <= hi) {
                *reinterpret_cast<unsigned*>(og + 4 * wd) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
            } else {
                const unsigned bytes[4] = {b0, b1, b2, b3};
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (kb + i >= lo && kb + i < hi) og[4 * wd + i] = (unsigned char)bytes[i];
            }
        }
    }
}

// the second launch of an advancing call: stream order puts it behind every workgroup that had to read the old positions
__global__ __launch_bounds__(256) void kv_advance_kernel(int* seqlens, const int* new_lens, int B, int T, int capacity) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int p, end;
    kv_append_range(seqlens, new_lens, b, T, capacity, p, end);
    seqlens[b] = end;
}

template <int D>
static int launch_kv_append(const KvAppendArgs& a, int in_fmt, int fp8_fmt, dim3 grid, hipStream_t st) {
    dim3 block(256);
#define QATTN_KVA(IN, OUT) hipLaunchKernelGGL((kv_append_kernel<D, IN, OUT>), grid, block, 0, st, a)
    if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E4M3) QATTN_KVA(QATTN_FMT_BF16, QATTN_FMT_E4M3);
    else if (in_fmt == QATTN_FMT_BF16 && fp8_fmt == QATTN_FMT_E5M2) QATTN_KVA(QATTN_FMT_BF16, QATTN_FMT_E5M2);
    else if (in_fmt == QATTN_FMT_FP16 && fp8_fmt == QATTN_FMT_E4M3) QATTN_KVA(QATTN_FMT_FP16, QATTN_FMT_E4M3);
    else if (in_fmt == QATTN_FMT_FP16 && fp8_fmt == QATTN_FMT_E5M2) QATTN_KVA(QATTN_FMT_FP16, QATTN_FMT_E5M2);
    else return QATTN_ERR_UNSUPPORTED_FMT;
#undef QATTN_KVA
    return QATTN_OK;
}

}  // namespace qattn

using namespace qattn;

extern "C" int qattn_kv_cache_append_fp8(const void* k16, const void* v16, int in_fmt, const long long* k_strides3, const long long* v_strides3,
                                         void* k8_kfrag, void* v8_vfrag, const float* scale_k, const float* scale_v, int* seqlens,
                                         const int* new_lens, int advance, int B, int Hkv, int T, int capacity, int D, int fp8_fmt, void* stream) {
    if (!k16 || !v16 || !k_strides3 || !v_strides3 || !k8_kfrag || !v8_vfrag || !scale_k || !scale_v || !seqlens) return QATTN_ERR_INVALID_ARG;
    if (B <= 0 || Hkv <= 0 || T <= 0 || capacity <= 0 || D <= 0) return QATTN_ERR_INVALID_ARG;
    if (D != 64 && D != 128 && D != 256) return QATTN_ERR_UNSUPPORTED_DIM;
    if (in_fmt != QATTN_FMT_BF16 && in_fmt != QATTN_FMT_FP16) return QATTN_ERR_UNSUPPORTED_FMT;
    if (fp8_fmt != QATTN_FMT_E4M3 && fp8_fmt != QATTN_FMT_E5M2) return QATTN_ERR_UNSUPPORTED_FMT;
    if (((size_t)k8_kfrag | (size_t)v8_vfrag) % 16 != 0) return QATTN_ERR_INVALID_ARG;
    if (((size_t)k16 | (size_t)v16) % 16 != 0) return QATTN_ERR_INVALID_ARG;   // rows: 16-byte loads
    for (int i = 0; i < 3; i++)   // (a negative stride would read in front of the base pointer)
        if (k_strides3[i] < 0 || v_strides3[i] < 0 || k_strides3[i] % 8 != 0 || v_strides3[i] % 8 != 0) return QATTN_ERR_INVALID_ARG;
    if (capacity > 0x7fffffff - 64) return QATTN_ERR_INVALID_ARG;   // (p_b + n_b and the padded length stay in 32 bits)
    const int nchunk = (int)(((long long)T + 63) / 64 + 1);
    if ((long long)B * Hkv * nchunk > 0x7fffffffLL) return QATTN_ERR_INVALID_ARG;   // (one workgroup per (b, kv head, chunk): a 32-bit grid)
    KvAppendArgs a;
    a.x[0] = (const uint4*)k16; a.x[1] = (const uint4*)v16;
    a.img[0] = (unsigned char*)k8_kfrag; a.img[1] = (unsigned char*)v8_vfrag;
    a.scale[0] = scale_k; a.scale[1] = scale_v;
    a.sb[0] = (long)(k_strides3[0] / 8); a.sh[0] = (long)(k_strides3[1] / 8); a.st[0] = (long)(k_strides3[2] / 8);
    a.sb[1] = (long)(v_strides3[0] / 8); a.sh[1] = (long)(v_strides3[1] / 8); a.st[1] = (long)(v_strides3[2] / 8);
    a.seqlens = seqlens; a.new_lens = new_lens;
    a.Hkv = Hkv; a.T = T; a.capacity = capacity; a.nchunk = nchunk;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)(B * Hkv * nchunk), 2, 1);
    int rc;
    if (D == 64) rc = launch_kv_append<64>(a, in_fmt, fp8_fmt, grid, st);
    else if (D == 128) rc = launch_kv_append<128>(a, in_fmt, fp8_fmt, grid, st);
    else rc = launch_kv_append<256>(a, in_fmt, fp8_fmt, grid, st);
    if (rc != QATTN_OK) return rc;
    if (advance) hipLaunchKernelGGL(kv_advance_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, seqlens, new_lens, B, T, capacity);
    return hipGetLastError() == hipSuccess ? QATTN_OK : QATTN_ERR_LAUNCH;
}

// qattn_varlen_fp8.h -- what the packed FP8-PV units share: the tile shape, the attention launch's arguments and the small device helpers
// of attn_vfp8_kernel (qattn_varlen_fp8.hip), the entries' body there (argument checks, zeroing node, pre-pass launches, attention launch)
// and the sliding-window attention launch (qattn_varlen_window_fp8.hip) that the body runs behind its pre-pass.
#pragma once
#include "qattn_attn.h"

namespace qattn {

constexpr int kVfpTile = 128;   // query rows per workgroup
constexpr int kVfpWaves = 4;
constexpr int kVfpStages = 2;
static_assert(kVfpTile == kVfpWaves * kQPerWave && kVfpTile == 2 * 64, "a workgroup is one 128-row tile; its diagonal spans two 64-key chunks");

// the attention launch's arguments
struct VfpAttn {
    const unsigned char* q8;   // row-major slabs
    const unsigned char* k8;   // KFRAG images
    const unsigned char* v8;   // VFRAG images, laid out like k8's
    void* out;                 // dense [total_q, Hq, D]
    float* lse;                // [Hq, total_q] or nullptr
    unsigned char* path;       // [Hq, total_q] or nullptr
    const float* sq;           // [B, Hq]
    const float* sk;           // [B, Hkv]
    const float* sv;           // [B, Hkv]
    const int *cu_q, *cu_k, *used;
    int B, Hq, Hkv, total_q, total_k, nblk, out_fmt, xcd_remap, two_term_keys;
    float sm_log2e;
};

// LIGHT = the byte-exponential kernel (the lean register budget); the exact / two-term variants get one wave per SIMD less
// (BsfShape of qattn_block_sparse_fp8.hip)
template <int D, bool LIGHT> struct VfpShape {
    static constexpr int WPS = D == 256 ? 2 : (D == 64 ? (LIGHT ? 4 : 3) : (LIGHT ? 3 : 2));
};

// 4 scores -> 4 e4m3 bytes of 2^x (byte_exp4 of qattn_attn_v4.hip)
__device__ __forceinline__ int vfp_byte_exp4(float s0, float s1, float s2, float s3, float c8, float off8) {
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const us2 qa = __builtin_amdgcn_cvt_pknorm_u16(__builtin_fmaf(s0, c8, off8), __builtin_fmaf(s1, c8, off8));
    const us2 qb = __builtin_amdgcn_cvt_pknorm_u16(__builtin_fmaf(s2, c8, off8), __builtin_fmaf(s3, c8, off8));
    unsigned ua, ub;
    __builtin_memcpy(&ua, &qa, 4);
    __builtin_memcpy(&ub, &qb, 4);
    return (int)__builtin_amdgcn_perm(ub, ua, 0x06040200u);
}

constexpr int kVfpSelAll = 0, kVfpSelMany = 1, kVfpSelFew = 2;   // which tiles a launch attends: all / rows see >= two_term_keys keys / fewer

// LDS of the attention kernels: the K / V ring and the parked Q^T fragments (D = 256: 96 KiB)
constexpr int vfp_lds_bytes(int D) { return kVfpStages * 2 * 64 * D + kVfpWaves * kQPerWave * D; }
static_assert(vfp_lds_bytes(256) <= 160 * 1024, "the ring and the Q slots fit a CU's LDS");

// the body of the packed FP8-PV entries (qattn_varlen_fp8.hip).  window = nullptr: attn_vfp8_kernel under is_causal; else {left, right}
// (both >= -1, checked by the caller) and the sliding-window launch below, is_causal ignored
int varlen_fp8pv_forward_impl(const void* q, const void* k, const void* v, const long long* strides, int in_fmt, void* out, float* lse,
                              const int* cu_seqlens_q, const int* cu_seqlens_k, const int* seqused_k, int B, int Hq, int Hkv, int total_q,
                              int total_k, int D, int fp8_fmt, int numerics, int is_causal, float sm_scale, int precision, void* q8, void* k8,
                              void* v8, float* scale_q, float* scale_k, float* scale_v, unsigned char* row_path, float* k_mean, void* workspace,
                              size_t workspace_bytes, void* stream, const int* window);

// the sliding-window FP8-PV attention launch(es) (qattn_varlen_window_fp8.hip): window_left / window_right >= -1, -1 = unbounded;
// precision QATTN_PRECISION_FAST or _ACCURATE
int launch_varlen_window_fp8_attn(const VfpAttn& a, int D, int fp8_fmt, int precision, int window_left, int window_right, hipStream_t st);

}  // namespace qattn

// qattn_varlen_fp8.h -- what the two packed FP8-PV units pass each other: the attention launch's arguments, the entries' body
// (qattn_varlen_fp8.hip: argument checks, zeroing node, pre-pass launches, attention launch) and the sliding-window attention launch
// (qattn_varlen_window_fp8.hip) that the body runs behind its pre-pass.  The kernels' chunk sweep is qattn_fp8pv_sweep.h.
#pragma once
#include "qattn_fp8pv_sweep.h"

namespace qattn {

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

// qattn_varlen_attn.h -- what the packed variable-length units share on the host side: the attention launch's arguments, the entry's
// body (qattn_varlen.hip) and the sliding-window attention launch (qattn_varlen_window.hip) that the body runs behind its pre-pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace qattn {

// the attention launch's arguments: everything but the per-sequence parts of AttnParams
struct VarlenAttn {
    const unsigned char* q8;   // row-major slabs
    const unsigned char* k8;   // KFRAG images
    const unsigned char* v;    // caller's 16-bit V
    long v_ts, v_hs;           // its byte strides of token and head
    void* out;                 // dense [total_q, Hq, D]
    float* lse;                // [Hq, total_q] or nullptr
    const float* sq;           // [B, Hq]
    const float* sk;           // [B, Hkv]
    const int *cu_q, *cu_k, *used;
    int B, Hq, Hkv, total_q, total_k, nblk, out_fmt, xcd_remap;
    float sm_log2e;
};

// the body of the packed entries (qattn_varlen.hip): argument checks, then zeroing node, pre-pass launches and the attention launch
int varlen_forward_impl(const void* q, const void* k, const void* v, const long long* strides, int in_fmt, void* out, float* lse,
                        const int* cu_seqlens_q, const int* cu_seqlens_k, const int* seqused_k, int B, int Hq, int Hkv, int total_q, int total_k,
                        int D, int fp8_fmt, int numerics, int is_causal, float sm_scale, void* q8, void* k8, float* scale_q, float* scale_k,
                        void* workspace, size_t workspace_bytes, void* stream, float* k_mean, const int* window);

// the packed pre-pass on q alone (qattn_varlen.hip): per sequence the bytes and scales of qattn_quant_fp8(..., QATTN_SCALE_HEAD) on that
// sequence's queries; q8 [Hq total_q D] bytes (sequence i's [Hq, L_i, D] slab at byte Hq D start_i), scale_q [B, Hq], amax: B Hq scratch
// words.  token_stride / head_stride in elements.  No argument is checked here.
int varlen_quant_q(const void* q16, long token_stride, long head_stride, int in_fmt, const int* cu_seqlens_q, int B, int Hq, int total_q, int D,
                   int fp8_fmt, int numerics, unsigned* amax, void* q8, float* scale_q, hipStream_t st);

// the sliding-window attention launch (qattn_varlen_window.hip): window_left / window_right >= -1, -1 = unbounded
int launch_varlen_window_attn(const VarlenAttn& a, int D, int qk_fmt, int v16_fmt, int window_left, int window_right, hipStream_t st);

}  // namespace qattn

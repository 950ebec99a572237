// qattn_splitkv_softcap_fp8.hip -- qattn_fp8_attention_splitkv_softcap_forward (include/qattn_softcap.h): the split-KV window entry over
// contiguous prepared K / V with the scaled scores soft-capped, y = softcap tanh(x / softcap), before the mask and the softmax.
//
// The kernel is qattn_splitkv_attn.h's body with QATTN_SKV_WINDOW and QATTN_SKV_SOFTCAP on, the host driver that header's skv_forward with
// WINDOW = SOFTCAP = true: the partials of a call with more splits are states over capped scores and go through the window entry's merge
// chain.
#include "qattn_splitkv_attn.h"

using namespace qattn;

extern "C" int qattn_fp8_attention_splitkv_softcap_forward(const void* q16, int in_fmt, const void* k8_kfrag, const void* v8_vfrag,
                                                           const float* scale_k, const float* scale_v, void* out, float* lse,
                                                           const int* seqused_k, int B, int Hq, int Hkv, int Sq, int Skv, int D, int fp8_fmt,
                                                           int numerics, int window_left, int window_right, float softcap, float sm_scale,
                                                           int precision, int num_splits, void* q8, float* scale_q, unsigned char* row_path,
                                                           float* partial_o, float* partial_lse, unsigned char* partial_path, void* workspace,
                                                           size_t workspace_bytes, void* stream) {
    return skv_forward<false, true, false, true>(q16, in_fmt, k8_kfrag, v8_vfrag, SkvPages{}, scale_k, scale_v, out, lse, seqused_k, B, Hq, Hkv,
                                                 Sq, Skv, D, fp8_fmt, numerics, 0, sm_scale, precision, num_splits, q8, scale_q, row_path,
                                                 partial_o, partial_lse, partial_path, workspace, workspace_bytes, stream, window_left,
                                                 window_right, nullptr, softcap);
}

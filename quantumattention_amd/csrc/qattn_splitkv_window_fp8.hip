// qattn_splitkv_window_fp8.hip -- qattn_fp8_attention_splitkv_window_forward (include/qattn_splitkv_window.h): the split-KV entry over
// contiguous prepared K / V under a sliding window, and the two num_splits = 0 rules of the window entries.
//
// The kernel is qattn_splitkv_attn.h's body with QATTN_SKV_WINDOW on, the host driver that header's skv_forward with WINDOW = true: the quant
// pre-pass of q, the partial buffers, the merge chain and the path launch are the entry's without a window, unchanged.  What differs
// (qattn_splitkv_body.h): the split plan cuts the sequence's interval [lo_i, L), the tile sweeps the chunks klo / 64 .. khi / 64 alone, the
// token mask has a lower edge, and the V bytes of the keys below lo_i in its chunk are zeroed in LDS.
#include "qattn_splitkv_attn.h"
#include "../../include/qattn_paged_varlen.h"
#include "../../include/qattn_splitkv_window.h"

using namespace qattn;

extern "C" int qattn_splitkv_window_auto_splits(int B, int Hq, int Hkv, int Sq, int Skv, int D, int window_left, int num_cus) {
    if (!skv_dims_ok(B, Hq, Hkv, Sq, Skv) || window_left < -1) return 1;
    return qattn_splitkv_auto_splits(B, Hq, Hkv, Sq, skv_window_keys(Skv, Sq, window_left), D, num_cus);
}

extern "C" int qattn_paged_varlen_window_auto_splits(int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int Skv, int D, int window_left,
                                                     int num_cus) {
    if (Skv < 1 || max_seqlen_q < 1 || window_left < -1) return 1;
    return qattn_paged_varlen_auto_splits(B, Hq, Hkv, total_q, max_seqlen_q, skv_window_keys(Skv, max_seqlen_q, window_left), D, num_cus);
}

extern "C" int qattn_fp8_attention_splitkv_window_forward(const void* q16, int in_fmt, const void* k8_kfrag, const void* v8_vfrag,
                                                          const float* scale_k, const float* scale_v, void* out, float* lse,
                                                          const int* seqused_k, int B, int Hq, int Hkv, int Sq, int Skv, int D, int fp8_fmt,
                                                          int numerics, int window_left, int window_right, float sm_scale, int precision,
                                                          int num_splits, void* q8, float* scale_q, unsigned char* row_path, float* partial_o,
                                                          float* partial_lse, unsigned char* partial_path, void* workspace,
                                                          size_t workspace_bytes, void* stream) {
    return skv_forward<false, true>(q16, in_fmt, k8_kfrag, v8_vfrag, SkvPages{}, scale_k, scale_v, out, lse, seqused_k, B, Hq, Hkv, Sq, Skv, D,
                                    fp8_fmt, numerics, 0, sm_scale, precision, num_splits, q8, scale_q, row_path, partial_o, partial_lse,
                                    partial_path, workspace, workspace_bytes, stream, window_left, window_right);
}

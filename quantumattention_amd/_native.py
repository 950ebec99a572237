"""ctypes binding of libqattn_hip.so (include/qattn.h).  No CPU fallback: a missing library is a hard error."""
import ctypes
import math
import os
from typing import Optional, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (QUANTUM_ATTN_LIBRARY: another build of the same library, e.g. a tuning variant from `build.py --variant=...`; development aid)
LIB_PATH = os.environ.get("QUANTUM_ATTN_LIBRARY") or os.path.join(_HERE, "libqattn_hip.so")

FMT_E4M3, FMT_E5M2, FMT_BF16, FMT_FP16 = 0, 1, 2, 3
SCALE_HEAD, SCALE_TOKEN = 0, 1
LAYOUT_ROWMAJOR, LAYOUT_KFRAG, LAYOUT_VFRAG, LAYOUT_K16FRAG, LAYOUT_V16FRAG = 0, 1, 2, 3, 4
NUMERICS = {"compiled": 0, "eager": 1}
ABI_VERSION = 8
PRECISION = {"auto": 0, "fast": 1, "accurate": 2}
LSE_NATURAL, LSE_REFERENCE = 0, 1
PATH_ONE_TERM, PATH_TWO_TERM, PATH_V16 = 0, 1, 2   # QATTN_PATH_*: the fused entry's per-row debug output

_FMT_OF_DTYPE = {
    torch.float8_e4m3fn: FMT_E4M3,
    torch.float8_e5m2: FMT_E5M2,
    torch.bfloat16: FMT_BF16,
    torch.float16: FMT_FP16,
}
FP8_DTYPE = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}

EXPORTS = (
    "qattn_abi_version", "qattn_strerror", "qattn_check_device", "qattn_fp8_tensor_bytes",
    "qattn_quant_workspace_bytes", "qattn_quant_fp8", "qattn_quant_qkv_workspace_bytes", "qattn_quant_qkv_fp8",
    "qattn_pack_fp8", "qattn_fp8_attention_forward",
    "qattn_16bit_tensor_bytes", "qattn_pack16", "qattn_attention_forward_16", "qattn_fp8_quant_attention_forward",
    "qattn_attention_workspace_bytes", "qattn_lse_row_stride", "qattn_fp8_quant_attention_workspace_bytes",
    "qattn_profile_attention", "qattn_last_attention_ms", "qattn_vblock_exponent", "qattn_fp8_quant_attention_forward_ex",
    "qattn_attention_stamp_bytes", "qattn_fp8_quant_attention_forward_stamped", "qattn_mfma_probe_bytes", "qattn_mfma_probe",
    "qattn_fp8_attention_rowmajor_workspace_bytes", "qattn_fp8_attention_forward_rowmajor", "qattn_describe_path",
    "qattn_fp8_quant_attention_forward_strided", "qattn_pack16_strided", "qattn_attention_forward_16_strided",
    "qattn_varlen_tensor_bytes", "qattn_fp8_quant_attention_varlen_workspace_bytes", "qattn_fp8_quant_attention_varlen_forward",
    "qattn_fp8_block_sparse_attention_workspace_bytes", "qattn_fp8_block_sparse_attention_forward",
    "qattn_fp8_quant_attention_smooth_workspace_bytes", "qattn_fp8_quant_attention_forward_smooth",
    "qattn_fp8_quant_attention_varlen_smooth_workspace_bytes", "qattn_fp8_quant_attention_varlen_forward_smooth",
    "qattn_fp8_block_sparse_attention_smooth_workspace_bytes", "qattn_fp8_block_sparse_attention_forward_smooth",
    "qattn_fp8_quant_attention_varlen_window_workspace_bytes", "qattn_fp8_quant_attention_varlen_window_forward",
    "qattn_fp8_block_sparse_attention_fp8pv_workspace_bytes", "qattn_fp8_block_sparse_attention_fp8pv_smooth_workspace_bytes",
    "qattn_fp8_block_sparse_attention_forward_fp8pv",
    "qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes", "qattn_fp8_quant_attention_varlen_fp8pv_smooth_workspace_bytes",
    "qattn_fp8_quant_attention_varlen_forward_fp8pv",
    "qattn_fp8_quant_attention_varlen_window_forward_fp8pv",
    "qattn_attention_state_merge",
    "qattn_rope_quant_qk_workspace_bytes", "qattn_rope_quant_qk_fp8",
    "qattn_fp8_rope_quant_attention_workspace_bytes", "qattn_fp8_rope_quant_attention_forward",
    "qattn_fp8_attention_splitkv_workspace_bytes", "qattn_splitkv_auto_splits", "qattn_fp8_attention_splitkv_forward",
    "qattn_kv_cache_append_fp8",
    "qattn_paged_kv_cache_append_fp8", "qattn_fp8_attention_paged_splitkv_workspace_bytes", "qattn_fp8_attention_paged_splitkv_forward",
    "qattn_fp8_attention_paged_varlen_workspace_bytes", "qattn_paged_varlen_auto_splits", "qattn_fp8_attention_paged_varlen_forward",
    "qattn_splitkv_window_auto_splits", "qattn_paged_varlen_window_auto_splits", "qattn_fp8_attention_splitkv_window_forward",
    "qattn_fp8_attention_paged_splitkv_window_forward", "qattn_fp8_attention_paged_varlen_window_forward",
    "qattn_paged_kv_cache_append_varlen_fp8",
    "qattn_paged_kv_cache_append_varlen_rope_fp8", "qattn_rope_paged_varlen",
    "qattn_attention_state_merge_sink", "qattn_fp8_attention_splitkv_sink_forward", "qattn_fp8_attention_paged_splitkv_sink_forward",
    "qattn_fp8_attention_paged_varlen_sink_forward",
    "qattn_fp8_attention_paged_varlen_tree_forward", "qattn_paged_kv_cache_compact_fp8",
    "qattn_fp8_attention_paged_varlen_tree_window_forward",
    "qattn_paged_kv_cache_append_varlen_rope_pos_fp8", "qattn_rope_packed_positions",
    "qattn_fp8_attention_splitkv_softcap_forward", "qattn_fp8_attention_paged_splitkv_softcap_forward",
    "qattn_fp8_attention_paged_varlen_softcap_forward",
)
FMT_FP32 = 4               # QATTN_FMT_FP32 (include/qattn_merge.h): a partial / the output of the state merge, no other entry takes it
MERGE_MAX_PARTIALS = 8     # QATTN_MERGE_MAX_PARTIALS
_MERGE_FMT = {torch.bfloat16: FMT_BF16, torch.float16: FMT_FP16, torch.float32: FMT_FP32}
BLOCK_SPARSE_BLOCK = 128   # QATTN_BLOCK_SPARSE_BLOCK (include/qattn_block_sparse.h): rows / keys per mask block
SPLITKV_MAX_SPLITS = 64    # QATTN_SPLITKV_MAX_SPLITS (include/qattn_splitkv.h)


class PathDesc(ctypes.Structure):
    """qattn_path_desc (include/qattn.h): what an entry runs for given arguments."""
    _fields_ = [(n, ctypes.c_int) for n in ("kernel", "q_quant", "v_format", "sweep_p", "precise", "early", "start_mode", "lse")]


ENTRY = {"separate": 0, "separate16": 1, "fused": 2}
# names of the enum values of qattn_path_desc's fields, in the order of their codes (the vocabulary of the header's path table)
PATH_DESC_NAMES = {
    "kernel": ("v2", "v4", "pv16"), "q_quant": ("caller", "prepass", "kernel"), "v_format": ("head", "block", "16bit"),
    "sweep_p": ("byte", "exact", "p16"), "precise": ("two-term", "v16", "none"), "early": ("two-term", "v16-inline", "v16-launch", "none"),
    "start_mode": ("keys", "moments", "none"), "lse": ("exact", "quantised"),
}

_lib = None


def lib() -> ctypes.CDLL:
    """Load the library (once).  Raises if it has not been built -- the HIP path has no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m quantumattention_amd.build` "
            "(hipcc --offload-arch=gfx950). The gfx950 FP8 attention path has no CPU or eager fallback."
        )
    if os.path.abspath(LIB_PATH) != os.path.join(_HERE, "libqattn_hip.so"):
        # never silent: a stale variant with the right ABI number would otherwise be timed or shipped unnoticed
        import warnings

        warnings.warn(f"quantumattention_amd: loading a NON-DEFAULT kernel library {LIB_PATH} (QUANTUM_ATTN_LIBRARY / LIB_PATH "
                      "override; development aid)", RuntimeWarning, stacklevel=2)
    L = ctypes.CDLL(LIB_PATH)
    vp, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    L.qattn_abi_version.restype = i
    L.qattn_strerror.restype = ctypes.c_char_p
    L.qattn_strerror.argtypes = [i]
    L.qattn_check_device.restype = i
    L.qattn_vblock_exponent.restype = i
    L.qattn_vblock_exponent.argtypes = [ctypes.c_uint, i]
    L.qattn_fp8_tensor_bytes.restype = sz
    L.qattn_fp8_tensor_bytes.argtypes = [i, i, i, i, i]
    L.qattn_quant_workspace_bytes.restype = sz
    L.qattn_quant_workspace_bytes.argtypes = [i, i, i, i, i]
    L.qattn_quant_fp8.restype = i
    L.qattn_quant_fp8.argtypes = [vp, i, vp, vp, i, i, i, i, i, i, i, i, vp, sz, vp]
    L.qattn_quant_qkv_workspace_bytes.restype = sz
    L.qattn_quant_qkv_workspace_bytes.argtypes = [i, i, i]
    L.qattn_quant_qkv_fp8.restype = i
    L.qattn_quant_qkv_fp8.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, vp, sz, vp]
    L.qattn_pack_fp8.restype = i
    L.qattn_pack_fp8.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.qattn_attention_workspace_bytes.restype = sz
    L.qattn_attention_workspace_bytes.argtypes = [i, i, i]
    L.qattn_lse_row_stride.restype = sz
    L.qattn_lse_row_stride.argtypes = [i, i]
    L.qattn_fp8_attention_forward.restype = i
    L.qattn_fp8_attention_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i, i, f, i, i, vp, sz, vp]
    L.qattn_16bit_tensor_bytes.restype = sz
    L.qattn_16bit_tensor_bytes.argtypes = [i, i, i, i, i]
    L.qattn_pack16.restype = i
    L.qattn_pack16.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.qattn_attention_forward_16.restype = i
    L.qattn_attention_forward_16.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, f, i, vp]
    L.qattn_profile_attention.restype = None
    L.qattn_profile_attention.argtypes = [i]
    L.qattn_last_attention_ms.restype = ctypes.c_float
    L.qattn_fp8_quant_attention_workspace_bytes.restype = sz
    L.qattn_fp8_quant_attention_workspace_bytes.argtypes = [i, i, i, i]
    L.qattn_fp8_quant_attention_forward.restype = i
    L.qattn_fp8_quant_attention_forward.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i, f, i, vp, sz, vp]
    L.qattn_fp8_quant_attention_forward_ex.restype = i
    L.qattn_fp8_quant_attention_forward_ex.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                       i, i, i, i, i, i, i, i, i, i, f, i, vp, i, vp, vp, sz, vp]
    L.qattn_pack16_strided.restype = i
    L.qattn_pack16_strided.argtypes = [vp, vp, vp, i, i, i, i, i, vp]
    L.qattn_attention_forward_16_strided.restype = i
    L.qattn_attention_forward_16_strided.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, f, i, vp]
    L.qattn_fp8_quant_attention_forward_strided.restype = i
    L.qattn_fp8_quant_attention_forward_strided.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                            i, i, i, i, i, i, i, i, i, i, f, i, vp, i, vp, vp, sz, vp]
    L.qattn_attention_stamp_bytes.restype = sz
    L.qattn_attention_stamp_bytes.argtypes = [i, i, i]
    L.qattn_fp8_quant_attention_forward_stamped.restype = i
    L.qattn_fp8_quant_attention_forward_stamped.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i, f, i, vp, sz, vp, sz, vp]
    L.qattn_mfma_probe_bytes.restype = sz
    L.qattn_mfma_probe_bytes.argtypes = []
    L.qattn_mfma_probe.restype = i
    L.qattn_mfma_probe.argtypes = [vp, sz, i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), vp]
    L.qattn_fp8_attention_rowmajor_workspace_bytes.restype = sz
    L.qattn_fp8_attention_rowmajor_workspace_bytes.argtypes = [i, i, i, i, i, i]
    L.qattn_fp8_attention_forward_rowmajor.restype = i
    L.qattn_fp8_attention_forward_rowmajor.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i, i, f, i, i, vp, sz, vp]
    L.qattn_describe_path.restype = i
    L.qattn_describe_path.argtypes = [i, i, i, i, i, i, ctypes.POINTER(PathDesc)]
    L.qattn_varlen_tensor_bytes.restype = sz
    L.qattn_varlen_tensor_bytes.argtypes = [i, i, i, i, i]
    L.qattn_fp8_quant_attention_varlen_workspace_bytes.restype = sz
    L.qattn_fp8_quant_attention_varlen_workspace_bytes.argtypes = [i, i, i, i, i, i]
    L.qattn_fp8_quant_attention_varlen_forward.restype = i
    L.qattn_fp8_quant_attention_varlen_forward.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, f,
                                                           vp, vp, vp, vp, vp, sz, vp]
    L.qattn_fp8_block_sparse_attention_workspace_bytes.restype = sz
    L.qattn_fp8_block_sparse_attention_workspace_bytes.argtypes = [i, i, i, i, i, i]
    L.qattn_fp8_block_sparse_attention_forward.restype = i
    L.qattn_fp8_block_sparse_attention_forward.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, i, i, i, i, i, i, i, i, f, vp, vp, vp, vp, vp, sz, vp]
    L.qattn_fp8_quant_attention_smooth_workspace_bytes.restype = sz
    L.qattn_fp8_quant_attention_smooth_workspace_bytes.argtypes = [i, i, i, i, i, i]
    L.qattn_fp8_quant_attention_forward_smooth.restype = i   # (..._forward_strided's arguments + float* k_mean: include/qattn_smooth.h)
    L.qattn_fp8_quant_attention_forward_smooth.argtypes = L.qattn_fp8_quant_attention_forward_strided.argtypes + [vp]
    # the varlen and block-sparse entries with key smoothing: their plain entry's arguments + float* k_mean
    L.qattn_fp8_quant_attention_varlen_smooth_workspace_bytes.restype = sz
    L.qattn_fp8_quant_attention_varlen_smooth_workspace_bytes.argtypes = [i, i, i, i, i, i]
    L.qattn_fp8_quant_attention_varlen_forward_smooth.restype = i
    L.qattn_fp8_quant_attention_varlen_forward_smooth.argtypes = L.qattn_fp8_quant_attention_varlen_forward.argtypes + [vp]
    L.qattn_fp8_block_sparse_attention_smooth_workspace_bytes.restype = sz
    L.qattn_fp8_block_sparse_attention_smooth_workspace_bytes.argtypes = [i, i, i, i, i, i]
    L.qattn_fp8_block_sparse_attention_forward_smooth.restype = i
    L.qattn_fp8_block_sparse_attention_forward_smooth.argtypes = L.qattn_fp8_block_sparse_attention_forward.argtypes + [vp]
    # the sliding-window entry (include/qattn_window.h): the varlen entry's arguments with (window_left, window_right) for is_causal, + float* k_mean
    L.qattn_fp8_quant_attention_varlen_window_workspace_bytes.restype = sz
    L.qattn_fp8_quant_attention_varlen_window_workspace_bytes.argtypes = [i, i, i, i, i, i]
    L.qattn_fp8_quant_attention_varlen_window_forward.restype = i
    L.qattn_fp8_quant_attention_varlen_window_forward.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i, f,
                                                                  vp, vp, vp, vp, vp, sz, vp, vp]
    # the block-sparse entry with FP8 P.V (include/qattn_block_sparse.h): ... sm_scale, precision, q8, k8, v8, scale_q, scale_k, scale_v,
    # row_path, k_mean (NULL: no smoothing), workspace, workspace_bytes, stream
    L.qattn_fp8_block_sparse_attention_fp8pv_workspace_bytes.restype = sz
    L.qattn_fp8_block_sparse_attention_fp8pv_workspace_bytes.argtypes = [i, i, i, i, i, i]
    L.qattn_fp8_block_sparse_attention_fp8pv_smooth_workspace_bytes.restype = sz
    L.qattn_fp8_block_sparse_attention_fp8pv_smooth_workspace_bytes.argtypes = [i, i, i, i, i, i]
    L.qattn_fp8_block_sparse_attention_forward_fp8pv.restype = i
    L.qattn_fp8_block_sparse_attention_forward_fp8pv.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, i, i, i, i, i, i, i, i, f, i,
                                                                 vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    # the packed entry with FP8 P.V (include/qattn_varlen.h): the plain entry's arguments up to sm_scale, then precision, q8, k8, v8,
    # scale_q, scale_k, scale_v, row_path, k_mean (NULL: no smoothing), workspace, workspace_bytes, stream
    L.qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes.restype = sz
    L.qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes.argtypes = [i, i, i, i, i, i]
    L.qattn_fp8_quant_attention_varlen_fp8pv_smooth_workspace_bytes.restype = sz
    L.qattn_fp8_quant_attention_varlen_fp8pv_smooth_workspace_bytes.argtypes = [i, i, i, i, i, i]
    L.qattn_fp8_quant_attention_varlen_forward_fp8pv.restype = i
    L.qattn_fp8_quant_attention_varlen_forward_fp8pv.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, f, i,
                                                                 vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    # the sliding-window entry with FP8 P.V (include/qattn_window.h): the packed FP8-PV entry's arguments with (window_left, window_right)
    # for is_causal; its workspace is sized by the two packed FP8-PV functions above
    L.qattn_fp8_quant_attention_varlen_window_forward_fp8pv.restype = i
    L.qattn_fp8_quant_attention_varlen_window_forward_fp8pv.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i, f, i,
                                                                        vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    # merging of attention states (include/qattn_merge.h): n, o[], o_fmt[], o_strides[3n], lse[], lse_strides[3n], out, out_fmt, out_strides[3],
    # lse_out, lse_out_strides[3], B, H, S, D, stream -- the tables are host arrays
    L.qattn_attention_state_merge.restype = i
    L.qattn_attention_state_merge.argtypes = [i, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, i, i, i, i, vp]
    # RoPE fused into the q / k pre-pass (include/qattn_rope.h): q, k, strides[6], in_fmt, then per table pair (cos, sin, batch stride, row
    # stride) for q and for k, interleaved, ...
    ll = ctypes.c_longlong
    L.qattn_rope_quant_qk_workspace_bytes.restype = sz
    L.qattn_rope_quant_qk_workspace_bytes.argtypes = [i, i, i]
    L.qattn_rope_quant_qk_fp8.restype = i
    L.qattn_rope_quant_qk_fp8.argtypes = [vp, vp, vp, i, vp, vp, ll, ll, vp, vp, ll, ll, i, vp, vp, i, vp, vp, i, i, i, i, i, i, i, i, i, vp, sz, vp]
    L.qattn_fp8_rope_quant_attention_workspace_bytes.restype = sz
    L.qattn_fp8_rope_quant_attention_workspace_bytes.argtypes = [i, i, i, i, i, i]
    L.qattn_fp8_rope_quant_attention_forward.restype = i
    L.qattn_fp8_rope_quant_attention_forward.argtypes = [vp, vp, vp, vp, i, vp, vp, ll, ll, vp, vp, ll, ll, i, vp, vp, vp, vp, vp, vp, vp, vp,
                                                         i, i, i, i, i, i, i, i, i, i, i, f, i, i, vp, sz, vp]
    # split-KV attention over prepared K / V (include/qattn_splitkv.h): q16, in_fmt, k8_kfrag, v8_vfrag, scale_k, scale_v, out, lse, seqused_k,
    # B, Hq, Hkv, Sq, Skv, D, fp8_fmt, numerics, is_causal, sm_scale, precision, num_splits, q8, scale_q, row_path, partial_o, partial_lse,
    # partial_path, workspace, workspace_bytes, stream
    L.qattn_fp8_attention_splitkv_workspace_bytes.restype = sz
    L.qattn_fp8_attention_splitkv_workspace_bytes.argtypes = [i, i, i, i, i, i, i]
    L.qattn_splitkv_auto_splits.restype = i
    L.qattn_splitkv_auto_splits.argtypes = [i, i, i, i, i, i, i]
    L.qattn_fp8_attention_splitkv_forward.restype = i
    L.qattn_fp8_attention_splitkv_forward.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, f, i, i,
                                                      vp, vp, vp, vp, vp, vp, vp, sz, vp]
    # appending to an FP8 K/V cache with fixed scales (include/qattn_kvcache.h): k16, v16, in_fmt, k_strides3, v_strides3, k8_kfrag, v8_vfrag,
    # scale_k, scale_v, seqlens, new_lens, advance, B, Hkv, T, capacity, D, fp8_fmt, stream
    L.qattn_kv_cache_append_fp8.restype = i
    L.qattn_kv_cache_append_fp8.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, vp]
    # the paged cache (include/qattn_paged.h).  Append: k16, v16, in_fmt, k_strides3, v_strides3, k_pool, v_pool, scale_k, scale_v, block_table,
    # table_stride, seqlens, new_lens, advance, B, Hkv, T, num_pages, page_size, max_pages, D, fp8_fmt, stream.  Attention: q16, in_fmt, k_pool,
    # v_pool, block_table, table_stride, num_pages, page_size, max_pages, then the split-KV entry's arguments from scale_k on
    L.qattn_paged_kv_cache_append_fp8.restype = i
    L.qattn_paged_kv_cache_append_fp8.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, vp, vp, ll, vp, vp, i, i, i, i, i, i, i, i, i, vp]
    L.qattn_fp8_attention_paged_splitkv_workspace_bytes.restype = sz
    L.qattn_fp8_attention_paged_splitkv_workspace_bytes.argtypes = [i, i, i, i, i, i, i]
    L.qattn_fp8_attention_paged_splitkv_forward.restype = i
    L.qattn_fp8_attention_paged_splitkv_forward.argtypes = [vp, i, vp, vp, vp, ll, i, i, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, f, i, i,
                                                            vp, vp, vp, vp, vp, vp, vp, sz, vp]
    # packed queries over the paged cache (include/qattn_paged_varlen.h): q16, q_strides2, in_fmt, k_pool, v_pool, block_table, table_stride,
    # num_pages, page_size, max_pages, scale_k, scale_v, out, lse, cu_seqlens_q, seqused_k, B, Hq, Hkv, total_q, max_seqlen_q, Skv, D, fp8_fmt,
    # numerics, is_causal, sm_scale, precision, num_splits, q8, scale_q, row_path, partial_o, partial_lse, partial_path, workspace, bytes, stream
    L.qattn_fp8_attention_paged_varlen_workspace_bytes.restype = sz
    L.qattn_fp8_attention_paged_varlen_workspace_bytes.argtypes = [i, i, i, i, i, i, i]
    L.qattn_paged_varlen_auto_splits.restype = i
    L.qattn_paged_varlen_auto_splits.argtypes = [i, i, i, i, i, i, i, i]
    L.qattn_fp8_attention_paged_varlen_forward.restype = i
    L.qattn_fp8_attention_paged_varlen_forward.argtypes = [vp, vp, i, vp, vp, vp, ll, i, i, i, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i,
                                                           f, i, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    # the three split-KV entries under a sliding window (include/qattn_splitkv_window.h): the sibling's arguments with is_causal replaced by
    # window_left, window_right; the auto-split rules take window_left before num_cus
    L.qattn_splitkv_window_auto_splits.restype = i
    L.qattn_splitkv_window_auto_splits.argtypes = [i, i, i, i, i, i, i, i]
    L.qattn_paged_varlen_window_auto_splits.restype = i
    L.qattn_paged_varlen_window_auto_splits.argtypes = [i, i, i, i, i, i, i, i, i]
    L.qattn_fp8_attention_splitkv_window_forward.restype = i
    L.qattn_fp8_attention_splitkv_window_forward.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i, f, i, i,
                                                             vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.qattn_fp8_attention_paged_splitkv_window_forward.restype = i
    L.qattn_fp8_attention_paged_splitkv_window_forward.argtypes = [vp, i, vp, vp, vp, ll, i, i, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i,
                                                                   f, i, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.qattn_fp8_attention_paged_varlen_window_forward.restype = i
    L.qattn_fp8_attention_paged_varlen_window_forward.argtypes = [vp, vp, i, vp, vp, vp, ll, i, i, i, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i,
                                                                  i, i, i, f, i, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    # the paged append on packed tokens (include/qattn_paged_varlen_append.h): k16, v16, in_fmt, k_strides2, v_strides2, k_pool, v_pool, scale_k,
    # scale_v, block_table, table_stride, seqlens, cu_seqlens, advance, B, Hkv, total, num_pages, page_size, max_pages, D, fp8_fmt, stream
    L.qattn_paged_kv_cache_append_varlen_fp8.restype = i
    L.qattn_paged_kv_cache_append_varlen_fp8.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, vp, vp, ll, vp, vp, i, i, i, i, i, i, i, i, i, vp]
    # the same with K rotated inside it (include/qattn_paged_varlen_rope.h): ..., fp8_fmt, cos, sin, table_row_stride, T, interleaved, stream
    L.qattn_paged_kv_cache_append_varlen_rope_fp8.restype = i
    L.qattn_paged_kv_cache_append_varlen_rope_fp8.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, vp, vp, ll, vp, vp, i, i, i, i, i, i, i, i, i, vp, vp,
                                                              ll, i, i, vp]
    # packed rows rotated at the cache's positions: x16, in_fmt, x_strides2, out16, cu_seqlens, seqlens, appended, B, H, total, capacity, D, cos,
    # sin, table_row_stride, T, interleaved, stream
    L.qattn_rope_paged_varlen.restype = i
    L.qattn_rope_paged_varlen.argtypes = [vp, i, vp, vp, vp, vp, i, i, i, i, ll, i, vp, vp, ll, i, i, vp]
    # learned attention sinks (include/qattn_sinks.h): the merge's arguments + sink; the window entries' arguments with sinks after window_right
    L.qattn_attention_state_merge_sink.restype = i
    L.qattn_attention_state_merge_sink.argtypes = [i, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, i, i, i, i, vp, vp]
    L.qattn_fp8_attention_splitkv_sink_forward.restype = i
    L.qattn_fp8_attention_splitkv_sink_forward.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i, vp, f, i, i,
                                                           vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.qattn_fp8_attention_paged_splitkv_sink_forward.restype = i
    L.qattn_fp8_attention_paged_splitkv_sink_forward.argtypes = [vp, i, vp, vp, vp, ll, i, i, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i,
                                                                 vp, f, i, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.qattn_fp8_attention_paged_varlen_sink_forward.restype = i
    L.qattn_fp8_attention_paged_varlen_sink_forward.argtypes = [vp, vp, i, vp, vp, vp, ll, i, i, i, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i,
                                                                i, i, i, vp, f, i, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    # tree-shaped speculative decoding (include/qattn_paged_varlen_tree.h): the packed paged entry's arguments with tree_mask in is_causal's
    # place; k_pool, v_pool, block_table, table_stride, seqlens, cu_seqlens, accept_index, accept_lens, B, Hkv, total, num_pages, page_size,
    # max_pages, D, stream
    L.qattn_fp8_attention_paged_varlen_tree_forward.restype = i
    L.qattn_fp8_attention_paged_varlen_tree_forward.argtypes = [vp, vp, i, vp, vp, vp, ll, i, i, i, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i,
                                                                i, vp, f, i, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.qattn_paged_kv_cache_compact_fp8.restype = i
    L.qattn_paged_kv_cache_compact_fp8.argtypes = [vp, vp, vp, ll, vp, vp, vp, vp, i, i, i, i, i, i, i, vp]
    # the tree under a window, optionally with sinks (include/qattn_paged_varlen_tree_window.h): the tree entry's arguments with window_left,
    # window_right, sinks (NULL: none) after tree_mask
    L.qattn_fp8_attention_paged_varlen_tree_window_forward.restype = i
    L.qattn_fp8_attention_paged_varlen_tree_window_forward.argtypes = [vp, vp, i, vp, vp, vp, ll, i, i, i, vp, vp, vp, vp, vp, vp, i, i, i, i, i,
                                                                       i, i, i, i, vp, i, i, vp, f, i, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    # the rotary embedding at the caller's positions (include/qattn_paged_varlen_rope_pos.h): the rope append's arguments with positions before
    # stream; x16, in_fmt, x_strides2, out16, positions, H, total, D, cos, sin, table_row_stride, T, interleaved, stream
    L.qattn_paged_kv_cache_append_varlen_rope_pos_fp8.restype = i
    L.qattn_paged_kv_cache_append_varlen_rope_pos_fp8.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, vp, vp, ll, vp, vp, i, i, i, i, i, i, i, i, i, vp,
                                                                  vp, ll, i, i, vp, vp]
    L.qattn_rope_packed_positions.restype = i
    L.qattn_rope_packed_positions.argtypes = [vp, i, vp, vp, vp, i, i, i, vp, vp, ll, i, i, vp]
    # logit soft-capping (include/qattn_softcap.h): the window entries' arguments with the host float softcap after window_right
    L.qattn_fp8_attention_splitkv_softcap_forward.restype = i
    L.qattn_fp8_attention_splitkv_softcap_forward.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i, f, f, i, i,
                                                              vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.qattn_fp8_attention_paged_splitkv_softcap_forward.restype = i
    L.qattn_fp8_attention_paged_splitkv_softcap_forward.argtypes = [vp, i, vp, vp, vp, ll, i, i, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i,
                                                                    i, f, f, i, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.qattn_fp8_attention_paged_varlen_softcap_forward.restype = i
    L.qattn_fp8_attention_paged_varlen_softcap_forward.argtypes = [vp, vp, i, vp, vp, vp, ll, i, i, i, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i,
                                                                   i, i, i, i, f, f, i, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    if L.qattn_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libqattn_hip.so ABI {L.qattn_abi_version()} != expected {ABI_VERSION}; rebuild it")
    _lib = L
    return L


def _require(cond: bool, what: str) -> None:
    """Argument checks of the binding raise (they must survive `python -O`, unlike assert)."""
    if not cond:
        raise ValueError(what)


def _scale_mode(scaling: str) -> int:
    _require(scaling in ("head-wise", "token-wise"), f"Unsupported scaling_method: {scaling}")
    return SCALE_HEAD if scaling == "head-wise" else SCALE_TOKEN


def _precision(name) -> int:
    _require(name in PRECISION, f"Unsupported precision: {name!r} (expected one of {sorted(PRECISION)})")
    return PRECISION[name]


def _numerics(name) -> int:
    _require(name in NUMERICS, f"Unsupported quant_numerics: {name!r} (expected one of {sorted(NUMERICS)})")
    return NUMERICS[name]


def fp8_dtype_of(name) -> torch.dtype:
    """config.attention.fp8_format / the ops' fp8_format argument -> torch dtype; anything else is a ValueError, not a KeyError."""
    _require(name in FP8_DTYPE, f"Unsupported fp8_format: {name!r} (expected one of {sorted(FP8_DTYPE)})")
    return FP8_DTYPE[name]


def _check_qkv(q, k, v):
    """q [B,Hq,Sq,D], k / v [B,Hkv,Skv,D] on one device with one 16-bit dtype (tk/attention.py:362-400)."""
    _require(q.is_cuda and q.dim() == 4 and k.dim() == 4 and v.dim() == 4, "query, key and value must be 4-D device tensors")
    _require(q.device == k.device == v.device, "query, key and value must be on the same device")
    _require(q.dtype == k.dtype == v.dtype, f"query, key and value must share a dtype, got {q.dtype}, {k.dtype}, {v.dtype}")
    B, Hq, Sq, D = q.shape
    _require(k.shape == v.shape, f"key and value shapes differ: {tuple(k.shape)} vs {tuple(v.shape)}")
    _require(k.shape[0] == B and k.shape[3] == D, f"key/value batch or head_dim {tuple(k.shape)} do not match the query {tuple(q.shape)}")
    Hkv, Skv = k.shape[1], k.shape[2]
    _require(Hkv > 0 and Hq % Hkv == 0, f"Hq={Hq} is not a multiple of Hkv={Hkv}")
    return B, Hq, Hkv, Sq, Skv, D


def _strided_ok(t: torch.Tensor) -> bool:
    """A 4-D view the kernels address directly (include/qattn_strided.h): head_dim innermost and dense, every other stride a non-negative
    multiple of 8 elements (rows 16-byte aligned), rows at most 2^23 elements apart, base 16-byte aligned."""
    if t.is_contiguous():
        return True
    D = t.shape[3]
    return (t.stride(3) == 1 and all(t.shape[i] == 1 or (t.stride(i) >= 0 and t.stride(i) % 8 == 0) for i in (0, 1, 2))
            and (t.shape[2] == 1 or D <= t.stride(2) <= 2 ** 23) and t.data_ptr() % 16 == 0)


def empty_output(query: torch.Tensor, dtype, output_layout: str = "contiguous") -> torch.Tensor:
    """The output tensor of an attention call on `query` [B,H,S,D]: dense (the reference: tk/attention.py:434-437), or -- output_layout
    "like_query" and a query whose (b, s, h, d) order is dense in memory, i.e. x.view(B, S, H, D).transpose(1, 2) -- the transposed view
    of a dense [B,S,H,D] tensor (config.attention.output_layout)."""
    _require(output_layout in ("contiguous", "like_query"), f"output_layout must be 'contiguous' or 'like_query', got {output_layout!r}")
    B, H, S, D = query.shape
    if output_layout == "like_query" and not query.is_contiguous() and query.transpose(1, 2).is_contiguous():
        return torch.empty((B, S, H, D), dtype=dtype, device=query.device).transpose(1, 2)
    return torch.empty((B, H, S, D), dtype=dtype, device=query.device)


def _strides3(t: torch.Tensor):
    """{batch, head, row} element strides of a view `_strided_ok` accepted, as the C entries take them (None: dense)."""
    if t.is_contiguous():
        return None
    H, S, D = t.shape[1], t.shape[2], t.shape[3]
    dense = (H * S * D, S * D, D)     # (a dimension of size 1 has no stride of its own)
    return (ctypes.c_longlong * 3)(*[t.stride(i) if t.shape[i] > 1 else dense[i] for i in (0, 1, 2)])


def _check_scales(scale_q, scale_k, scale_v, mode, B, Hq, Hkv, Sq, Skv, device) -> None:
    """fp32, on `device`, exactly [B,H] (head-wise) or [B,H,S] (token-wise): tk/attention.py:402-414."""
    want_q = (B, Hq) if mode == SCALE_HEAD else (B, Hq, Sq)
    want_k = (B, Hkv) if mode == SCALE_HEAD else (B, Hkv, Skv)
    for name, s, want in (("scale_q", scale_q, want_q), ("scale_k", scale_k, want_k), ("scale_v", scale_v, (B, Hkv))):
        if s is None and name == "scale_v":
            continue
        _require(s is not None and s.dtype == torch.float32 and s.device == device and tuple(s.shape) == want,
                 f"{name} must be float32 {want} on {device}")


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed: {lib().qattn_strerror(rc).decode()} (code {rc})")


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def fmt_of(dtype: torch.dtype) -> int:
    try:
        return _FMT_OF_DTYPE[dtype]
    except KeyError:
        raise ValueError(f"unsupported dtype {dtype}") from None


def quant_fp8(x: torch.Tensor, *, scaling: str = "head-wise", fp8_dtype=torch.float8_e4m3fn,
              layout: int = LAYOUT_ROWMAJOR, numerics: str = "compiled") -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16/fp16 [B,H,S,D] -> (fp8 payload, fp32 scale).  Row-major payloads come back as an fp8 tensor of
    x's shape; fragment layouts as a flat uint8 buffer (their layout is private to the library)."""
    _require(x.is_cuda and x.dim() == 4, "quant_fp8 needs a 4-D device tensor")
    x = x.contiguous()
    B, H, S, D = x.shape
    L = lib()
    mode = _scale_mode(scaling)
    nbytes = L.qattn_fp8_tensor_bytes(layout, B, H, S, D)
    with torch.cuda.device(x.device):
        if layout == LAYOUT_ROWMAJOR:
            out = torch.empty((B, H, S, D), dtype=fp8_dtype, device=x.device)
        else:
            out = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
        scale = torch.empty((B, H) if mode == SCALE_HEAD else (B, H, S), dtype=torch.float32, device=x.device)
        ws_bytes = L.qattn_quant_workspace_bytes(B, H, S, D, mode)
        ws = torch.empty((max(ws_bytes, 4),), dtype=torch.uint8, device=x.device)
        rc = L.qattn_quant_fp8(x.data_ptr(), fmt_of(x.dtype), out.data_ptr(), scale.data_ptr(), B, H, S, D,
                               fmt_of(fp8_dtype), mode, _numerics(numerics), layout, ws.data_ptr(), ws_bytes,
                               _stream(x))
    _check(rc, "qattn_quant_fp8")
    return out, scale


def quant_qkv_fp8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, scaling: str = "head-wise",
                  fp8_dtype=torch.float8_e4m3fn, numerics: str = "compiled"):
    """Fused pre-pass: (q8 row-major fp8, k_frag, v_frag, scale_q, scale_k, scale_v) in two launches."""
    B, Hq, Hkv, Sq, Skv, D = _check_qkv(q, k, v)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    L = lib()
    mode = _scale_mode(scaling)
    dev = q.device
    with torch.cuda.device(dev):
        q8 = torch.empty((B, Hq, Sq, D), dtype=fp8_dtype, device=dev)
        kf = torch.empty((L.qattn_fp8_tensor_bytes(LAYOUT_KFRAG, B, Hkv, Skv, D),), dtype=torch.uint8, device=dev)
        vf = torch.empty((L.qattn_fp8_tensor_bytes(LAYOUT_VFRAG, B, Hkv, Skv, D),), dtype=torch.uint8, device=dev)
        sq = torch.empty((B, Hq) if mode == SCALE_HEAD else (B, Hq, Sq), dtype=torch.float32, device=dev)
        sk = torch.empty((B, Hkv) if mode == SCALE_HEAD else (B, Hkv, Skv), dtype=torch.float32, device=dev)
        sv = torch.empty((B, Hkv), dtype=torch.float32, device=dev)
        ws_bytes = L.qattn_quant_qkv_workspace_bytes(B, Hq, Hkv)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        rc = L.qattn_quant_qkv_fp8(q.data_ptr(), k.data_ptr(), v.data_ptr(), fmt_of(q.dtype), q8.data_ptr(),
                                   kf.data_ptr(), vf.data_ptr(), sq.data_ptr(), sk.data_ptr(), sv.data_ptr(),
                                   B, Hq, Hkv, Sq, Skv, D, fmt_of(fp8_dtype), mode, _numerics(numerics),
                                   ws.data_ptr(), ws_bytes, _stream(q))
    _check(rc, "qattn_quant_qkv_fp8")
    return q8, kf, vf, sq, sk, sv


def pack_fp8(x8: torch.Tensor, layout: int) -> torch.Tensor:
    """row-major fp8 [B,H,S,D] -> flat uint8 buffer in KFRAG / VFRAG layout."""
    _require(x8.is_cuda and x8.dim() == 4 and x8.dtype.itemsize == 1, "pack_fp8 needs a 4-D fp8 device tensor")
    x8 = x8.contiguous()
    B, H, S, D = x8.shape
    L = lib()
    with torch.cuda.device(x8.device):
        out = torch.empty((L.qattn_fp8_tensor_bytes(layout, B, H, S, D),), dtype=torch.uint8, device=x8.device)
        rc = L.qattn_pack_fp8(x8.data_ptr(), out.data_ptr(), B, H, S, D, layout, _stream(x8))
    _check(rc, "qattn_pack_fp8")
    return out


def fp8_attention_forward(q8: torch.Tensor, k_frag: torch.Tensor, v_frag: torch.Tensor, scale_q: torch.Tensor,
                          scale_k: torch.Tensor, scale_v: Optional[torch.Tensor], *, Hkv: int, Skv: int,
                          out_dtype: torch.dtype, is_causal: bool, scaling: str = "head-wise",
                          sm_scale: float = 0.0, return_lse: bool = False, precision: str = "auto",
                          lse_layout: int = LSE_NATURAL):
    """q8: row-major fp8 [B,Hq,Sq,D]; k_frag / v_frag: fragment-layout buffers for [B,Hkv,Skv,D].
    v_frag may instead be the ORIGINAL 16-bit value tensor, row-major bf16 / fp16 [B,Hkv,Skv,D] (scale_v = None): the call then runs
    the reference kernel's own P.V numerics -- 16-bit P on the un-quantised V (tk/attention.py:72,286,318) -- for every row.
    return_lse: also the log-sum-exp rows; LSE_REFERENCE gives the reference-defined strided view (include/qattn.h)."""
    _require(q8.is_cuda and q8.dim() == 4, "fp8_attention_forward needs a 4-D device query")
    q8 = q8.contiguous()
    B, Hq, Sq, D = q8.shape
    L = lib()
    mode = _scale_mode(scaling)
    v_is_16 = v_frag.dtype in (torch.bfloat16, torch.float16)
    if v_is_16:
        _require(tuple(v_frag.shape) == (B, Hkv, Skv, D) and scale_v is None and out_dtype == v_frag.dtype,
                 f"a 16-bit value tensor must be [B,Hkv,Skv,D] = {(B, Hkv, Skv, D)} with scale_v=None and out_dtype = its dtype")
        v_frag = v_frag.contiguous()
    _check_scales(scale_q, scale_k, scale_v, mode, B, Hq, Hkv, Sq, Skv, q8.device)
    _require(k_frag.numel() * k_frag.element_size() >= L.qattn_fp8_tensor_bytes(LAYOUT_KFRAG, B, Hkv, Skv, D)
             and (v_is_16 or v_frag.numel() * v_frag.element_size() >= L.qattn_fp8_tensor_bytes(LAYOUT_VFRAG, B, Hkv, Skv, D)),
             "k_frag / v_frag are smaller than the fragment layouts of [B,Hkv,Skv,D]")
    with torch.cuda.device(q8.device):
        out = torch.empty((B, Hq, Sq, D), dtype=out_dtype, device=q8.device)
        lse = None
        if return_lse:
            stride = L.qattn_lse_row_stride(Sq, lse_layout)
            lse = torch.empty((B, Hq, stride), dtype=torch.float32, device=q8.device)
        ws_bytes = L.qattn_attention_workspace_bytes(B, Hq, Sq)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=q8.device)
        rc = L.qattn_fp8_attention_forward(
            q8.data_ptr(), k_frag.data_ptr(), v_frag.data_ptr(), out.data_ptr(), _ptr(lse),
            scale_q.contiguous().data_ptr(), scale_k.contiguous().data_ptr(),
            _ptr(scale_v.contiguous() if scale_v is not None else None),
            B, Hq, Hkv, Sq, Skv, D, fmt_of(q8.dtype), fmt_of(v_frag.dtype if v_is_16 else q8.dtype), fmt_of(out_dtype), mode, int(is_causal),
            float(sm_scale), _precision(precision), lse_layout, ws.data_ptr(), ws_bytes, _stream(q8))
    _check(rc, "qattn_fp8_attention_forward")
    if return_lse:
        return out, lse[..., :Sq]  # [B,Hq,Sq] view; strides (Hq*ld, ld, 1) with ld = the padded row for LSE_REFERENCE
    return out


def describe_path(entry: str, D: int, in_dtype=torch.bfloat16, scaling: str = "head-wise", Skv: int = 4096, want_lse: bool = False) -> dict:
    """qattn_describe_path as a dict of names (host-only: no device call)."""
    _require(entry in ENTRY, f"unknown entry {entry!r} (expected one of {sorted(ENTRY)})")
    d = PathDesc()
    _check(lib().qattn_describe_path(ENTRY[entry], D, fmt_of(in_dtype), _scale_mode(scaling), Skv, int(want_lse), ctypes.byref(d)), "qattn_describe_path")
    return {n: PATH_DESC_NAMES[n][getattr(d, n)] for n, _ in PathDesc._fields_}


def fp8_attention_forward_rowmajor(q8: torch.Tensor, k8: torch.Tensor, v16: torch.Tensor, scale_q: torch.Tensor, scale_k: torch.Tensor, *,
                                   is_causal: bool, pv_16bit: bool = False, sm_scale: float = 0.0, precision: str = "auto",
                                   return_lse: bool = False, lse_layout: int = LSE_NATURAL):
    """The pybind function's contract in one C call (qattn_fp8_attention_forward_rowmajor; tk/attention.py:357-360): row-major fp8 q8
    [B,Hq,Sq,D] / k8 [B,Hkv,Skv,D], 16-bit v16, fp32 scales -> out in v16's dtype.  pv_16bit: V and P stay 16-bit (the reference kernel's
    numerics) instead of both GEMMs on FP8 MFMA."""
    _require(q8.is_cuda and q8.dim() == 4 and k8.dim() == 4 and v16.dim() == 4, "q8, k8 and v16 must be 4-D device tensors")
    _require(q8.dtype in (torch.float8_e4m3fn, torch.float8_e5m2) and k8.dtype == q8.dtype, "q8 / k8 must share an fp8 dtype")
    _require(v16.dtype in (torch.bfloat16, torch.float16), "v16 must be bf16 or fp16")
    q8, k8, v16 = q8.contiguous(), k8.contiguous(), v16.contiguous()
    B, Hq, Sq, D = q8.shape
    _require(k8.shape == v16.shape and k8.shape[0] == B and k8.shape[3] == D, "k8 / v16 shapes do not match q8")
    Hkv, Skv = k8.shape[1], k8.shape[2]
    _require(Hkv > 0 and Hq % Hkv == 0, f"Hq={Hq} is not a multiple of Hkv={Hkv}")
    mode = SCALE_HEAD if scale_q.dim() == 2 else SCALE_TOKEN
    _check_scales(scale_q, scale_k, None, mode, B, Hq, Hkv, Sq, Skv, q8.device)
    L = lib()
    with torch.cuda.device(q8.device):
        out = torch.empty((B, Hq, Sq, D), dtype=v16.dtype, device=q8.device)
        lse = torch.empty((B, Hq, L.qattn_lse_row_stride(Sq, lse_layout)), dtype=torch.float32, device=q8.device) if return_lse else None
        ws_bytes = L.qattn_fp8_attention_rowmajor_workspace_bytes(B, Hq, Hkv, Sq, Skv, D)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=q8.device)
        rc = L.qattn_fp8_attention_forward_rowmajor(
            q8.data_ptr(), k8.data_ptr(), v16.data_ptr(), out.data_ptr(), _ptr(lse), scale_q.contiguous().data_ptr(),
            scale_k.contiguous().data_ptr(), B, Hq, Hkv, Sq, Skv, D, fmt_of(q8.dtype), fmt_of(v16.dtype),
            fmt_of(v16.dtype) if pv_16bit else fmt_of(q8.dtype), mode, int(is_causal), float(sm_scale), _precision(precision), lse_layout,
            ws.data_ptr(), ws_bytes, _stream(q8))
    _check(rc, "qattn_fp8_attention_forward_rowmajor")
    return (out, lse[..., :Sq]) if return_lse else out


def pack16(x: torch.Tensor, layout: int) -> torch.Tensor:
    """row-major bf16/fp16 [B,H,S,D] -> flat uint8 buffer in K16FRAG / V16FRAG layout."""
    _require(x.is_cuda and x.dim() == 4 and x.dtype in (torch.bfloat16, torch.float16), "pack16 needs a 4-D bf16/fp16 device tensor")
    x = x if _strided_ok(x) else x.contiguous()     # (a strided view with head_dim innermost is read as it is: include/qattn_strided.h)
    B, H, S, D = x.shape
    L = lib()
    with torch.cuda.device(x.device):
        out = torch.empty((L.qattn_16bit_tensor_bytes(layout, B, H, S, D),), dtype=torch.uint8, device=x.device)
        rc = L.qattn_pack16_strided(x.data_ptr(), _strides3(x), out.data_ptr(), B, H, S, D, layout, _stream(x))
    _check(rc, "qattn_pack16_strided")
    return out


def attention_forward_16(q: torch.Tensor, k_frag: torch.Tensor, v_frag: torch.Tensor, *, Hkv: int, Skv: int,
                         is_causal: bool, sm_scale: float = 0.0, return_lse: bool = False, fast_exp: bool = False,
                         output_layout: str = "contiguous"):
    """q: row-major bf16/fp16 [B,Hq,Sq,D]; k_frag / v_frag: K16FRAG / V16FRAG buffers for [B,Hkv,Skv,D]."""
    _require(q.is_cuda and q.dim() == 4, "attention_forward_16 needs a 4-D device query")
    q = q if _strided_ok(q) else q.contiguous()
    B, Hq, Sq, D = q.shape
    L = lib()
    _require(k_frag.numel() * k_frag.element_size() >= L.qattn_16bit_tensor_bytes(LAYOUT_K16FRAG, B, Hkv, Skv, D)
             and v_frag.numel() * v_frag.element_size() >= L.qattn_16bit_tensor_bytes(LAYOUT_V16FRAG, B, Hkv, Skv, D),
             "k_frag / v_frag are smaller than the fragment layouts of [B,Hkv,Skv,D]")
    with torch.cuda.device(q.device):
        out = empty_output(q, q.dtype, output_layout)   # dense whatever the strides of q, unless the caller asks for q's layout
        strides = None
        if not (q.is_contiguous() and out.is_contiguous()):
            dense = (Hq * Sq * D, Sq * D, D)
            strides = (ctypes.c_longlong * 6)(*[t.stride(i) if t.shape[i] > 1 else dense[i] for t in (q, out) for i in (0, 1, 2)])
        lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=q.device) if return_lse else None
        rc = L.qattn_attention_forward_16_strided(q.data_ptr(), strides, k_frag.data_ptr(), v_frag.data_ptr(), out.data_ptr(), _ptr(lse),
                                                  B, Hq, Hkv, Sq, Skv, D, fmt_of(q.dtype), int(is_causal), float(sm_scale),
                                                  int(fast_exp), _stream(q))
    _check(rc, "qattn_attention_forward_16_strided")
    return (out, lse) if return_lse else out


def _per_head(name, t, B, H, device):
    """producer-side per-head figure: fp32 [B,H] on the tensors' device (qattn_fp8_quant_attention_forward_ex)"""
    if t is None:
        return None
    _require(t.dtype == torch.float32 and t.device == device and tuple(t.shape) == (B, H), f"{name} must be float32 {(B, H)} on {device}")
    return t.contiguous()


def fp8_quant_attention_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, is_causal: bool, scaling: str = "head-wise",
                                fp8_dtype=torch.float8_e4m3fn, numerics: str = "compiled", sm_scale: float = 0.0,
                                precision: str = "auto", amax_q: Optional[torch.Tensor] = None,
                                amax_k: Optional[torch.Tensor] = None, amax_v: Optional[torch.Tensor] = None,
                                ssq_q: Optional[torch.Tensor] = None, ssq_k: Optional[torch.Tensor] = None,
                                return_lse: bool = False, lse_layout: int = LSE_NATURAL, return_path: bool = False,
                                output_layout: str = "contiguous", smooth_k: bool = False, return_quant: bool = False):
    """16-bit q, k, v -> attention output: the quant pre-pass and the attention launch(es) in ONE C call
    (qattn_fp8_quant_attention_forward_ex); the pre-pass skips Q where the attention kernel quantises it itself.
    amax_* / ssq_*: per-head abs-max / sum of squares a producer of q, k, v already has (head-wise scaling only): the
    abs-max launch then skips those tensors, or is skipped.
    return_lse: also the per-row log-sum-exp [B,Hq,Sq] (the vector the reference defines, tk/attention.py:333-346), written by the same
    launch as the output.  return_path: also the uint8 [B,Hq,Sq] PATH_* code of every row (test / debug output).
    smooth_k: key smoothing (qattn_fp8_quant_attention_forward_smooth, include/qattn_smooth.h): K is quantised as fp32(k) - its channel mean
    over the sequence; amax_k / ssq_k describe the unsmoothed K and are refused.  return_quant (test / debug output): also a dict of what
    the call left behind -- k8 (KFRAG bytes), scale_q, scale_k, scale_v and, with smooth_k, k_mean fp32 [B,Hkv,D] -- as the last element.
    Returns out, or (out, lse), (out, path), (out, lse, path)."""
    _require(not smooth_k or (amax_k is None and ssq_k is None), "amax_k / ssq_k describe the unsmoothed key: not with smooth_k")
    B, Hq, Hkv, Sq, Skv, D = _check_qkv(q, k, v)
    # strided views (q = x.view(B, S, H, D).transpose(1, 2), slices of a packed QKV projection, ...) go to the kernels as they are
    # (include/qattn_strided.h); only what the kernels cannot address -- a head_dim that is not innermost and dense, rows off 16 bytes -- is copied
    q, k, v = (t if _strided_ok(t) else t.contiguous() for t in (q, k, v))
    out = empty_output(q, q.dtype, output_layout)
    strides = None
    if not (q.is_contiguous() and k.is_contiguous() and v.is_contiguous() and out.is_contiguous()):
        dense = lambda t: (t.shape[1] * t.shape[2] * D, t.shape[2] * D, D)     # (a dimension of size 1 has no stride of its own)
        strides = (ctypes.c_longlong * 12)(*[t.stride(i) if t.shape[i] > 1 else dense(t)[i] for t in (q, k, v, out) for i in (0, 1, 2)])
    L = lib()
    mode = _scale_mode(scaling)
    dev = q.device
    given = [x is not None for x in (amax_q, amax_k, amax_v, ssq_q, ssq_k)]
    _require(not any(given) or mode == SCALE_HEAD, "amax_* / ssq_* are per-head figures: head-wise scaling only")
    _require((ssq_q is None) == (ssq_k is None), "ssq_q and ssq_k must be both provided or both not provided")
    amax_q, ssq_q = _per_head("amax_q", amax_q, B, Hq, dev), _per_head("ssq_q", ssq_q, B, Hq, dev)
    amax_k, amax_v, ssq_k = (_per_head(n, t, B, Hkv, dev) for n, t in (("amax_k", amax_k), ("amax_v", amax_v), ("ssq_k", ssq_k)))
    with torch.cuda.device(dev):
        q8 = torch.empty((B, Hq, Sq, D), dtype=torch.uint8, device=dev)
        kf = torch.empty((L.qattn_fp8_tensor_bytes(LAYOUT_KFRAG, B, Hkv, Skv, D),), dtype=torch.uint8, device=dev)
        vf = torch.empty((L.qattn_fp8_tensor_bytes(LAYOUT_VFRAG, B, Hkv, Skv, D),), dtype=torch.uint8, device=dev)
        sq = torch.empty((B, Hq) if mode == SCALE_HEAD else (B, Hq, Sq), dtype=torch.float32, device=dev)
        sk = torch.empty((B, Hkv) if mode == SCALE_HEAD else (B, Hkv, Skv), dtype=torch.float32, device=dev)
        sv = torch.empty((B, Hkv), dtype=torch.float32, device=dev)
        if not smooth_k:
            ws_bytes = L.qattn_fp8_quant_attention_workspace_bytes(B, Hq, Hkv, Sq)
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        lse = torch.empty((B, Hq, L.qattn_lse_row_stride(Sq, lse_layout)), dtype=torch.float32, device=dev) if return_lse else None
        path = torch.empty((B, Hq, Sq), dtype=torch.uint8, device=dev) if return_path else None
        args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), strides, fmt_of(q.dtype), out.data_ptr(), q8.data_ptr(), kf.data_ptr(),
                vf.data_ptr(), sq.data_ptr(), sk.data_ptr(), sv.data_ptr(), _ptr(amax_q), _ptr(amax_k), _ptr(amax_v), _ptr(ssq_q),
                _ptr(ssq_k), B, Hq, Hkv, Sq, Skv, D, fmt_of(fp8_dtype), mode,
                _numerics(numerics), int(is_causal), float(sm_scale), _precision(precision), _ptr(lse), lse_layout, _ptr(path))
        k_mean = None
        if smooth_k:
            k_mean = torch.empty((B, Hkv, D), dtype=torch.float32, device=dev)
            ws_bytes = L.qattn_fp8_quant_attention_smooth_workspace_bytes(B, Hq, Hkv, Sq, Skv, D)
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
            rc = L.qattn_fp8_quant_attention_forward_smooth(*args, ws.data_ptr(), ws_bytes, _stream(q), k_mean.data_ptr())
        else:
            rc = L.qattn_fp8_quant_attention_forward_strided(*args, ws.data_ptr(), ws_bytes, _stream(q))
    _check(rc, "qattn_fp8_quant_attention_forward_smooth" if smooth_k else "qattn_fp8_quant_attention_forward_strided")
    if not (return_lse or return_path or return_quant):
        return out
    quant = {"k8": kf, "scale_q": sq, "scale_k": sk, "scale_v": sv, "k_mean": k_mean}
    return (out,) + ((lse[..., :Sq],) if return_lse else ()) + ((path,) if return_path else ()) + ((quant,) if return_quant else ())


def measure_attention_clock(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, is_causal: bool = False, precision: str = "auto",
                            fp8_dtype=torch.float8_e4m3fn, calls: int = 50):
    """Measurement aid: run the fused step `calls` times back to back on the stamped instantiation of the attention kernel
    (qattn_fp8_quant_attention_forward_stamped) and return (median in-kernel clock in GHz over the waves of the LAST call, median
    sweep cycles per wave, output of the last call).  D = 128, bf16, head-wise, e4m3 only."""
    B, Hq, Hkv, Sq, Skv, D = _check_qkv(q, k, v)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    L = lib()
    dev = q.device
    with torch.cuda.device(dev):
        out = torch.empty_like(q)
        q8 = torch.empty((B, Hq, Sq, D), dtype=torch.uint8, device=dev)
        kf = torch.empty((L.qattn_fp8_tensor_bytes(LAYOUT_KFRAG, B, Hkv, Skv, D),), dtype=torch.uint8, device=dev)
        vf = torch.empty((L.qattn_fp8_tensor_bytes(LAYOUT_VFRAG, B, Hkv, Skv, D),), dtype=torch.uint8, device=dev)
        sq = torch.empty((B, Hq), dtype=torch.float32, device=dev)
        sk, sv = (torch.empty((B, Hkv), dtype=torch.float32, device=dev) for _ in range(2))
        ws_bytes = L.qattn_fp8_quant_attention_workspace_bytes(B, Hq, Hkv, Sq)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        st_bytes = L.qattn_attention_stamp_bytes(B, Hq, Sq)
        stamps = torch.zeros((st_bytes // 8,), dtype=torch.int64, device=dev)
        for _ in range(calls):
            rc = L.qattn_fp8_quant_attention_forward_stamped(
                q.data_ptr(), k.data_ptr(), v.data_ptr(), fmt_of(q.dtype), out.data_ptr(), q8.data_ptr(), kf.data_ptr(), vf.data_ptr(),
                sq.data_ptr(), sk.data_ptr(), sv.data_ptr(), B, Hq, Hkv, Sq, Skv, D, fmt_of(fp8_dtype), SCALE_HEAD, NUMERICS["compiled"],
                int(is_causal), 0.0, _precision(precision), ws.data_ptr(), ws_bytes, stamps.data_ptr(), st_bytes, _stream(q))
            _check(rc, "qattn_fp8_quant_attention_forward_stamped")
        torch.cuda.synchronize(dev)
    s = stamps.view(-1, 2).double().cpu()
    s = s[s[:, 1] > 0]
    clock = (s[:, 0] / s[:, 1] * 0.1)
    return float(clock.median()), float(s[:, 0].median()), out


def measure_mfma_peak(device=None, *, seconds: float = 0.3, iters: int = 20000, constant: bool = False):
    """Measurement aid (qattn_mfma_probe): TFLOP/s and in-kernel clock (GHz) of a bare v_mfma_f32_32x32x64_f8f6f4 loop on random
    e4m3 operand bytes (|x| in [2^-2, 2^2), random sign and mantissa -- the regime of quantised N(0,1) data), two waves per SIMD on
    every CU, launched back to back for `seconds`; the figures are those of the last third of the run (settled clocks)."""
    L = lib()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        nbytes = L.qattn_mfma_probe_bytes()
        scratch = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        n_op = 2048 * 32
        if constant:
            scratch[:n_op] = 0x38
        else:
            expo = torch.randint(0x28, 0x48, (n_op,), generator=g, device=dev, dtype=torch.int32)
            sign = torch.randint(0, 2, (n_op,), generator=g, device=dev, dtype=torch.int32) << 7
            scratch[:n_op] = (expo | sign).to(torch.uint8)
        fl, nw = ctypes.c_double(0.0), ctypes.c_int(0)
        call = lambda: _check(L.qattn_mfma_probe(scratch.data_ptr(), nbytes, iters, ctypes.byref(fl), ctypes.byref(nw), _stream(scratch)),
                              "qattn_mfma_probe")
        call()
        torch.cuda.synchronize(dev)
        # the lap count bounds GPU time, not host time: launches are asynchronous (6 ms each), and a loop bounded by the host clock
        # queued 5500 of them -- 33 s of dense matrix work in front of every later measurement
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize(dev)
        n_laps = max(3, min(200, int(math.ceil(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))))
        laps = []
        for _ in range(n_laps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            laps.append((e0, e1))
        torch.cuda.synchronize(dev)
        ms = sorted(a.elapsed_time(b) for a, b in laps[len(laps) * 2 // 3:])
        med = ms[len(ms) // 2]
        st = scratch[n_op:n_op + 16 * nw.value].view(torch.int64).view(-1, 2).double().cpu()
        st = st[st[:, 1] > 0]
        clock = float((st[:, 0] / st[:, 1] * 0.1).median())
    return {"TFLOPs": fl.value / (med * 1e-3) / 1e12, "in_kernel_clock_ghz": clock, "ms_per_launch": med, "launches": len(laps),
            "waves": nw.value, "operands": "constant 1.0" if constant else "random e4m3, |x| in [2^-2, 2^2)"}


def varlen_strided_ok(t: torch.Tensor) -> bool:
    """A packed [total, H, D] view the varlen kernels address directly (include/qattn_varlen.h): the rule of `_strided_ok` -- head_dim
    innermost and dense, the token and head strides non-negative multiples of 8 elements, base 16-byte aligned."""
    if t.is_contiguous():
        return True
    return (t.stride(2) == 1 and all(t.shape[i] == 1 or (t.stride(i) >= 0 and t.stride(i) % 8 == 0) for i in (0, 1))
            and t.data_ptr() % 16 == 0)


def fp8_quant_attention_varlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor, cu_seqlens_k: torch.Tensor,
                               seqused_k: Optional[torch.Tensor] = None, *, is_causal: bool = False, fp8_dtype=torch.float8_e4m3fn,
                               numerics: str = "compiled", sm_scale: float = 0.0, return_lse: bool = False, return_quant: bool = False,
                               smooth_k: bool = False):
    """Packed variable-length sequences (qattn_fp8_quant_attention_varlen_forward): q [total_q, Hq, D], k / v [total_k, Hkv, D] bf16 / fp16,
    int32 cu_seqlens_* [B+1], optional int32 seqused_k [B] -> out [total_q, Hq, D] (and lse fp32 [Hq, total_q]).  The caller has validated
    the arguments (varlen.py); views that `varlen_strided_ok` accepts are read in place, others copied.  return_quant (test output): also
    (q8, k8, scale_q, scale_k) -- q8 the row-major per-sequence slabs (uint8, Hq D cu_q[i] bytes in), k8 the KFRAG images (Hkv D (cu_k[i] + 64 i)).
    smooth_k: key smoothing (qattn_fp8_quant_attention_varlen_forward_smooth, include/qattn_varlen.h): every sequence's K is quantised as
    fp32(k) - the channel mean of its used keys; return_quant then also returns k_mean fp32 [B, Hkv, D].
    Returns out, or a tuple of out, [lse], [q8, k8, scale_q, scale_k, [k_mean]]."""
    q, k, v = (t if varlen_strided_ok(t) else t.contiguous() for t in (q, k, v))
    total_q, Hq, D = q.shape
    total_k, Hkv = k.shape[0], k.shape[1]
    B = cu_seqlens_q.shape[0] - 1
    strides = None
    if not (q.is_contiguous() and k.is_contiguous() and v.is_contiguous()):
        dense = lambda t: (t.shape[1] * D, D)     # (a dimension of size 1 has no stride of its own)
        strides = (ctypes.c_longlong * 6)(*[t.stride(i) if t.shape[i] > 1 else dense(t)[i] for t in (q, k, v) for i in (0, 1)])
    L = lib()
    dev = q.device
    with torch.cuda.device(dev):
        out = torch.empty((total_q, Hq, D), dtype=q.dtype, device=dev)
        lse = torch.empty((Hq, total_q), dtype=torch.float32, device=dev) if return_lse else None
        q8 = k8 = sq = sk = None
        if return_quant:
            q8 = torch.empty((max(L.qattn_varlen_tensor_bytes(LAYOUT_ROWMAJOR, B, Hq, total_q, D), 1),), dtype=torch.uint8, device=dev)
            k8 = torch.empty((max(L.qattn_varlen_tensor_bytes(LAYOUT_KFRAG, B, Hkv, total_k, D), 1),), dtype=torch.uint8, device=dev)
            sq = torch.empty((B, Hq), dtype=torch.float32, device=dev)
            sk = torch.empty((B, Hkv), dtype=torch.float32, device=dev)
        ws_of = L.qattn_fp8_quant_attention_varlen_smooth_workspace_bytes if smooth_k else L.qattn_fp8_quant_attention_varlen_workspace_bytes
        ws_bytes = ws_of(B, Hq, Hkv, total_q, total_k, D)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
        args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), strides, fmt_of(q.dtype), out.data_ptr(), _ptr(lse), cu_seqlens_q.data_ptr(),
                cu_seqlens_k.data_ptr(), _ptr(seqused_k), B, Hq, Hkv, total_q, total_k, D, fmt_of(fp8_dtype), _numerics(numerics), int(is_causal),
                float(sm_scale), _ptr(q8), _ptr(k8), _ptr(sq), _ptr(sk), ws.data_ptr(), ws_bytes, _stream(q))
        k_mean = None
        if smooth_k:
            k_mean = torch.zeros((B, Hkv, D), dtype=torch.float32, device=dev) if total_q == 0 else torch.empty((B, Hkv, D), dtype=torch.float32, device=dev)
            rc = L.qattn_fp8_quant_attention_varlen_forward_smooth(*args, k_mean.data_ptr())
        else:
            rc = L.qattn_fp8_quant_attention_varlen_forward(*args)
    _check(rc, "qattn_fp8_quant_attention_varlen_forward_smooth" if smooth_k else "qattn_fp8_quant_attention_varlen_forward")
    if not (return_lse or return_quant):
        return out
    return (out,) + ((lse,) if return_lse else ()) + ((q8, k8, sq, sk) + ((k_mean,) if smooth_k else ()) if return_quant else ())


def _varlen_fp8pv(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, is_causal, window, fp8_dtype, numerics, sm_scale, precision, return_lse,
                  return_quant, return_path, smooth_k):
    """The two packed FP8-PV entries through one body: window None -> qattn_fp8_quant_attention_varlen_forward_fp8pv under is_causal,
    (left, right) -> qattn_fp8_quant_attention_varlen_window_forward_fp8pv.  Same buffers, same workspace functions, same results."""
    q, k, v = (t if varlen_strided_ok(t) else t.contiguous() for t in (q, k, v))
    total_q, Hq, D = q.shape
    total_k, Hkv = k.shape[0], k.shape[1]
    B = cu_seqlens_q.shape[0] - 1
    strides = None
    if not (q.is_contiguous() and k.is_contiguous() and v.is_contiguous()):
        dense = lambda t: (t.shape[1] * D, D)     # (a dimension of size 1 has no stride of its own)
        strides = (ctypes.c_longlong * 6)(*[t.stride(i) if t.shape[i] > 1 else dense(t)[i] for t in (q, k, v) for i in (0, 1)])
    L = lib()
    dev = q.device
    with torch.cuda.device(dev):
        out = torch.empty((total_q, Hq, D), dtype=q.dtype, device=dev)
        lse = torch.empty((Hq, total_q), dtype=torch.float32, device=dev) if return_lse else None
        q8 = k8 = v8 = sq = sk = sv = None
        if return_quant:
            q8 = torch.empty((max(L.qattn_varlen_tensor_bytes(LAYOUT_ROWMAJOR, B, Hq, total_q, D), 1),), dtype=torch.uint8, device=dev)
            k8 = torch.empty((max(L.qattn_varlen_tensor_bytes(LAYOUT_KFRAG, B, Hkv, total_k, D), 1),), dtype=torch.uint8, device=dev)
            v8 = torch.empty((max(L.qattn_varlen_tensor_bytes(LAYOUT_KFRAG, B, Hkv, total_k, D), 1),), dtype=torch.uint8, device=dev)
            sq = torch.empty((B, Hq), dtype=torch.float32, device=dev)
            sk = torch.empty((B, Hkv), dtype=torch.float32, device=dev)
            sv = torch.empty((B, Hkv), dtype=torch.float32, device=dev)
        path = torch.empty((Hq, total_q), dtype=torch.uint8, device=dev) if return_path else None
        k_mean = None
        if smooth_k:
            k_mean = torch.zeros((B, Hkv, D), dtype=torch.float32, device=dev) if total_q == 0 else torch.empty((B, Hkv, D), dtype=torch.float32, device=dev)
        ws_of = (L.qattn_fp8_quant_attention_varlen_fp8pv_smooth_workspace_bytes if smooth_k
                 else L.qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes)
        ws_bytes = ws_of(B, Hq, Hkv, total_q, total_k, D)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
        entry = L.qattn_fp8_quant_attention_varlen_forward_fp8pv if window is None else L.qattn_fp8_quant_attention_varlen_window_forward_fp8pv
        i32max = 2 ** 31 - 1
        mask = (int(is_causal),) if window is None else (min(int(window[0]), i32max), min(int(window[1]), i32max))
        rc = entry(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), strides, fmt_of(q.dtype), out.data_ptr(), _ptr(lse), cu_seqlens_q.data_ptr(),
            cu_seqlens_k.data_ptr(), _ptr(seqused_k), B, Hq, Hkv, total_q, total_k, D, fmt_of(fp8_dtype), _numerics(numerics), *mask,
            float(sm_scale), _precision(precision), _ptr(q8), _ptr(k8), _ptr(v8), _ptr(sq), _ptr(sk), _ptr(sv), _ptr(path), _ptr(k_mean),
            ws.data_ptr(), ws_bytes, _stream(q))
    _check(rc, "qattn_fp8_quant_attention_varlen_forward_fp8pv" if window is None else "qattn_fp8_quant_attention_varlen_window_forward_fp8pv")
    if not (return_lse or return_quant or return_path):
        return out
    return ((out,) + ((lse,) if return_lse else ()) + ((q8, k8, v8, sq, sk, sv) + ((k_mean,) if smooth_k else ()) if return_quant else ())
            + ((path,) if return_path else ()))


def fp8_quant_attention_varlen_fp8pv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor, cu_seqlens_k: torch.Tensor,
                                     seqused_k: Optional[torch.Tensor] = None, *, is_causal: bool = False, fp8_dtype=torch.float8_e4m3fn,
                                     numerics: str = "compiled", sm_scale: float = 0.0, precision: str = "accurate", return_lse: bool = False,
                                     return_quant: bool = False, return_path: bool = False, smooth_k: bool = False):
    """Packed variable-length sequences with FP8 P.V (qattn_fp8_quant_attention_varlen_forward_fp8pv, include/qattn_varlen.h): the arguments
    of `fp8_quant_attention_varlen`; every sequence's v is quantised head-wise over its used keys (finite there), precision "accurate"
    (two-term e4m3 P everywhere) or "fast" (one-term byte-exponential P for the 128-row tiles whose rows see >= 1024 keys).
    return_quant (test output): also (q8, k8, v8, scale_q, scale_k, scale_v) -- q8 the row-major per-sequence slabs (uint8, Hq D cu_q[i]
    bytes in), k8 / v8 the KFRAG / VFRAG images (Hkv D (cu_k[i] + 64 i) bytes in), scales fp32 [B, H] -- and, with smooth_k, k_mean fp32
    [B, Hkv, D]; return_path: also row_path uint8 [Hq, total_q] (PATH_*; columns of no sequence keep what the buffer held).
    Returns out, or a tuple of out, [lse], [q8, k8, v8, scale_q, scale_k, scale_v, [k_mean]], [row_path]."""
    _require(precision in ("fast", "accurate"), f"Unsupported precision for the packed FP8 P.V path: {precision!r} (expected 'fast' or 'accurate')")
    return _varlen_fp8pv(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, is_causal, None, fp8_dtype, numerics, sm_scale, precision, return_lse,
                         return_quant, return_path, smooth_k)


def fp8_quant_attention_varlen_window(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor, cu_seqlens_k: torch.Tensor,
                                      seqused_k: Optional[torch.Tensor] = None, *, window_left: int = -1, window_right: int = -1,
                                      fp8_dtype=torch.float8_e4m3fn, numerics: str = "compiled", sm_scale: float = 0.0, return_lse: bool = False,
                                      return_quant: bool = False, smooth_k: bool = False):
    """Sliding-window attention on packed sequences (qattn_fp8_quant_attention_varlen_window_forward, include/qattn_window.h): the arguments
    and results of `fp8_quant_attention_varlen` with (window_left, window_right) -- host ints >= -1, -1 = unbounded -- in place of is_causal.
    Row r of a sequence attends keys r + delta - window_left .. r + delta + window_right, delta = L_k(used) - L_q.
    Returns out, or a tuple of out, [lse], [q8, k8, scale_q, scale_k, [k_mean]]."""
    _require(int(window_left) >= -1 and int(window_right) >= -1, "window_left and window_right must be >= -1")
    q, k, v = (t if varlen_strided_ok(t) else t.contiguous() for t in (q, k, v))
    total_q, Hq, D = q.shape
    total_k, Hkv = k.shape[0], k.shape[1]
    B = cu_seqlens_q.shape[0] - 1
    strides = None
    if not (q.is_contiguous() and k.is_contiguous() and v.is_contiguous()):
        dense = lambda t: (t.shape[1] * D, D)     # (a dimension of size 1 has no stride of its own)
        strides = (ctypes.c_longlong * 6)(*[t.stride(i) if t.shape[i] > 1 else dense(t)[i] for t in (q, k, v) for i in (0, 1)])
    L = lib()
    dev = q.device
    i32max = 2 ** 31 - 1
    with torch.cuda.device(dev):
        out = torch.empty((total_q, Hq, D), dtype=q.dtype, device=dev)
        lse = torch.empty((Hq, total_q), dtype=torch.float32, device=dev) if return_lse else None
        q8 = k8 = sq = sk = None
        if return_quant:
            q8 = torch.empty((max(L.qattn_varlen_tensor_bytes(LAYOUT_ROWMAJOR, B, Hq, total_q, D), 1),), dtype=torch.uint8, device=dev)
            k8 = torch.empty((max(L.qattn_varlen_tensor_bytes(LAYOUT_KFRAG, B, Hkv, total_k, D), 1),), dtype=torch.uint8, device=dev)
            sq = torch.empty((B, Hq), dtype=torch.float32, device=dev)
            sk = torch.empty((B, Hkv), dtype=torch.float32, device=dev)
        ws_bytes = L.qattn_fp8_quant_attention_varlen_window_workspace_bytes(B, Hq, Hkv, total_q, total_k, D)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
        k_mean = None
        if smooth_k:
            k_mean = torch.zeros((B, Hkv, D), dtype=torch.float32, device=dev) if total_q == 0 else torch.empty((B, Hkv, D), dtype=torch.float32, device=dev)
        rc = L.qattn_fp8_quant_attention_varlen_window_forward(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), strides, fmt_of(q.dtype), out.data_ptr(), _ptr(lse), cu_seqlens_q.data_ptr(),
            cu_seqlens_k.data_ptr(), _ptr(seqused_k), B, Hq, Hkv, total_q, total_k, D, fmt_of(fp8_dtype), _numerics(numerics),
            min(int(window_left), i32max), min(int(window_right), i32max), float(sm_scale), _ptr(q8), _ptr(k8), _ptr(sq), _ptr(sk),
            ws.data_ptr(), ws_bytes, _stream(q), _ptr(k_mean))
    _check(rc, "qattn_fp8_quant_attention_varlen_window_forward")
    if not (return_lse or return_quant):
        return out
    return (out,) + ((lse,) if return_lse else ()) + ((q8, k8, sq, sk) + ((k_mean,) if smooth_k else ()) if return_quant else ())


def fp8_quant_attention_varlen_window_fp8pv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor,
                                            cu_seqlens_k: torch.Tensor, seqused_k: Optional[torch.Tensor] = None, *, window_left: int = -1,
                                            window_right: int = -1, fp8_dtype=torch.float8_e4m3fn, numerics: str = "compiled",
                                            sm_scale: float = 0.0, precision: str = "accurate", return_lse: bool = False,
                                            return_quant: bool = False, return_path: bool = False, smooth_k: bool = False):
    """Sliding-window attention on packed sequences with FP8 P.V (qattn_fp8_quant_attention_varlen_window_forward_fp8pv,
    include/qattn_window.h): the arguments and results of `fp8_quant_attention_varlen_fp8pv` with (window_left, window_right) -- host ints
    >= -1, -1 = unbounded -- in place of is_causal.  Row r of a sequence attends keys r + delta - window_left .. r + delta + window_right,
    delta = L_k(used) - L_q; precision "fast" runs the one-term sweep on the 128-row tiles whose rows attend an interval of >= 1024 keys.
    Returns out, or a tuple of out, [lse], [q8, k8, v8, scale_q, scale_k, scale_v, [k_mean]], [row_path]."""
    _require(int(window_left) >= -1 and int(window_right) >= -1, "window_left and window_right must be >= -1")
    _require(precision in ("fast", "accurate"), f"Unsupported precision for the sliding-window FP8 P.V path: {precision!r} (expected 'fast' or 'accurate')")
    return _varlen_fp8pv(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, False, (window_left, window_right), fp8_dtype, numerics, sm_scale,
                         precision, return_lse, return_quant, return_path, smooth_k)


def fp8_block_sparse_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_mask: torch.Tensor, *, fp8_dtype=torch.float8_e4m3fn,
                               numerics: str = "compiled", sm_scale: float = 0.0, return_lse: bool = False, return_quant: bool = False,
                               smooth_k: bool = False):
    """Block-sparse attention (qattn_fp8_block_sparse_attention_forward): q [B,Hq,Sq,D], k / v [B,Hkv,Skv,D] bf16 / fp16; block_mask bool,
    broadcastable to [B, Hq, ceil(Sq/128), ceil(Skv/128)] and read through its strides (an expanded view costs no copy) -> out [B,Hq,Sq,D]
    (and lse fp32 [B,Hq,Sq]).  return_quant (test output): also (q8, k8, scale_q, scale_k), row-major fp8 and fp32 [B,H].
    smooth_k: key smoothing (qattn_fp8_block_sparse_attention_forward_smooth, include/qattn_block_sparse.h): K is quantised as fp32(k) - its channel
    mean over the whole Skv; return_quant then returns k8 as the KFRAG image the kernel reads (flat uint8, the dense smoothing entry's k8)
    and also k_mean fp32 [B, Hkv, D].
    Returns out, or a tuple of out, [lse], [q8, k8, scale_q, scale_k, [k_mean]]."""
    B, Hq, Hkv, Sq, Skv, D = _check_qkv(q, k, v)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    nb = BLOCK_SPARSE_BLOCK
    m = block_mask.expand(B, Hq, -(-Sq // nb), -(-Skv // nb))
    _require(m.dtype == torch.bool and m.device == q.device, f"block_mask must be a torch.bool tensor on {q.device}")
    strides = (ctypes.c_longlong * 4)(*[m.stride(i) if m.shape[i] > 1 else 0 for i in range(4)])   # (0: broadcast)
    L = lib()
    dev = q.device
    with torch.cuda.device(dev):
        out = torch.empty((B, Hq, Sq, D), dtype=q.dtype, device=dev)
        lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=dev) if return_lse else None
        q8 = k8 = sq = sk = None
        if return_quant:
            q8 = torch.empty((B, Hq, Sq, D), dtype=fp8_dtype, device=dev)
            if smooth_k:
                k8 = torch.empty((L.qattn_fp8_tensor_bytes(LAYOUT_KFRAG, B, Hkv, Skv, D),), dtype=torch.uint8, device=dev)
            else:
                k8 = torch.empty((B, Hkv, Skv, D), dtype=fp8_dtype, device=dev)
            sq = torch.empty((B, Hq), dtype=torch.float32, device=dev)
            sk = torch.empty((B, Hkv), dtype=torch.float32, device=dev)
        ws_of = L.qattn_fp8_block_sparse_attention_smooth_workspace_bytes if smooth_k else L.qattn_fp8_block_sparse_attention_workspace_bytes
        ws_bytes = ws_of(B, Hq, Hkv, Sq, Skv, D)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
        args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), fmt_of(q.dtype), out.data_ptr(), _ptr(lse), m.data_ptr(), strides, B, Hq, Hkv, Sq, Skv, D,
                fmt_of(fp8_dtype), _numerics(numerics), float(sm_scale), _ptr(q8), _ptr(k8), _ptr(sq), _ptr(sk), ws.data_ptr(), ws_bytes, _stream(q))
        k_mean = None
        if smooth_k:
            k_mean = torch.empty((B, Hkv, D), dtype=torch.float32, device=dev)
            rc = L.qattn_fp8_block_sparse_attention_forward_smooth(*args, k_mean.data_ptr())
        else:
            rc = L.qattn_fp8_block_sparse_attention_forward(*args)
    _check(rc, "qattn_fp8_block_sparse_attention_forward_smooth" if smooth_k else "qattn_fp8_block_sparse_attention_forward")
    if not (return_lse or return_quant):
        return out
    return (out,) + ((lse,) if return_lse else ()) + ((q8, k8, sq, sk) + ((k_mean,) if smooth_k else ()) if return_quant else ())


def fp8_block_sparse_attention_fp8pv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_mask: torch.Tensor, *,
                                     fp8_dtype=torch.float8_e4m3fn, numerics: str = "compiled", sm_scale: float = 0.0,
                                     precision: str = "accurate", return_lse: bool = False, return_quant: bool = False,
                                     return_path: bool = False, smooth_k: bool = False):
    """Block-sparse attention with FP8 P.V (qattn_fp8_block_sparse_attention_forward_fp8pv, include/qattn_block_sparse.h): the arguments of
    fp8_block_sparse_attention; v is quantised head-wise over the whole tensor (it must be finite everywhere), precision "accurate"
    (two-term e4m3 P everywhere) or "fast" (one-term byte-exponential P for the query blocks that list >= 1024 keys).
    return_quant (test output): also (q8, k8, v8, scale_q, scale_k, scale_v), row-major fp8 and fp32 [B,H] -- with smooth_k k8 is the KFRAG
    image (flat uint8) and k_mean fp32 [B, Hkv, D] follows; return_path: also row_path uint8 [B, Hq, Sq] (PATH_*).
    Returns out, or a tuple of out, [lse], [q8, k8, v8, scale_q, scale_k, scale_v, [k_mean]], [row_path]."""
    _require(precision in ("fast", "accurate"), f"Unsupported precision for the block-sparse FP8 P.V path: {precision!r} (expected 'fast' or 'accurate')")
    B, Hq, Hkv, Sq, Skv, D = _check_qkv(q, k, v)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    nb = BLOCK_SPARSE_BLOCK
    m = block_mask.expand(B, Hq, -(-Sq // nb), -(-Skv // nb))
    _require(m.dtype == torch.bool and m.device == q.device, f"block_mask must be a torch.bool tensor on {q.device}")
    strides = (ctypes.c_longlong * 4)(*[m.stride(i) if m.shape[i] > 1 else 0 for i in range(4)])   # (0: broadcast)
    L = lib()
    dev = q.device
    with torch.cuda.device(dev):
        out = torch.empty((B, Hq, Sq, D), dtype=q.dtype, device=dev)
        lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=dev) if return_lse else None
        q8 = k8 = v8 = sq = sk = sv = None
        if return_quant:
            q8 = torch.empty((B, Hq, Sq, D), dtype=fp8_dtype, device=dev)
            if smooth_k:
                k8 = torch.empty((L.qattn_fp8_tensor_bytes(LAYOUT_KFRAG, B, Hkv, Skv, D),), dtype=torch.uint8, device=dev)
            else:
                k8 = torch.empty((B, Hkv, Skv, D), dtype=fp8_dtype, device=dev)
            v8 = torch.empty((B, Hkv, Skv, D), dtype=fp8_dtype, device=dev)
            sq = torch.empty((B, Hq), dtype=torch.float32, device=dev)
            sk = torch.empty((B, Hkv), dtype=torch.float32, device=dev)
            sv = torch.empty((B, Hkv), dtype=torch.float32, device=dev)
        path = torch.empty((B, Hq, Sq), dtype=torch.uint8, device=dev) if return_path else None
        k_mean = torch.empty((B, Hkv, D), dtype=torch.float32, device=dev) if smooth_k else None
        ws_of = (L.qattn_fp8_block_sparse_attention_fp8pv_smooth_workspace_bytes if smooth_k
                 else L.qattn_fp8_block_sparse_attention_fp8pv_workspace_bytes)
        ws_bytes = ws_of(B, Hq, Hkv, Sq, Skv, D)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
        rc = L.qattn_fp8_block_sparse_attention_forward_fp8pv(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), fmt_of(q.dtype), out.data_ptr(), _ptr(lse), m.data_ptr(), strides, B, Hq, Hkv, Sq, Skv, D,
            fmt_of(fp8_dtype), _numerics(numerics), float(sm_scale), _precision(precision), _ptr(q8), _ptr(k8), _ptr(v8), _ptr(sq), _ptr(sk),
            _ptr(sv), _ptr(path), _ptr(k_mean), ws.data_ptr(), ws_bytes, _stream(q))
    _check(rc, "qattn_fp8_block_sparse_attention_forward_fp8pv")
    if not (return_lse or return_quant or return_path):
        return out
    return ((out,) + ((lse,) if return_lse else ()) + ((q8, k8, v8, sq, sk, sv) + ((k_mean,) if smooth_k else ()) if return_quant else ())
            + ((path,) if return_path else ()))


def merge_addressable(o: torch.Tensor) -> bool:
    """An O tensor ([B,H,S,D] or packed [total,H,D]) the merge kernel addresses as it is (include/qattn_merge.h): head_dim innermost and
    dense, base and rows 16-byte aligned, no negative stride."""
    per16 = 16 // o.element_size()
    return (o.stride(-1) == 1 and o.data_ptr() % 16 == 0
            and all(o.shape[i] == 1 or (o.stride(i) >= 0 and o.stride(i) % per16 == 0) for i in range(o.dim() - 1)))


def _merge_strides(o: torch.Tensor, lse: torch.Tensor):
    """{batch, head, row} element strides of one state's O and LSE: dense [B,H,S,D] / [B,H,S], or packed [total,H,D] / [H,total] (B = 1)."""
    if o.dim() == 4:
        return (o.stride(0), o.stride(1), o.stride(2)), (lse.stride(0), lse.stride(1), lse.stride(2))
    return (0, o.stride(1), o.stride(0)), (0, lse.stride(0), lse.stride(1))


def attention_state_merge(outs, lses, *, out: Optional[torch.Tensor] = None, lse_out: Optional[torch.Tensor] = None,
                          out_dtype: Optional[torch.dtype] = None, return_lse: bool = True):
    return _attention_state_merge(outs, lses, None, out, lse_out, out_dtype, return_lse)


def attention_state_merge_sink(outs, lses, sinks: torch.Tensor, *, out: Optional[torch.Tensor] = None, lse_out: Optional[torch.Tensor] = None,
                               out_dtype: Optional[torch.dtype] = None, return_lse: bool = True):
    """qattn_attention_state_merge_sink (include/qattn_sinks.h): `attention_state_merge` of 1 .. 8 states with sinks, fp32 [H] on the
    device -- the learned sink of every head as one more state without an O row."""
    return _attention_state_merge(outs, lses, sinks, out, lse_out, out_dtype, return_lse)


def _attention_state_merge(outs, lses, sinks, out, lse_out, out_dtype, return_lse):
    """qattn_attention_state_merge (include/qattn_merge.h) in one launch: 2 .. 8 partial states (outs[i], lses[i]) of the same queries over
    disjoint key sets -> the state over the union.  outs[i]: [B,H,S,D] with lses[i] fp32 [B,H,S], or packed [total,H,D] with [H,total];
    bf16 / fp16 / fp32, each its own; any strides with head_dim innermost and 16-byte rows go to the kernel as they are (the stride table
    is built from the tensors; anything else is copied).  out / lse_out: caller's buffers (never copied: they must be addressable), e.g.
    outs[0] / lses[0] themselves for the in-place accumulate; else fresh dense tensors of out_dtype (default: outs[0]'s).  The caller has
    validated shapes and dtypes (merge.merge_attn_states).  Returns (out, lse_out), or out without return_lse (no LSE is written then,
    unless lse_out is given).  (sinks: the entry of `attention_state_merge_sink` instead.)"""
    n = len(outs)
    _require((2 if sinks is None else 1) <= n <= MERGE_MAX_PARTIALS and len(lses) == n,
             f"attention_state_merge takes {2 if sinks is None else 1} .. {MERGE_MAX_PARTIALS} states per launch, got {n}")
    o0 = outs[0]
    _require(o0.is_cuda and o0.dim() in (3, 4) and lses[0].dim() == o0.dim() - 1, "states must be device tensors [B,H,S,D] / [B,H,S] or [total,H,D] / [H,total]")
    outs = [o if merge_addressable(o) else o.contiguous() for o in outs]
    dev = o0.device
    if o0.dim() == 4:
        B, H, S, D = o0.shape
    else:
        (S, H, D), B = o0.shape, 1
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(o0.shape, dtype=out_dtype or o0.dtype, device=dev)
        if lse_out is None and return_lse:
            lse_out = torch.empty(lses[0].shape, dtype=torch.float32, device=dev)
        _require(out.shape == o0.shape and out.dtype in _MERGE_FMT and merge_addressable(out),
                 "out must have the states' shape, head_dim innermost and dense, 16-byte aligned rows")
        _require(lse_out is None or (lse_out.shape == lses[0].shape and lse_out.dtype == torch.float32), "lse_out must be float32 of the LSEs' shape")
        if B * H * S == 0:
            return (out, lse_out) if return_lse else out
        o_str, l_str = zip(*(_merge_strides(o, l) for o, l in zip(outs, lses)))
        out_str, lout_str = _merge_strides(out, lse_out if lse_out is not None else lses[0])
        ll = ctypes.c_longlong
        entry, sink_arg = lib().qattn_attention_state_merge, ()
        if sinks is not None:
            _require(sinks.dtype == torch.float32 and sinks.device == dev and tuple(sinks.shape) == (H,) and sinks.is_contiguous(),
                     f"sinks must be a dense float32 [H={H}] tensor on {dev}")
            entry, sink_arg = lib().qattn_attention_state_merge_sink, (sinks.data_ptr(),)
        rc = entry(
            n, (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs]), (ctypes.c_int * n)(*[_MERGE_FMT[o.dtype] for o in outs]),
            (ll * (3 * n))(*[x for st in o_str for x in st]), (ctypes.c_void_p * n)(*[l.data_ptr() for l in lses]),
            (ll * (3 * n))(*[x for st in l_str for x in st]), out.data_ptr(), _MERGE_FMT[out.dtype], (ll * 3)(*out_str), _ptr(lse_out),
            (ll * 3)(*lout_str), B, H, S, D, _stream(o0), *sink_arg)
    _check(rc, "qattn_attention_state_merge" if sinks is None else "qattn_attention_state_merge_sink")
    return (out, lse_out) if return_lse else out


def rope_table_args(cos: torch.Tensor, sin: torch.Tensor):
    """A cos / sin pair (fp32 [T, D/2] or [B, T, D/2], already validated by rope.py) as the C entries take it (include/qattn_rope.h):
    (cos, sin, batch stride, row stride) in floats.  Slices and other views go as they are when the kernels can address them -- entries of a
    row dense, base 16-byte aligned, strides multiples of 4 floats, the same strides for both tables; anything else is copied."""
    def ok(t):
        return (t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(t.shape[d] == 1 or t.stride(d) % 4 == 0 for d in range(t.dim() - 1)))
    if not (ok(cos) and ok(sin) and cos.stride() == sin.stride()):
        cos, sin = cos.contiguous(), sin.contiguous()
    tb = cos.stride(0) if (cos.dim() == 3 and cos.shape[0] > 1) else 0
    tr = cos.stride(-2) if cos.shape[-2] > 1 else cos.shape[-1]
    return cos, sin, tb, tr


def _strides6(q: torch.Tensor, k: torch.Tensor):
    """{batch, head, row} element strides of q then of k for the RoPE entries (None: both dense)."""
    if q.is_contiguous() and k.is_contiguous():
        return None
    D = q.shape[3]
    dense = lambda t: (t.shape[1] * t.shape[2] * D, t.shape[2] * D, D)     # (a dimension of size 1 has no stride of its own)
    return (ctypes.c_longlong * 6)(*[t.stride(i) if t.shape[i] > 1 else dense(t)[i] for t in (q, k) for i in (0, 1, 2)])


def rope_quant_fp8(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *, interleaved: bool = False, scaling: str = "head-wise",
                   fp8_dtype=torch.float8_e4m3fn, numerics: str = "compiled", layout: int = LAYOUT_ROWMAJOR):
    """qattn_rope_quant_qk_fp8 on ONE tensor x [B,H,S,D] (include/qattn_rope.h): rotate with the tables, quantise -> (payload, scale), the
    payload row-major fp8 of x's shape or (layout = LAYOUT_KFRAG, through the entry's k slot) a flat uint8 KFRAG image."""
    _require(x.is_cuda and x.dim() == 4 and x.dtype in (torch.bfloat16, torch.float16), "rope_quant_fp8 needs a 4-D bf16 / fp16 device tensor")
    _require(layout in (LAYOUT_ROWMAJOR, LAYOUT_KFRAG), "rope_quant_fp8 writes the row-major or the KFRAG layout")
    x = x if _strided_ok(x) else x.contiguous()
    B, H, S, D = x.shape
    L = lib()
    mode = _scale_mode(scaling)
    cos, sin, tb, tr = rope_table_args(cos, sin)
    dev = x.device
    with torch.cuda.device(dev):
        if layout == LAYOUT_ROWMAJOR:
            out = torch.empty((B, H, S, D), dtype=fp8_dtype, device=dev)
        else:
            out = torch.empty((L.qattn_fp8_tensor_bytes(layout, B, H, S, D),), dtype=torch.uint8, device=dev)
        scale = torch.empty((B, H) if mode == SCALE_HEAD else (B, H, S), dtype=torch.float32, device=dev)
        ws_bytes = L.qattn_rope_quant_qk_workspace_bytes(B, H, H)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
        strides = _strides6(x, x)
        as_k = layout == LAYOUT_KFRAG
        tab = (cos.data_ptr(), sin.data_ptr(), tb, tr)
        none = (None, None, 0, 0)
        rc = L.qattn_rope_quant_qk_fp8(None if as_k else x.data_ptr(), x.data_ptr() if as_k else None, strides, fmt_of(x.dtype),
                                       *(none if as_k else tab), *(tab if as_k else none), int(bool(interleaved)),
                                       None if as_k else out.data_ptr(), out.data_ptr() if as_k else None, layout,
                                       None if as_k else scale.data_ptr(), scale.data_ptr() if as_k else None, B, H, H, S, S, D,
                                       fmt_of(fp8_dtype), mode, _numerics(numerics), ws.data_ptr(), ws_bytes, _stream(x))
    _check(rc, "qattn_rope_quant_qk_fp8")
    return out, scale


def fp8_rope_quant_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos_q: torch.Tensor, sin_q: torch.Tensor,
                             cos_k: torch.Tensor, sin_k: torch.Tensor, *, interleaved: bool = False, is_causal: bool = False,
                             scaling: str = "head-wise", fp8_dtype=torch.float8_e4m3fn, numerics: str = "compiled", sm_scale: float = 0.0,
                             precision: str = "auto", pv_16bit: bool = False, return_lse: bool = False, return_quant: bool = False):
    """qattn_fp8_rope_quant_attention_forward (include/qattn_rope.h): unrotated 16-bit q, k with their cos / sin tables, 16-bit v -> attention
    output, in one C call: the RoPE + quantise pre-pass of q and k, V through the head-wise quantiser (pv_16bit: kept 16-bit), then the
    existing fp8 attention entry.  q and k may be strided views (include/qattn_strided.h's rules); v is made dense.
    return_quant (test output): also a dict of q8 (row-major fp8), k8 (KFRAG bytes), scale_q, scale_k, and v8 / scale_v with an fp8 V.
    Returns out, or a tuple of out, [lse], [quant]."""
    B, Hq, Hkv, Sq, Skv, D = _check_qkv(q, k, v)
    q, k = (t if _strided_ok(t) else t.contiguous() for t in (q, k))
    v = v.contiguous()
    L = lib()
    mode = _scale_mode(scaling)
    dev = q.device
    cos_q, sin_q, qtb, qtr = rope_table_args(cos_q, sin_q)
    cos_k, sin_k, ktb, ktr = rope_table_args(cos_k, sin_k)
    with torch.cuda.device(dev):
        out = torch.empty((B, Hq, Sq, D), dtype=q.dtype, device=dev)
        lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=dev) if return_lse else None
        q8 = torch.empty((B, Hq, Sq, D), dtype=fp8_dtype, device=dev)
        kf = torch.empty((L.qattn_fp8_tensor_bytes(LAYOUT_KFRAG, B, Hkv, Skv, D),), dtype=torch.uint8, device=dev)
        sq = torch.empty((B, Hq) if mode == SCALE_HEAD else (B, Hq, Sq), dtype=torch.float32, device=dev)
        sk = torch.empty((B, Hkv) if mode == SCALE_HEAD else (B, Hkv, Skv), dtype=torch.float32, device=dev)
        vf = sv = None
        if not pv_16bit:
            vf = torch.empty((L.qattn_fp8_tensor_bytes(LAYOUT_VFRAG, B, Hkv, Skv, D),), dtype=torch.uint8, device=dev)
            sv = torch.empty((B, Hkv), dtype=torch.float32, device=dev)
        ws_bytes = L.qattn_fp8_rope_quant_attention_workspace_bytes(B, Hq, Hkv, Sq, Skv, D)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        rc = L.qattn_fp8_rope_quant_attention_forward(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), _strides6(q, k), fmt_of(q.dtype), cos_q.data_ptr(), sin_q.data_ptr(), qtb, qtr,
            cos_k.data_ptr(), sin_k.data_ptr(), ktb, ktr, int(bool(interleaved)), out.data_ptr(), _ptr(lse), q8.data_ptr(), kf.data_ptr(),
            _ptr(vf), sq.data_ptr(), sk.data_ptr(), _ptr(sv), B, Hq, Hkv, Sq, Skv, D, fmt_of(fp8_dtype),
            fmt_of(q.dtype) if pv_16bit else fmt_of(fp8_dtype), mode, _numerics(numerics), int(is_causal), float(sm_scale),
            _precision(precision), LSE_NATURAL, ws.data_ptr(), ws_bytes, _stream(q))
    _check(rc, "qattn_fp8_rope_quant_attention_forward")
    if not (return_lse or return_quant):
        return out
    quant = {"q8": q8, "k8": kf, "v8": vf, "scale_q": sq, "scale_k": sk, "scale_v": sv}
    return (out,) + ((lse,) if return_lse else ()) + ((quant,) if return_quant else ())


def splitkv_window_auto_splits(B: int, Hq: int, Hkv: int, Sq: int, Skv: int, D: int, window_left: int, num_cus: int) -> int:
    """qattn_splitkv_window_auto_splits (include/qattn_splitkv_window.h): the num_splits = 0 rule of the dense window entries."""
    return int(lib().qattn_splitkv_window_auto_splits(B, Hq, Hkv, Sq, Skv, D, window_left, num_cus))


def paged_varlen_window_auto_splits(B: int, Hq: int, Hkv: int, total_q: int, max_seqlen_q: int, Skv: int, D: int, window_left: int,
                                    num_cus: int) -> int:
    """qattn_paged_varlen_window_auto_splits (include/qattn_splitkv_window.h): the num_splits = 0 rule of the packed window entry."""
    return int(lib().qattn_paged_varlen_window_auto_splits(B, Hq, Hkv, total_q, max_seqlen_q, Skv, D, window_left, num_cus))


def _window_args(window):
    """(window_left, window_right) of a window entry as C ints."""
    _require(len(window) == 2 and all(isinstance(w, int) and not isinstance(w, bool) and w >= -1 for w in window),
             f"window must be a pair of integers >= -1, got {window!r}")
    return int(window[0]), int(window[1])


def _sink_args(sinks, window, Hq, dev):
    """() without sinks, else (the pointer,): the sink entries (include/qattn_sinks.h) take it right after window_left, window_right."""
    if sinks is None:
        return ()
    _require(window is not None, "sinks are offered by the window entries: pass window=(left, right)")
    _require(sinks.dtype == torch.float32 and sinks.device == dev and tuple(sinks.shape) == (Hq,) and sinks.is_contiguous(),
             f"sinks must be a dense float32 [Hq={Hq}] tensor on {dev}")
    return (sinks.data_ptr(),)


def _softcap_args(softcap, window, sinks, tree_mask=None):
    """() without a soft cap, else (the float,): the soft-cap entries (include/qattn_softcap.h) take it right after window_left, window_right."""
    if softcap is None:
        return ()
    _require(window is not None, "softcap is offered by the window entries: pass window=(left, right)")
    _require(sinks is None and tree_mask is None, "softcap is not offered with sinks or under a draft tree")
    _require(isinstance(softcap, (int, float)) and not isinstance(softcap, bool) and math.isfinite(softcap) and softcap > 0,
             f"softcap must be a finite float > 0, got {softcap!r}")
    return (float(softcap),)


def splitkv_auto_splits(B: int, Hq: int, Hkv: int, Sq: int, Skv: int, D: int, num_cus: int) -> int:
    """qattn_splitkv_auto_splits (include/qattn_splitkv.h): the num_splits = 0 rule, a pure host function of the shape and the CU count."""
    return int(lib().qattn_splitkv_auto_splits(B, Hq, Hkv, Sq, Skv, D, num_cus))


def fp8_attention_splitkv(q: torch.Tensor, k_frag: torch.Tensor, v_frag: torch.Tensor, scale_k: torch.Tensor, scale_v: torch.Tensor, *,
                          Skv: int, fp8_dtype=torch.float8_e4m3fn, numerics: str = "compiled", is_causal: bool = False,
                          sm_scale: float = 0.0, precision: str = "accurate", num_splits: int = 0,
                          seqused_k: Optional[torch.Tensor] = None, return_lse: bool = False, return_partials: bool = False,
                          return_quant: bool = False, return_path: bool = False, window: Optional[Tuple[int, int]] = None,
                          sinks: Optional[torch.Tensor] = None, softcap: Optional[float] = None):
    """Split-KV attention over prepared K / V (qattn_fp8_attention_splitkv_forward, include/qattn_splitkv.h).  q [B, Hq, Sq, D] bf16 / fp16;
    k_frag / v_frag: the KFRAG / VFRAG images (flat uint8) of [B, Hkv, Skv, D] in fp8_dtype with scale_k / scale_v fp32 [B, Hkv];
    seqused_k int32 [B] on the device or None.  num_splits 0: the auto rule on the device's CU count (resolved here, on the host).
    Returns out, or a tuple of out, [lse], [partial_o fp32 [ns, B, Hq, Sq, D], partial_lse [ns, B, Hq, Sq], partial_path uint8 -- three
    empty tensors when the call ran one split], [q8, scale_q], [row_path uint8 [B, Hq, Sq]].
    window = (left, right): qattn_fp8_attention_splitkv_window_forward (include/qattn_splitkv_window.h) instead -- the window stands in
    is_causal's place, which is then not read; the same for the two paged functions below.
    sinks (with window; fp32 [Hq] on the device): qattn_fp8_attention_splitkv_sink_forward (include/qattn_sinks.h) -- a learned sink logit
    per query head in the softmax denominator; the partials stay free of it.  Again the same for the two paged functions.
    softcap (with window, without sinks; a finite float > 0): qattn_fp8_attention_splitkv_softcap_forward (include/qattn_softcap.h) --
    y = softcap tanh(x / softcap) on the scaled scores, before the mask.  Again the same for the two paged functions."""
    _require(precision in ("fast", "accurate"), f"Unsupported precision for the split-KV entry: {precision!r} (expected 'fast' or 'accurate')")
    _require(q.is_cuda and q.dim() == 4 and q.dtype in (torch.bfloat16, torch.float16), "query must be a 4-D bf16 / fp16 device tensor")
    _require(0 <= int(num_splits) <= SPLITKV_MAX_SPLITS, f"num_splits must be 0 (auto) or 1 .. {SPLITKV_MAX_SPLITS}, got {num_splits}")
    mask_args = (int(bool(is_causal)),) if window is None else _window_args(window)
    q = q.contiguous()
    B, Hq, Sq, D = q.shape
    mask_args += _sink_args(sinks, window, Hq, q.device) + _softcap_args(softcap, window, sinks)
    _require(scale_k.dim() == 2 and scale_k.shape[0] == B and scale_k.shape == scale_v.shape, "scale_k / scale_v must be fp32 [B, Hkv]")
    Hkv = scale_k.shape[1]
    _require(Hkv > 0 and Hq % Hkv == 0, f"Hq={Hq} is not a multiple of Hkv={Hkv}")
    L = lib()
    dev = q.device
    for name, img, layout in (("k", k_frag, LAYOUT_KFRAG), ("v", v_frag, LAYOUT_VFRAG)):
        _require(img.device == dev and img.dtype == torch.uint8 and img.is_contiguous()
                 and img.numel() == L.qattn_fp8_tensor_bytes(layout, B, Hkv, Skv, D), f"the prepared {name} image does not fit [B={B}, Hkv={Hkv}, Skv={Skv}, D={D}]")
    for name, sc in (("scale_k", scale_k), ("scale_v", scale_v)):
        _require(sc.dtype == torch.float32 and sc.device == dev and sc.is_contiguous(), f"{name} must be a dense float32 tensor on {dev}")
    if seqused_k is not None:
        _require(seqused_k.dtype == torch.int32 and seqused_k.device == dev and tuple(seqused_k.shape) == (B,) and seqused_k.is_contiguous(),
                 f"seqused_k must be a dense int32 [B] tensor on {dev}")
    ns = int(num_splits)
    if ns == 0:
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        ns = splitkv_auto_splits(B, Hq, Hkv, Sq, Skv, D, cus) if window is None else splitkv_window_auto_splits(B, Hq, Hkv, Sq, Skv, D, window[0], cus)
    with torch.cuda.device(dev):
        out = torch.empty((B, Hq, Sq, D), dtype=q.dtype, device=dev)
        lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=dev) if return_lse else None
        po = plse = ppath = q8 = sq = path = None
        if return_partials:
            n = ns if ns > 1 else 0
            po = torch.empty((n, B, Hq, Sq, D), dtype=torch.float32, device=dev)
            plse = torch.empty((n, B, Hq, Sq), dtype=torch.float32, device=dev)
            ppath = torch.empty((n, B, Hq, Sq), dtype=torch.uint8, device=dev)
        if return_quant:
            q8 = torch.empty((B, Hq, Sq, D), dtype=fp8_dtype, device=dev)
            sq = torch.empty((B, Hq), dtype=torch.float32, device=dev)
        if return_path:
            path = torch.empty((B, Hq, Sq), dtype=torch.uint8, device=dev)
        ws_bytes = L.qattn_fp8_attention_splitkv_workspace_bytes(B, Hq, Hkv, Sq, Skv, D, ns)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
        live = lambda t: _ptr(t) if t is not None and t.numel() else None
        fwd = (L.qattn_fp8_attention_splitkv_softcap_forward if softcap is not None
               else L.qattn_fp8_attention_splitkv_forward if window is None else L.qattn_fp8_attention_splitkv_window_forward if sinks is None
               else L.qattn_fp8_attention_splitkv_sink_forward)
        rc = fwd(
            q.data_ptr(), fmt_of(q.dtype), k_frag.data_ptr(), v_frag.data_ptr(), scale_k.data_ptr(), scale_v.data_ptr(), out.data_ptr(),
            _ptr(lse), _ptr(seqused_k), B, Hq, Hkv, Sq, Skv, D, fmt_of(fp8_dtype), _numerics(numerics), *mask_args, float(sm_scale),
            _precision(precision), ns, _ptr(q8), _ptr(sq), _ptr(path), live(po), live(plse), live(ppath), ws.data_ptr(), ws_bytes, _stream(q))
    _check(rc, "qattn_fp8_attention_splitkv_softcap_forward" if softcap is not None
           else "qattn_fp8_attention_splitkv_forward" if window is None else "qattn_fp8_attention_splitkv_window_forward" if sinks is None
           else "qattn_fp8_attention_splitkv_sink_forward")
    if not (return_lse or return_partials or return_quant or return_path):
        return out
    return ((out,) + ((lse,) if return_lse else ()) + ((po, plse, ppath) if return_partials else ()) + ((q8, sq) if return_quant else ())
            + ((path,) if return_path else ()))


def kv_append_addressable(t: torch.Tensor) -> bool:
    """A 4-D view [B, Hkv, T, D] qattn_kv_cache_append_fp8 reads in place (include/qattn_kvcache.h): head_dim innermost and dense, every
    other stride of a dimension longer than 1 a non-negative multiple of 8 elements, base 16-byte aligned (rows 16-byte aligned)."""
    return (t.dim() == 4 and (t.shape[3] == 1 or t.stride(3) == 1) and t.data_ptr() % 16 == 0
            and all(t.shape[i] == 1 or (t.stride(i) >= 0 and t.stride(i) % 8 == 0) for i in (0, 1, 2)))


def kv_cache_append_fp8(k_frag: torch.Tensor, v_frag: torch.Tensor, scale_k: torch.Tensor, scale_v: torch.Tensor, seqlens: torch.Tensor,
                        k_new: torch.Tensor, v_new: torch.Tensor, *, capacity: int, fp8_dtype=torch.float8_e4m3fn,
                        new_lens: Optional[torch.Tensor] = None, advance: bool = True) -> None:
    """qattn_kv_cache_append_fp8 (include/qattn_kvcache.h): quantise k_new / v_new [B, Hkv, T, D] (bf16 / fp16; dense or a view
    `kv_append_addressable` accepts, read in place) with the cache's scales fp32 [B, Hkv] and write them into the KFRAG / VFRAG images
    (flat uint8) of [B, Hkv, capacity, D] from key seqlens[b] on; seqlens int32 [B] and new_lens (int32 [B] or None) are read on the
    device, seqlens is advanced unless advance is False.  Mutates k_frag, v_frag and seqlens."""
    _require(k_new.is_cuda and k_new.dim() == 4 and k_new.dtype in (torch.bfloat16, torch.float16), "k_new must be a 4-D bf16 / fp16 device tensor")
    _require(v_new.shape == k_new.shape and v_new.dtype == k_new.dtype and v_new.device == k_new.device, "k_new and v_new must agree in shape, dtype and device")
    _require(kv_append_addressable(k_new) and kv_append_addressable(v_new), "k_new / v_new need head_dim innermost and 16-byte-aligned rows")
    B, Hkv, T, D = k_new.shape
    L = lib()
    dev = k_new.device
    for name, img, layout in (("k", k_frag, LAYOUT_KFRAG), ("v", v_frag, LAYOUT_VFRAG)):
        _require(img.device == dev and img.dtype == torch.uint8 and img.is_contiguous()
                 and img.numel() == L.qattn_fp8_tensor_bytes(layout, B, Hkv, capacity, D), f"the cache's {name} image does not fit [B={B}, Hkv={Hkv}, capacity={capacity}, D={D}]")
    for name, sc in (("scale_k", scale_k), ("scale_v", scale_v)):
        _require(sc.dtype == torch.float32 and sc.device == dev and sc.is_contiguous() and tuple(sc.shape) == (B, Hkv), f"{name} must be a dense float32 [B, Hkv] tensor on {dev}")
    for name, t in (("seqlens", seqlens), ("new_lens", new_lens)):
        _require(t is None and name == "new_lens" or (t is not None and t.dtype == torch.int32 and t.device == dev and tuple(t.shape) == (B,) and t.is_contiguous()),
                 f"{name} must be a dense int32 [B] tensor on {dev}")
    dense = (Hkv * T * D, T * D, D)     # (a dimension of size 1 has no stride of its own)
    s3 = lambda t: (ctypes.c_longlong * 3)(*[t.stride(i) if t.shape[i] > 1 else dense[i] for i in (0, 1, 2)])
    with torch.cuda.device(dev):
        rc = L.qattn_kv_cache_append_fp8(k_new.data_ptr(), v_new.data_ptr(), fmt_of(k_new.dtype), s3(k_new), s3(v_new), k_frag.data_ptr(),
                                         v_frag.data_ptr(), scale_k.data_ptr(), scale_v.data_ptr(), seqlens.data_ptr(), _ptr(new_lens),
                                         int(bool(advance)), B, Hkv, T, capacity, D, fmt_of(fp8_dtype), _stream(k_new))
    _check(rc, "qattn_kv_cache_append_fp8")


def _paged_pool_checks(L, k_pool, v_pool, block_table, scale_k, scale_v, dev, B, Hkv, num_pages, page_size, D):
    """the pools, the table and the scales of a paged cache (include/qattn_paged.h); returns (max_pages, table_stride)"""
    _require(isinstance(page_size, int) and page_size >= 64 and page_size % 64 == 0, f"page_size must be a positive multiple of 64, got {page_size}")
    _require(isinstance(num_pages, int) and num_pages > 0, f"num_pages must be positive, got {num_pages}")
    for name, img, layout in (("k", k_pool, LAYOUT_KFRAG), ("v", v_pool, LAYOUT_VFRAG)):
        _require(img.device == dev and img.dtype == torch.uint8 and img.is_contiguous()
                 and img.numel() == L.qattn_fp8_tensor_bytes(layout, num_pages, Hkv, page_size, D),
                 f"the {name} pool does not fit [num_pages={num_pages}, Hkv={Hkv}, page_size={page_size}, D={D}]")
    _require(block_table.dtype == torch.int32 and block_table.device == dev and block_table.dim() == 2 and block_table.shape[0] == B
             and block_table.shape[1] > 0 and block_table.stride(1) == 1 and (B == 1 or block_table.stride(0) >= block_table.shape[1]),
             f"block_table must be an int32 [B={B}, max_pages] tensor on {dev} with dense rows")
    for name, sc in (("scale_k", scale_k), ("scale_v", scale_v)):
        _require(sc.dtype == torch.float32 and sc.device == dev and sc.is_contiguous() and tuple(sc.shape) == (B, Hkv), f"{name} must be a dense float32 [B, Hkv] tensor on {dev}")
    max_pages = block_table.shape[1]
    return max_pages, (block_table.stride(0) if B > 1 else max_pages)


def paged_kv_cache_append_fp8(k_pool: torch.Tensor, v_pool: torch.Tensor, scale_k: torch.Tensor, scale_v: torch.Tensor, block_table: torch.Tensor,
                              seqlens: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, *, num_pages: int, page_size: int,
                              fp8_dtype=torch.float8_e4m3fn, new_lens: Optional[torch.Tensor] = None, advance: bool = True) -> None:
    """qattn_paged_kv_cache_append_fp8 (include/qattn_paged.h): kv_cache_append_fp8 into the pools k_pool / v_pool (flat uint8: the KFRAG /
    VFRAG images of [num_pages, Hkv, page_size, D]) through block_table int32 [B, max_pages]; capacity = max_pages page_size.  The table,
    seqlens and new_lens are read on the device.  Mutates k_pool, v_pool and seqlens."""
    _require(k_new.is_cuda and k_new.dim() == 4 and k_new.dtype in (torch.bfloat16, torch.float16), "k_new must be a 4-D bf16 / fp16 device tensor")
    _require(v_new.shape == k_new.shape and v_new.dtype == k_new.dtype and v_new.device == k_new.device, "k_new and v_new must agree in shape, dtype and device")
    _require(kv_append_addressable(k_new) and kv_append_addressable(v_new), "k_new / v_new need head_dim innermost and 16-byte-aligned rows")
    B, Hkv, T, D = k_new.shape
    L = lib()
    dev = k_new.device
    max_pages, tstride = _paged_pool_checks(L, k_pool, v_pool, block_table, scale_k, scale_v, dev, B, Hkv, num_pages, page_size, D)
    for name, t in (("seqlens", seqlens), ("new_lens", new_lens)):
        _require(t is None and name == "new_lens" or (t is not None and t.dtype == torch.int32 and t.device == dev and tuple(t.shape) == (B,) and t.is_contiguous()),
                 f"{name} must be a dense int32 [B] tensor on {dev}")
    dense = (Hkv * T * D, T * D, D)     # (a dimension of size 1 has no stride of its own)
    s3 = lambda t: (ctypes.c_longlong * 3)(*[t.stride(i) if t.shape[i] > 1 else dense[i] for i in (0, 1, 2)])
    with torch.cuda.device(dev):
        rc = L.qattn_paged_kv_cache_append_fp8(k_new.data_ptr(), v_new.data_ptr(), fmt_of(k_new.dtype), s3(k_new), s3(v_new), k_pool.data_ptr(),
                                               v_pool.data_ptr(), scale_k.data_ptr(), scale_v.data_ptr(), block_table.data_ptr(), tstride,
                                               seqlens.data_ptr(), _ptr(new_lens), int(bool(advance)), B, Hkv, T, num_pages, page_size, max_pages,
                                               D, fmt_of(fp8_dtype), _stream(k_new))
    _check(rc, "qattn_paged_kv_cache_append_fp8")


def paged_kv_cache_append_varlen_fp8(k_pool: torch.Tensor, v_pool: torch.Tensor, scale_k: torch.Tensor, scale_v: torch.Tensor,
                                     block_table: torch.Tensor, seqlens: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor,
                                     cu_seqlens: torch.Tensor, *, num_pages: int, page_size: int, fp8_dtype=torch.float8_e4m3fn,
                                     advance: bool = True) -> None:
    """qattn_paged_kv_cache_append_varlen_fp8 (include/qattn_paged_varlen_append.h): paged_kv_cache_append_fp8 on PACKED tokens k_new / v_new
    [total, Hkv, D] (dense or views `paged_varlen_q_addressable` accepts, read in place), slot b owning the rows cu_seqlens[b] ..
    cu_seqlens[b + 1] (int32 [B + 1]).  The table, seqlens and cu_seqlens are read on the device.  Mutates k_pool, v_pool and seqlens."""
    _require(k_new.is_cuda and k_new.dim() == 3 and k_new.dtype in (torch.bfloat16, torch.float16), "k_new must be a 3-D bf16 / fp16 device tensor")
    _require(v_new.shape == k_new.shape and v_new.dtype == k_new.dtype and v_new.device == k_new.device, "k_new and v_new must agree in shape, dtype and device")
    total, Hkv, D = k_new.shape
    if total == 0:
        return
    _require(paged_varlen_q_addressable(k_new) and paged_varlen_q_addressable(v_new), "k_new / v_new need head_dim innermost and 16-byte-aligned rows")
    B = block_table.shape[0] if block_table.dim() == 2 else 0
    L = lib()
    dev = k_new.device
    max_pages, tstride = _paged_pool_checks(L, k_pool, v_pool, block_table, scale_k, scale_v, dev, B, Hkv, num_pages, page_size, D)
    _require(seqlens.dtype == torch.int32 and seqlens.device == dev and tuple(seqlens.shape) == (B,) and seqlens.is_contiguous(),
             f"seqlens must be a dense int32 [B] tensor on {dev}")
    _require(cu_seqlens.dtype == torch.int32 and cu_seqlens.device == dev and tuple(cu_seqlens.shape) == (B + 1,) and cu_seqlens.is_contiguous(),
             f"cu_seqlens must be a dense int32 [B + 1] tensor on {dev}")
    dense = (Hkv * D, D)     # (a dimension of size 1 has no stride of its own)
    s2 = lambda t: (ctypes.c_longlong * 2)(*[t.stride(i) if t.shape[i] > 1 else dense[i] for i in (0, 1)])
    with torch.cuda.device(dev):
        rc = L.qattn_paged_kv_cache_append_varlen_fp8(k_new.data_ptr(), v_new.data_ptr(), fmt_of(k_new.dtype), s2(k_new), s2(v_new),
                                                      k_pool.data_ptr(), v_pool.data_ptr(), scale_k.data_ptr(), scale_v.data_ptr(),
                                                      block_table.data_ptr(), tstride, seqlens.data_ptr(), cu_seqlens.data_ptr(),
                                                      int(bool(advance)), B, Hkv, total, num_pages, page_size, max_pages, D, fmt_of(fp8_dtype),
                                                      _stream(k_new))
    _check(rc, "qattn_paged_kv_cache_append_varlen_fp8")


def paged_kv_cache_compact_fp8(k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor, seqlens: torch.Tensor,
                               cu_seqlens: torch.Tensor, accept_index: torch.Tensor, accept_lens: torch.Tensor, *, Hkv: int, D: int,
                               num_pages: int, page_size: int) -> None:
    """qattn_paged_kv_cache_compact_fp8 (include/qattn_paged_varlen_tree.h): in every compactable slot the accepted draft keys
    accept_index[cu[b] + i], i < accept_lens[b], become the keys base + i, base = seqlens[b] - (cu[b + 1] - cu[b]), and seqlens[b] becomes
    base + accept_lens[b].  Everything is read on the device.  Mutates k_pool, v_pool and seqlens."""
    dev = k_pool.device
    _require(k_pool.is_cuda, "the pools must be device tensors")
    _require(isinstance(page_size, int) and page_size >= 64 and page_size % 64 == 0, f"page_size must be a positive multiple of 64, got {page_size}")
    _require(isinstance(num_pages, int) and num_pages > 0, f"num_pages must be positive, got {num_pages}")
    L = lib()
    for name, img, layout in (("k", k_pool, LAYOUT_KFRAG), ("v", v_pool, LAYOUT_VFRAG)):
        _require(img.device == dev and img.dtype == torch.uint8 and img.is_contiguous()
                 and img.numel() == L.qattn_fp8_tensor_bytes(layout, num_pages, Hkv, page_size, D),
                 f"the {name} pool does not fit [num_pages={num_pages}, Hkv={Hkv}, page_size={page_size}, D={D}]")
    _require(block_table.dtype == torch.int32 and block_table.device == dev and block_table.dim() == 2 and block_table.shape[1] > 0
             and block_table.stride(1) == 1 and (block_table.shape[0] == 1 or block_table.stride(0) >= block_table.shape[1]),
             f"block_table must be an int32 [B, max_pages] tensor on {dev} with dense rows")
    B, max_pages = block_table.shape
    tstride = block_table.stride(0) if B > 1 else max_pages
    total = accept_index.shape[0] if accept_index.dim() == 1 else -1
    for name, t, shape in (("seqlens", seqlens, (B,)), ("cu_seqlens", cu_seqlens, (B + 1,)), ("accept_lens", accept_lens, (B,)),
                           ("accept_index", accept_index, (total,))):
        _require(t.dtype == torch.int32 and t.device == dev and tuple(t.shape) == shape and t.is_contiguous(),
                 f"{name} must be a dense int32 {list(shape)} tensor on {dev}")
    if total == 0:
        return
    with torch.cuda.device(dev):
        rc = L.qattn_paged_kv_cache_compact_fp8(k_pool.data_ptr(), v_pool.data_ptr(), block_table.data_ptr(), tstride, seqlens.data_ptr(),
                                                cu_seqlens.data_ptr(), accept_index.data_ptr(), accept_lens.data_ptr(), B, Hkv, total,
                                                num_pages, page_size, max_pages, D, torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "qattn_paged_kv_cache_compact_fp8")


def _paged_rope_tables(cos: torch.Tensor, sin: torch.Tensor, dev, D: int):
    """cos / sin fp32 [T, D/2] as include/qattn_paged_varlen_rope.h takes them: (T, row stride in floats).  Read in place: no copy is made."""
    for name, t in (("cos", cos), ("sin", sin)):
        _require(t.dtype == torch.float32 and t.device == dev and t.dim() == 2 and t.shape[0] >= 1 and t.shape[1] == D // 2,
                 f"{name} must be a float32 [T, D/2 = {D // 2}] tensor on {dev}")
        _require(t.stride(1) == 1 and t.data_ptr() % 16 == 0 and (t.shape[0] == 1 or (t.stride(0) >= 0 and t.stride(0) % 4 == 0)),
                 f"{name} needs dense rows, a 16-byte-aligned base and a row stride that is a non-negative multiple of 4 floats")
    _require(cos.shape == sin.shape and (cos.shape[0] == 1 or cos.stride(0) == sin.stride(0)), "cos and sin must share shape and row stride")
    return cos.shape[0], (cos.stride(0) if cos.shape[0] > 1 else D // 2)


def paged_kv_cache_append_varlen_rope_fp8(k_pool: torch.Tensor, v_pool: torch.Tensor, scale_k: torch.Tensor, scale_v: torch.Tensor,
                                          block_table: torch.Tensor, seqlens: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor,
                                          cu_seqlens: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *, num_pages: int, page_size: int,
                                          fp8_dtype=torch.float8_e4m3fn, interleaved: bool = False, advance: bool = True) -> None:
    """qattn_paged_kv_cache_append_varlen_rope_fp8 (include/qattn_paged_varlen_rope.h): paged_kv_cache_append_varlen_fp8 with key p + t of a
    slot rotated with row min(p + t, T - 1) of cos / sin (fp32 [T, D/2], read in place) before it is quantised.  Any T >= 1 is taken: the
    capacity rule is the Python entry's.  Mutates k_pool, v_pool and seqlens."""
    _require(k_new.is_cuda and k_new.dim() == 3 and k_new.dtype in (torch.bfloat16, torch.float16), "k_new must be a 3-D bf16 / fp16 device tensor")
    _require(v_new.shape == k_new.shape and v_new.dtype == k_new.dtype and v_new.device == k_new.device, "k_new and v_new must agree in shape, dtype and device")
    total, Hkv, D = k_new.shape
    if total == 0:
        return
    _require(paged_varlen_q_addressable(k_new) and paged_varlen_q_addressable(v_new), "k_new / v_new need head_dim innermost and 16-byte-aligned rows")
    B = block_table.shape[0] if block_table.dim() == 2 else 0
    L = lib()
    dev = k_new.device
    max_pages, tstride = _paged_pool_checks(L, k_pool, v_pool, block_table, scale_k, scale_v, dev, B, Hkv, num_pages, page_size, D)
    _require(seqlens.dtype == torch.int32 and seqlens.device == dev and tuple(seqlens.shape) == (B,) and seqlens.is_contiguous(),
             f"seqlens must be a dense int32 [B] tensor on {dev}")
    _require(cu_seqlens.dtype == torch.int32 and cu_seqlens.device == dev and tuple(cu_seqlens.shape) == (B + 1,) and cu_seqlens.is_contiguous(),
             f"cu_seqlens must be a dense int32 [B + 1] tensor on {dev}")
    T, tr = _paged_rope_tables(cos, sin, dev, D)
    dense = (Hkv * D, D)     # (a dimension of size 1 has no stride of its own)
    s2 = lambda t: (ctypes.c_longlong * 2)(*[t.stride(i) if t.shape[i] > 1 else dense[i] for i in (0, 1)])
    with torch.cuda.device(dev):
        rc = L.qattn_paged_kv_cache_append_varlen_rope_fp8(k_new.data_ptr(), v_new.data_ptr(), fmt_of(k_new.dtype), s2(k_new), s2(v_new),
                                                           k_pool.data_ptr(), v_pool.data_ptr(), scale_k.data_ptr(), scale_v.data_ptr(),
                                                           block_table.data_ptr(), tstride, seqlens.data_ptr(), cu_seqlens.data_ptr(),
                                                           int(bool(advance)), B, Hkv, total, num_pages, page_size, max_pages, D,
                                                           fmt_of(fp8_dtype), cos.data_ptr(), sin.data_ptr(), tr, T, int(bool(interleaved)),
                                                           _stream(k_new))
    _check(rc, "qattn_paged_kv_cache_append_varlen_rope_fp8")


def rope_paged_varlen(x: torch.Tensor, seqlens: torch.Tensor, cu_seqlens: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *, capacity: int,
                      interleaved: bool = False, appended: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qattn_rope_paged_varlen (include/qattn_paged_varlen_rope.h): packed rows x [total, H, D] (dense or a view `paged_varlen_q_addressable`
    accepts, read in place) rotated at the positions of a paged cache's slots -> dense [total, H, D] (`out`, or a new tensor).  seqlens
    int32 [B], cu_seqlens int32 [B + 1] and the tables are read on the device."""
    _require(x.is_cuda and x.dim() == 3 and x.dtype in (torch.bfloat16, torch.float16), "x must be a 3-D bf16 / fp16 device tensor")
    total, H, D = x.shape
    dev = x.device
    if out is None:
        with torch.cuda.device(dev):
            out = torch.empty((total, H, D), dtype=x.dtype, device=dev)
    _require(out.shape == x.shape and out.dtype == x.dtype and out.device == dev and out.is_contiguous() and out.data_ptr() % 16 == 0,
             "out must be a dense, 16-byte-aligned tensor of x's shape, dtype and device")
    if total == 0:
        return out
    _require(H > 0 and paged_varlen_q_addressable(x), "x needs head_dim innermost and 16-byte-aligned rows")
    B = seqlens.shape[0] if seqlens.dim() == 1 else 0
    _require(B > 0 and seqlens.dtype == torch.int32 and seqlens.device == dev and seqlens.is_contiguous(), f"seqlens must be a dense int32 [B] tensor on {dev}")
    _require(cu_seqlens.dtype == torch.int32 and cu_seqlens.device == dev and tuple(cu_seqlens.shape) == (B + 1,) and cu_seqlens.is_contiguous(),
             f"cu_seqlens must be a dense int32 [B + 1] tensor on {dev}")
    _require(isinstance(capacity, int) and capacity >= 1, f"capacity must be a positive integer, got {capacity!r}")
    T, tr = _paged_rope_tables(cos, sin, dev, D)
    dense = (H * D, D)     # (a dimension of size 1 has no stride of its own)
    s2 = (ctypes.c_longlong * 2)(*[x.stride(i) if x.shape[i] > 1 else dense[i] for i in (0, 1)])
    with torch.cuda.device(dev):
        rc = lib().qattn_rope_paged_varlen(x.data_ptr(), fmt_of(x.dtype), s2, out.data_ptr(), cu_seqlens.data_ptr(), seqlens.data_ptr(),
                                           int(bool(appended)), B, H, total, capacity, D, cos.data_ptr(), sin.data_ptr(), tr, T,
                                           int(bool(interleaved)), _stream(x))
    _check(rc, "qattn_rope_paged_varlen")
    return out


def _positions_check(positions: torch.Tensor, total: int, dev) -> None:
    _require(positions.dtype == torch.int64 and positions.device == dev and tuple(positions.shape) == (total,) and positions.is_contiguous(),
             f"positions must be a dense int64 [total={total}] tensor on {dev}")


def paged_kv_cache_append_varlen_rope_pos_fp8(k_pool: torch.Tensor, v_pool: torch.Tensor, scale_k: torch.Tensor, scale_v: torch.Tensor,
                                              block_table: torch.Tensor, seqlens: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor,
                                              cu_seqlens: torch.Tensor, positions: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *,
                                              num_pages: int, page_size: int, fp8_dtype=torch.float8_e4m3fn, interleaved: bool = False,
                                              advance: bool = True) -> None:
    """qattn_paged_kv_cache_append_varlen_rope_pos_fp8 (include/qattn_paged_varlen_rope_pos.h): paged_kv_cache_append_varlen_rope_fp8 with
    token t rotated with row clamp(positions[t], 0, T - 1) of cos / sin; positions int64 [total] on the device.  Where a key is stored
    does not change.  Mutates k_pool, v_pool and seqlens."""
    _require(k_new.is_cuda and k_new.dim() == 3 and k_new.dtype in (torch.bfloat16, torch.float16), "k_new must be a 3-D bf16 / fp16 device tensor")
    _require(v_new.shape == k_new.shape and v_new.dtype == k_new.dtype and v_new.device == k_new.device, "k_new and v_new must agree in shape, dtype and device")
    total, Hkv, D = k_new.shape
    if total == 0:
        return
    _require(paged_varlen_q_addressable(k_new) and paged_varlen_q_addressable(v_new), "k_new / v_new need head_dim innermost and 16-byte-aligned rows")
    B = block_table.shape[0] if block_table.dim() == 2 else 0
    L = lib()
    dev = k_new.device
    max_pages, tstride = _paged_pool_checks(L, k_pool, v_pool, block_table, scale_k, scale_v, dev, B, Hkv, num_pages, page_size, D)
    _require(seqlens.dtype == torch.int32 and seqlens.device == dev and tuple(seqlens.shape) == (B,) and seqlens.is_contiguous(),
             f"seqlens must be a dense int32 [B] tensor on {dev}")
    _require(cu_seqlens.dtype == torch.int32 and cu_seqlens.device == dev and tuple(cu_seqlens.shape) == (B + 1,) and cu_seqlens.is_contiguous(),
             f"cu_seqlens must be a dense int32 [B + 1] tensor on {dev}")
    _positions_check(positions, total, dev)
    T, tr = _paged_rope_tables(cos, sin, dev, D)
    dense = (Hkv * D, D)     # (a dimension of size 1 has no stride of its own)
    s2 = lambda t: (ctypes.c_longlong * 2)(*[t.stride(i) if t.shape[i] > 1 else dense[i] for i in (0, 1)])
    with torch.cuda.device(dev):
        rc = L.qattn_paged_kv_cache_append_varlen_rope_pos_fp8(k_new.data_ptr(), v_new.data_ptr(), fmt_of(k_new.dtype), s2(k_new), s2(v_new),
                                                               k_pool.data_ptr(), v_pool.data_ptr(), scale_k.data_ptr(), scale_v.data_ptr(),
                                                               block_table.data_ptr(), tstride, seqlens.data_ptr(), cu_seqlens.data_ptr(),
                                                               int(bool(advance)), B, Hkv, total, num_pages, page_size, max_pages, D,
                                                               fmt_of(fp8_dtype), cos.data_ptr(), sin.data_ptr(), tr, T,
                                                               int(bool(interleaved)), positions.data_ptr(), _stream(k_new))
    _check(rc, "qattn_paged_kv_cache_append_varlen_rope_pos_fp8")


def rope_packed_positions(x: torch.Tensor, positions: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *, interleaved: bool = False,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qattn_rope_packed_positions (include/qattn_paged_varlen_rope_pos.h): packed rows x [total, H, D] (dense or a view
    `paged_varlen_q_addressable` accepts, read in place), row t rotated with row clamp(positions[t], 0, T - 1) of cos / sin -> dense
    [total, H, D] (`out`, or a new tensor).  positions int64 [total] and the tables are read on the device."""
    _require(x.is_cuda and x.dim() == 3 and x.dtype in (torch.bfloat16, torch.float16), "x must be a 3-D bf16 / fp16 device tensor")
    total, H, D = x.shape
    dev = x.device
    if out is None:
        with torch.cuda.device(dev):
            out = torch.empty((total, H, D), dtype=x.dtype, device=dev)
    _require(out.shape == x.shape and out.dtype == x.dtype and out.device == dev and out.is_contiguous() and out.data_ptr() % 16 == 0,
             "out must be a dense, 16-byte-aligned tensor of x's shape, dtype and device")
    _positions_check(positions, total, dev)
    if total == 0:
        return out
    _require(H > 0 and paged_varlen_q_addressable(x), "x needs head_dim innermost and 16-byte-aligned rows")
    T, tr = _paged_rope_tables(cos, sin, dev, D)
    dense = (H * D, D)     # (a dimension of size 1 has no stride of its own)
    s2 = (ctypes.c_longlong * 2)(*[x.stride(i) if x.shape[i] > 1 else dense[i] for i in (0, 1)])
    with torch.cuda.device(dev):
        rc = lib().qattn_rope_packed_positions(x.data_ptr(), fmt_of(x.dtype), s2, out.data_ptr(), positions.data_ptr(), H, total, D,
                                               cos.data_ptr(), sin.data_ptr(), tr, T, int(bool(interleaved)), _stream(x))
    _check(rc, "qattn_rope_packed_positions")
    return out


def fp8_attention_paged_splitkv(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, scale_k: torch.Tensor, scale_v: torch.Tensor,
                                block_table: torch.Tensor, seqused_k: torch.Tensor, *, Skv: int, num_pages: int, page_size: int,
                                fp8_dtype=torch.float8_e4m3fn, numerics: str = "compiled", is_causal: bool = False, sm_scale: float = 0.0,
                                precision: str = "accurate", num_splits: int = 0, return_lse: bool = False, return_partials: bool = False,
                                return_quant: bool = False, return_path: bool = False, window: Optional[Tuple[int, int]] = None,
                                sinks: Optional[torch.Tensor] = None, softcap: Optional[float] = None):
    """Split-KV attention over a paged cache (qattn_fp8_attention_paged_splitkv_forward, include/qattn_paged.h): fp8_attention_splitkv with
    the pools (flat uint8: the KFRAG / VFRAG images of [num_pages, Hkv, page_size, D]) and block_table int32 [B, max_pages] in place of the
    contiguous images; Skv <= max_pages page_size is the logical bound, seqused_k int32 [B] is required.  Returns what
    fp8_attention_splitkv returns."""
    _require(precision in ("fast", "accurate"), f"Unsupported precision for the split-KV entry: {precision!r} (expected 'fast' or 'accurate')")
    _require(q.is_cuda and q.dim() == 4 and q.dtype in (torch.bfloat16, torch.float16), "query must be a 4-D bf16 / fp16 device tensor")
    _require(0 <= int(num_splits) <= SPLITKV_MAX_SPLITS, f"num_splits must be 0 (auto) or 1 .. {SPLITKV_MAX_SPLITS}, got {num_splits}")
    mask_args = (int(bool(is_causal)),) if window is None else _window_args(window)
    q = q.contiguous()
    B, Hq, Sq, D = q.shape
    mask_args += _sink_args(sinks, window, Hq, q.device) + _softcap_args(softcap, window, sinks)
    _require(scale_k.dim() == 2 and scale_k.shape[0] == B, "scale_k / scale_v must be fp32 [B, Hkv]")
    Hkv = scale_k.shape[1]
    _require(Hkv > 0 and Hq % Hkv == 0, f"Hq={Hq} is not a multiple of Hkv={Hkv}")
    L = lib()
    dev = q.device
    max_pages, tstride = _paged_pool_checks(L, k_pool, v_pool, block_table, scale_k, scale_v, dev, B, Hkv, num_pages, page_size, D)
    _require(isinstance(Skv, int) and 0 < Skv <= max_pages * page_size, f"Skv must be in 1 .. max_pages * page_size = {max_pages * page_size}, got {Skv}")
    _require(seqused_k is not None and seqused_k.dtype == torch.int32 and seqused_k.device == dev and tuple(seqused_k.shape) == (B,)
             and seqused_k.is_contiguous(), f"seqused_k must be a dense int32 [B] tensor on {dev}")
    ns = int(num_splits)
    if ns == 0:
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        ns = splitkv_auto_splits(B, Hq, Hkv, Sq, Skv, D, cus) if window is None else splitkv_window_auto_splits(B, Hq, Hkv, Sq, Skv, D, window[0], cus)
    with torch.cuda.device(dev):
        out = torch.empty((B, Hq, Sq, D), dtype=q.dtype, device=dev)
        lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=dev) if return_lse else None
        po = plse = ppath = q8 = sq = path = None
        if return_partials:
            n = ns if ns > 1 else 0
            po = torch.empty((n, B, Hq, Sq, D), dtype=torch.float32, device=dev)
            plse = torch.empty((n, B, Hq, Sq), dtype=torch.float32, device=dev)
            ppath = torch.empty((n, B, Hq, Sq), dtype=torch.uint8, device=dev)
        if return_quant:
            q8 = torch.empty((B, Hq, Sq, D), dtype=fp8_dtype, device=dev)
            sq = torch.empty((B, Hq), dtype=torch.float32, device=dev)
        if return_path:
            path = torch.empty((B, Hq, Sq), dtype=torch.uint8, device=dev)
        ws_bytes = L.qattn_fp8_attention_paged_splitkv_workspace_bytes(B, Hq, Hkv, Sq, Skv, D, ns)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
        live = lambda t: _ptr(t) if t is not None and t.numel() else None
        fwd = (L.qattn_fp8_attention_paged_splitkv_softcap_forward if softcap is not None
               else L.qattn_fp8_attention_paged_splitkv_forward if window is None else L.qattn_fp8_attention_paged_splitkv_window_forward
               if sinks is None else L.qattn_fp8_attention_paged_splitkv_sink_forward)
        rc = fwd(
            q.data_ptr(), fmt_of(q.dtype), k_pool.data_ptr(), v_pool.data_ptr(), block_table.data_ptr(), tstride, num_pages, page_size, max_pages,
            scale_k.data_ptr(), scale_v.data_ptr(), out.data_ptr(), _ptr(lse), seqused_k.data_ptr(), B, Hq, Hkv, Sq, Skv, D, fmt_of(fp8_dtype),
            _numerics(numerics), *mask_args, float(sm_scale), _precision(precision), ns, _ptr(q8), _ptr(sq), _ptr(path), live(po),
            live(plse), live(ppath), ws.data_ptr(), ws_bytes, _stream(q))
    _check(rc, "qattn_fp8_attention_paged_splitkv_softcap_forward" if softcap is not None
           else "qattn_fp8_attention_paged_splitkv_forward" if window is None else "qattn_fp8_attention_paged_splitkv_window_forward"
           if sinks is None else "qattn_fp8_attention_paged_splitkv_sink_forward")
    if not (return_lse or return_partials or return_quant or return_path):
        return out
    return ((out,) + ((lse,) if return_lse else ()) + ((po, plse, ppath) if return_partials else ()) + ((q8, sq) if return_quant else ())
            + ((path,) if return_path else ()))


def paged_varlen_auto_splits(B: int, Hq: int, Hkv: int, total_q: int, max_seqlen_q: int, Skv: int, D: int, num_cus: int) -> int:
    """qattn_paged_varlen_auto_splits (include/qattn_paged_varlen.h): the num_splits = 0 rule of the packed paged entry, a pure host function."""
    return int(lib().qattn_paged_varlen_auto_splits(B, Hq, Hkv, total_q, max_seqlen_q, Skv, D, num_cus))


def paged_varlen_q_addressable(q: torch.Tensor) -> bool:
    """A 3-D view [total_q, Hq, D] qattn_fp8_attention_paged_varlen_forward reads in place: head_dim innermost and dense, token and head
    strides of a dimension longer than 1 non-negative multiples of 8 elements, base 16-byte aligned (rows 16-byte aligned)."""
    return (q.dim() == 3 and (q.shape[2] == 1 or q.stride(2) == 1) and q.data_ptr() % 16 == 0
            and all(q.shape[i] == 1 or (q.stride(i) >= 0 and q.stride(i) % 8 == 0) for i in (0, 1)))


def fp8_attention_paged_varlen(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, scale_k: torch.Tensor, scale_v: torch.Tensor,
                               block_table: torch.Tensor, seqused_k: torch.Tensor, cu_seqlens_q: torch.Tensor, *, max_seqlen_q: int, Skv: int,
                               num_pages: int, page_size: int, fp8_dtype=torch.float8_e4m3fn, numerics: str = "compiled",
                               is_causal: bool = False, sm_scale: float = 0.0, precision: str = "accurate", num_splits: int = 0,
                               return_lse: bool = False, return_partials: bool = False, return_quant: bool = False, return_path: bool = False,
                               window: Optional[Tuple[int, int]] = None, sinks: Optional[torch.Tensor] = None,
                               tree_mask: Optional[torch.Tensor] = None, softcap: Optional[float] = None):
    """Split-KV attention of PACKED queries over a paged cache (qattn_fp8_attention_paged_varlen_forward, include/qattn_paged_varlen.h).
    q [total_q, Hq, D] bf16 / fp16, dense or a view `paged_varlen_q_addressable` accepts (read in place); cu_seqlens_q int32 [B + 1] and
    seqused_k int32 [B] on the device; the pools, the table and the scales as fp8_attention_paged_splitkv.  num_splits 0: the auto rule on
    the device's CU count (resolved here, on the host).  Returns out [total_q, Hq, D], or a tuple of out, [lse [Hq, total_q]], [partial_o
    fp32 [ns, total_q, Hq, D], partial_lse [ns, Hq, total_q], partial_path uint8 -- three empty tensors when the call ran one split],
    [q8 [Hq total_q D] flat, scale_q [B, Hq]], [row_path uint8 [Hq, total_q]].
    tree_mask (int64 [total_q] on the device): qattn_fp8_attention_paged_varlen_tree_forward (include/qattn_paged_varlen_tree.h) -- the
    causal call under a draft tree per slot; is_causal is not read.  With window (and, optionally, sinks):
    qattn_fp8_attention_paged_varlen_tree_window_forward (include/qattn_paged_varlen_tree_window.h)."""
    _require(precision in ("fast", "accurate"), f"Unsupported precision for the split-KV entry: {precision!r} (expected 'fast' or 'accurate')")
    _require(q.is_cuda and q.dim() == 3 and q.dtype in (torch.bfloat16, torch.float16), "query must be a 3-D bf16 / fp16 device tensor [total_q, Hq, D]")
    _require(0 <= int(num_splits) <= SPLITKV_MAX_SPLITS, f"num_splits must be 0 (auto) or 1 .. {SPLITKV_MAX_SPLITS}, got {num_splits}")
    mask_args = (int(bool(is_causal)),) if window is None else _window_args(window)
    total_q, Hq, D = q.shape
    mask_args += _sink_args(sinks, window, Hq, q.device) + _softcap_args(softcap, window, sinks, tree_mask)
    tree_window = tree_mask is not None and window is not None
    if tree_mask is not None:
        _require(tree_mask.dtype == torch.int64 and tree_mask.device == q.device and tuple(tree_mask.shape) == (total_q,)
                 and tree_mask.is_contiguous(), f"tree_mask must be a dense int64 [total_q={total_q}] tensor on {q.device}")
        # without a window: the tree entry.  With one: the tree-window entry, its sinks pointer NULL without sinks
        mask_args = (tree_mask.data_ptr(),) + ((mask_args + (None,))[:3] if tree_window else ())
    if total_q and not paged_varlen_q_addressable(q):
        q = q.contiguous()
    _require(scale_k.dim() == 2, "scale_k / scale_v must be fp32 [B, Hkv]")
    B, Hkv = scale_k.shape
    _require(Hkv > 0 and Hq % Hkv == 0, f"Hq={Hq} is not a multiple of Hkv={Hkv}")
    L = lib()
    dev = q.device
    max_pages, tstride = _paged_pool_checks(L, k_pool, v_pool, block_table, scale_k, scale_v, dev, B, Hkv, num_pages, page_size, D)
    _require(isinstance(Skv, int) and 0 < Skv <= max_pages * page_size, f"Skv must be in 1 .. max_pages * page_size = {max_pages * page_size}, got {Skv}")
    _require(isinstance(max_seqlen_q, int) and max_seqlen_q >= 1, f"max_seqlen_q must be an integer >= 1, got {max_seqlen_q}")
    _require(seqused_k is not None and seqused_k.dtype == torch.int32 and seqused_k.device == dev and tuple(seqused_k.shape) == (B,)
             and seqused_k.is_contiguous(), f"seqused_k must be a dense int32 [B] tensor on {dev}")
    _require(cu_seqlens_q.dtype == torch.int32 and cu_seqlens_q.device == dev and tuple(cu_seqlens_q.shape) == (B + 1,)
             and cu_seqlens_q.is_contiguous(), f"cu_seqlens_q must be a dense int32 [B + 1] tensor on {dev}")
    ns = int(num_splits)
    if ns == 0:
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        ns = (paged_varlen_auto_splits(B, Hq, Hkv, total_q, max_seqlen_q, Skv, D, cus) if window is None
              else paged_varlen_window_auto_splits(B, Hq, Hkv, total_q, max_seqlen_q, Skv, D, window[0], cus))
    with torch.cuda.device(dev):
        out = torch.empty((total_q, Hq, D), dtype=q.dtype, device=dev)
        lse = torch.empty((Hq, total_q), dtype=torch.float32, device=dev) if return_lse else None
        po = plse = ppath = q8 = sq = path = None
        if return_partials:
            n = ns if ns > 1 else 0
            po = torch.empty((n, total_q, Hq, D), dtype=torch.float32, device=dev)
            plse = torch.empty((n, Hq, total_q), dtype=torch.float32, device=dev)
            ppath = torch.empty((n, Hq, total_q), dtype=torch.uint8, device=dev)
        if return_quant:
            q8 = torch.empty((Hq * total_q * D,), dtype=fp8_dtype, device=dev)
            sq = torch.empty((B, Hq), dtype=torch.float32, device=dev)
        if return_path:
            path = torch.empty((Hq, total_q), dtype=torch.uint8, device=dev)
        rc = 0
        if total_q:
            ws_bytes = L.qattn_fp8_attention_paged_varlen_workspace_bytes(B, Hq, Hkv, total_q, Skv, D, ns)
            ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
            live = lambda t: _ptr(t) if t is not None and t.numel() else None
            dense = (Hq * D, D)     # (a dimension of size 1 has no stride of its own)
            s2 = (ctypes.c_longlong * 2)(*[q.stride(i) if q.shape[i] > 1 else dense[i] for i in (0, 1)])
            fwd = (L.qattn_fp8_attention_paged_varlen_softcap_forward if softcap is not None
                   else L.qattn_fp8_attention_paged_varlen_tree_window_forward if tree_window
                   else L.qattn_fp8_attention_paged_varlen_tree_forward if tree_mask is not None
                   else L.qattn_fp8_attention_paged_varlen_forward if window is None else L.qattn_fp8_attention_paged_varlen_window_forward
                   if sinks is None else L.qattn_fp8_attention_paged_varlen_sink_forward)
            rc = fwd(
                q.data_ptr(), s2, fmt_of(q.dtype), k_pool.data_ptr(), v_pool.data_ptr(), block_table.data_ptr(), tstride, num_pages, page_size,
                max_pages, scale_k.data_ptr(), scale_v.data_ptr(), out.data_ptr(), _ptr(lse), cu_seqlens_q.data_ptr(), seqused_k.data_ptr(), B, Hq,
                Hkv, total_q, max_seqlen_q, Skv, D, fmt_of(fp8_dtype), _numerics(numerics), *mask_args, float(sm_scale),
                _precision(precision), ns, live(q8), _ptr(sq), live(path), live(po), live(plse), live(ppath), ws.data_ptr(), ws_bytes, _stream(q))
    _check(rc, "qattn_fp8_attention_paged_varlen_softcap_forward" if softcap is not None
           else "qattn_fp8_attention_paged_varlen_tree_window_forward" if tree_window
           else "qattn_fp8_attention_paged_varlen_tree_forward" if tree_mask is not None
           else "qattn_fp8_attention_paged_varlen_forward" if window is None else "qattn_fp8_attention_paged_varlen_window_forward"
           if sinks is None else "qattn_fp8_attention_paged_varlen_sink_forward")
    if not (return_lse or return_partials or return_quant or return_path):
        return out
    return ((out,) + ((lse,) if return_lse else ()) + ((po, plse, ppath) if return_partials else ()) + ((q8, sq) if return_quant else ())
            + ((path,) if return_path else ()))

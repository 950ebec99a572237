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
    "qattn_mla_pool_bytes", "qattn_mla_auto_splits", "qattn_fp8_mla_paged_workspace_bytes", "qattn_paged_mla_cache_append_fp8",
    "qattn_fp8_mla_paged_forward",
    "qattn_mla_row_pool_bytes", "qattn_mla_sparse_auto_splits", "qattn_fp8_mla_paged_sparse_workspace_bytes",
    "qattn_paged_mla_row_cache_append_fp8", "qattn_fp8_mla_paged_sparse_forward",
    "qattn_mla_index_pool_bytes", "qattn_fp8_mla_index_workspace_bytes", "qattn_paged_mla_index_cache_append_fp8",
    "qattn_fp8_mla_index_scores", "qattn_mla_index_select", "qattn_fp8_mla_index_topk",
    "qattn_mla_index_select_split_workspace_bytes", "qattn_mla_index_select_auto_splits", "qattn_mla_index_select_split",
    "qattn_fp8_mla_index_topk_split_workspace_bytes", "qattn_fp8_mla_index_topk_split",
    "qattn_fp8_mla_prefill_varlen_workspace_bytes", "qattn_fp8_mla_prefill_varlen_forward",
    "qattn_fp8_mla_index_varlen_workspace_bytes", "qattn_fp8_mla_index_scores_varlen", "qattn_fp8_mla_index_topk_varlen",
    "qattn_fp8_mla_paged_sparse_varlen_forward",
    "qattn_mla_varlen_auto_splits", "qattn_fp8_mla_paged_varlen_workspace_bytes", "qattn_fp8_mla_paged_varlen_forward",
)
FMT_FP32 = 4               # QATTN_FMT_FP32 (include/qattn_merge.h): a partial / the output of the state merge, no other entry takes it
MERGE_MAX_PARTIALS = 8     # QATTN_MERGE_MAX_PARTIALS
_MERGE_FMT = {torch.bfloat16: FMT_BF16, torch.float16: FMT_FP16, torch.float32: FMT_FP32}
BLOCK_SPARSE_BLOCK = 128   # QATTN_BLOCK_SPARSE_BLOCK (include/qattn_block_sparse.h): rows / keys per mask block
SPLITKV_MAX_SPLITS = 64    # QATTN_SPLITKV_MAX_SPLITS (include/qattn_splitkv.h)
MLA_D, MLA_D_LATENT, MLA_D_ROPE, MLA_MAX_SPLITS = 576, 512, 64, 64   # QATTN_MLA_* (include/qattn_mla.h)
MLA_SPARSE_SPLIT_ENTRIES = 2048                                      # QATTN_MLA_SPARSE_SPLIT_ENTRIES (include/qattn_mla_sparse.h)
MLA_SPARSE_MAX_TOPK = MLA_SPARSE_SPLIT_ENTRIES * MLA_MAX_SPLITS      # QATTN_MLA_SPARSE_MAX_TOPK
MLA_SPARSE_PREFILL_ROWS = 128                                        # QATTN_MLA_SPARSE_PREFILL_ROWS (include/qattn_mla_sparse_prefill.h)
MLA_VARLEN_ROWS = 128                                                # QATTN_MLA_VARLEN_ROWS (include/qattn_mla_varlen.h)
MLA_INDEX_D, MLA_INDEX_MAX_HEADS = 128, 64                         # QATTN_MLA_INDEX_* (include/qattn_mla_index.h)
MLA_INDEX_WG_KEYS, MLA_INDEX_LDS_CANDIDATES = 512, 8192
MLA_INDEX_MAX_SELECT_SPLITS = 256                                    # QATTN_MLA_INDEX_MAX_SELECT_SPLITS (include/qattn_mla_index_split.h)
MLA_INDEX_AUTO_MIN_SEG, MLA_INDEX_AUTO_MIN_KEYS = 2048, 16384         # QATTN_MLA_INDEX_AUTO_MIN_SEG, QATTN_MLA_INDEX_AUTO_MIN_KEYS
MLA_INDEX_AUTO_MIN_SPLITS = 8                                         # QATTN_MLA_INDEX_AUTO_MIN_SPLITS
MLA_INDEX_PREFILL_TOKENS, MLA_INDEX_PREFILL_KEYS, MLA_INDEX_PREFILL_WG_KEYS = 8, 128, 2048   # QATTN_MLA_INDEX_PREFILL_* (include/qattn_mla_index_prefill.h)
MLA_PREFILL_D_QK, MLA_PREFILL_D_NOPE, MLA_PREFILL_D_ROPE, MLA_PREFILL_D_V = 192, 128, 64, 128   # QATTN_MLA_PREFILL_* (include/qattn_mla_prefill.h)


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
    # multi-head latent attention (include/qattn_mla.h)
    L.qattn_mla_pool_bytes.restype = sz
    L.qattn_mla_pool_bytes.argtypes = [i, i]
    L.qattn_mla_auto_splits.restype = i
    L.qattn_mla_auto_splits.argtypes = [i, i, i, i, i]
    L.qattn_fp8_mla_paged_workspace_bytes.restype = sz
    L.qattn_fp8_mla_paged_workspace_bytes.argtypes = [i, i, i, i]
    L.qattn_paged_mla_cache_append_fp8.restype = i
    L.qattn_paged_mla_cache_append_fp8.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, ll, vp, vp, i, i, i, i, i, i, i, vp]
    L.qattn_fp8_mla_paged_forward.restype = i
    L.qattn_fp8_mla_paged_forward.argtypes = [vp, i, vp, vp, vp, ll, i, i, i, vp, vp, vp, vp, i, i, i, i, i, i, f, i, vp, vp, vp, vp, vp, sz, vp]
    # sparse multi-head latent attention on the row-major latent cache (include/qattn_mla_sparse.h)
    L.qattn_mla_row_pool_bytes.restype = sz
    L.qattn_mla_row_pool_bytes.argtypes = [i, i]
    L.qattn_mla_sparse_auto_splits.restype = i
    L.qattn_mla_sparse_auto_splits.argtypes = [i, i, i, i, i]
    L.qattn_fp8_mla_paged_sparse_workspace_bytes.restype = sz
    L.qattn_fp8_mla_paged_sparse_workspace_bytes.argtypes = [i, i, i, i]
    L.qattn_paged_mla_row_cache_append_fp8.restype = i
    L.qattn_paged_mla_row_cache_append_fp8.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, ll, vp, vp, i, i, i, i, i, i, i, vp]
    L.qattn_fp8_mla_paged_sparse_forward.restype = i
    L.qattn_fp8_mla_paged_sparse_forward.argtypes = [vp, i, vp, vp, vp, ll, i, i, i, vp, vp, vp, i, vp, vp, vp, i, i, i, i, i, f, i, vp, vp, vp, vp,
                                                     vp, sz, vp]
    # ... for packed variable-length queries (include/qattn_mla_sparse_prefill.h)
    L.qattn_fp8_mla_paged_sparse_varlen_forward.restype = i
    L.qattn_fp8_mla_paged_sparse_varlen_forward.argtypes = [vp, i, vp, vp, vp, ll, i, i, i, vp, vp, ll, i, vp, vp, vp, vp, i, i, i, i, i, f, vp, vp, vp]
    # dense multi-head latent attention for packed variable-length queries (include/qattn_mla_varlen.h)
    L.qattn_mla_varlen_auto_splits.restype = i
    L.qattn_mla_varlen_auto_splits.argtypes = [i, i, i]
    L.qattn_fp8_mla_paged_varlen_workspace_bytes.restype = sz
    L.qattn_fp8_mla_paged_varlen_workspace_bytes.argtypes = [i, i, i]
    L.qattn_fp8_mla_paged_varlen_forward.restype = i
    L.qattn_fp8_mla_paged_varlen_forward.argtypes = [vp, i, vp, vp, vp, ll, i, i, i, vp, vp, i, vp, vp, vp, i, i, i, i, i, i, f, i, vp, vp, vp, vp,
                                                     vp, sz, vp]
    # the lightning indexer of sparse multi-head latent attention (include/qattn_mla_index.h)
    L.qattn_mla_index_pool_bytes.restype = sz
    L.qattn_mla_index_pool_bytes.argtypes = [i, i]
    L.qattn_fp8_mla_index_workspace_bytes.restype = sz
    L.qattn_fp8_mla_index_workspace_bytes.argtypes = [i, i, i]
    L.qattn_paged_mla_index_cache_append_fp8.restype = i
    L.qattn_paged_mla_index_cache_append_fp8.argtypes = [vp, i, vp, vp, vp, vp, ll, vp, vp, i, i, i, i, i, i, i, vp]
    L.qattn_fp8_mla_index_scores.restype = i
    L.qattn_fp8_mla_index_scores.argtypes = [vp, i, vp, vp, vp, vp, vp, ll, i, i, i, vp, vp, i, i, i, i, i, i, vp, vp, i, vp, vp, vp]
    L.qattn_mla_index_select.restype = i
    L.qattn_mla_index_select.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp]
    L.qattn_fp8_mla_index_topk.restype = i
    L.qattn_fp8_mla_index_topk.argtypes = [vp, i, vp, vp, vp, vp, vp, ll, i, i, i, vp, vp, i, i, i, i, i, i, i, vp, vp, vp, vp, vp, sz, vp]
    # ... its packed variable-length (prefill) form (include/qattn_mla_index_prefill.h)
    L.qattn_fp8_mla_index_varlen_workspace_bytes.restype = sz
    L.qattn_fp8_mla_index_varlen_workspace_bytes.argtypes = [i, i]
    L.qattn_fp8_mla_index_scores_varlen.restype = i
    L.qattn_fp8_mla_index_scores_varlen.argtypes = [vp, i, vp, vp, ll, vp, vp, ll, i, i, i, vp, vp, vp, i, i, i, i, i, i, vp, ll, i, vp, vp, vp, vp]
    L.qattn_fp8_mla_index_topk_varlen.restype = i
    L.qattn_fp8_mla_index_topk_varlen.argtypes = [vp, i, vp, vp, ll, vp, vp, ll, i, i, i, vp, vp, vp, i, i, i, i, i, i, i, vp, vp, vp, vp, vp, sz, vp]
    # ... and its selection with one row cut across workgroups (include/qattn_mla_index_split.h)
    L.qattn_mla_index_select_split_workspace_bytes.restype = sz
    L.qattn_mla_index_select_split_workspace_bytes.argtypes = [i, i, i, i]
    L.qattn_mla_index_select_auto_splits.restype = i
    L.qattn_mla_index_select_auto_splits.argtypes = [i, i, i, i]
    L.qattn_mla_index_select_split.restype = i
    L.qattn_mla_index_select_split.argtypes = [vp, vp, vp, i, i, i, i, i, i, vp, vp, sz, vp]
    L.qattn_fp8_mla_index_topk_split_workspace_bytes.restype = sz
    L.qattn_fp8_mla_index_topk_split_workspace_bytes.argtypes = [i, i, i, i, i]
    L.qattn_fp8_mla_index_topk_split.restype = i
    L.qattn_fp8_mla_index_topk_split.argtypes = [vp, i, vp, vp, vp, vp, vp, ll, i, i, i, vp, vp, i, i, i, i, i, i, i, i, vp, vp, vp, vp, vp, sz, vp]
    # the non-absorbed prefill form of multi-head latent attention on packed sequences (include/qattn_mla_prefill.h)
    L.qattn_fp8_mla_prefill_varlen_workspace_bytes.restype = sz
    L.qattn_fp8_mla_prefill_varlen_workspace_bytes.argtypes = [i, i, i, i]
    L.qattn_fp8_mla_prefill_varlen_forward.restype = i
    L.qattn_fp8_mla_prefill_varlen_forward.argtypes = [vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, f, vp, vp, vp, vp, vp, sz, vp]
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


def mla_auto_splits(B: int, Hq: int, Sq: int, Skv: int, num_cus: int) -> int:
    """qattn_mla_auto_splits (include/qattn_mla.h): a pure function of the shape and the CU count (no device needed)."""
    return lib().qattn_mla_auto_splits(B, Hq, Sq, Skv, num_cus)


def _mla_pool_checks(L, pool, block_table, scale, dev, B, num_pages, page_size):
    """the pool, the table and the scales of a paged latent cache (include/qattn_mla.h); returns (max_pages, table_stride)"""
    _require(isinstance(page_size, int) and page_size >= 64 and page_size % 64 == 0, f"page_size must be a positive multiple of 64, got {page_size}")
    _require(isinstance(num_pages, int) and num_pages > 0, f"num_pages must be positive, got {num_pages}")
    _require(pool.device == dev and pool.dtype == torch.uint8 and pool.is_contiguous() and pool.numel() == L.qattn_mla_pool_bytes(num_pages, page_size),
             f"the pool does not fit [num_pages={num_pages}, page_size={page_size}] latents of {MLA_D} bytes")
    _require(block_table.dtype == torch.int32 and block_table.device == dev and block_table.dim() == 2 and block_table.shape[0] == B
             and block_table.shape[1] > 0 and block_table.stride(1) == 1 and (B == 1 or block_table.stride(0) >= block_table.shape[1]),
             f"block_table must be an int32 [B={B}, max_pages] tensor on {dev} with dense rows")
    _require(scale.dtype == torch.float32 and scale.device == dev and scale.is_contiguous() and tuple(scale.shape) == (B,),
             f"scale must be a dense float32 [B] tensor on {dev}")
    max_pages = block_table.shape[1]
    return max_pages, (block_table.stride(0) if B > 1 else max_pages)


def mla_rows_addressable(t: torch.Tensor) -> bool:
    """a view the MLA kernels address directly: channels innermost and dense, every other stride a non-negative multiple of 8 elements, a
    16-byte-aligned base"""
    return (t.stride(-1) == 1 and all(t.shape[i] == 1 or (t.stride(i) >= 0 and t.stride(i) % 8 == 0) for i in range(t.dim() - 1))
            and t.data_ptr() % 16 == 0)


def _lens_check(name, t, B, dev, optional=False):
    _require((t is None and optional) or (t is not None and t.dtype == torch.int32 and t.device == dev and tuple(t.shape) == (B,) and t.is_contiguous()),
             f"{name} must be a dense int32 [B] tensor on {dev}")


def paged_mla_cache_append_fp8(pool: torch.Tensor, scale: torch.Tensor, block_table: torch.Tensor, seqlens: torch.Tensor, ckv_new: torch.Tensor,
                               kpe_new: torch.Tensor, *, num_pages: int, page_size: int, fp8_dtype=torch.float8_e4m3fn,
                               new_lens: Optional[torch.Tensor] = None, advance: bool = True) -> None:
    """qattn_paged_mla_cache_append_fp8 (include/qattn_mla.h): ckv_new [B, T, 512] and kpe_new [B, T, 64] (views accepted) into the one-image
    pool through block_table.  The table, seqlens and new_lens are read on the device.  Mutates pool and seqlens."""
    _require(ckv_new.is_cuda and ckv_new.dim() == 3 and ckv_new.dtype in (torch.bfloat16, torch.float16) and ckv_new.shape[2] == MLA_D_LATENT,
             f"ckv_new must be a bf16 / fp16 device tensor [B, T, {MLA_D_LATENT}]")
    _require(kpe_new.dim() == 3 and kpe_new.dtype == ckv_new.dtype and kpe_new.device == ckv_new.device
             and tuple(kpe_new.shape) == (ckv_new.shape[0], ckv_new.shape[1], MLA_D_ROPE), f"kpe_new must be [B, T, {MLA_D_ROPE}] beside ckv_new")
    _require(mla_rows_addressable(ckv_new) and mla_rows_addressable(kpe_new), "ckv_new / kpe_new need dense channels and 16-byte-aligned rows")
    B, T, _ = ckv_new.shape
    _require(T > 0, "T must be positive")
    L = lib()
    dev = ckv_new.device
    max_pages, tstride = _mla_pool_checks(L, pool, block_table, scale, dev, B, num_pages, page_size)
    _lens_check("seqlens", seqlens, B, dev)
    _lens_check("new_lens", new_lens, B, dev, optional=True)
    s2 = lambda t: (ctypes.c_longlong * 2)(*[t.stride(i) if t.shape[i] > 1 else (T * t.shape[2], t.shape[2])[i] for i in (0, 1)])
    with torch.cuda.device(dev):
        rc = L.qattn_paged_mla_cache_append_fp8(ckv_new.data_ptr(), kpe_new.data_ptr(), fmt_of(ckv_new.dtype), s2(ckv_new), s2(kpe_new),
                                                pool.data_ptr(), scale.data_ptr(), block_table.data_ptr(), tstride, seqlens.data_ptr(),
                                                _ptr(new_lens), int(bool(advance)), B, T, num_pages, page_size, max_pages, fmt_of(fp8_dtype),
                                                _stream(ckv_new))
    _check(rc, "qattn_paged_mla_cache_append_fp8")


def fp8_mla_paged_attention(q: torch.Tensor, pool: torch.Tensor, scale: torch.Tensor, block_table: torch.Tensor, seqused_k: torch.Tensor, *,
                            Skv: int, num_pages: int, page_size: int, fp8_dtype=torch.float8_e4m3fn, is_causal: bool, sm_scale: float,
                            num_splits: int, return_partials: bool = False, return_q8: bool = False):
    """qattn_fp8_mla_paged_forward (include/qattn_mla.h) with num_splits >= 1 resolved by the caller.  Returns (out [B, Hq, Sq, 512],
    lse [B, Hq, Sq], partial_o, partial_lse, q8, scale_q); the last four are empty unless asked for (partials: and num_splits > 1)."""
    _require(q.is_cuda and q.dim() == 4 and q.dtype in (torch.bfloat16, torch.float16) and q.shape[3] == MLA_D,
             f"q must be a bf16 / fp16 device tensor [B, Hq, Sq, {MLA_D}]")
    _require(mla_rows_addressable(q), "q needs dense channels and 16-byte-aligned rows")
    _require(isinstance(num_splits, int) and 1 <= num_splits <= MLA_MAX_SPLITS, f"num_splits must be in 1 .. {MLA_MAX_SPLITS} here, got {num_splits}")
    B, Hq, Sq, _ = q.shape
    L = lib()
    dev = q.device
    max_pages, tstride = _mla_pool_checks(L, pool, block_table, scale, dev, B, num_pages, page_size)
    _lens_check("seqused_k", seqused_k, B, dev)
    _require(isinstance(Skv, int) and 1 <= Skv <= max_pages * page_size, f"Skv must be in 1 .. max_pages * page_size, got {Skv}")
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = torch.empty((B, Hq, Sq, MLA_D_LATENT), dtype=q.dtype, device=dev)
    lse = f32(B, Hq, Sq)
    parts = num_splits > 1 and return_partials
    po, pl = (f32(num_splits, B, Hq, Sq, MLA_D_LATENT), f32(num_splits, B, Hq, Sq)) if parts else (f32(0), f32(0))
    q8 = torch.empty((B, Hq, Sq, MLA_D) if return_q8 else (0,), dtype=torch.uint8, device=dev)
    sq = f32(B, Hq, Sq) if return_q8 else f32(0)
    wsb = 0 if parts else L.qattn_fp8_mla_paged_workspace_bytes(B, Hq, Sq, num_splits)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev) if wsb else None
    dense = (Hq * Sq * MLA_D, Sq * MLA_D, MLA_D)
    s3 = None if q.is_contiguous() else (ctypes.c_longlong * 3)(*[q.stride(i) if q.shape[i] > 1 else dense[i] for i in (0, 1, 2)])
    with torch.cuda.device(dev):
        rc = L.qattn_fp8_mla_paged_forward(q.data_ptr(), fmt_of(q.dtype), s3, pool.data_ptr(), block_table.data_ptr(), tstride, num_pages, page_size,
                                           max_pages, scale.data_ptr(), out.data_ptr(), lse.data_ptr(), seqused_k.data_ptr(), B, Hq, Sq, Skv,
                                           fmt_of(fp8_dtype), int(bool(is_causal)), float(sm_scale), num_splits,
                                           q8.data_ptr() if return_q8 else None, sq.data_ptr() if return_q8 else None,
                                           po.data_ptr() if parts else None, pl.data_ptr() if parts else None, _ptr(ws), wsb, _stream(q))
    _check(rc, "qattn_fp8_mla_paged_forward")
    return out, lse, po, pl, (q8.view(torch.float8_e4m3fn) if return_q8 else q8), sq


def mla_sparse_auto_splits(B: int, Hq: int, Sq: int, topk: int, num_cus: int) -> int:
    """qattn_mla_sparse_auto_splits (include/qattn_mla_sparse.h): a pure function of the shape and the CU count (no device needed)."""
    return lib().qattn_mla_sparse_auto_splits(B, Hq, Sq, topk, num_cus)


def _mla_row_pool_checks(L, pool, block_table, scale, dev, B, num_pages, page_size):
    """the pool, the table and the scales of a row-major paged latent cache (include/qattn_mla_sparse.h); returns (max_pages, table_stride)"""
    _require(isinstance(page_size, int) and page_size >= 1 and isinstance(num_pages, int) and num_pages > 0
             and num_pages * page_size <= 2 ** 31 - 1, f"num_pages and page_size must be positive with a product below 2^31, got {num_pages}, {page_size}")
    _require(pool.device == dev and pool.element_size() == 1 and pool.is_contiguous() and tuple(pool.shape) == (num_pages, page_size, MLA_D),
             f"the pool must be a dense fp8 [num_pages={num_pages}, page_size={page_size}, {MLA_D}] tensor on {dev}")
    _require(block_table.dtype == torch.int32 and block_table.device == dev and block_table.dim() == 2 and block_table.shape[0] == B
             and block_table.shape[1] > 0 and block_table.stride(1) == 1 and (B == 1 or block_table.stride(0) >= block_table.shape[1]),
             f"block_table must be an int32 [B={B}, max_pages] tensor on {dev} with dense rows")
    _require(scale.dtype == torch.float32 and scale.device == dev and scale.is_contiguous() and tuple(scale.shape) == (B,),
             f"scale must be a dense float32 [B] tensor on {dev}")
    max_pages = block_table.shape[1]
    _require(max_pages * page_size <= 2 ** 31 - 65, "max_pages * page_size must stay below 2^31 - 64")
    return max_pages, (block_table.stride(0) if B > 1 else max_pages)


def paged_mla_row_cache_append_fp8(pool: torch.Tensor, scale: torch.Tensor, block_table: torch.Tensor, seqlens: torch.Tensor,
                                   ckv_new: torch.Tensor, kpe_new: torch.Tensor, *, num_pages: int, page_size: int,
                                   fp8_dtype=torch.float8_e4m3fn, new_lens: Optional[torch.Tensor] = None, advance: bool = True) -> None:
    """qattn_paged_mla_row_cache_append_fp8 (include/qattn_mla_sparse.h): ckv_new [B, T, 512] and kpe_new [B, T, 64] (views accepted) into the
    row-major pool [num_pages, page_size, 576] through block_table.  The table, seqlens and new_lens are read on the device.  Mutates pool
    and seqlens."""
    _require(ckv_new.is_cuda and ckv_new.dim() == 3 and ckv_new.dtype in (torch.bfloat16, torch.float16) and ckv_new.shape[2] == MLA_D_LATENT,
             f"ckv_new must be a bf16 / fp16 device tensor [B, T, {MLA_D_LATENT}]")
    _require(kpe_new.dim() == 3 and kpe_new.dtype == ckv_new.dtype and kpe_new.device == ckv_new.device
             and tuple(kpe_new.shape) == (ckv_new.shape[0], ckv_new.shape[1], MLA_D_ROPE), f"kpe_new must be [B, T, {MLA_D_ROPE}] beside ckv_new")
    _require(mla_rows_addressable(ckv_new) and mla_rows_addressable(kpe_new), "ckv_new / kpe_new need dense channels and 16-byte-aligned rows")
    B, T, _ = ckv_new.shape
    _require(T > 0, "T must be positive")
    L = lib()
    dev = ckv_new.device
    max_pages, tstride = _mla_row_pool_checks(L, pool, block_table, scale, dev, B, num_pages, page_size)
    _lens_check("seqlens", seqlens, B, dev)
    _lens_check("new_lens", new_lens, B, dev, optional=True)
    s2 = lambda t: (ctypes.c_longlong * 2)(*[t.stride(i) if t.shape[i] > 1 else (T * t.shape[2], t.shape[2])[i] for i in (0, 1)])
    with torch.cuda.device(dev):
        rc = L.qattn_paged_mla_row_cache_append_fp8(ckv_new.data_ptr(), kpe_new.data_ptr(), fmt_of(ckv_new.dtype), s2(ckv_new), s2(kpe_new),
                                                    pool.data_ptr(), scale.data_ptr(), block_table.data_ptr(), tstride, seqlens.data_ptr(),
                                                    _ptr(new_lens), int(bool(advance)), B, T, num_pages, page_size, max_pages,
                                                    fmt_of(fp8_dtype), _stream(ckv_new))
    _check(rc, "qattn_paged_mla_row_cache_append_fp8")


def fp8_mla_paged_sparse_attention(q: torch.Tensor, pool: torch.Tensor, scale: torch.Tensor, block_table: torch.Tensor, seqused_k: torch.Tensor,
                                   indices: torch.Tensor, *, num_pages: int, page_size: int, fp8_dtype=torch.float8_e4m3fn, is_causal: bool,
                                   sm_scale: float, num_splits: int, return_partials: bool = False, return_q8: bool = False):
    """qattn_fp8_mla_paged_sparse_forward (include/qattn_mla_sparse.h) with num_splits >= 1 resolved by the caller; indices int32
    [B, Sq, topk] with a dense last dimension.  Returns (out [B, Hq, Sq, 512], lse [B, Hq, Sq], partial_o, partial_lse, q8, scale_q); the
    last four are empty unless asked for (partials: and num_splits > 1)."""
    _require(q.is_cuda and q.dim() == 4 and q.dtype in (torch.bfloat16, torch.float16) and q.shape[3] == MLA_D,
             f"q must be a bf16 / fp16 device tensor [B, Hq, Sq, {MLA_D}]")
    _require(mla_rows_addressable(q), "q needs dense channels and 16-byte-aligned rows")
    B, Hq, Sq, _ = q.shape
    dev = q.device
    _require(indices.dtype == torch.int32 and indices.device == dev and indices.dim() == 3 and tuple(indices.shape[:2]) == (B, Sq)
             and 1 <= indices.shape[2] <= MLA_SPARSE_MAX_TOPK and (indices.shape[2] == 1 or indices.stride(2) == 1)
             and all(indices.shape[i] == 1 or indices.stride(i) >= 0 for i in (0, 1)),
             f"indices must be an int32 [B={B}, Sq={Sq}, 1 <= topk <= {MLA_SPARSE_MAX_TOPK}] tensor on {dev} with a dense last dimension")
    topk = indices.shape[2]
    _require(isinstance(num_splits, int) and max(1, -(-topk // MLA_SPARSE_SPLIT_ENTRIES)) <= num_splits <= MLA_MAX_SPLITS,
             f"num_splits must be in ceil(topk / {MLA_SPARSE_SPLIT_ENTRIES}) .. {MLA_MAX_SPLITS} here, got {num_splits}")
    L = lib()
    max_pages, tstride = _mla_row_pool_checks(L, pool, block_table, scale, dev, B, num_pages, page_size)
    _lens_check("seqused_k", seqused_k, B, dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = torch.empty((B, Hq, Sq, MLA_D_LATENT), dtype=q.dtype, device=dev)
    lse = f32(B, Hq, Sq)
    parts = num_splits > 1 and return_partials
    po, pl = (f32(num_splits, B, Hq, Sq, MLA_D_LATENT), f32(num_splits, B, Hq, Sq)) if parts else (f32(0), f32(0))
    q8 = torch.empty((B, Hq, Sq, MLA_D) if return_q8 else (0,), dtype=torch.uint8, device=dev)
    sq = f32(B, Hq, Sq) if return_q8 else f32(0)
    wsb = 0 if parts else L.qattn_fp8_mla_paged_sparse_workspace_bytes(B, Hq, Sq, num_splits)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev) if wsb else None
    dense = (Hq * Sq * MLA_D, Sq * MLA_D, MLA_D)
    s3 = None if q.is_contiguous() else (ctypes.c_longlong * 3)(*[q.stride(i) if q.shape[i] > 1 else dense[i] for i in (0, 1, 2)])
    idense = (Sq * topk, topk)
    i2 = None if indices.is_contiguous() else (ctypes.c_longlong * 2)(*[indices.stride(i) if indices.shape[i] > 1 else idense[i] for i in (0, 1)])
    with torch.cuda.device(dev):
        rc = L.qattn_fp8_mla_paged_sparse_forward(q.data_ptr(), fmt_of(q.dtype), s3, pool.data_ptr(), block_table.data_ptr(), tstride, num_pages,
                                                  page_size, max_pages, scale.data_ptr(), indices.data_ptr(), i2, topk, out.data_ptr(),
                                                  lse.data_ptr(), seqused_k.data_ptr(), B, Hq, Sq, fmt_of(fp8_dtype), int(bool(is_causal)),
                                                  float(sm_scale), num_splits, q8.data_ptr() if return_q8 else None,
                                                  sq.data_ptr() if return_q8 else None, po.data_ptr() if parts else None,
                                                  pl.data_ptr() if parts else None, _ptr(ws), wsb, _stream(q))
    _check(rc, "qattn_fp8_mla_paged_sparse_forward")
    return out, lse, po, pl, (q8.view(torch.float8_e4m3fn) if return_q8 else q8), sq


def fp8_mla_paged_sparse_varlen_attention(q: torch.Tensor, pool: torch.Tensor, scale: torch.Tensor, block_table: torch.Tensor,
                                          seqused_k: torch.Tensor, indices: torch.Tensor, cu_seqlens_q: torch.Tensor, *, num_pages: int,
                                          page_size: int, fp8_dtype=torch.float8_e4m3fn, is_causal: bool, sm_scale: float,
                                          return_q8: bool = False):
    """qattn_fp8_mla_paged_sparse_varlen_forward (include/qattn_mla_sparse_prefill.h): q [total_q, Hq, 576] (a view with dense channels is
    read through its strides), indices int32 [total_q, topk] with a dense last dimension, cu_seqlens_q int32 [B + 1].  Returns (out
    [total_q, Hq, 512], lse [Hq, total_q], q8, scale_q); the last two are empty unless asked for."""
    _require(q.is_cuda and q.dim() == 3 and q.dtype in (torch.bfloat16, torch.float16) and q.shape[2] == MLA_D and q.shape[0] > 0 and q.shape[1] > 0,
             f"q must be a bf16 / fp16 device tensor [total_q, Hq, {MLA_D}]")
    _require(mla_rows_addressable(q), "q needs dense channels and 16-byte-aligned rows")
    total_q, Hq, _ = q.shape
    dev = q.device
    _require(indices.dtype == torch.int32 and indices.device == dev and indices.dim() == 2 and indices.shape[0] == total_q
             and 1 <= indices.shape[1] <= MLA_SPARSE_MAX_TOPK and (indices.shape[1] == 1 or indices.stride(1) == 1)
             and (total_q == 1 or indices.stride(0) >= 0),
             f"indices must be an int32 [total_q={total_q}, 1 <= topk <= {MLA_SPARSE_MAX_TOPK}] tensor on {dev} with a dense last dimension")
    topk = indices.shape[1]
    B = block_table.shape[0] if block_table.dim() == 2 else 0
    _require(cu_seqlens_q.dtype == torch.int32 and cu_seqlens_q.device == dev and cu_seqlens_q.is_contiguous()
             and tuple(cu_seqlens_q.shape) == (B + 1,), f"cu_seqlens_q must be a dense int32 [B + 1 = {B + 1}] tensor on {dev}")
    L = lib()
    max_pages, tstride = _mla_row_pool_checks(L, pool, block_table, scale, dev, B, num_pages, page_size)
    _lens_check("seqused_k", seqused_k, B, dev)
    out = torch.empty((total_q, Hq, MLA_D_LATENT), dtype=q.dtype, device=dev)
    lse = torch.empty((Hq, total_q), dtype=torch.float32, device=dev)
    q8 = torch.empty((total_q, Hq, MLA_D) if return_q8 else (0,), dtype=torch.uint8, device=dev)
    sq = torch.empty((total_q, Hq) if return_q8 else (0,), dtype=torch.float32, device=dev)
    dense = (Hq * MLA_D, MLA_D)
    s2 = None if q.is_contiguous() else (ctypes.c_longlong * 2)(*[q.stride(i) if q.shape[i] > 1 else dense[i] for i in (0, 1)])
    with torch.cuda.device(dev):
        rc = L.qattn_fp8_mla_paged_sparse_varlen_forward(q.data_ptr(), fmt_of(q.dtype), s2, pool.data_ptr(), block_table.data_ptr(), tstride,
                                                         num_pages, page_size, max_pages, scale.data_ptr(), indices.data_ptr(),
                                                         indices.stride(0) if total_q > 1 else topk, topk, cu_seqlens_q.data_ptr(),
                                                         out.data_ptr(), lse.data_ptr(), seqused_k.data_ptr(), B, total_q, Hq,
                                                         fmt_of(fp8_dtype), int(bool(is_causal)), float(sm_scale),
                                                         q8.data_ptr() if return_q8 else None, sq.data_ptr() if return_q8 else None,
                                                         _stream(q))
    _check(rc, "qattn_fp8_mla_paged_sparse_varlen_forward")
    return out, lse, (q8.view(torch.float8_e4m3fn) if return_q8 else q8), sq


def mla_varlen_tile_slots(B: int, total_q: int, Hq: int) -> int:
    """the host bound of the packed dense entry's tile grid (include/qattn_mla_varlen.h): ceil(total_q Hq / 128) + B"""
    return -(-total_q * Hq // MLA_VARLEN_ROWS) + B


def mla_varlen_auto_splits(tile_slots: int, Skv: int, num_cus: int) -> int:
    """qattn_mla_varlen_auto_splits (include/qattn_mla_varlen.h): a pure function of its arguments (no device needed)."""
    return lib().qattn_mla_varlen_auto_splits(tile_slots, Skv, num_cus)


def fp8_mla_paged_varlen_attention(q: torch.Tensor, pool: torch.Tensor, scale: torch.Tensor, block_table: torch.Tensor, seqused_k: torch.Tensor,
                                   cu_seqlens_q: torch.Tensor, *, max_seqlen_q: int, Skv: int, num_pages: int, page_size: int,
                                   fp8_dtype=torch.float8_e4m3fn, is_causal: bool, sm_scale: float, num_splits: int,
                                   return_partials: bool = False, return_q8: bool = False):
    """qattn_fp8_mla_paged_varlen_forward (include/qattn_mla_varlen.h) with num_splits >= 1 resolved by the caller: q [total_q, Hq, 576] (a view
    with dense channels is read through its strides), cu_seqlens_q int32 [B + 1].  Returns (out [total_q, Hq, 512], lse [Hq, total_q],
    partial_o [ns, total_q, Hq, 512], partial_lse [ns, total_q, Hq], q8, scale_q); the last four are empty unless asked for (partials: and
    num_splits > 1)."""
    _require(q.is_cuda and q.dim() == 3 and q.dtype in (torch.bfloat16, torch.float16) and q.shape[2] == MLA_D and q.shape[0] > 0 and q.shape[1] > 0,
             f"q must be a bf16 / fp16 device tensor [total_q, Hq, {MLA_D}]")
    _require(mla_rows_addressable(q), "q needs dense channels and 16-byte-aligned rows")
    _require(isinstance(num_splits, int) and 1 <= num_splits <= MLA_MAX_SPLITS, f"num_splits must be in 1 .. {MLA_MAX_SPLITS} here, got {num_splits}")
    total_q, Hq, _ = q.shape
    _require(isinstance(max_seqlen_q, int) and 1 <= max_seqlen_q <= total_q, f"max_seqlen_q must be in 1 .. total_q = {total_q}, got {max_seqlen_q}")
    dev = q.device
    B = block_table.shape[0] if block_table.dim() == 2 else 0
    _require(cu_seqlens_q.dtype == torch.int32 and cu_seqlens_q.device == dev and cu_seqlens_q.is_contiguous()
             and tuple(cu_seqlens_q.shape) == (B + 1,), f"cu_seqlens_q must be a dense int32 [B + 1 = {B + 1}] tensor on {dev}")
    L = lib()
    max_pages, tstride = _mla_pool_checks(L, pool, block_table, scale, dev, B, num_pages, page_size)
    _lens_check("seqused_k", seqused_k, B, dev)
    _require(isinstance(Skv, int) and 1 <= Skv <= max_pages * page_size, f"Skv must be in 1 .. max_pages * page_size, got {Skv}")
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = torch.empty((total_q, Hq, MLA_D_LATENT), dtype=q.dtype, device=dev)
    lse = f32(Hq, total_q)
    parts = num_splits > 1 and return_partials
    po, pl = (f32(num_splits, total_q, Hq, MLA_D_LATENT), f32(num_splits, total_q, Hq)) if parts else (f32(0), f32(0))
    q8 = torch.empty((total_q, Hq, MLA_D) if return_q8 else (0,), dtype=torch.uint8, device=dev)
    sq = f32(total_q, Hq) if return_q8 else f32(0)
    wsb = 0 if parts else L.qattn_fp8_mla_paged_varlen_workspace_bytes(total_q, Hq, num_splits)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev) if wsb else None
    dense = (Hq * MLA_D, MLA_D)
    s2 = None if q.is_contiguous() else (ctypes.c_longlong * 2)(*[q.stride(i) if q.shape[i] > 1 else dense[i] for i in (0, 1)])
    with torch.cuda.device(dev):
        rc = L.qattn_fp8_mla_paged_varlen_forward(q.data_ptr(), fmt_of(q.dtype), s2, pool.data_ptr(), block_table.data_ptr(), tstride, num_pages,
                                                  page_size, max_pages, scale.data_ptr(), cu_seqlens_q.data_ptr(), max_seqlen_q, out.data_ptr(),
                                                  lse.data_ptr(), seqused_k.data_ptr(), B, total_q, Hq, Skv, fmt_of(fp8_dtype),
                                                  int(bool(is_causal)), float(sm_scale), num_splits, q8.data_ptr() if return_q8 else None,
                                                  sq.data_ptr() if return_q8 else None, po.data_ptr() if parts else None,
                                                  pl.data_ptr() if parts else None, _ptr(ws), wsb, _stream(q))
    _check(rc, "qattn_fp8_mla_paged_varlen_forward")
    return out, lse, po, pl, (q8.view(torch.float8_e4m3fn) if return_q8 else q8), sq


def _mla_index_pool_checks(pool, block_table, scale, dev, B, num_pages, page_size):
    """the pool, the table and the scales of a paged index-key cache (include/qattn_mla_index.h); returns (max_pages, table_stride)"""
    _require(isinstance(page_size, int) and page_size >= 1 and isinstance(num_pages, int) and num_pages > 0
             and num_pages * page_size <= 2 ** 31 - 1, f"num_pages and page_size must be positive with a product below 2^31, got {num_pages}, {page_size}")
    _require(pool.device == dev and pool.element_size() == 1 and pool.is_contiguous() and tuple(pool.shape) == (num_pages, page_size, MLA_INDEX_D),
             f"the pool must be a dense fp8 [num_pages={num_pages}, page_size={page_size}, {MLA_INDEX_D}] tensor on {dev}")
    _require(block_table.dtype == torch.int32 and block_table.device == dev and block_table.dim() == 2 and block_table.shape[0] == B
             and block_table.shape[1] > 0 and block_table.stride(1) == 1 and (B == 1 or block_table.stride(0) >= block_table.shape[1]),
             f"block_table must be an int32 [B={B}, max_pages] tensor on {dev} with dense rows")
    _require(scale.dtype == torch.float32 and scale.device == dev and scale.is_contiguous() and tuple(scale.shape) == (B,),
             f"scale must be a dense float32 [B] tensor on {dev}")
    max_pages = block_table.shape[1]
    _require(max_pages * page_size <= 2 ** 31 - 65, "max_pages * page_size must stay below 2^31 - 64")
    return max_pages, (block_table.stride(0) if B > 1 else max_pages)


def paged_mla_index_cache_append_fp8(pool: torch.Tensor, scale: torch.Tensor, block_table: torch.Tensor, seqlens: torch.Tensor,
                                     k_new: torch.Tensor, *, num_pages: int, page_size: int, fp8_dtype=torch.float8_e4m3fn,
                                     new_lens: Optional[torch.Tensor] = None, advance: bool = True) -> None:
    """qattn_paged_mla_index_cache_append_fp8 (include/qattn_mla_index.h): k_new [B, T, 128] (views accepted) into the row-major pool
    [num_pages, page_size, 128] through block_table.  The table, seqlens and new_lens are read on the device.  Mutates pool and seqlens."""
    _require(k_new.is_cuda and k_new.dim() == 3 and k_new.dtype in (torch.bfloat16, torch.float16) and k_new.shape[2] == MLA_INDEX_D,
             f"k_new must be a bf16 / fp16 device tensor [B, T, {MLA_INDEX_D}]")
    _require(mla_rows_addressable(k_new), "k_new needs dense channels and 16-byte-aligned rows")
    B, T, _ = k_new.shape
    _require(T > 0, "T must be positive")
    dev = k_new.device
    max_pages, tstride = _mla_index_pool_checks(pool, block_table, scale, dev, B, num_pages, page_size)
    _lens_check("seqlens", seqlens, B, dev)
    _lens_check("new_lens", new_lens, B, dev, optional=True)
    s2 = (ctypes.c_longlong * 2)(*[k_new.stride(i) if k_new.shape[i] > 1 else (T * MLA_INDEX_D, MLA_INDEX_D)[i] for i in (0, 1)])
    with torch.cuda.device(dev):
        rc = lib().qattn_paged_mla_index_cache_append_fp8(k_new.data_ptr(), fmt_of(k_new.dtype), s2, pool.data_ptr(), scale.data_ptr(),
                                                          block_table.data_ptr(), tstride, seqlens.data_ptr(), _ptr(new_lens),
                                                          int(bool(advance)), B, T, num_pages, page_size, max_pages, fmt_of(fp8_dtype),
                                                          _stream(k_new))
    _check(rc, "qattn_paged_mla_index_cache_append_fp8")


def _rows2(t: torch.Tensor):
    """the {batch, position} element strides of a [B, Sq, n] tensor with a dense last dimension, or None for a dense tensor"""
    if t.is_contiguous():
        return None
    dense = (t.shape[1] * t.shape[2], t.shape[2])
    return (ctypes.c_longlong * 2)(*[t.stride(i) if t.shape[i] > 1 else dense[i] for i in (0, 1)])


def mla_index_select(logits: torch.Tensor, seqused_k: torch.Tensor, topk: int, *, is_causal: bool) -> torch.Tensor:
    """qattn_mla_index_select (include/qattn_mla_index.h): logits fp32 [B, Sq, N] (last dimension dense) -> indices int32 [B, Sq, topk]."""
    _require(logits.is_cuda and logits.dim() == 3 and logits.dtype == torch.float32 and logits.numel() > 0
             and (logits.shape[2] == 1 or logits.stride(2) == 1) and all(logits.shape[i] == 1 or logits.stride(i) >= 0 for i in (0, 1)),
             "logits must be a float32 device tensor [B, Sq, N] with a dense last dimension")
    _require(isinstance(topk, int) and 1 <= topk <= MLA_SPARSE_MAX_TOPK, f"topk must be in 1 .. {MLA_SPARSE_MAX_TOPK}, got {topk}")
    B, Sq, N = logits.shape
    _lens_check("seqused_k", seqused_k, B, logits.device)
    out = torch.empty((B, Sq, topk), dtype=torch.int32, device=logits.device)
    with torch.cuda.device(logits.device):
        rc = lib().qattn_mla_index_select(logits.data_ptr(), _rows2(logits), seqused_k.data_ptr(), B, Sq, N, topk, int(bool(is_causal)),
                                          out.data_ptr(), _stream(logits))
    _check(rc, "qattn_mla_index_select")
    return out


def mla_index_select_auto_splits(rows: int, N: int, topk: int, num_cus: int) -> int:
    """qattn_mla_index_select_auto_splits (include/qattn_mla_index_split.h): a pure function of the shape and the CU count (no device needed)."""
    return lib().qattn_mla_index_select_auto_splits(rows, N, topk, num_cus)


def mla_index_resolve_splits(num_splits, rows: int, N: int, topk: int, dev) -> int:
    """The ONE place where num_splits / select_splits = 0 becomes a count: qattn_mla_index_select_auto_splits on the device's CU count.  Any
    other value is returned as it is, checked.  The library's entries take the result, 1 .. 256; they reject 0."""
    _require(isinstance(num_splits, int) and 0 <= num_splits <= MLA_INDEX_MAX_SELECT_SPLITS,
             f"num_splits must be in 0 .. {MLA_INDEX_MAX_SELECT_SPLITS}, got {num_splits}")
    return num_splits or mla_index_select_auto_splits(rows, N, topk, torch.cuda.get_device_properties(dev).multi_processor_count)


def mla_index_select_split(logits: torch.Tensor, seqused_k: torch.Tensor, topk: int, *, is_causal: bool, num_splits: int = 0,
                           workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qattn_mla_index_select_split (include/qattn_mla_index_split.h): `mla_index_select` with every row cut across num_splits workgroups
    (0: resolved by mla_index_resolve_splits; 1: the one-workgroup kernel).  workspace: the caller's uint8 device tensor of at least
    qattn_mla_index_select_split_workspace_bytes bytes, 16-byte aligned; its contents do not matter.  Default: allocated here."""
    _require(logits.is_cuda and logits.dim() == 3 and logits.dtype == torch.float32 and logits.numel() > 0
             and (logits.shape[2] == 1 or logits.stride(2) == 1) and all(logits.shape[i] == 1 or logits.stride(i) >= 0 for i in (0, 1)),
             "logits must be a float32 device tensor [B, Sq, N] with a dense last dimension")
    _require(isinstance(topk, int) and 1 <= topk <= MLA_SPARSE_MAX_TOPK, f"topk must be in 1 .. {MLA_SPARSE_MAX_TOPK}, got {topk}")
    B, Sq, N = logits.shape
    dev = logits.device
    _lens_check("seqused_k", seqused_k, B, dev)
    ns = mla_index_resolve_splits(num_splits, B * Sq, N, topk, dev)
    _require(ns == 1 or (B <= 65535 and Sq <= 65535), "a split selection needs B, Sq <= 65535")
    wsb = lib().qattn_mla_index_select_split_workspace_bytes(B, Sq, N, ns)
    if workspace is None:
        workspace = torch.empty((wsb,), dtype=torch.uint8, device=dev) if wsb else None
    else:
        _require(workspace.dtype == torch.uint8 and workspace.device == dev and workspace.is_contiguous() and workspace.numel() >= wsb
                 and workspace.data_ptr() % 16 == 0, f"workspace must be a dense 16-byte-aligned uint8 tensor of at least {wsb} bytes on {dev}")
    out = torch.empty((B, Sq, topk), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib().qattn_mla_index_select_split(logits.data_ptr(), _rows2(logits), seqused_k.data_ptr(), B, Sq, N, topk, int(bool(is_causal)),
                                                ns, out.data_ptr(), _ptr(workspace), wsb, _stream(logits))
    _check(rc, "qattn_mla_index_select_split")
    return out


def fp8_mla_index_topk(q: torch.Tensor, weights: torch.Tensor, pool: torch.Tensor, scale: torch.Tensor, block_table: torch.Tensor,
                       seqused_k: torch.Tensor, *, Skv: int, topk: int, num_pages: int, page_size: int, fp8_dtype=torch.float8_e4m3fn,
                       is_causal: bool, return_logits: bool = False, return_q8: bool = False, select: bool = True, select_splits: int = 1):
    """qattn_fp8_mla_index_topk (include/qattn_mla_index.h), with select_splits != 1 qattn_fp8_mla_index_topk_split
    (include/qattn_mla_index_split.h; 0: resolved by mla_index_resolve_splits), or with select=False qattn_fp8_mla_index_scores alone (logits with a filled
    tail).  Returns (indices int32 [B, Sq, topk], logits fp32 [B, Sq, Skv], q8 [B, Hi, Sq, 128] e4m3, scale_q [B, Hi, Sq]); what was not
    asked for (or not computed) is empty."""
    _require(q.is_cuda and q.dim() == 4 and q.dtype in (torch.bfloat16, torch.float16) and q.shape[3] == MLA_INDEX_D
             and 1 <= q.shape[1] <= MLA_INDEX_MAX_HEADS, f"q must be a bf16 / fp16 device tensor [B, Hi <= {MLA_INDEX_MAX_HEADS}, Sq, {MLA_INDEX_D}]")
    _require(mla_rows_addressable(q), "q needs dense channels and 16-byte-aligned rows")
    B, Hi, Sq, _ = q.shape
    dev = q.device
    _require(weights.dtype == torch.float32 and weights.device == dev and tuple(weights.shape) == (B, Sq, Hi)
             and (Hi == 1 or weights.stride(2) == 1) and all(weights.shape[i] == 1 or weights.stride(i) >= 0 for i in (0, 1)),
             f"weights must be a float32 [B={B}, Sq={Sq}, Hi={Hi}] tensor on {dev} with dense heads")
    _require(isinstance(topk, int) and 1 <= topk <= MLA_SPARSE_MAX_TOPK, f"topk must be in 1 .. {MLA_SPARSE_MAX_TOPK}, got {topk}")
    max_pages, tstride = _mla_index_pool_checks(pool, block_table, scale, dev, B, num_pages, page_size)
    _require(isinstance(Skv, int) and 1 <= Skv <= max_pages * page_size and Skv <= 2 ** 30, f"max_seqlen_k must be in 1 .. the capacity, got {Skv}")
    _lens_check("seqused_k", seqused_k, B, dev)
    L = lib()
    own = return_logits or not select
    logits = torch.empty((B, Sq, Skv) if own else (0,), dtype=torch.float32, device=dev)
    indices = torch.empty((B, Sq, topk) if select else (0,), dtype=torch.int32, device=dev)
    q8 = torch.empty((B, Hi, Sq, MLA_INDEX_D) if return_q8 else (0,), dtype=torch.uint8, device=dev)
    sq = torch.empty((B, Hi, Sq) if return_q8 else (0,), dtype=torch.float32, device=dev)
    ns = mla_index_resolve_splits(select_splits, B * Sq, Skv, topk, dev) if select else 1
    wsb = L.qattn_fp8_mla_index_topk_split_workspace_bytes(B, Sq, Skv, ns, int(own))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev) if wsb else None
    dense = (Hi * Sq * MLA_INDEX_D, Sq * MLA_INDEX_D, MLA_INDEX_D)
    s3 = None if q.is_contiguous() else (ctypes.c_longlong * 3)(*[q.stride(i) if q.shape[i] > 1 else dense[i] for i in (0, 1, 2)])
    head = (q.data_ptr(), fmt_of(q.dtype), s3, weights.data_ptr(), _rows2(weights), pool.data_ptr(), block_table.data_ptr(), tstride, num_pages,
            page_size, max_pages, scale.data_ptr(), seqused_k.data_ptr(), B, Hi, Sq, Skv)
    q8p, sqp = (q8.data_ptr(), sq.data_ptr()) if return_q8 else (None, None)
    with torch.cuda.device(dev):
        if select and ns > 1:
            rc = L.qattn_fp8_mla_index_topk_split(*head, topk, fmt_of(fp8_dtype), int(bool(is_causal)), ns, indices.data_ptr(),
                                                  logits.data_ptr() if own else None, q8p, sqp, _ptr(ws), wsb, _stream(q))
        elif select:
            rc = L.qattn_fp8_mla_index_topk(*head, topk, fmt_of(fp8_dtype), int(bool(is_causal)), indices.data_ptr(),
                                            logits.data_ptr() if own else None, q8p, sqp, _ptr(ws), wsb, _stream(q))
        else:
            rc = L.qattn_fp8_mla_index_scores(*head, fmt_of(fp8_dtype), int(bool(is_causal)), logits.data_ptr(), None, 1, q8p, sqp, _stream(q))
    _check(rc, ("qattn_fp8_mla_index_topk_split" if ns > 1 else "qattn_fp8_mla_index_topk") if select else "qattn_fp8_mla_index_scores")
    return indices, logits, (q8.view(torch.float8_e4m3fn) if return_q8 else q8), sq


def fp8_mla_index_topk_varlen(q: torch.Tensor, weights: torch.Tensor, pool: torch.Tensor, scale: torch.Tensor, block_table: torch.Tensor,
                              cu_seqlens_q: torch.Tensor, seqused_k: torch.Tensor, *, Skv: int, topk: int, num_pages: int, page_size: int,
                              fp8_dtype=torch.float8_e4m3fn, is_causal: bool, return_logits: bool = False, return_q8: bool = False,
                              select: bool = True):
    """qattn_fp8_mla_index_topk_varlen (include/qattn_mla_index_prefill.h), or with select=False qattn_fp8_mla_index_scores_varlen alone
    (logits with a filled tail): q [total_q, Hi, 128] (a view `mla_rows_addressable` accepts), weights fp32 [total_q, Hi], cu_seqlens_q
    int32 [B + 1] read on the device.  Returns (indices int32 [total_q, topk], logits fp32 [total_q, Skv], q8 [total_q, Hi, 128] e4m3,
    scale_q [total_q, Hi], kend int32 [total_q]); what was not asked for (or not computed) is empty."""
    _require(q.is_cuda and q.dim() == 3 and q.dtype in (torch.bfloat16, torch.float16) and q.shape[2] == MLA_INDEX_D and q.shape[0] > 0
             and 1 <= q.shape[1] <= MLA_INDEX_MAX_HEADS, f"q must be a bf16 / fp16 device tensor [total_q >= 1, Hi <= {MLA_INDEX_MAX_HEADS}, {MLA_INDEX_D}]")
    _require(mla_rows_addressable(q), "q needs dense channels and 16-byte-aligned rows")
    total_q, Hi, _ = q.shape
    dev, B = q.device, block_table.shape[0]
    _require(weights.dtype == torch.float32 and weights.device == dev and tuple(weights.shape) == (total_q, Hi)
             and (Hi == 1 or weights.stride(1) == 1) and (total_q == 1 or weights.stride(0) > 0),
             f"weights must be a float32 [total_q={total_q}, Hi={Hi}] tensor on {dev} with dense heads")
    _require(isinstance(topk, int) and 1 <= topk <= MLA_SPARSE_MAX_TOPK, f"topk must be in 1 .. {MLA_SPARSE_MAX_TOPK}, got {topk}")
    max_pages, tstride = _mla_index_pool_checks(pool, block_table, scale, dev, B, num_pages, page_size)
    _require(isinstance(Skv, int) and 1 <= Skv <= max_pages * page_size and Skv <= 2 ** 30, f"max_seqlen_k must be in 1 .. the capacity, got {Skv}")
    _lens_check("seqused_k", seqused_k, B, dev)
    _require(cu_seqlens_q.dtype == torch.int32 and cu_seqlens_q.device == dev and tuple(cu_seqlens_q.shape) == (B + 1,) and cu_seqlens_q.is_contiguous(),
             f"cu_seqlens_q must be a dense int32 [B + 1 = {B + 1}] tensor on {dev}")
    L = lib()
    own = return_logits or not select
    logits = torch.empty((total_q, Skv) if own else (0,), dtype=torch.float32, device=dev)
    indices = torch.empty((total_q, topk) if select else (0,), dtype=torch.int32, device=dev)
    q8 = torch.empty((total_q, Hi, MLA_INDEX_D) if return_q8 else (0,), dtype=torch.uint8, device=dev)
    sq = torch.empty((total_q, Hi) if return_q8 else (0,), dtype=torch.float32, device=dev)
    kend_bytes = (4 * total_q + 255) // 256 * 256
    wsb = kend_bytes if own else L.qattn_fp8_mla_index_varlen_workspace_bytes(total_q, Skv)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    kend = ws[: 4 * total_q].view(torch.int32)
    s2 = None if q.is_contiguous() else (ctypes.c_longlong * 2)(*[q.stride(i) if q.shape[i] > 1 else (Hi * MLA_INDEX_D, MLA_INDEX_D)[i] for i in (0, 1)])
    head = (q.data_ptr(), fmt_of(q.dtype), s2, weights.data_ptr(), weights.stride(0) if total_q > 1 else Hi, pool.data_ptr(), block_table.data_ptr(),
            tstride, num_pages, page_size, max_pages, scale.data_ptr(), cu_seqlens_q.data_ptr(), seqused_k.data_ptr(), B, Hi, total_q, Skv)
    q8p, sqp = (q8.data_ptr(), sq.data_ptr()) if return_q8 else (None, None)
    with torch.cuda.device(dev):
        if select:
            rc = L.qattn_fp8_mla_index_topk_varlen(*head, topk, fmt_of(fp8_dtype), int(bool(is_causal)), indices.data_ptr(),
                                                   logits.data_ptr() if own else None, q8p, sqp, ws.data_ptr(), wsb, _stream(q))
        else:
            rc = L.qattn_fp8_mla_index_scores_varlen(*head, fmt_of(fp8_dtype), int(bool(is_causal)), logits.data_ptr(), 0, 1, kend.data_ptr(), q8p, sqp,
                                                     _stream(q))
    _check(rc, "qattn_fp8_mla_index_topk_varlen" if select else "qattn_fp8_mla_index_scores_varlen")
    return indices, logits, (q8.view(torch.float8_e4m3fn) if return_q8 else q8), sq, kend


def fp8_mla_prefill_varlen(q: torch.Tensor, k_nope: torch.Tensor, k_pe: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor,
                           cu_seqlens_k: torch.Tensor, seqused_k: Optional[torch.Tensor] = None, *, is_causal: bool, sm_scale: float,
                           fp8_dtype=torch.float8_e4m3fn, return_quantized: bool = False):
    """qattn_fp8_mla_prefill_varlen_forward (include/qattn_mla_prefill.h): q [total_q, H, 192], k_nope / v [total_k, H, 128], k_pe [total_k, 64]
    (views that `mla_rows_addressable` accepts, read in place), int32 tables on the device.  Returns (out [total_q, H, 128], lse fp32
    [H, total_q], q8 [total_q, H, 192] e4m3, scale_q [total_q, H], scale_k [B, H], scale_v [B, H]); the last four are empty unless
    return_quantized (then zero-filled where no sequence has a token)."""
    _require(q.is_cuda and q.dim() == 3 and q.dtype in (torch.bfloat16, torch.float16) and q.shape[2] == MLA_PREFILL_D_QK and q.shape[1] > 0,
             f"q must be a bf16 / fp16 device tensor [total_q, H, {MLA_PREFILL_D_QK}]")
    total_q, H, _ = q.shape
    total_k = k_nope.shape[0]
    for name, t, shape in (("k_nope", k_nope, (total_k, H, MLA_PREFILL_D_NOPE)), ("k_pe", k_pe, (total_k, MLA_PREFILL_D_ROPE)),
                           ("v", v, (total_k, H, MLA_PREFILL_D_V))):
        _require(tuple(t.shape) == shape and t.dtype == q.dtype and t.device == q.device, f"{name} must be {list(shape)} in q's dtype on q's device")
    _require(all(mla_rows_addressable(t) for t in (q, k_nope, k_pe, v)), "q / k_nope / k_pe / v need dense channels and 16-byte-aligned rows")
    B = cu_seqlens_q.shape[0] - 1
    dev = q.device
    for name, t, n in (("cu_seqlens_q", cu_seqlens_q, B + 1), ("cu_seqlens_k", cu_seqlens_k, B + 1), ("seqused_k", seqused_k, B)):
        _require((t is None and name == "seqused_k") or (t is not None and B >= 1 and t.dtype == torch.int32 and t.device == dev
                                                          and tuple(t.shape) == (n,) and t.is_contiguous()),
                 f"{name} must be a dense int32 [{n}] tensor on {dev}")
    dense = ((H * MLA_PREFILL_D_QK, MLA_PREFILL_D_QK), (H * MLA_PREFILL_D_NOPE, MLA_PREFILL_D_NOPE), (MLA_PREFILL_D_ROPE,),
             (H * MLA_PREFILL_D_V, MLA_PREFILL_D_V))     # (a dimension of size 1 has no stride of its own)
    strides = (ctypes.c_longlong * 7)(*[t.stride(i) if t.shape[i] > 1 else d[i] for t, d in zip((q, k_nope, k_pe, v), dense) for i in range(len(d))])
    L = lib()
    with torch.cuda.device(dev):
        out = torch.empty((total_q, H, MLA_PREFILL_D_V), dtype=q.dtype, device=dev)
        lse = torch.empty((H, total_q), dtype=torch.float32, device=dev)
        rq = bool(return_quantized)
        q8 = torch.zeros((total_q, H, MLA_PREFILL_D_QK) if rq else (0,), dtype=torch.uint8, device=dev)
        sq = torch.zeros((total_q, H) if rq else (0,), dtype=torch.float32, device=dev)
        sk, sv = (torch.zeros((B, H) if rq else (0,), dtype=torch.float32, device=dev) for _ in range(2))
        wsb = L.qattn_fp8_mla_prefill_varlen_workspace_bytes(B, H, total_q, total_k)
        _require(wsb > 0, f"unsupported extents B={B}, H={H}, total_q={total_q}, total_k={total_k}")
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        rc = L.qattn_fp8_mla_prefill_varlen_forward(
            q.data_ptr(), k_nope.data_ptr(), k_pe.data_ptr(), v.data_ptr(), strides, fmt_of(q.dtype), out.data_ptr(), lse.data_ptr(),
            cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(), _ptr(seqused_k), B, H, total_q, total_k, fmt_of(fp8_dtype), int(bool(is_causal)),
            float(sm_scale), *((q8.data_ptr(), sq.data_ptr(), sk.data_ptr(), sv.data_ptr()) if rq else (None,) * 4), ws.data_ptr(), wsb,
            _stream(q))
    _check(rc, "qattn_fp8_mla_prefill_varlen_forward")
    return out, lse, (q8.view(torch.float8_e4m3fn) if rq else q8), sq, sk, sv

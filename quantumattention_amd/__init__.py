"""MI355X-native (gfx950 / CDNA4) FP8 fused attention with the call surface of WaveSpeedAI/QuantumAttention.

Swap `import quantum_attn` for `import quantumattention_amd as quantum_attn`: the exported names are the ones of
src/quantum_attn/__init__.py:23-31.  The hot path runs hand-written HIP kernels through a C ABI
(include/qattn.h, libqattn_hip.so); see DESIGN.md.
"""
import torch  # noqa: F401

from . import config, nn, ops  # noqa: F401
from .quantum_attn_interface import (
    attn_func,
    attn_func_with_fallback,
    dynamically_quantize_fp8,
    fp8_attn_func,
    fp8_attn_func_with_fallback,
    fp8_token_wise_attn_func,
    fp8_token_wise_attn_func_with_fallback,
)

# packed variable-length sequences (flash-attn's varlen call shape): a package attribute beyond the reference's seven exported names
from .varlen import fp8_attn_varlen_func  # noqa: E402

# ... with the P.V path as an argument (pv_precision="fp8": both products on the FP8 matrix pipe): a package attribute too, not in __all__
from .varlen import fp8_attn_varlen_pv_func  # noqa: E402

# sliding-window (local) attention, packed and dense call shapes: package attributes too, not in __all__
from .varlen import fp8_attn_varlen_window_func, fp8_window_attn_func  # noqa: E402

# ... with the P.V path as an argument (pv_precision="fp8"): package attributes too, not in __all__
from .varlen import fp8_attn_varlen_window_pv_func, fp8_window_attn_pv_func  # noqa: E402

# block-sparse attention over 128 x 128 tiles of a boolean block mask: package attributes too, not in __all__
from .block_sparse import BLOCK_M, BLOCK_N, fp8_block_sparse_attn_func, fp8_block_sparse_attn_pv_func  # noqa: E402

# merging of attention states by their log-sum-exps, the dense fused step with its LSE, attention over several (k, v) sources: package
# attributes too, not in __all__
from .merge import fp8_attn_lse_func, fp8_attn_multi_kv_func, merge_attn_states  # noqa: E402

# rotary position embedding fused into the quant pre-pass of q and k (include/qattn_rope.h): package attributes too, not in __all__
from .rope import apply_rope_eager, fp8_attn_rope_func, rope_quantize_fp8  # noqa: E402

# split-KV attention of short queries over prepared (quantised once) K / V (include/qattn_splitkv.h): package attributes too, not in __all__
from .splitkv import PreparedKV, fp8_attn_splitkv_func, prepare_kv_fp8  # noqa: E402

# an appendable FP8 K/V cache with fixed scales for the split-KV entry (include/qattn_kvcache.h): package attributes too, not in __all__
from .kvcache import KVCacheFP8, alloc_kv_cache_fp8, kv_cache_append_fp8, kv_cache_from_prefill_fp8  # noqa: E402

# a paged FP8 K/V cache (a pool of pages behind a block table) for split-KV decode (include/qattn_paged.h): package attributes too, not in __all__
from .paged import PagedKVCacheFP8, alloc_paged_kv_cache_fp8, fp8_attn_paged_func, paged_kv_cache_append_fp8  # noqa: E402
# ... under PACKED queries, a different count per sequence slot (include/qattn_paged_varlen.h): a package attribute, not in __all__
from .paged_varlen import fp8_attn_paged_varlen_func  # noqa: E402
# ... and the append of PACKED tokens under the same cu_seqlens (include/qattn_paged_varlen_append.h): a package attribute, not in __all__
from .paged_varlen import paged_kv_cache_append_varlen_fp8  # noqa: E402
# ... and the same with the rotary embedding of K inside the append, and q's packed rotation at the same positions
# (include/qattn_paged_varlen_rope.h): package attributes, not in __all__
from .paged_varlen import apply_rope_paged_varlen, paged_kv_cache_append_varlen_rope_fp8  # noqa: E402
# ... and at the caller's positions (include/qattn_paged_varlen_rope_pos.h): package attributes, not in __all__
from .paged_varlen import apply_rope_positions, paged_kv_cache_append_varlen_rope_pos_fp8  # noqa: E402
# sliding windows for the split-KV, paged and packed-paged entries (include/qattn_splitkv_window.h): package attributes, not in __all__
from .splitkv_window import (  # noqa: E402
    fp8_attn_paged_varlen_window_func,
    fp8_attn_paged_window_func,
    fp8_attn_splitkv_window_func,
    paged_window_dead_pages,
)
# learned attention sinks for the three window entries and the state merge (include/qattn_sinks.h): package attributes, not in __all__
from .sinks import (  # noqa: E402
    fp8_attn_paged_sink_func,
    fp8_attn_paged_varlen_sink_func,
    fp8_attn_splitkv_sink_func,
    merge_attn_states_with_sinks,
)
# tree-shaped speculative decoding on the paged cache: the verify pass under a draft tree and the compaction of the accepted path
# (include/qattn_paged_varlen_tree.h): package attributes, not in __all__
from .tree import fp8_attn_paged_varlen_tree_func, paged_kv_cache_compact_fp8, tree_mask_from_parents  # noqa: E402
# ... on windowed layers and layers with learned sinks, and the drafts' rotary positions (include/qattn_paged_varlen_tree_window.h,
# include/qattn_paged_varlen_rope_pos.h): package attributes, not in __all__ (the reason functions stay in their modules, as the others)
from .tree import fp8_attn_paged_varlen_tree_window_func, tree_positions  # noqa: E402
# logit soft-capping for the three window entries (Gemma-2, Grok-1; include/qattn_softcap.h): package attributes, not in __all__
from .softcap import (  # noqa: E402
    fp8_attn_paged_softcap_func,
    fp8_attn_paged_varlen_softcap_func,
    fp8_attn_splitkv_softcap_func,
    softcap_input_reason,
)

__version__ = "0.1.0"

__all__ = [
    "attn_func",
    "attn_func_with_fallback",
    "dynamically_quantize_fp8",
    "fp8_attn_func",
    "fp8_attn_func_with_fallback",
    "fp8_token_wise_attn_func",
    "fp8_token_wise_attn_func_with_fallback",
]

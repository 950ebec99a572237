"""Sliding-window attention for the split-KV, cached and paged entries (include/qattn_splitkv_window.h):
`fp8_attn_splitkv_window_func`, `fp8_attn_paged_window_func`, `fp8_attn_paged_varlen_window_func` and `paged_window_dead_pages`.

Mistral, Gemma-2/3, gpt-oss and Phi-3 decode half or all of their layers under a sliding window; flash-attn's kv-cache entry and vLLM take
`window_size` next to `block_table` for it.  Each function here is its sibling without a window (`fp8_attn_splitkv_func`,
`fp8_attn_paged_func`, `fp8_attn_paged_varlen_func`) with `window_size = (left, right)` in `causal`'s place -- flash-attn's meaning,
include/qattn_window.h: each >= -1, -1 = unbounded; with Sq queries over L used keys, position p attends the keys j with
p + (L - Sq) - left <= j <= p + (L - Sq) + right.  (-1, 0) is causal=True, (-1, -1) is causal=False; vLLM's sliding_window = W is
(W - 1, 0).  A row whose window holds no key is a zero row with LSE -inf.

    out = fp8_attn_paged_window_func(q, cache, (4095, 0), max_seqlen_k=longest_live_sequence)          # decode under a 4096-key window
    dead = paged_window_dead_pages(cache.seqlens, 4095, cache.page_size)                                 # leading pages nobody reads again

The window kernels sweep -- and split -- only the keys a sequence's queries can attend: the split plan cuts [lo, L), lo =
max(L - Sq - left, 0), not [0, L) (`split_plan_window`), and no chunk and no block-table entry outside it is read.  They always run, also
for (-1, 0) and (-1, -1), where every output bit is the sibling's.

Package attributes, not names of `__all__`.  Learned attention sinks (gpt-oss): the siblings of `sinks.py`.  Not offered: "sink tokens +
window" in one call (two calls and `merge_attn_states`: INTEGRATION.md section 2e), windows on the 16-bit-P.V numerics."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native, nn
from .kvcache import _is_int
from .paged import PagedKVCacheFP8, _attend_eager, paged_attn_input_reason
from .paged_varlen import _attend_varlen_eager, paged_varlen_attn_input_reason
from .splitkv import _CPU_NUM_CUS, PreparedKV, _splitkv_eager, prepare_kv_fp8, split_plan_window, splitkv_input_reason  # noqa: F401
from .utils import checks
from .varlen import window_size_reason


def _check_common(precision, window_size) -> Tuple[int, int]:
    if precision not in ("accurate", "fast"):
        raise ValueError(f"Unsupported precision: {precision!r} (expected 'accurate' or 'fast'; 'auto' is not offered by the split-KV entries)")
    reason = window_size_reason(window_size)   # (always: the pair is unpacked below)
    if reason:
        raise ValueError(reason)
    return int(window_size[0]), int(window_size[1])


def _cus(device) -> int:
    return torch.cuda.get_device_properties(device).multi_processor_count if torch.device(device).type == "cuda" else _CPU_NUM_CUS


@torch.compiler.assume_constant_result
def _resolve_window_splits(num_splits: int, B: int, Hq: int, Hkv: int, Sq: int, Skv: int, D: int, window_left: int, device) -> int:
    """num_splits = 0 -> qattn_splitkv_window_auto_splits: the siblings' rule on min(Skv, left + Sq + 127) keys.  A pure function of host
    ints, so a trace-time constant."""
    return num_splits if num_splits else _native.splitkv_window_auto_splits(B, Hq, Hkv, Sq, Skv, D, window_left, _cus(device))


@torch.compiler.assume_constant_result
def _resolve_varlen_window_splits(num_splits: int, B: int, Hq: int, Hkv: int, total_q: int, max_seqlen_q: int, Skv: int, D: int,
                                  window_left: int, device) -> int:
    """... for packed queries: qattn_paged_varlen_window_auto_splits (max_seqlen_q stands for Sq)."""
    if num_splits:
        return num_splits
    return _native.paged_varlen_window_auto_splits(B, Hq, Hkv, total_q, max_seqlen_q, Skv, D, window_left, _cus(device))


def _result(out, lse, po, plse, ppath, return_lse, return_partials):
    res: Tuple = (out,)
    if return_lse:
        res += (lse,)
    if return_partials:
        res += (po, plse, ppath)
    return res if len(res) > 1 else out


def paged_window_dead_pages(seqlens: Tensor, window_left: int, page_size: int, *, num_queries: int = 1) -> Tensor:
    """int32 [B]: clamp(seqlens - num_queries - window_left, 0) // page_size -- the number of LEADING block-table entries of each slot that
    no window call with window_left and at most `num_queries` queries per slot reads, at the slot's current or any later length (a slot
    with L keys and Sq <= num_queries queries reads no key below L - Sq - window_left, and lengths only grow).  The caller's allocator may
    reuse those pages and leave -- or overwrite -- the entries.  A few torch ops on seqlens' device, no host synchronisation."""
    if not isinstance(seqlens, Tensor) or seqlens.dtype != torch.int32 or seqlens.dim() != 1:
        raise ValueError(f"Expected seqlens to be a 1-D torch.int32 tensor, but got {getattr(seqlens, 'dtype', type(seqlens))}")
    if not _is_int(window_left) or window_left < 0:
        raise ValueError(f"window_left must be an integer >= 0 (an unbounded window frees nothing), got {window_left!r}")
    if not _is_int(page_size) or page_size < 1:
        raise ValueError(f"page_size must be an integer >= 1, got {page_size!r}")
    if not _is_int(num_queries) or num_queries < 1:
        raise ValueError(f"num_queries must be an integer >= 1, got {num_queries!r}")
    below = (seqlens.to(torch.int64) - (num_queries + window_left)).clamp_min(0)
    return torch.div(below, page_size, rounding_mode="floor").to(torch.int32)


def fp8_attn_splitkv_window_func(q, kv, window_size, *, scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, num_splits: int = 0,
                                 precision: str = "accurate", return_lse: bool = False, return_partials: bool = False):
    """`fp8_attn_splitkv_func` under a sliding window: the same q, kv (a PreparedKV, a KVCacheFP8 or a (k, v) pair), seqused_k, scale,
    num_splits, precision ("auto" raises), outputs and partial shapes, with window_size = (left, right) in `causal`'s place (module
    docstring).  num_splits = 0 follows the window: the siblings' rule on min(Skv, left + Sq + 127) keys.  (-1, 0) / (-1, -1) give the bits
    of causal=True / False; with num_splits=1 and Hq = Hkv, out and lse are bit for bit those of `fp8_window_attn_pv_func(q, k, v,
    window_size, pv_precision="fp8", return_lse=True)`; out, lse = merge_attn_states(partials) bit for bit.  Keys outside the window of
    every query -- below max(L_b - Sq - left, 0) or at and beyond L_b -- influence no output bit, NaN bytes included.  Read on the
    device: no host synchronisation, graph-capture safe.  CPU tensors and config.attention.force_eager_fallback run the eager definition
    (`splitkv._splitkv_eager` with window=); on the device there is no fallback.  Unsupported input raises ValueError(reason)."""
    left, right = _check_common(precision, window_size)
    if isinstance(kv, (tuple, list)):
        if len(kv) != 2:
            raise ValueError("Expected kv to be a PreparedKV (prepare_kv_fp8) or a (key, value) pair")
        if isinstance(q, Tensor) and isinstance(kv[0], Tensor) and kv[0].device != q.device:
            raise ValueError(f"Expected query, key, and value to be on the same device, but got {q.device} and {kv[0].device} instead.")
        kv = prepare_kv_fp8(kv[0], kv[1])
    if not checks.config_value("attention.skip_supported_check"):
        reason = splitkv_input_reason(q, kv, seqused_k, scale, num_splits)
        if reason:
            raise ValueError(reason)
    B, Hq, Sq, D = q.shape
    _, Hkv, Skv, _ = kv.shape
    ns = _resolve_window_splits(num_splits, B, Hq, Hkv, Sq, Skv, D, left, q.device)
    eager = (not q.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if kv.layout != "rowmajor":
            raise ValueError("the eager definition needs a PreparedKV made on CPU tensors or under config.attention.force_eager_fallback")
        res = _splitkv_eager(q, kv, False, scale, seqused_k, ns, precision, window=(left, right))
    else:
        if kv.layout != "frag":
            raise ValueError("this PreparedKV holds row-major bytes for the eager definition; prepare it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        res = nn._ops().fp8_splitkv_window_attention_forward(
            q.contiguous(), kv.k, kv.v, kv.scale_k, kv.scale_v, seqused_k, Skv, ns, left, right, kv.fp8_format, kv.numerics, precision,
            bool(return_lse), bool(return_partials), scale=scale)
    return _result(*res, return_lse, return_partials)


def fp8_attn_paged_window_func(q, cache: PagedKVCacheFP8, window_size, *, scale: Optional[float] = None, seqused_k: Optional[Tensor] = None,
                               max_seqlen_k: Optional[int] = None, num_splits: int = 0, precision: str = "accurate", return_lse: bool = False,
                               return_partials: bool = False):
    """`fp8_attn_paged_func` under a sliding window: the arguments, outputs and BITS of `fp8_attn_splitkv_window_func` on the cache gathered
    through the block table.  Of slot b's table only the entries from max(L_b - Sq - left, 0) // page_size up to
    ceil(L_b / page_size) - 1 are read, each clamped into the pool before it forms an address: the leading
    `paged_window_dead_pages(...)` entries may hold anything and their pages may belong to someone else.  Table and lengths are read on
    the device: a captured call follows the window as seqlens advance.  CPU tensors and config.attention.force_eager_fallback run the
    eager definition (`paged._attend_eager` with window=).  Unsupported input raises ValueError(reason)."""
    left, right = _check_common(precision, window_size)
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_attn_input_reason(q, cache, seqused_k, scale, num_splits, max_seqlen_k)
        if reason:
            raise ValueError(reason)
    B, Hq, Sq, D = q.shape
    Hkv = cache.shape[1]
    Skv = cache.capacity if max_seqlen_k is None else int(max_seqlen_k)
    used = cache.seqlens if seqused_k is None else seqused_k
    ns = _resolve_window_splits(num_splits, B, Hq, Hkv, Sq, Skv, D, left, q.device)
    eager = (not q.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if cache.layout != "rowmajor":
            raise ValueError("the eager definition needs a cache made on a CPU device or under config.attention.force_eager_fallback")
        res = _attend_eager(q, cache, False, scale, used, Skv, ns, precision, window=(left, right))
    else:
        if cache.layout != "frag":
            raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        res = nn._ops().fp8_paged_splitkv_window_attention_forward(
            q.contiguous(), cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, used, Skv, cache.num_pages, cache.page_size, ns,
            left, right, cache.fp8_format, cache.numerics, precision, bool(return_lse), bool(return_partials), scale=scale)
    return _result(*res, return_lse, return_partials)


def fp8_attn_paged_varlen_window_func(q, cache: PagedKVCacheFP8, cu_seqlens_q: Tensor, max_seqlen_q: int, window_size, *,
                                      scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None,
                                      num_splits: int = 0, precision: str = "accurate", return_lse: bool = False,
                                      return_partials: bool = False):
    """`fp8_attn_paged_varlen_func` under a sliding window PER SEQUENCE: slot b with Sq_b queries and L_b keys attends, at position p, the
    keys p + (L_b - Sq_b) - left .. p + (L_b - Sq_b) + right.  Shapes and layouts are the sibling's (lse [Hq, total_q]); for every slot with
    queries the rows are, bit for bit, `fp8_attn_paged_window_func` on that slot alone.  max_seqlen_q is read by the num_splits = 0 rule
    only.  CPU tensors and config.attention.force_eager_fallback run the eager definition (`paged_varlen._attend_varlen_eager` with
    window=).  Unsupported input raises ValueError(reason)."""
    left, right = _check_common(precision, window_size)
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_varlen_attn_input_reason(q, cache, cu_seqlens_q, max_seqlen_q, seqused_k, scale, num_splits, max_seqlen_k)
        if reason:
            raise ValueError(reason)
    total_q, Hq, D = q.shape
    B, Hkv = cache.batch_size, cache.shape[1]
    Skv = cache.capacity if max_seqlen_k is None else int(max_seqlen_k)
    used = cache.seqlens if seqused_k is None else seqused_k
    ns = _resolve_varlen_window_splits(num_splits, B, Hq, Hkv, total_q, int(max_seqlen_q), Skv, D, left, q.device)
    eager = (not q.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if cache.layout != "rowmajor":
            raise ValueError("the eager definition needs a cache made on a CPU device or under config.attention.force_eager_fallback")
        res = _attend_varlen_eager(q, cache, cu_seqlens_q, False, scale, used, Skv, ns, precision, window=(left, right))
    else:
        if cache.layout != "frag":
            raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        res = nn._ops().fp8_paged_varlen_splitkv_window_attention_forward(
            q, cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, used, cu_seqlens_q, int(max_seqlen_q), Skv, cache.num_pages,
            cache.page_size, ns, left, right, cache.fp8_format, cache.numerics, precision, bool(return_lse), bool(return_partials), scale=scale)
    return _result(*res, return_lse, return_partials)

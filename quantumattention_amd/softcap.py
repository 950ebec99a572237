"""Logit soft-capping for the split-KV, cached and paged window entries (include/qattn_softcap.h):
`fp8_attn_splitkv_softcap_func`, `fp8_attn_paged_softcap_func` and `fp8_attn_paged_varlen_softcap_func`.

Every Gemma-2 attention layer computes softmax(cap tanh(scale q.k / cap)) with cap = attn_logit_softcapping = 50, on its 4096-key window
layers and its full layers alike; Grok-1 caps at 30.  flash-attn and vLLM pass it as `softcap=`.  Each function here is its sibling of
`splitkv_window.py` with `softcap` before `window_size`: a host float.  For a row with scaled scores x_j over the keys j its window admits:

    y_j = softcap * tanh(x_j / softcap),    L = log(sum_j exp(y_j)),    out = sum_j exp(y_j - L) v_j

    scale = query_pre_attn_scalar ** -0.5
    out = fp8_attn_paged_softcap_func(q, cache, 50.0, (4095, 0), scale=scale, max_seqlen_k=longest_live_sequence)   # a Gemma-2 window layer
    out = fp8_attn_paged_softcap_func(q, cache, 50.0, scale=scale, max_seqlen_k=longest_live_sequence)              # a full layer: (-1, 0)

The cap is applied BEFORE the mask: a masked key weighs exactly 0, and key bytes outside the window or behind seqused_k influence no
output bit.  The returned LSE is L of the capped scores; `return_partials` returns ordinary attention states over capped scores, and
out, lse = merge_attn_states(list(partial_o), list(partial_lse), out_dtype=q.dtype), bit for bit.  A row without a key is a zero row with
lse = -inf.  softcap == 0.0 is flash-attn's "off": the call is forwarded to the window sibling, bit for bit.  A negative, NaN or infinite
softcap raises ValueError.  Under precision="fast" the soft-cap entries take the exact one-term sweep where the sibling would take the
byte-exponential one: their bits are those of themselves called with return_lse=True.  softcap is a kernel ARGUMENT, a model constant:
a captured graph -- and a torch.compile trace -- keeps the value it was captured with; seqlens, the table and cu_seqlens_q are still read
on the device and followed.

Package attributes, not names of `__all__`.  Not offered: a soft cap with sinks or under a draft tree, on the dense, packed 16-bit and
block-sparse entries, ALiBi, a device-side softcap tensor, precision="auto"."""
import math
from typing import Optional

import torch
from torch import Tensor

from . import nn
from .paged import PagedKVCacheFP8, _attend_eager, paged_attn_input_reason
from .paged_varlen import _attend_varlen_eager, paged_varlen_attn_input_reason
from .splitkv import _splitkv_eager, prepare_kv_fp8, splitkv_input_reason
from .splitkv_window import (_check_common, _resolve_varlen_window_splits, _resolve_window_splits, _result, fp8_attn_paged_varlen_window_func,
                             fp8_attn_paged_window_func, fp8_attn_splitkv_window_func)
from .utils import checks


def softcap_input_reason(softcap) -> Optional[str]:
    """Why `softcap` cannot be a soft cap (None: it can).  0.0 is accepted: flash-attn's "no cap"."""
    if isinstance(softcap, bool) or not isinstance(softcap, (int, float)):
        return f"Expected softcap to be a host float (a model constant), but got {type(softcap).__name__}"
    if math.isnan(softcap):
        return "Expected softcap to be a finite float >= 0 (0.0: no cap), but got NaN"
    if math.isinf(softcap):
        return f"Expected softcap to be a finite float >= 0 (0.0: no cap), but got {softcap}"
    if softcap < 0:
        return f"Expected softcap to be a finite float >= 0 (0.0: no cap), but got a negative value: {softcap}"
    if float(softcap) > torch.finfo(torch.float32).max:
        return f"Expected softcap to be finite as a float32, but got {softcap}"
    return None


def _checked_softcap(softcap) -> float:
    reason = softcap_input_reason(softcap)
    if reason:
        raise ValueError(reason)
    return float(softcap)


def fp8_attn_splitkv_softcap_func(q, kv, softcap, window_size=(-1, 0), *, scale: Optional[float] = None, seqused_k: Optional[Tensor] = None,
                                  num_splits: int = 0, precision: str = "accurate", return_lse: bool = False, return_partials: bool = False):
    """`fp8_attn_splitkv_window_func` with soft-capped scores (module docstring): the same q, kv (a PreparedKV, a KVCacheFP8 or a (k, v)
    pair), window_size (default (-1, 0): causal), seqused_k, scale, num_splits, precision ("auto" raises), outputs and partial shapes;
    softcap a host float, 0.0 = the sibling itself.  CPU tensors and config.attention.force_eager_fallback run the eager definition
    (`splitkv._splitkv_eager` with softcap=); on the device there is no fallback.  Unsupported input raises ValueError(reason)."""
    cap = _checked_softcap(softcap)
    if cap == 0.0:
        return fp8_attn_splitkv_window_func(q, kv, window_size, scale=scale, seqused_k=seqused_k, num_splits=num_splits, precision=precision,
                                            return_lse=return_lse, return_partials=return_partials)
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
        res = _splitkv_eager(q, kv, False, scale, seqused_k, ns, precision, softcap=cap, window=(left, right))
    else:
        if kv.layout != "frag":
            raise ValueError("this PreparedKV holds row-major bytes for the eager definition; prepare it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        res = nn._ops().fp8_splitkv_softcap_attention_forward(
            q.contiguous(), kv.k, kv.v, kv.scale_k, kv.scale_v, seqused_k, Skv, ns, left, right, cap, kv.fp8_format, kv.numerics, precision,
            bool(return_lse), bool(return_partials), scale=scale)
    return _result(*res, return_lse, return_partials)


def fp8_attn_paged_softcap_func(q, cache: PagedKVCacheFP8, softcap, window_size=(-1, 0), *, scale: Optional[float] = None,
                                seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, num_splits: int = 0,
                                precision: str = "accurate", return_lse: bool = False, return_partials: bool = False):
    """`fp8_attn_paged_window_func` with soft-capped scores: the arguments, outputs and BITS of `fp8_attn_splitkv_softcap_func` on the
    cache gathered through the block table; the table reads are the window sibling's.  Table and lengths are read on the device and a
    captured call follows them; softcap is baked into the capture.  CPU tensors and config.attention.force_eager_fallback run the eager
    definition (`paged._attend_eager` with softcap=).  Unsupported input raises ValueError(reason)."""
    cap = _checked_softcap(softcap)
    if cap == 0.0:
        return fp8_attn_paged_window_func(q, cache, window_size, scale=scale, seqused_k=seqused_k, max_seqlen_k=max_seqlen_k,
                                          num_splits=num_splits, precision=precision, return_lse=return_lse, return_partials=return_partials)
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
        res = _attend_eager(q, cache, False, scale, used, Skv, ns, precision, softcap=cap, window=(left, right))
    else:
        if cache.layout != "frag":
            raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        res = nn._ops().fp8_paged_splitkv_softcap_attention_forward(
            q.contiguous(), cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, used, Skv, cache.num_pages, cache.page_size, ns,
            left, right, cap, cache.fp8_format, cache.numerics, precision, bool(return_lse), bool(return_partials), scale=scale)
    return _result(*res, return_lse, return_partials)


def fp8_attn_paged_varlen_softcap_func(q, cache: PagedKVCacheFP8, cu_seqlens_q: Tensor, max_seqlen_q: int, softcap, window_size=(-1, 0), *,
                                       scale: Optional[float] = None, seqused_k: Optional[Tensor] = None,
                                       max_seqlen_k: Optional[int] = None, num_splits: int = 0, precision: str = "accurate",
                                       return_lse: bool = False, return_partials: bool = False):
    """`fp8_attn_paged_varlen_window_func` with soft-capped scores: packed queries, a window per sequence.  Shapes and layouts are the
    sibling's (lse [Hq, total_q]); for every slot with queries the rows are, bit for bit, `fp8_attn_paged_softcap_func` on that slot
    alone.  CPU tensors and config.attention.force_eager_fallback run the eager definition (`paged_varlen._attend_varlen_eager` with
    softcap=).  Unsupported input raises ValueError(reason)."""
    cap = _checked_softcap(softcap)
    if cap == 0.0:
        return fp8_attn_paged_varlen_window_func(q, cache, cu_seqlens_q, max_seqlen_q, window_size, scale=scale, seqused_k=seqused_k,
                                                 max_seqlen_k=max_seqlen_k, num_splits=num_splits, precision=precision,
                                                 return_lse=return_lse, return_partials=return_partials)
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
        res = _attend_varlen_eager(q, cache, cu_seqlens_q, False, scale, used, Skv, ns, precision, softcap=cap, window=(left, right))
    else:
        if cache.layout != "frag":
            raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        res = nn._ops().fp8_paged_varlen_splitkv_softcap_attention_forward(
            q, cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, used, cu_seqlens_q, int(max_seqlen_q), Skv, cache.num_pages,
            cache.page_size, ns, left, right, cap, cache.fp8_format, cache.numerics, precision, bool(return_lse), bool(return_partials),
            scale=scale)
    return _result(*res, return_lse, return_partials)

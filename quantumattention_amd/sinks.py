"""Learned attention sinks for the split-KV, cached and paged window entries (include/qattn_sinks.h):
`fp8_attn_splitkv_sink_func`, `fp8_attn_paged_sink_func`, `fp8_attn_paged_varlen_sink_func` and `merge_attn_states_with_sinks`.

Every gpt-oss attention layer, windowed (128 keys) and full alike, adds a learned per-head logit to the softmax denominator; vLLM passes
it as `sinks=`, flash-attn 3 as `s_aux`.  Each function here is its sibling of `splitkv_window.py` with `sinks` before `window_size`:
fp32 / bf16 / fp16 [Hq] on q's device, one logit per QUERY head in the units of the scaled scores (natural log; `scale` applies to the
scores, not to the sink).  For a row of head h with attended keys j and scores x_j:

    L = log(exp(sink_h) + sum_j exp(x_j)),    out = sum_j exp(x_j - L) v_j

    out = fp8_attn_paged_sink_func(q, cache, sinks, (127, 0), max_seqlen_k=longest_live_sequence)     # a gpt-oss window layer
    out = fp8_attn_paged_sink_func(q, cache, sinks)                                                   # a gpt-oss full layer: (-1, 0)

The returned LSE is L, sink included -- do not merge such a state with another one that also counted the sink.  A row without a key is
a zero row with lse = sink_h.  sink_h = -inf is no sink for that head: with every sink -inf the bits are the window sibling's (under
precision="fast" those of the sibling called with return_lse=True: the sink entries never take the byte-exponential sweep).  +inf or
NaN makes the head's rows NaN.  `return_partials` returns the SINK-FREE partials -- bit for bit the sibling's -- and
out, lse = merge_attn_states_with_sinks(list(partial_o), list(partial_lse), sinks, out_dtype=q.dtype), bit for bit.  sinks is read on
the device alone: no host synchronisation, graph-capture safe, and a captured call follows rewritten sink values.

Package attributes, not names of `__all__`.  Not offered: sinks on the dense, packed 16-bit and block-sparse entries, "sink tokens +
window" in one call, sink gradients, precision="auto"."""
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _native, nn
from .merge import _MERGE_HEAD_DIMS, _check_states, merge_attn_states_eager
from .nn import _cfg
from .paged import PagedKVCacheFP8, _attend_eager, paged_attn_input_reason
from .paged_varlen import _attend_varlen_eager, paged_varlen_attn_input_reason
from .splitkv import _splitkv_eager, prepare_kv_fp8, splitkv_input_reason
from .splitkv_window import _check_common, _resolve_varlen_window_splits, _resolve_window_splits, _result
from .utils import checks

_SINK_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def sinks_input_reason(sinks, num_heads: int, device) -> Optional[str]:
    """Why `sinks` cannot be the sink logits of `num_heads` query heads on `device` (None: it can)."""
    if not isinstance(sinks, Tensor):
        return f"Expected sinks to be a tensor [Hq] of one logit per query head, but got {type(sinks).__name__}"
    if sinks.dtype not in _SINK_DTYPES:
        return f"Expected sinks to have dtype torch.float32, torch.bfloat16 or torch.float16, but got sinks.dtype: {sinks.dtype} instead."
    if tuple(sinks.shape) != (num_heads,):
        return f"Expected sinks to have shape [{num_heads}] (one logit per query head), but got {list(sinks.shape)}."
    if sinks.device != torch.device(device):
        return f"Expected sinks to be on {device}, but got {sinks.device} instead."
    if sinks.requires_grad:
        return "NYI: sinks must not require grad (no backward)"
    return None


def _sinks_f32(sinks, num_heads: int, device) -> Tensor:
    """The checked sinks as the kernels take them: dense fp32 (16-bit sinks are up-cast: exact)."""
    reason = sinks_input_reason(sinks, num_heads, device)
    if reason:
        raise ValueError(reason)
    return sinks.to(torch.float32).contiguous()


def fp8_attn_splitkv_sink_func(q, kv, sinks, window_size=(-1, 0), *, scale: Optional[float] = None, seqused_k: Optional[Tensor] = None,
                               num_splits: int = 0, precision: str = "accurate", return_lse: bool = False, return_partials: bool = False):
    """`fp8_attn_splitkv_window_func` with learned sinks (module docstring): the same q, kv (a PreparedKV, a KVCacheFP8 or a (k, v) pair),
    window_size (default (-1, 0): causal), seqused_k, scale, num_splits, precision ("auto" raises), outputs and partial shapes; sinks
    [Hq].  With one split the sink is folded into the sweep kernel's epilogue -- no extra launch, one rounding of out --, with more it
    enters the last launch of the merge chain once.  CPU tensors and config.attention.force_eager_fallback run the eager definition
    (`splitkv._splitkv_eager` with sinks=); on the device there is no fallback.  Unsupported input raises ValueError(reason)."""
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
    sinks = _sinks_f32(sinks, Hq, q.device)
    ns = _resolve_window_splits(num_splits, B, Hq, Hkv, Sq, Skv, D, left, q.device)
    eager = (not q.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if kv.layout != "rowmajor":
            raise ValueError("the eager definition needs a PreparedKV made on CPU tensors or under config.attention.force_eager_fallback")
        res = _splitkv_eager(q, kv, False, scale, seqused_k, ns, precision, sinks=sinks, window=(left, right))
    else:
        if kv.layout != "frag":
            raise ValueError("this PreparedKV holds row-major bytes for the eager definition; prepare it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        res = nn._ops().fp8_splitkv_sink_attention_forward(
            q.contiguous(), kv.k, kv.v, kv.scale_k, kv.scale_v, seqused_k, Skv, ns, left, right, sinks, kv.fp8_format, kv.numerics, precision,
            bool(return_lse), bool(return_partials), scale=scale)
    return _result(*res, return_lse, return_partials)


def fp8_attn_paged_sink_func(q, cache: PagedKVCacheFP8, sinks, window_size=(-1, 0), *, scale: Optional[float] = None,
                             seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, num_splits: int = 0,
                             precision: str = "accurate", return_lse: bool = False, return_partials: bool = False):
    """`fp8_attn_paged_window_func` with learned sinks: the arguments, outputs and BITS of `fp8_attn_splitkv_sink_func` on the cache
    gathered through the block table; the table reads are the window sibling's.  Table, lengths and sinks are read on the device: a
    captured call follows all three.  CPU tensors and config.attention.force_eager_fallback run the eager definition
    (`paged._attend_eager` with sinks=).  Unsupported input raises ValueError(reason)."""
    left, right = _check_common(precision, window_size)
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_attn_input_reason(q, cache, seqused_k, scale, num_splits, max_seqlen_k)
        if reason:
            raise ValueError(reason)
    B, Hq, Sq, D = q.shape
    Hkv = cache.shape[1]
    sinks = _sinks_f32(sinks, Hq, q.device)
    Skv = cache.capacity if max_seqlen_k is None else int(max_seqlen_k)
    used = cache.seqlens if seqused_k is None else seqused_k
    ns = _resolve_window_splits(num_splits, B, Hq, Hkv, Sq, Skv, D, left, q.device)
    eager = (not q.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if cache.layout != "rowmajor":
            raise ValueError("the eager definition needs a cache made on a CPU device or under config.attention.force_eager_fallback")
        res = _attend_eager(q, cache, False, scale, used, Skv, ns, precision, sinks=sinks, window=(left, right))
    else:
        if cache.layout != "frag":
            raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        res = nn._ops().fp8_paged_splitkv_sink_attention_forward(
            q.contiguous(), cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, used, Skv, cache.num_pages, cache.page_size, ns,
            left, right, sinks, cache.fp8_format, cache.numerics, precision, bool(return_lse), bool(return_partials), scale=scale)
    return _result(*res, return_lse, return_partials)


def fp8_attn_paged_varlen_sink_func(q, cache: PagedKVCacheFP8, cu_seqlens_q: Tensor, max_seqlen_q: int, sinks, window_size=(-1, 0), *,
                                    scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None,
                                    num_splits: int = 0, precision: str = "accurate", return_lse: bool = False,
                                    return_partials: bool = False):
    """`fp8_attn_paged_varlen_window_func` with learned sinks: packed queries, a window per sequence, the sink of a row its HEAD's.  Shapes
    and layouts are the sibling's (lse [Hq, total_q]); for every slot with queries the rows are, bit for bit, `fp8_attn_paged_sink_func`
    on that slot alone.  CPU tensors and config.attention.force_eager_fallback run the eager definition
    (`paged_varlen._attend_varlen_eager` with sinks=).  Unsupported input raises ValueError(reason)."""
    left, right = _check_common(precision, window_size)
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_varlen_attn_input_reason(q, cache, cu_seqlens_q, max_seqlen_q, seqused_k, scale, num_splits, max_seqlen_k)
        if reason:
            raise ValueError(reason)
    total_q, Hq, D = q.shape
    B, Hkv = cache.batch_size, cache.shape[1]
    sinks = _sinks_f32(sinks, Hq, q.device)
    Skv = cache.capacity if max_seqlen_k is None else int(max_seqlen_k)
    used = cache.seqlens if seqused_k is None else seqused_k
    ns = _resolve_varlen_window_splits(num_splits, B, Hq, Hkv, total_q, int(max_seqlen_q), Skv, D, left, q.device)
    eager = (not q.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if cache.layout != "rowmajor":
            raise ValueError("the eager definition needs a cache made on a CPU device or under config.attention.force_eager_fallback")
        res = _attend_varlen_eager(q, cache, cu_seqlens_q, False, scale, used, Skv, ns, precision, sinks=sinks, window=(left, right))
    else:
        if cache.layout != "frag":
            raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        res = nn._ops().fp8_paged_varlen_splitkv_sink_attention_forward(
            q, cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, used, cu_seqlens_q, int(max_seqlen_q), Skv, cache.num_pages,
            cache.page_size, ns, left, right, sinks, cache.fp8_format, cache.numerics, precision, bool(return_lse), bool(return_partials),
            scale=scale)
    return _result(*res, return_lse, return_partials)


def merge_attn_states_with_sinks(outs: Sequence[Tensor], lses: Sequence[Tensor], sinks: Tensor, *, out_dtype: Optional[torch.dtype] = None,
                                 return_lse: bool = True):
    """`merge_attn_states` of N >= 1 SINK-FREE states with the learned sink of every head as one more state: lse = sink_h, no O row.

    outs / lses: as `merge_attn_states` (dense [B, H, S, D] / [B, H, S] or packed [total, H, D] / [H, total]); sinks [H], fp32 / bf16 /
    fp16 on the states' device.  out = (sum_i e_i O_i) / (sum_i e_i + exp(sink_h - m)) with m = max(max_i lse_i, sink_h); lse = m + log of
    the denominator -- the sink counted, so the result does not merge with sinks again.  A row whose states are all at -inf is a zero row
    with lse = sink_h.  More than 8 states are chained as `merge_attn_states` chains them and the sink enters the LAST launch only: the
    partials of a sink entry give its out and lse bit for bit.  CPU tensors and config.attention.force_eager_fallback run
    `merge_attn_states_eager` with sinks=.  Returns (out, lse), or out with return_lse=False."""
    _check_states(outs, lses, out_dtype, False)
    outs, lses = list(outs), list(lses)
    packed = lses[0].dim() == 2
    sinks = _sinks_f32(sinks, lses[0].shape[0 if packed else 1], outs[0].device)
    n = len(outs)
    want = out_dtype or outs[0].dtype
    if not outs[0].is_cuda or _cfg("force_eager_fallback"):
        out, lse = merge_attn_states_eager(outs, lses, want, sinks=sinks)
        return (out, lse) if return_lse else out
    if outs[0].shape[-1] not in _MERGE_HEAD_DIMS:
        raise ValueError(f"head_dim must be one of {list(_MERGE_HEAD_DIMS)} for the gfx950 merge kernel, got {outs[0].shape[-1]}")
    ops = nn._ops()
    top = _native.MERGE_MAX_PARTIALS
    if n <= top:
        out, lse = ops.attention_state_merge_sink(outs, lses, sinks, want)
        return (out, lse) if return_lse else out
    # the chain of merge_attn_states -- 8 states into an fp32 accumulator, 7 more per launch in place -- with the sink in the last launch
    acc, acc_lse = ops.attention_state_merge(outs[:top], lses[:top], torch.float32)
    done = top
    while n - done > top - 1:
        ops.attention_state_merge_(acc, acc_lse, outs[done:done + top - 1], lses[done:done + top - 1])
        done += top - 1
    out, lse = ops.attention_state_merge_sink([acc] + outs[done:], [acc_lse] + lses[done:], sinks, want)
    return (out, lse) if return_lse else out

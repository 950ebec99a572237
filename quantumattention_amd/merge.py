"""Merging of attention states, and what it makes possible without a concatenation: attention over K / V that arrive in pieces.

A partial attention result over a key set comes with the natural log-sum-exp of its rows; partial results over DISJOINT key sets combine
exactly (include/qattn_merge.h):

    O = sum_i exp(lse_i - L) O_i,    L = log sum_i exp(lse_i).

`merge_attn_states` is that step (one HIP launch per 8 states), `fp8_attn_lse_func` the dense fused step with its LSE, and
`fp8_attn_multi_kv_func` attention of one query over several (k, v) sources.  Package attributes, not names of `__all__` (that list
mirrors the reference)."""
import math
from typing import Optional, Sequence, Tuple

import torch

from . import _native, nn
from .nn import _cfg

_STATE_DTYPES = (torch.bfloat16, torch.float16, torch.float32)
_MERGE_HEAD_DIMS = (64, 128, 256)


def sink_or_nan(sinks: torch.Tensor) -> torch.Tensor:
    """fp32 sinks with +inf replaced by NaN: a sink of +inf or NaN makes its head's rows NaN (include/qattn_sinks.h)."""
    s = sinks.to(torch.float32)
    return torch.where(s < math.inf, s, torch.full_like(s, math.nan))


def merge_attn_states_eager(outs: Sequence[torch.Tensor], lses: Sequence[torch.Tensor], out_dtype: Optional[torch.dtype] = None, *,
                            sinks: Optional[torch.Tensor] = None):
    """The merge in torch ops on the tensors' device: the definition the HIP kernel implements and the reference implementation of the op
    `quantumattention_amd::attention_state_merge` -- fp32, m = max_i lse_i, e_i = exp(lse_i - m), partials summed in index order, one
    rounding to out_dtype.  A partial of weight zero (lse_i = -inf) contributes nothing whatever its rows hold; rows whose partials are
    all at -inf are zero rows with an LSE of -inf; an LSE of +inf or NaN makes the row NaN.  Returns (out, lse), both dense.
    sinks (fp32 [H], None: none): the definition of `quantumattention_amd::attention_state_merge_sink` (include/qattn_sinks.h) -- the
    head's sink is one more state with LSE sink_h and no O row: it joins m, is summed into den after the partials, and a row whose
    partials are all at -inf is a zero row with LSE sink_h."""
    packed = lses[0].dim() == 2
    L = torch.stack([l.to(torch.float32) for l in lses])
    m = L.max(dim=0).values                                   # (propagates NaN)
    if sinks is not None:
        snk = sink_or_nan(sinks)[:, None] if packed else sink_or_nan(sinks)[None, :, None]
        m = torch.where((snk > m) | (snk != snk), snk.expand_as(m), m)
    empty = m == -math.inf
    e = torch.exp(L - torch.where(empty, torch.zeros_like(m), m))   # an empty row: exp(-inf - 0) = 0 for every partial
    den = e[0].clone()
    for i in range(1, len(lses)):
        den = den + e[i]
    if sinks is not None:
        den = den + torch.exp(snk - torch.where(empty, torch.zeros_like(m), m))
    rows = (lambda w: w.transpose(0, 1)[..., None]) if packed else (lambda w: w[..., None])   # a per-row figure over the rows of O
    acc = None
    for i, o in enumerate(outs):
        w = rows(e[i])
        term = w * torch.where(w != 0, o.to(torch.float32), torch.zeros((), dtype=torch.float32, device=o.device))
        acc = term if acc is None else acc + term
    out = torch.where(rows(empty), torch.zeros_like(acc), acc * (1.0 / rows(den)))
    lse = torch.where(empty, m, m + torch.log(den))
    return out.to(out_dtype or outs[0].dtype).contiguous(), lse.contiguous()


def _check_states(outs, lses, out_dtype, inplace):
    if not isinstance(outs, (list, tuple)) or not isinstance(lses, (list, tuple)):
        raise TypeError("outs and lses must be sequences (list or tuple) of tensors")
    if len(outs) != len(lses) or len(outs) < 1:
        raise ValueError(f"outs and lses must be sequences of the same length >= 1, got {len(outs)} and {len(lses)}")
    if not all(isinstance(t, torch.Tensor) for t in tuple(outs) + tuple(lses)):
        raise TypeError("outs and lses must hold tensors")
    o0, l0 = outs[0], lses[0]
    if l0.dim() not in (2, 3):
        raise ValueError(f"an LSE must be [B, H, S] (dense) or [H, total] (packed), got {l0.dim()} dimensions")
    packed = l0.dim() == 2
    for i, (o, l) in enumerate(zip(outs, lses)):
        if l.dim() != l0.dim():
            raise ValueError(f"state {i} mixes the dense [B,H,S,D] / [B,H,S] and the packed [total,H,D] / [H,total] conventions with state 0")
        if o.dim() != l.dim() + 1:
            raise ValueError(f"state {i}: out has {o.dim()} dimensions and lse {l.dim()}; expected [B,H,S,D] / [B,H,S] or [total,H,D] / [H,total]")
        want = (o.shape[1], o.shape[0]) if packed else tuple(o.shape[:3])
        if tuple(o.shape) != tuple(o0.shape) or tuple(l.shape) != want:
            raise ValueError(f"state {i}: out {tuple(o.shape)} / lse {tuple(l.shape)} do not match state 0's {tuple(o0.shape)} / {tuple(l0.shape)}")
        if o.dtype not in _STATE_DTYPES:
            raise ValueError(f"state {i}: out must be bf16, fp16 or fp32, got {o.dtype}")
        if l.dtype != torch.float32:
            raise ValueError(f"state {i}: lse must be float32 (the natural log-sum-exp the attention entries return), got {l.dtype}")
        if o.device != o0.device or l.device != o0.device:
            raise ValueError(f"state {i} is not on state 0's device {o0.device}")
    if out_dtype is not None and out_dtype not in _STATE_DTYPES:
        raise ValueError(f"out_dtype must be bf16, fp16 or fp32, got {out_dtype}")
    if inplace and out_dtype is not None and out_dtype != o0.dtype:
        raise ValueError(f"inplace=True writes into outs[0] ({o0.dtype}): out_dtype {out_dtype} cannot be honoured")


def merge_attn_states(outs: Sequence[torch.Tensor], lses: Sequence[torch.Tensor], *, out_dtype: Optional[torch.dtype] = None,
                      return_lse: bool = True, inplace: bool = False):
    """Merge N >= 1 attention states (outs[i], lses[i]) -- partial results of the SAME queries over DISJOINT key sets, as every entry of
    this library returns them with return_lse=True -- into the state over the union of the keys.

    outs[i] [B, H, S, D] with lses[i] fp32 [B, H, S] (dense), or [total, H, D] with [H, total] (packed); the convention is read off
    lses[0].dim() and a mix is refused.  bf16 / fp16 / fp32, each state its own; views (the permuted ones fp8_window_attn_func returns,
    padded LSE rows, an fp32 accumulator next to 16-bit partials) go to the kernel through their strides, without a copy.
    out_dtype: format of the result (default: outs[0]'s).  inplace=True: the result is written into outs[0] / lses[0] (the accumulate of a
    ring step) and those are returned.  Returns (out, lse), or out with return_lse=False.

    lses[i] = -inf marks rows for which partial i attended no key (the zero rows of the window and block-sparse entries): the partial
    contributes nothing there, whatever its rows hold; rows empty in every partial stay zero rows with LSE -inf.
    One launch merges up to 8 states; more are chained 8 at a time through an fp32 accumulator.  N = 1 returns its input (converted when
    out_dtype differs).  CPU tensors and config.attention.force_eager_fallback run `merge_attn_states_eager`; on the device there is no
    fallback: head_dim must be 64, 128 or 256."""
    _check_states(outs, lses, out_dtype, inplace)
    outs, lses = list(outs), list(lses)
    n = len(outs)
    if n == 1:
        out = outs[0] if out_dtype in (None, outs[0].dtype) else outs[0].to(out_dtype)
        return (out, lses[0]) if return_lse else out
    want = out_dtype or outs[0].dtype
    if not outs[0].is_cuda or _cfg("force_eager_fallback"):
        out, lse = merge_attn_states_eager(outs, lses, want)
        if inplace:
            outs[0].copy_(out)
            lses[0].copy_(lse)
            out, lse = outs[0], lses[0]
        return (out, lse) if return_lse else out
    if outs[0].shape[-1] not in _MERGE_HEAD_DIMS:
        raise ValueError(f"head_dim must be one of {list(_MERGE_HEAD_DIMS)} for the gfx950 merge kernel, got {outs[0].shape[-1]}")
    ops = nn._ops()
    top = _native.MERGE_MAX_PARTIALS
    if n <= top:
        if inplace:
            ops.attention_state_merge_(outs[0], lses[0], outs[1:], lses[1:])
            out, lse = outs[0], lses[0]
        else:
            out, lse = ops.attention_state_merge(outs, lses, want)
        return (out, lse) if return_lse else out
    # more than one launch: the first 8 states into an fp32 accumulator, then 7 more per launch in place; the last launch rounds once
    acc, acc_lse = ops.attention_state_merge(outs[:top], lses[:top], torch.float32)
    done = top
    while n - done > top - 1:
        ops.attention_state_merge_(acc, acc_lse, outs[done:done + top - 1], lses[done:done + top - 1])
        done += top - 1
    out, lse = ops.attention_state_merge([acc] + outs[done:], [acc_lse] + lses[done:], want)
    if inplace:
        outs[0].copy_(out)
        lses[0].copy_(lse)
        out, lse = outs[0], lses[0]
    return (out, lse) if return_lse else out


def lse_request_keeps_out_bits(head_dim: int, dtype: torch.dtype = torch.bfloat16, seqlen_k: int = 4096) -> bool:
    """Whether asking the dense fused step for its LSE leaves every bit of `out` as it is, read from the library's own path table
    (qattn_describe_path with and without want_lse; host-only): True for head_dim 128 -- the hand-scheduled kernel sums the weights it
    already has --, False for 64 and 256, where the LSE request switches the sweep to exact exponentials (same bound, other bits)."""
    with_lse, without = (_native.describe_path("fused", head_dim, dtype, "head-wise", seqlen_k, want_lse=w) for w in (True, False))
    return all(with_lse[k] == without[k] for k in with_lse if k != "lse")


def _lse_eager(query, key, value, is_causal, scale):
    """force_eager_fallback: the eager definition of the fused step (nn._fp8_attention_eager) and the LSE of the same de-quantised scores."""
    out = nn._fp8_attention_eager(query, key, value, is_causal, scale, None, None, "head-wise")
    dims = [query.dim() - 2, query.dim() - 1]
    q8, sq = nn._dynamically_quantize_fp8(query, reduction_dim=dims)
    k = key
    if _cfg("smooth_k"):
        k = key.to(torch.float32)
        k = k - k.mean(dim=-2, keepdim=True)
    k8, sk = nn._dynamically_quantize_fp8(k, reduction_dim=dims)
    dq = q8.to(torch.float32) * sq[..., None, None]
    dk = nn._expand_kv_heads(k8.to(torch.float32) * sk[..., None, None], query.size(-3))
    s = (dq @ dk.transpose(-1, -2)) * (1.0 / math.sqrt(query.size(-1)) if scale is None else scale)
    if _cfg("smooth_k"):   # the rows' common shift q.k_mean goes back in: the LSE is that of the unsmoothed scores
        mean = nn._expand_kv_heads(key.to(torch.float32).mean(dim=-2, keepdim=True), query.size(-3))
        s = s + (dq @ mean.transpose(-1, -2)) * (1.0 / math.sqrt(query.size(-1)) if scale is None else scale)
    if is_causal:
        i, j = torch.arange(s.shape[-2], device=s.device)[:, None], torch.arange(s.shape[-1], device=s.device)[None, :]
        s = s.masked_fill(j > i, -math.inf)
    return out, torch.logsumexp(s, dim=-1)


def fp8_attn_lse_func(query, key, value, is_causal: bool = False, *, scale: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`fp8_attn_func(query, key, value, is_causal=is_causal, scale=scale)` (16-bit inputs, head-wise scales) together with the natural
    log-sum-exp of every row: (out [B, Hq, Sq, D], lse fp32 [B, Hq, Sq]) from ONE fused call -- the state `merge_attn_states` takes.
    Follows config.attention.* (fp8_format, quant_numerics, precision, smooth_k, output_layout) exactly as fp8_attn_func does.

    `out` against fp8_attn_func's, by the library's path table (include/qattn.h; `lse_request_keeps_out_bits` asks it):
      head_dim 128          bit for bit the same -- the LSE is summed from the e4m3 weights the second product consumed (within 2e-2 of
                            the exact one on one-term rows, 4e-3 on 16-bit-V rows);
      head_dim 64 and 256   the same error bound but OTHER BITS: the LSE request switches the one-term sweep from byte exponentials to
                            exact ones (LSE within 2e-3; rows on the 16-bit V are the same bits either way).
    Not traced by torch.compile as an op (it calls the C entry directly): a compiled region breaks the graph around it."""
    supported, reason = nn.can_use_attention(query, key, value, is_causal=is_causal, scale=scale, scaling_method="head-wise")
    if not supported:
        raise ValueError(reason)
    if query.dtype not in nn._HALF_DTYPES:
        raise ValueError(f"fp8_attn_lse_func quantises 16-bit query / key itself, got {query.dtype}")
    if _cfg("force_eager_fallback"):
        return _lse_eager(query, key, value, is_causal, scale)
    return _native.fp8_quant_attention_forward(
        query, key, value, is_causal=is_causal, scaling="head-wise", fp8_dtype=_native.fp8_dtype_of(_cfg("fp8_format")),
        numerics=_cfg("quant_numerics"), sm_scale=0.0 if scale is None else float(scale), precision=_cfg("precision"), return_lse=True,
        output_layout=_cfg("output_layout"), smooth_k=bool(_cfg("smooth_k")))


def fp8_attn_multi_kv_func(query, kvs, *, scale: Optional[float] = None, return_lse: bool = False):
    """Non-causal attention of `query` [B, Hq, Sq, D] over the CONCATENATION of several key / value sources -- text + image + adapter keys,
    a cached context + new tokens -- without concatenating them: kvs is a sequence of (key, value) pairs [B, Hkv, Skv_i, D], each with a
    length (and a number of kv heads dividing Hq) of its own.  One `fp8_attn_lse_func` call per pair, then ONE N-way `merge_attn_states`.

    Every source is quantised with ITS OWN scales (per head: over that source's keys, its values per 64-key chunk or head).  That is
    usually better than one scale over the concatenation -- a source with small keys is not crushed by another's range -- and it means the
    result is NOT bit-equal to `fp8_attn_func` on the concatenated tensors; both meet the same error bound against exact attention.
    Returns out, or (out, lse) with return_lse=True -- a state that merges further."""
    if not isinstance(kvs, (list, tuple)) or len(kvs) < 1:
        raise ValueError("kvs must be a non-empty sequence of (key, value) pairs")
    for i, kv in enumerate(kvs):
        if not isinstance(kv, (list, tuple)) or len(kv) != 2 or not all(isinstance(t, torch.Tensor) for t in kv):
            raise ValueError(f"kvs[{i}] must be a (key, value) pair of tensors")
    states = [fp8_attn_lse_func(query, k, v, False, scale=scale) for k, v in kvs]
    return merge_attn_states([s[0] for s in states], [s[1] for s in states], return_lse=return_lse)

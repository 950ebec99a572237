"""Variable-length (packed) FP8 attention: `fp8_attn_varlen_func`, the call shape of flash-attn's `flash_attn_varlen_func`.

B sequences of different lengths travel packed along the token axis -- q [total_q, Hq, D], k / v [total_k, Hkv, D] -- with int32 offset
tables cu_seqlens_q / cu_seqlens_k [B+1]; an optional int32 seqused_k [B] counts the keys each sequence uses from its start, so that a
padded [B, S_pad, H, D] K / V can be passed as a [B S_pad, H, D] view with cu_seqlens_k = arange(B+1) S_pad and seqused_k = k_lens,
without a copy (Wan-style cross-attention).

Numerics (include/qattn_varlen.h): q and k are quantised head-wise PER (sequence, head) -- exactly `dynamically_quantize_fp8` of each
sequence on its own, under config.attention.fp8_format / quant_numerics, over the used keys only -- and P.V runs on the reference
kernel's own numerics, 16-bit P on the original 16-bit value (every row is QATTN_PATH_V16).  config.attention.precision and
pv_precision do not apply; config.attention.smooth_k does: key smoothing per sequence over its used keys.  Row r of sequence i equals, bit for bit, `fp8_attention_forward_rowmajor(..., pv_16bit=True)` on that
sequence alone.  `causal` masks top-left per sequence (key j <= query r), as the dense entry and torch SDPA's is_causal; flash-attn >= 2.1
aligns the diagonal bottom-right when L_q != L_k -- the two agree for self-attention (cu_seqlens_q == cu_seqlens_k).
"""
import math
from typing import Optional

import torch
from torch import Tensor

from . import nn
from .utils import checks

_INDEX_DTYPE = torch.int32


def _is_int(x) -> bool:
    return isinstance(x, (int, torch.SymInt)) and not isinstance(x, bool)


def varlen_input_reason(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p=0.0, softmax_scale=None,
                        seqused_k=None) -> Optional[str]:
    """The first rule the arguments break, or None.  Shapes, dtypes and devices only: the tables' CONTENTS are read on the device
    (no host synchronisation), where every extent is clamped to its tensor (include/qattn_varlen.h)."""
    if dropout_p != 0.0:
        return "NYI: dropout_p must be 0.0"
    if not all(isinstance(t, Tensor) for t in (q, k, v)) or q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
        return "NYI: query, key and value must be 3-D packed tensors [total_tokens, heads, head_dim]"
    if any(t.requires_grad for t in (q, k, v)):
        return "NYI: query, key, and value must be leaf tensors (no backward)"
    if q.dtype not in (torch.float16, torch.bfloat16):
        return f"Expected query to have dtype torch.float16 or torch.bfloat16, but got query.dtype: {q.dtype} instead."
    if k.dtype != q.dtype or v.dtype != q.dtype:
        return f"Expected query, key and value to share a dtype, but got {q.dtype}, {k.dtype}, {v.dtype} instead."
    if q.shape[-1] != k.shape[-1] or q.shape[-1] != v.shape[-1]:
        return f"Expect query, key and value to have the same head dimension but got {q.shape[-1]}, {k.shape[-1]} and {v.shape[-1]}."
    if q.shape[-1] not in nn._HIP_SUPPORTED_HEAD_DIMS:
        return f"Unsupported head dimension: {q.shape[-1]}"
    if k.shape != v.shape:
        return f"Expect key and value to have the same shape but got {tuple(k.shape)} and {tuple(v.shape)}."
    if k.shape[1] == 0 or q.shape[1] % k.shape[1] != 0:
        return f"Expect the number of query heads to be a multiple of the key/value heads but got Hq={q.shape[1]} and Hkv={k.shape[1]}."
    if q.device != k.device or q.device != v.device:
        return f"Expected query, key, and value to be on the same device, but got {q.device}, {k.device} and {v.device} instead."
    if q.device.type != "cuda":
        return "Expected query, key, and value to be on a CUDA device"
    for name, t in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if not isinstance(t, Tensor) or t.dtype != _INDEX_DTYPE or t.dim() != 1 or t.shape[0] < 2:
            return f"Expected {name} to be a 1-D torch.int32 tensor of length B+1 >= 2"
        if t.device != q.device:
            return f"Expected {name} to be on {q.device}, but got {t.device} instead."
    if cu_seqlens_q.shape[0] != cu_seqlens_k.shape[0]:
        return f"Expected cu_seqlens_q and cu_seqlens_k of the same length B+1, but got {cu_seqlens_q.shape[0]} and {cu_seqlens_k.shape[0]}."
    if seqused_k is not None:
        if not isinstance(seqused_k, Tensor) or seqused_k.dtype != _INDEX_DTYPE or seqused_k.dim() != 1:
            return "Expected seqused_k to be a 1-D torch.int32 tensor of length B"
        if seqused_k.shape[0] != cu_seqlens_q.shape[0] - 1:
            return f"Expected seqused_k of length B = {cu_seqlens_q.shape[0] - 1}, but got {seqused_k.shape[0]}."
        if seqused_k.device != q.device:
            return f"Expected seqused_k to be on {q.device}, but got {seqused_k.device} instead."
    if not (_is_int(max_seqlen_q) and _is_int(max_seqlen_k)) or max_seqlen_q < 0 or max_seqlen_k < 0:
        return "Expected max_seqlen_q and max_seqlen_k to be non-negative host ints"
    if softmax_scale is not None and not (isinstance(softmax_scale, (int, float)) and math.isfinite(softmax_scale) and softmax_scale > 0):
        return f"softmax_scale must be a finite number > 0 (or None for 1/sqrt(head_dim)), got {softmax_scale!r}"
    return None


def _varlen_eager(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, softmax_scale, causal, return_lse, smooth_k=False):
    """config.attention.force_eager_fallback: the per-sequence loop of the eager fp8 definition (eager quantiser per sequence and head,
    de-quantise, aten SDPA: nn._fp8_attention_eager), with the log-sum-exp of the same de-quantised scores.
    smooth_k restated: the fp32 mean over the sequence's USED keys, one fp32 subtraction, the same eager quantiser on the result, and the
    LSE corrected by scale * q.m (the caller's 16-bit q)."""
    fp8_dtype = nn._fp8_dtype()
    total_q, Hq, D = q.shape
    scale = 1.0 / math.sqrt(D) if softmax_scale is None else float(softmax_scale)
    cq, ck = cu_seqlens_q.tolist(), cu_seqlens_k.tolist()
    used = None if seqused_k is None else seqused_k.tolist()
    out = torch.zeros((total_q, Hq, D), dtype=q.dtype, device=q.device)
    lse = torch.full((Hq, total_q), -math.inf, dtype=torch.float32, device=q.device)
    for i in range(len(cq) - 1):
        lq = cq[i + 1] - cq[i]
        lk = ck[i + 1] - ck[i] if used is None else min(used[i], ck[i + 1] - ck[i])
        if lq <= 0 or lk <= 0:
            continue   # (no key: zero rows, LSE -inf)
        qi = q[cq[i]:cq[i + 1]].transpose(0, 1)[None]
        ki, vi = (t[ck[i]:ck[i] + lk].transpose(0, 1)[None] for t in (k, v))
        q8, sq = nn._dynamically_quantize_fp8(qi, reduction_dim=[2, 3], fp8_dtype=fp8_dtype)
        mean = None
        if smooth_k:
            ki = ki.to(torch.float32)
            mean = ki.mean(dim=-2, keepdim=True)   # [1, Hkv, 1, D]
            ki = ki - mean
        k8, sk = nn._dynamically_quantize_fp8(ki, reduction_dim=[2, 3], fp8_dtype=fp8_dtype)
        o = nn._eager_fp8_attention(q8, k8, vi, sq, sk, causal, softmax_scale)
        out[cq[i]:cq[i + 1]] = o[0].transpose(0, 1)
        if return_lse:
            dq = q8.float() * sq[..., None, None]
            dk = nn._expand_kv_heads(k8.float() * sk[..., None, None], Hq)
            s = (dq @ dk.transpose(-1, -2)) * scale
            if causal:
                s = s.masked_fill(torch.ones(lq, lk, dtype=torch.bool, device=q.device).triu(1), -math.inf)
            l = torch.logsumexp(s[0], dim=-1)
            if smooth_k:
                l = l + scale * (qi[0].to(torch.float32) * nn._expand_kv_heads(mean, Hq)[0]).sum(-1)
            lse[:, cq[i]:cq[i + 1]] = l
    return (out, lse) if return_lse else out


def fp8_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p=0.0, softmax_scale=None, causal=False,
                         *, seqused_k=None, return_lse=False):
    """FP8 attention over packed variable-length sequences; flash-attn's `flash_attn_varlen_func` argument order (module docstring).
    q [total_q, Hq, D], k / v [total_k, Hkv, D] bf16 / fp16 (one dtype), D in {64, 128, 256}, Hq a multiple of Hkv; strided views with
    head_dim innermost are read in place.  cu_seqlens_q / cu_seqlens_k: int32 [B+1] on the device; max_seqlen_*: host ints, accepted for
    signature compatibility.  seqused_k: optional int32 [B], keys used per sequence (keys beyond it influence no output bit).
    Returns out [total_q, Hq, D] in the input dtype, or (out, lse) with return_lse (fp32 [Hq, total_q], natural log-sum-exp).  A sequence
    with no query has no rows; one with queries and no key gives zero rows and an LSE of -inf.  Unsupported input raises ValueError(reason).
    config.attention.smooth_k: key smoothing (include/qattn_smooth.h) -- every sequence's K is quantised as fp32(k) - the channel mean of
    its used keys; `out` is mathematically unchanged, the LSE is that of the true scores.  Read here and passed to the op as an argument,
    so a compiled graph bakes it in at trace time; `config.patch({"attention.smooth_k": ...})` around a call overrides it for that call."""
    smooth_k = bool(checks.config_value("attention.smooth_k"))
    if not checks.config_value("attention.skip_supported_check"):
        reason = varlen_input_reason(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p, softmax_scale, seqused_k)
        if reason is None:
            ok, reason = nn._pre_check_can_use_hip_attention(device=q.device)
            reason = None if ok else reason
        if reason:
            raise ValueError(reason)
    if checks.config_value("attention.force_eager_fallback") and not torch.compiler.is_dynamo_compiling():
        return _varlen_eager(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, softmax_scale, causal, return_lse, smooth_k)
    out, lse = nn._ops().fp8_varlen_attention_forward(
        q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, int(max_seqlen_q), int(max_seqlen_k), bool(causal),
        checks.config_value("attention.fp8_format"), checks.config_value("attention.quant_numerics"), bool(return_lse), smooth_k,
        scale=softmax_scale)
    return (out, lse) if return_lse else out


# ---- FP8 P.V on the packed call shape (include/qattn_varlen.h: qattn_fp8_quant_attention_varlen_forward_fp8pv) ---------------------------
def _varlen_eager_fp8pv(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, softmax_scale, causal, return_lse, smooth_k=False):
    """config.attention.force_eager_fallback with pv_precision="fp8": `_varlen_eager`'s per-sequence loop with V restated -- the eager
    quantiser per sequence and head on q, on the USED keys (smooth_k: on fp32(k) - their fp32 mean) and on the V of the used keys, all
    three de-quantised, then fp32 attention (top-left causal mask) and the log-sum-exp of the same scores, corrected by scale * q.m under
    smooth_k.  P stays fp32: both precisions of the kernel are within the fp8-V bound of this definition."""
    fp8_dtype = nn._fp8_dtype()
    total_q, Hq, D = q.shape
    scale = 1.0 / math.sqrt(D) if softmax_scale is None else float(softmax_scale)
    cq, ck = cu_seqlens_q.tolist(), cu_seqlens_k.tolist()
    used = None if seqused_k is None else seqused_k.tolist()
    out = torch.zeros((total_q, Hq, D), dtype=q.dtype, device=q.device)
    lse = torch.full((Hq, total_q), -math.inf, dtype=torch.float32, device=q.device)
    for i in range(len(cq) - 1):
        lq = cq[i + 1] - cq[i]
        lk = ck[i + 1] - ck[i] if used is None else min(used[i], ck[i + 1] - ck[i])
        if lq <= 0 or lk <= 0:
            continue   # (no key: zero rows, LSE -inf)
        qi = q[cq[i]:cq[i + 1]].transpose(0, 1)[None]
        ki, vi = (t[ck[i]:ck[i] + lk].transpose(0, 1)[None] for t in (k, v))
        q8, sq = nn._dynamically_quantize_fp8(qi, reduction_dim=[2, 3], fp8_dtype=fp8_dtype)
        mean = None
        if smooth_k:
            ki = ki.to(torch.float32)
            mean = ki.mean(dim=-2, keepdim=True)   # [1, Hkv, 1, D]
            ki = ki - mean
        k8, sk = nn._dynamically_quantize_fp8(ki, reduction_dim=[2, 3], fp8_dtype=fp8_dtype)
        v8, sv = nn._dynamically_quantize_fp8(vi, reduction_dim=[2, 3], fp8_dtype=fp8_dtype)
        dq = q8.float() * sq[..., None, None]
        dk = nn._expand_kv_heads(k8.float() * sk[..., None, None], Hq)
        dv = nn._expand_kv_heads(v8.float() * sv[..., None, None], Hq)
        s = (dq @ dk.transpose(-1, -2)) * scale
        if causal:
            s = s.masked_fill(torch.ones(lq, lk, dtype=torch.bool, device=q.device).triu(1), -math.inf)
        l = torch.logsumexp(s[0], dim=-1)
        out[cq[i]:cq[i + 1]] = (torch.exp(s[0] - l[..., None]) @ dv[0]).to(q.dtype).transpose(0, 1)
        if smooth_k:
            l = l + scale * (qi[0].to(torch.float32) * nn._expand_kv_heads(mean, Hq)[0]).sum(-1)
        lse[:, cq[i]:cq[i + 1]] = l
    return (out, lse) if return_lse else out


def fp8_attn_varlen_pv_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p=0.0, softmax_scale=None, causal=False,
                            *, seqused_k=None, return_lse=False, pv_precision="16bit", precision="accurate"):
    """fp8_attn_varlen_func with the P.V path as an explicit argument (same tensors, tables, results and config flags; a sibling function:
    fp8_attn_varlen_func keeps the signature it was released with).
    pv_precision "16bit" (default): exactly fp8_attn_varlen_func, bit for bit; `precision` must then be "accurate".
    pv_precision "fp8": both products on the FP8 matrix pipe.  Every sequence's V is quantised head-wise over its USED keys alone (the
    bytes and scale of the quant pre-pass on v_i[:used]; V must be finite there, and keys beyond seqused_k still influence no output
    bit), P is e4m3: precision "accurate" = exact exponentials and two-term (hi + lo) P on every row; "fast" = the one-term
    byte-exponential sweep for the 128-row tiles whose rows see n >= 1024 keys (n = used L_k, or min(L_k, 128 (t + 1)) for tile t when
    causal), two-term below, and exact exponentials on the one-term tiles when the LSE is asked for.  "fast" has no rescue pass and is
    stated for score variance softmax_scale^2 D <= 1.  Any other value of either argument -- "auto" included -- raises ValueError.
    config.attention.pv_precision / precision do not apply; fp8_format, quant_numerics, smooth_k, skip_supported_check and
    force_eager_fallback are followed as by fp8_attn_varlen_func."""
    if pv_precision not in ("16bit", "fp8"):
        raise ValueError(f"Unsupported pv_precision: {pv_precision!r} (expected '16bit' or 'fp8')")
    if pv_precision == "16bit":
        if precision != "accurate":
            raise ValueError(f"Unsupported precision for pv_precision='16bit': {precision!r} (the 16-bit P.V path has one precision, 'accurate')")
        return fp8_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p, softmax_scale, causal,
                                    seqused_k=seqused_k, return_lse=return_lse)
    if precision not in ("accurate", "fast"):
        raise ValueError(f"Unsupported precision for pv_precision='fp8': {precision!r} (expected 'accurate' or 'fast'; 'auto' is not offered "
                         "by the packed entry)")
    smooth_k = bool(checks.config_value("attention.smooth_k"))
    if not checks.config_value("attention.skip_supported_check"):
        reason = varlen_input_reason(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p, softmax_scale, seqused_k)
        if reason is None:
            ok, reason = nn._pre_check_can_use_hip_attention(device=q.device)
            reason = None if ok else reason
        if reason:
            raise ValueError(reason)
    if checks.config_value("attention.force_eager_fallback") and not torch.compiler.is_dynamo_compiling():
        return _varlen_eager_fp8pv(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, softmax_scale, causal, return_lse, smooth_k)
    out, lse = nn._ops().fp8_varlen_attention_forward_fp8pv(
        q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, int(max_seqlen_q), int(max_seqlen_k), bool(causal),
        checks.config_value("attention.fp8_format"), checks.config_value("attention.quant_numerics"), bool(return_lse), smooth_k, precision,
        scale=softmax_scale)
    return (out, lse) if return_lse else out


# ---- sliding-window (local) attention: flash-attn's window_size on the packed call shape (include/qattn_window.h) --------------------
def window_size_reason(window_size) -> Optional[str]:
    """The rule a `window_size` breaks, or None: a pair (left, right) of host ints >= -1 (-1: unbounded on that side)."""
    if not isinstance(window_size, (tuple, list)) or len(window_size) != 2:
        return f"Expected window_size to be a pair (left, right), but got {window_size!r}"
    if not all(_is_int(w) for w in window_size):
        return f"Expected window_size to hold host ints, but got {window_size!r}"
    if window_size[0] < -1 or window_size[1] < -1:
        return f"Expected window_size values >= -1 (-1: unbounded on that side), but got {tuple(window_size)!r}"
    return None


def _varlen_window_eager(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, softmax_scale, window_size, return_lse, smooth_k=False):
    """config.attention.force_eager_fallback: `_varlen_eager`'s per-sequence loop with the window mask -- the eager quantiser per sequence
    and head over ALL its queries and used keys (smooth_k: on fp32(k) - the fp32 mean of the used keys), de-quantise, fp32 attention with
    the scores outside row r's window [r + delta - left, r + delta + right] (delta = L_k - L_q) at -inf; a row without a key comes out as
    zeros (not NaN) with an LSE of -inf; the LSE of the other rows is corrected by scale * q.m under smooth_k."""
    fp8_dtype = nn._fp8_dtype()
    left, right = int(window_size[0]), int(window_size[1])
    total_q, Hq, D = q.shape
    scale = 1.0 / math.sqrt(D) if softmax_scale is None else float(softmax_scale)
    cq, ck = cu_seqlens_q.tolist(), cu_seqlens_k.tolist()
    used = None if seqused_k is None else seqused_k.tolist()
    out = torch.zeros((total_q, Hq, D), dtype=q.dtype, device=q.device)
    lse = torch.full((Hq, total_q), -math.inf, dtype=torch.float32, device=q.device)
    for i in range(len(cq) - 1):
        lq = cq[i + 1] - cq[i]
        lk = ck[i + 1] - ck[i] if used is None else min(used[i], ck[i + 1] - ck[i])
        if lq <= 0 or lk <= 0:
            continue   # (no key: zero rows, LSE -inf)
        qi = q[cq[i]:cq[i + 1]].transpose(0, 1)[None]
        ki, vi = (t[ck[i]:ck[i] + lk].transpose(0, 1)[None] for t in (k, v))
        q8, sq = nn._dynamically_quantize_fp8(qi, reduction_dim=[2, 3], fp8_dtype=fp8_dtype)
        mean = None
        if smooth_k:
            ki = ki.to(torch.float32)
            mean = ki.mean(dim=-2, keepdim=True)   # [1, Hkv, 1, D]
            ki = ki - mean
        k8, sk = nn._dynamically_quantize_fp8(ki, reduction_dim=[2, 3], fp8_dtype=fp8_dtype)
        dq = q8.float() * sq[..., None, None]
        dk = nn._expand_kv_heads(k8.float() * sk[..., None, None], Hq)
        dv = nn._expand_kv_heads(vi.float(), Hq)
        d = torch.arange(lk, device=q.device)[None, :] - torch.arange(lq, device=q.device)[:, None] - (lk - lq)   # j - (r + delta)
        alive = torch.ones(lq, lk, dtype=torch.bool, device=q.device)
        if left >= 0:
            alive &= d >= -left
        if right >= 0:
            alive &= d <= right
        s = ((dq @ dk.transpose(-1, -2)) * scale).masked_fill(~alive, -math.inf)
        l = torch.logsumexp(s[0], dim=-1)
        p = torch.exp(s[0] - l.clamp_min(torch.finfo(torch.float32).min)[..., None])   # (a row without keys: exp(-inf) = 0)
        out[cq[i]:cq[i + 1]] = (p @ dv[0]).to(q.dtype).transpose(0, 1)
        if smooth_k:   # (-inf rows stay -inf)
            l = l + scale * (qi[0].to(torch.float32) * nn._expand_kv_heads(mean, Hq)[0]).sum(-1)
        lse[:, cq[i]:cq[i + 1]] = l
    return (out, lse) if return_lse else out


def fp8_attn_varlen_window_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window_size, dropout_p=0.0, softmax_scale=None,
                                *, seqused_k=None, return_lse=False):
    """Sliding-window (local) FP8 attention over packed variable-length sequences: `fp8_attn_varlen_func`'s tensors, tables and results
    with flash-attn's `window_size=(left, right)` in place of `causal` (include/qattn_window.h).  Per sequence with L_q queries and L_k USED
    keys, delta = L_k - L_q: query r attends key j iff r + delta - left <= j <= r + delta + right (and 0 <= j < L_k); -1 means unbounded on
    that side, values larger than any length are legal.  (-1, 0) is the causal mask aligned bottom-right (flash-attn >= 2.1), (-1, -1)
    masks nothing.  A row whose window holds no key gives a zero row and an LSE of -inf.
    Numerics are the packed entry's: q and k quantised head-wise per (sequence, head) over all queries and all used keys -- keys outside
    every window still count toward K's scale -- and 16-bit P on the original 16-bit V.  A 256-row query block visits only the 64-key
    chunks its rows attend, and V rows outside them are never read.  config.attention.smooth_k, fp8_format and quant_numerics are followed as by
    `fp8_attn_varlen_func` (the mean over the used keys, the LSE corrected).  Unsupported input raises ValueError(reason)."""
    smooth_k = bool(checks.config_value("attention.smooth_k"))
    if not checks.config_value("attention.skip_supported_check"):
        reason = varlen_input_reason(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p, softmax_scale, seqused_k)
        if reason is None:
            reason = window_size_reason(window_size)
        if reason is None:
            ok, reason = nn._pre_check_can_use_hip_attention(device=q.device)
            reason = None if ok else reason
        if reason:
            raise ValueError(reason)
    if checks.config_value("attention.force_eager_fallback") and not torch.compiler.is_dynamo_compiling():
        return _varlen_window_eager(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, softmax_scale, window_size, return_lse, smooth_k)
    out, lse = nn._ops().fp8_varlen_window_attention_forward(
        q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, int(max_seqlen_q), int(max_seqlen_k), int(window_size[0]), int(window_size[1]),
        checks.config_value("attention.fp8_format"), checks.config_value("attention.quant_numerics"), bool(return_lse), smooth_k,
        scale=softmax_scale)
    return (out, lse) if return_lse else out


def _window_attn_dense(packed_call, q, k, v, window_size, return_lse):
    """The dense [B, H, S, D] call shape around a packed window function: checks, the packed [B S, H, D] views (free where
    `fp8_window_attn_func` says so, else one copy), the arange(B+1) S tables built on the device, and the views of the packed results.
    packed_call(qp, kp, vp, cu_q, cu_k, Sq, Skv) returns out or (out, lse)."""
    if not all(isinstance(t, Tensor) for t in (q, k, v)) or q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError("NYI: query, key and value must be 4-D tensors [B, heads, seq_len, head_dim]")
    if k.shape[0] != q.shape[0] or v.shape[0] != q.shape[0]:
        raise ValueError(f"Expect query and key/value to have the same batch size but got {q.shape[0]}, {k.shape[0]} and {v.shape[0]}.")
    if not checks.config_value("attention.skip_supported_check") and window_size_reason(window_size):
        raise ValueError(window_size_reason(window_size))   # (before the tables are built on the device)
    B, Hq, Sq, D = q.shape
    Skv = k.shape[2]
    # [B, H, S, D] -> [B, S, H, D] -> [B S, H, D]: reshape returns a view exactly where the rule above holds, else one copy
    qp, kp, vp = (t.permute(0, 2, 1, 3).reshape(t.shape[0] * t.shape[2], t.shape[1], t.shape[3]) for t in (q, k, v))
    steps = torch.arange(B + 1, dtype=_INDEX_DTYPE, device=q.device)
    res = packed_call(qp, kp, vp, steps * Sq, steps * Skv, Sq, Skv)
    out = (res[0] if return_lse else res).view(B, Sq, Hq, D).permute(0, 2, 1, 3)
    return (out, res[1].view(Hq, B, Sq).permute(1, 0, 2)) if return_lse else out


def fp8_window_attn_func(q, k, v, window_size, *, scale=None, return_lse=False):
    """Sliding-window FP8 attention on dense [B, H, S, D] tensors (the block-sparse entry's call shape): q [B, Hq, Sq, D], k / v
    [B, Hkv, Skv, D]; every batch entry is one sequence of `fp8_attn_varlen_window_func` (scales per (batch, head), delta = Skv - Sq).
    The packed [B S, H, D] views and the arange(B+1) S tables are built on the device, without a host synchronisation.  The view is free
    when B == 1, or when a tensor's batch stride equals S x its token stride (anything backed by [B, S, H, D] memory); any other layout
    with B > 1 -- a contiguous [B, H, S, D] among them -- costs ONE re-layout copy of that tensor.
    Returns out as a [B, Hq, Sq, D] view of the packed result, or (out, lse) with return_lse (lse fp32 [B, Hq, Sq], a view)."""
    return _window_attn_dense(
        lambda qp, kp, vp, cu_q, cu_k, Sq, Skv: fp8_attn_varlen_window_func(qp, kp, vp, cu_q, cu_k, Sq, Skv, window_size, softmax_scale=scale,
                                                                            return_lse=return_lse),
        q, k, v, window_size, return_lse)


# ---- FP8 P.V under the sliding window (include/qattn_window.h: qattn_fp8_quant_attention_varlen_window_forward_fp8pv) ---------------------
def _varlen_window_eager_fp8pv(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, softmax_scale, window_size, return_lse, smooth_k=False):
    """config.attention.force_eager_fallback with pv_precision="fp8": `_varlen_window_eager` with V restated as `_varlen_eager_fp8pv`
    restates it for `_varlen_eager` -- every sequence's V of the USED keys goes through the eager quantiser per head and back (fp32);
    everything else (q, k, mask, keyless rows, the LSE and its smooth_k correction) is `_varlen_window_eager`'s, whose fp32 P.V then runs
    on the de-quantised V.  Keys beyond seqused_k are replaced by zeros and attended by no row."""
    fp8_dtype = nn._fp8_dtype()
    cq, ck = cu_seqlens_q.tolist(), cu_seqlens_k.tolist()
    used = None if seqused_k is None else seqused_k.tolist()
    dv = torch.zeros(v.shape, dtype=torch.float32, device=v.device)
    for i in range(len(cq) - 1):
        lk = ck[i + 1] - ck[i] if used is None else min(used[i], ck[i + 1] - ck[i])
        if cq[i + 1] - cq[i] <= 0 or lk <= 0:
            continue
        vi = v[ck[i]:ck[i] + lk].transpose(0, 1)[None]
        v8, sv = nn._dynamically_quantize_fp8(vi, reduction_dim=[2, 3], fp8_dtype=fp8_dtype)
        dv[ck[i]:ck[i] + lk] = (v8.float() * sv[..., None, None])[0].transpose(0, 1)
    return _varlen_window_eager(q, k, dv, cu_seqlens_q, cu_seqlens_k, seqused_k, softmax_scale, window_size, return_lse, smooth_k)


def fp8_attn_varlen_window_pv_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window_size, dropout_p=0.0, softmax_scale=None,
                                   *, seqused_k=None, return_lse=False, pv_precision="16bit", precision="accurate"):
    """fp8_attn_varlen_window_func with the P.V path as an explicit argument (same tensors, tables, window, results and config flags; a
    sibling function: fp8_attn_varlen_window_func keeps the signature it was released with).
    pv_precision "16bit" (default): exactly fp8_attn_varlen_window_func, bit for bit; `precision` must then be "accurate".
    pv_precision "fp8": both products on the FP8 matrix pipe (include/qattn_window.h, ..._window_forward_fp8pv).  q, k and v are quantised
    as by fp8_attn_varlen_pv_func: head-wise per (sequence, head) over all queries and all USED keys, windowed or not.  V must be FINITE
    on the used keys -- unlike the 16-bit window path, which tolerates NaN in V rows that no row attends; keys beyond seqused_k still
    influence no output bit.  One workgroup per 128-row tile sweeps only the 64-key chunks of [klo, khi], the keys its rows attend.  P is
    e4m3: precision "accurate" = exact exponentials and two-term (hi + lo) P on every row; "fast" = the one-term byte-exponential sweep
    for the tiles with n = khi - klo + 1 >= 1024, two-term below, and exact exponentials on the one-term tiles when the LSE is asked
    for.  "fast" has no rescue pass and is stated for score variance softmax_scale^2 D <= 1.  A row whose window holds no key gives a
    zero row and an LSE of -inf.  Any other value of either argument -- "auto" included -- raises ValueError.
    config.attention.pv_precision / precision do not apply; fp8_format, quant_numerics, smooth_k, skip_supported_check and
    force_eager_fallback are followed as by fp8_attn_varlen_window_func."""
    if pv_precision not in ("16bit", "fp8"):
        raise ValueError(f"Unsupported pv_precision: {pv_precision!r} (expected '16bit' or 'fp8')")
    if pv_precision == "16bit":
        if precision != "accurate":
            raise ValueError(f"Unsupported precision for pv_precision='16bit': {precision!r} (the 16-bit P.V path has one precision, 'accurate')")
        return fp8_attn_varlen_window_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window_size, dropout_p, softmax_scale,
                                           seqused_k=seqused_k, return_lse=return_lse)
    if precision not in ("accurate", "fast"):
        raise ValueError(f"Unsupported precision for pv_precision='fp8': {precision!r} (expected 'accurate' or 'fast'; 'auto' is not offered "
                         "by the sliding-window entry)")
    smooth_k = bool(checks.config_value("attention.smooth_k"))
    if not checks.config_value("attention.skip_supported_check"):
        reason = varlen_input_reason(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p, softmax_scale, seqused_k)
        if reason is None:
            reason = window_size_reason(window_size)
        if reason is None:
            ok, reason = nn._pre_check_can_use_hip_attention(device=q.device)
            reason = None if ok else reason
        if reason:
            raise ValueError(reason)
    if checks.config_value("attention.force_eager_fallback") and not torch.compiler.is_dynamo_compiling():
        return _varlen_window_eager_fp8pv(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, softmax_scale, window_size, return_lse, smooth_k)
    out, lse = nn._ops().fp8_varlen_window_attention_forward_fp8pv(
        q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, int(max_seqlen_q), int(max_seqlen_k), int(window_size[0]), int(window_size[1]),
        checks.config_value("attention.fp8_format"), checks.config_value("attention.quant_numerics"), bool(return_lse), smooth_k, precision,
        scale=softmax_scale)
    return (out, lse) if return_lse else out


def fp8_window_attn_pv_func(q, k, v, window_size, *, scale=None, return_lse=False, pv_precision="16bit", precision="accurate"):
    """fp8_window_attn_func with the P.V path as an explicit argument: its dense [B, H, S, D] call shape and view logic around
    `fp8_attn_varlen_window_pv_func` (pv_precision / precision as there; "16bit" is fp8_window_attn_func bit for bit)."""
    return _window_attn_dense(
        lambda qp, kp, vp, cu_q, cu_k, Sq, Skv: fp8_attn_varlen_window_pv_func(qp, kp, vp, cu_q, cu_k, Sq, Skv, window_size, softmax_scale=scale,
                                                                               return_lse=return_lse, pv_precision=pv_precision,
                                                                               precision=precision),
        q, k, v, window_size, return_lse)

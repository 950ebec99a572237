"""Operator boundary.  Mirrors src/quantum_attn/ops.py: two torch custom ops with the reference's schemas
(ops.py:32-42, 98-110), registered for device type "cuda" (= HIP on PyTorch-ROCm) with fake impls so that
callers under torch.compile keep working.  The namespace is `quantumattention_amd` rather than `quantum_attn`
so the reference can be imported beside this package in one process (torch.library.define would collide).

Unlike the reference -- whose eager impl is aten SDPA on de-quantised inputs and whose real kernel is reached
only through an Inductor lowering (inductor/kernels/attention.py:1037-1065) -- the implementation here calls
the hand-written gfx950 kernels through the C ABI directly.  There is no eager/CPU fallback at this level.
"""
from typing import Optional, Sequence

import torch

from . import _native, config

_custom_op = torch.library.custom_op
_register_fake = torch.library.register_fake


def _out_like(query: torch.Tensor, value: torch.Tensor, output_layout: str = "contiguous") -> torch.Tensor:
    return _native.empty_output(query, value.dtype, output_layout)


def _check_op_args(attn_mask, dropout_p, scale):
    # same asserts as tk_fp8_attention_forward_kernel (inductor/kernels/attention.py:55-73)
    if attn_mask is not None:
        raise RuntimeError("attn_mask is not supported by the gfx950 attention kernel")
    if dropout_p != 0.0:
        raise RuntimeError("dropout_p must be 0.0 for the gfx950 attention kernel")


@_custom_op("quantumattention_amd::attention_forward", mutates_args=(), device_types=("cuda",))
def attention_forward(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    attn_mask: Optional[torch.Tensor] = None,
    dropout_p: float = 0.0,
    is_causal: bool = False,
    *,
    scale: Optional[float] = None,
) -> torch.Tensor:
    """16-bit sibling op, same schema as quantum_attn::attention_forward (ops.py:32-42): query/key/value bf16 or fp16
    [B,H,S,D]; K and V are re-laid into MFMA fragment order, then the bf16/fp16 MFMA kernel runs."""
    _check_op_args(attn_mask, dropout_p, scale)
    if query.dtype not in (torch.bfloat16, torch.float16) or key.dtype != query.dtype or value.dtype != query.dtype:
        raise RuntimeError(f"query/key/value must share bf16 or fp16, got {query.dtype}, {key.dtype}, {value.dtype}")
    _, _, Hkv, _, Skv, _ = _native._check_qkv(query, key, value)
    k_frag = _native.pack16(key, _native.LAYOUT_K16FRAG)
    v_frag = _native.pack16(value, _native.LAYOUT_V16FRAG)
    return _native.attention_forward_16(query, k_frag, v_frag, Hkv=Hkv, Skv=Skv, is_causal=is_causal,
                                        sm_scale=0.0 if scale is None else float(scale),
                                        fast_exp=bool(config.attention.fast_exp16), output_layout=config.attention.output_layout)


@_register_fake("quantumattention_amd::attention_forward")
def _(query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False, *, scale=None):
    return _out_like(query, value, config.attention.output_layout)


@_custom_op("quantumattention_amd::fp8_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_attention_forward(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    scale_q: Optional[torch.Tensor] = None,
    scale_k: Optional[torch.Tensor] = None,
    attn_mask: Optional[torch.Tensor] = None,
    dropout_p: float = 0.0,
    is_causal: bool = False,
    *,
    scale: Optional[float] = None,
) -> torch.Tensor:
    """query/key: fp8 (e4m3fn or e5m2) [B,H,S,D] row-major with fp32 scales [B,H] (head-wise) or [B,H,S]
    (token-wise); value: bf16/fp16.  Same contract as quantum_attn::fp8_attention_forward (ops.py:98-121)."""
    _check_op_args(attn_mask, dropout_p, scale)
    if scale_q is None or scale_k is None:
        raise RuntimeError("fp8_attention_forward needs scale_q and scale_k")
    if query.dtype not in (torch.float8_e4m3fn, torch.float8_e5m2) or key.dtype != query.dtype:
        raise RuntimeError(f"query/key must share an fp8 dtype, got {query.dtype} and {key.dtype}")
    if value.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError(f"value must be bf16 or fp16, got {value.dtype}")
    if query.dim() != 4 or key.dim() != 4 or value.dim() != 4:
        raise RuntimeError("query, key and value must be 4-D")
    B, Hq, Sq, D = query.shape
    if key.shape != value.shape or key.shape[0] != B or key.shape[3] != D or key.device != query.device or value.device != query.device:
        raise RuntimeError(f"key {tuple(key.shape)} / value {tuple(value.shape)} do not match query {tuple(query.shape)} "
                           "(same batch, head_dim, device; key and value the same shape)")
    Hkv, Skv = key.shape[1], key.shape[2]
    if Hkv == 0 or Hq % Hkv != 0:
        raise RuntimeError(f"Hq={Hq} is not a multiple of Hkv={Hkv}")
    # scale_q / scale_k: fp32 on the same device, exactly [B,H] (head-wise) or [B,H,S] (token-wise); tk/attention.py:402-414
    from .nn import scale_shapes_reason

    reason = scale_shapes_reason(query, key, scale_q, scale_k)
    if reason:
        raise RuntimeError(reason)
    if config.attention.pv_precision not in ("fp8", "16bit"):
        raise ValueError(f"Unsupported config.attention.pv_precision: {config.attention.pv_precision!r} (expected 'fp8' or '16bit')")
    # ONE C call with the pybind function's contract (tk/attention.py:357-360): the K re-lay and the V handling happen inside, in a
    # workspace.  pv_precision = "16bit": the reference kernel's own numerics, value stays 16-bit and P is cast to 16 bit
    # (tk/attention.py:72,286,318); "fp8" (default): V quantised head-wise, both GEMMs on FP8 MFMA.
    return _native.fp8_attention_forward_rowmajor(
        query, key, value, scale_q, scale_k, is_causal=is_causal, pv_16bit=config.attention.pv_precision == "16bit",
        sm_scale=0.0 if scale is None else float(scale), precision=config.attention.precision)


@_register_fake("quantumattention_amd::fp8_attention_forward")
def _(query, key, value, scale_q=None, scale_k=None, attn_mask=None, dropout_p=0.0, is_causal=False, *, scale=None):
    return _out_like(query, value)


@_custom_op("quantumattention_amd::fp8_quant_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_quant_attention_forward(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    is_causal: bool = False,
    scaling_method: str = "head-wise",
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    precision: str = "auto",
    amax_q: Optional[torch.Tensor] = None,
    amax_k: Optional[torch.Tensor] = None,
    ssq_q: Optional[torch.Tensor] = None,
    ssq_k: Optional[torch.Tensor] = None,
    amax_v: Optional[torch.Tensor] = None,
    output_layout: str = "contiguous",
    *,
    scale: Optional[float] = None,
    smooth_k: bool = False,
) -> torch.Tensor:
    """Fused entry for 16-bit inputs: the quant pre-pass (nn.py:410-418) writes K and V straight into the MFMA
    fragment layouts, then the attention kernel runs -- what `_fp8_attention_wrapper` (nn.py:394-430) does in the
    reference through Inductor, without the intermediate row-major K copy.  amax_q / amax_k (fp32 [B,H], head-wise only):
    per-head max |x| of query / key from the kernel that produced them; the abs-max launch then has nothing to read --
    the hand-off the reference gets from Inductor fusing the quantiser into the producer.  ssq_q / ssq_k (fp32 [B,H], both or
    neither): per-head sums of squares, which keep precision="auto" its score-spread estimate when the abs-max pass is skipped.
    amax_v (fp32 [B,Hkv]): the same for value, read only where V has one scale per head (token-wise scales, or more than 16384 keys per
    head; elsewhere the fused step scales V per 64-key chunk inside the quantise pass and needs no abs-max of it: include/qattn.h PATH TABLE).
    smooth_k: key smoothing (include/qattn_smooth.h; config.attention.smooth_k): key is quantised as fp32(key) - its per-channel mean over
    the sequence; amax_k / ssq_k (figures of the unsmoothed key) are refused with it."""
    return _native.fp8_quant_attention_forward(
        query, key, value, is_causal=is_causal, scaling=scaling_method, fp8_dtype=_native.fp8_dtype_of(fp8_format),
        numerics=numerics, sm_scale=0.0 if scale is None else float(scale), precision=precision, amax_q=amax_q, amax_k=amax_k,
        amax_v=amax_v, ssq_q=ssq_q, ssq_k=ssq_k, output_layout=output_layout, smooth_k=smooth_k)


@_register_fake("quantumattention_amd::fp8_quant_attention_forward")
def _(query, key, value, is_causal=False, scaling_method="head-wise", fp8_format="e4m3", numerics="compiled",
      precision="auto", amax_q=None, amax_k=None, ssq_q=None, ssq_k=None, amax_v=None, output_layout="contiguous", *, scale=None,
      smooth_k=False):
    return _out_like(query, value, output_layout)


@_custom_op("quantumattention_amd::dynamically_quantize_fp8", mutates_args=(), device_types=("cuda",))
def dynamically_quantize_fp8_op(t: torch.Tensor, token_wise: bool, fp8_format: str = "e4m3",
                                numerics: str = "compiled") -> tuple[torch.Tensor, torch.Tensor]:
    """HIP quant pre-pass for a 4-D [B,H,S,D] tensor (nn.py:14-19): head-wise (dims 2,3) or token-wise (dim 3)."""
    return _native.quant_fp8(t, scaling="token-wise" if token_wise else "head-wise",
                             fp8_dtype=_native.fp8_dtype_of(fp8_format), layout=_native.LAYOUT_ROWMAJOR,
                             numerics=numerics)


@_register_fake("quantumattention_amd::dynamically_quantize_fp8")
def _(t, token_wise, fp8_format="e4m3", numerics="compiled"):
    q = torch.empty(t.shape, dtype=_native.fp8_dtype_of(fp8_format), device=t.device)
    s = torch.empty(t.shape[:3] if token_wise else t.shape[:2], dtype=torch.float32, device=t.device)
    return q, s


@_custom_op("quantumattention_amd::fp8_varlen_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_varlen_attention_forward(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    cu_seqlens_k: torch.Tensor,
    seqused_k: Optional[torch.Tensor] = None,
    max_seqlen_q: int = 0,
    max_seqlen_k: int = 0,
    is_causal: bool = False,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    return_lse: bool = False,
    smooth_k: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Packed variable-length sequences (include/qattn_varlen.h): query [total_q, Hq, D], key / value [total_k, Hkv, D] bf16 / fp16, int32
    cu_seqlens_* [B+1], optional int32 seqused_k [B]; per-(sequence, head) fp8 scales, 16-bit P on the 16-bit value.  Returns (out
    [total_q, Hq, D], lse fp32 [Hq, total_q] -- or an empty [0] tensor without return_lse).  max_seqlen_*: signature compatibility only
    (the kernels read every length on the device).  smooth_k: key smoothing per sequence over its used keys (include/qattn_smooth.h;
    config.attention.smooth_k).  Arguments are validated by varlen.fp8_attn_varlen_func."""
    del max_seqlen_q, max_seqlen_k
    res = _native.fp8_quant_attention_varlen(
        query, key, value, cu_seqlens_q.contiguous(), cu_seqlens_k.contiguous(), None if seqused_k is None else seqused_k.contiguous(),
        is_causal=is_causal, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics, sm_scale=0.0 if scale is None else float(scale),
        return_lse=return_lse, smooth_k=smooth_k)
    if return_lse:
        return res
    return res, torch.empty((0,), dtype=torch.float32, device=query.device)


@_register_fake("quantumattention_amd::fp8_varlen_attention_forward")
def _(query, key, value, cu_seqlens_q, cu_seqlens_k, seqused_k=None, max_seqlen_q=0, max_seqlen_k=0, is_causal=False, fp8_format="e4m3",
      numerics="compiled", return_lse=False, smooth_k=False, *, scale=None):
    out = query.new_empty((query.shape[0], query.shape[1], value.shape[2]), dtype=value.dtype)
    lse = query.new_empty((query.shape[1], query.shape[0]) if return_lse else (0,), dtype=torch.float32)
    return out, lse


@_custom_op("quantumattention_amd::fp8_varlen_attention_forward_fp8pv", mutates_args=(), device_types=("cuda",))
def fp8_varlen_attention_forward_fp8pv(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    cu_seqlens_k: torch.Tensor,
    seqused_k: Optional[torch.Tensor] = None,
    max_seqlen_q: int = 0,
    max_seqlen_k: int = 0,
    is_causal: bool = False,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    return_lse: bool = False,
    smooth_k: bool = False,
    precision: str = "accurate",
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Packed variable-length sequences with FP8 P.V (include/qattn_varlen.h, ..._forward_fp8pv): the tensors and results of
    fp8_varlen_attention_forward; value is quantised head-wise per (sequence, head) over the used keys, P is e4m3 -- two-term everywhere
    (precision "accurate") or one-term byte-exponential for the 128-row tiles whose rows see >= 1024 keys ("fast").
    Arguments are validated by varlen.fp8_attn_varlen_pv_func."""
    del max_seqlen_q, max_seqlen_k
    res = _native.fp8_quant_attention_varlen_fp8pv(
        query, key, value, cu_seqlens_q.contiguous(), cu_seqlens_k.contiguous(), None if seqused_k is None else seqused_k.contiguous(),
        is_causal=is_causal, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics, sm_scale=0.0 if scale is None else float(scale),
        precision=precision, return_lse=return_lse, smooth_k=smooth_k)
    if return_lse:
        return res
    return res, torch.empty((0,), dtype=torch.float32, device=query.device)


@_register_fake("quantumattention_amd::fp8_varlen_attention_forward_fp8pv")
def _(query, key, value, cu_seqlens_q, cu_seqlens_k, seqused_k=None, max_seqlen_q=0, max_seqlen_k=0, is_causal=False, fp8_format="e4m3",
      numerics="compiled", return_lse=False, smooth_k=False, precision="accurate", *, scale=None):
    out = query.new_empty((query.shape[0], query.shape[1], value.shape[2]), dtype=value.dtype)
    lse = query.new_empty((query.shape[1], query.shape[0]) if return_lse else (0,), dtype=torch.float32)
    return out, lse


@_custom_op("quantumattention_amd::fp8_varlen_window_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_varlen_window_attention_forward(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    cu_seqlens_k: torch.Tensor,
    seqused_k: Optional[torch.Tensor] = None,
    max_seqlen_q: int = 0,
    max_seqlen_k: int = 0,
    window_left: int = -1,
    window_right: int = -1,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    return_lse: bool = False,
    smooth_k: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Sliding-window attention on packed sequences (include/qattn_window.h): the tensors and results of fp8_varlen_attention_forward;
    row r of a sequence attends keys r + delta - window_left .. r + delta + window_right, delta = L_k(used) - L_q (flash-attn's
    window_size; -1 = unbounded on that side).  A row without a key gives a zero row and an LSE of -inf.  max_seqlen_*: signature
    compatibility only.  Arguments are validated by varlen.fp8_attn_varlen_window_func."""
    del max_seqlen_q, max_seqlen_k
    res = _native.fp8_quant_attention_varlen_window(
        query, key, value, cu_seqlens_q.contiguous(), cu_seqlens_k.contiguous(), None if seqused_k is None else seqused_k.contiguous(),
        window_left=window_left, window_right=window_right, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics,
        sm_scale=0.0 if scale is None else float(scale), return_lse=return_lse, smooth_k=smooth_k)
    if return_lse:
        return res
    return res, torch.empty((0,), dtype=torch.float32, device=query.device)


@_register_fake("quantumattention_amd::fp8_varlen_window_attention_forward")
def _(query, key, value, cu_seqlens_q, cu_seqlens_k, seqused_k=None, max_seqlen_q=0, max_seqlen_k=0, window_left=-1, window_right=-1,
      fp8_format="e4m3", numerics="compiled", return_lse=False, smooth_k=False, *, scale=None):
    out = query.new_empty((query.shape[0], query.shape[1], value.shape[2]), dtype=value.dtype)
    lse = query.new_empty((query.shape[1], query.shape[0]) if return_lse else (0,), dtype=torch.float32)
    return out, lse


@_custom_op("quantumattention_amd::fp8_varlen_window_attention_forward_fp8pv", mutates_args=(), device_types=("cuda",))
def fp8_varlen_window_attention_forward_fp8pv(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    cu_seqlens_k: torch.Tensor,
    seqused_k: Optional[torch.Tensor] = None,
    max_seqlen_q: int = 0,
    max_seqlen_k: int = 0,
    window_left: int = -1,
    window_right: int = -1,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    return_lse: bool = False,
    smooth_k: bool = False,
    precision: str = "accurate",
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Sliding-window attention on packed sequences with FP8 P.V (include/qattn_window.h, ..._window_forward_fp8pv): the tensors, window and
    results of fp8_varlen_window_attention_forward; value is quantised head-wise per (sequence, head) over the used keys, P is e4m3 --
    two-term everywhere (precision "accurate") or one-term byte-exponential for the 128-row tiles whose rows attend an interval of
    >= 1024 keys ("fast").  Arguments are validated by varlen.fp8_attn_varlen_window_pv_func."""
    del max_seqlen_q, max_seqlen_k
    res = _native.fp8_quant_attention_varlen_window_fp8pv(
        query, key, value, cu_seqlens_q.contiguous(), cu_seqlens_k.contiguous(), None if seqused_k is None else seqused_k.contiguous(),
        window_left=window_left, window_right=window_right, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics,
        sm_scale=0.0 if scale is None else float(scale), precision=precision, return_lse=return_lse, smooth_k=smooth_k)
    if return_lse:
        return res
    return res, torch.empty((0,), dtype=torch.float32, device=query.device)


@_register_fake("quantumattention_amd::fp8_varlen_window_attention_forward_fp8pv")
def _(query, key, value, cu_seqlens_q, cu_seqlens_k, seqused_k=None, max_seqlen_q=0, max_seqlen_k=0, window_left=-1, window_right=-1,
      fp8_format="e4m3", numerics="compiled", return_lse=False, smooth_k=False, precision="accurate", *, scale=None):
    out = query.new_empty((query.shape[0], query.shape[1], value.shape[2]), dtype=value.dtype)
    lse = query.new_empty((query.shape[1], query.shape[0]) if return_lse else (0,), dtype=torch.float32)
    return out, lse


@_custom_op("quantumattention_amd::fp8_block_sparse_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_block_sparse_attention_forward(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    block_mask: torch.Tensor,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    return_lse: bool = False,
    smooth_k: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Block-sparse attention (include/qattn_block_sparse.h): query [B, Hq, Sq, D], key / value [B, Hkv, Skv, D] bf16 / fp16, block_mask
    bool [B, Hq, ceil(Sq/128), ceil(Skv/128)] (an expanded view is read through its strides); head-wise fp8 scales over the whole tensors,
    16-bit P on the 16-bit value.  Returns (out [B, Hq, Sq, D], lse fp32 [B, Hq, Sq] -- or an empty [0] tensor without return_lse).
    smooth_k: key smoothing over the whole key sequence (include/qattn_smooth.h; config.attention.smooth_k).
    Arguments are validated by block_sparse.fp8_block_sparse_attn_func."""
    res = _native.fp8_block_sparse_attention(query, key, value, block_mask, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics,
                                             sm_scale=0.0 if scale is None else float(scale), return_lse=return_lse, smooth_k=smooth_k)
    if return_lse:
        return res
    return res, torch.empty((0,), dtype=torch.float32, device=query.device)


@_register_fake("quantumattention_amd::fp8_block_sparse_attention_forward")
def _(query, key, value, block_mask, fp8_format="e4m3", numerics="compiled", return_lse=False, smooth_k=False, *, scale=None):
    B, Hq, Sq = query.shape[0], query.shape[1], query.shape[2]
    out = query.new_empty((B, Hq, Sq, value.shape[3]), dtype=value.dtype)
    lse = query.new_empty((B, Hq, Sq) if return_lse else (0,), dtype=torch.float32)
    return out, lse


@_custom_op("quantumattention_amd::fp8_block_sparse_attention_forward_fp8pv", mutates_args=(), device_types=("cuda",))
def fp8_block_sparse_attention_forward_fp8pv(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    block_mask: torch.Tensor,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    return_lse: bool = False,
    smooth_k: bool = False,
    precision: str = "accurate",
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Block-sparse attention with FP8 P.V (include/qattn_block_sparse.h, ..._forward_fp8pv): the tensors and results of
    fp8_block_sparse_attention_forward; value is quantised head-wise over the whole tensor, P is e4m3 -- two-term everywhere
    (precision "accurate") or one-term byte-exponential for the query blocks that list >= 1024 keys ("fast").
    Arguments are validated by block_sparse.fp8_block_sparse_attn_pv_func."""
    res = _native.fp8_block_sparse_attention_fp8pv(query, key, value, block_mask, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics,
                                                   sm_scale=0.0 if scale is None else float(scale), precision=precision,
                                                   return_lse=return_lse, smooth_k=smooth_k)
    if return_lse:
        return res
    return res, torch.empty((0,), dtype=torch.float32, device=query.device)


@_register_fake("quantumattention_amd::fp8_block_sparse_attention_forward_fp8pv")
def _(query, key, value, block_mask, fp8_format="e4m3", numerics="compiled", return_lse=False, smooth_k=False, precision="accurate", *,
      scale=None):
    B, Hq, Sq = query.shape[0], query.shape[1], query.shape[2]
    out = query.new_empty((B, Hq, Sq, value.shape[3]), dtype=value.dtype)
    lse = query.new_empty((B, Hq, Sq) if return_lse else (0,), dtype=torch.float32)
    return out, lse


@_custom_op("quantumattention_amd::attention_state_merge", mutates_args=(), device_types=("cuda",))
def attention_state_merge(outs: Sequence[torch.Tensor], lses: Sequence[torch.Tensor],
                          out_dtype: Optional[torch.dtype] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Merging of 2 .. 8 attention states in one launch (include/qattn_merge.h): outs[i] [B, H, S, D] with lses[i] fp32 [B, H, S], or packed
    [total, H, D] with [H, total] -- partial results of the same queries over disjoint key sets, bf16 / fp16 / fp32 each, read through
    their strides -> (out, lse) over the union, dense, out in out_dtype (default: outs[0]'s).  A partial whose LSE is -inf contributes
    nothing; a row whose partials are all at -inf is a zero row with LSE -inf.  Reference implementation: merge.merge_attn_states_eager.
    Arguments are validated by merge.merge_attn_states."""
    return _native.attention_state_merge(list(outs), list(lses), out_dtype=out_dtype, return_lse=True)


@_register_fake("quantumattention_amd::attention_state_merge")
def _(outs, lses, out_dtype=None):
    return (outs[0].new_empty(outs[0].shape, dtype=out_dtype or outs[0].dtype), lses[0].new_empty(lses[0].shape, dtype=torch.float32))


@_custom_op("quantumattention_amd::attention_state_merge_", mutates_args=("acc", "acc_lse"), device_types=("cuda",))
def attention_state_merge_(acc: torch.Tensor, acc_lse: torch.Tensor, outs: Sequence[torch.Tensor], lses: Sequence[torch.Tensor]) -> None:
    """The same merge IN PLACE: the state (acc, acc_lse) is partial 0 and receives the result -- the accumulate of a ring step; outs / lses
    are the 1 .. 7 further partials and may not overlap acc / acc_lse."""
    _native.attention_state_merge([acc] + list(outs), [acc_lse] + list(lses), out=acc, lse_out=acc_lse)


@_register_fake("quantumattention_amd::attention_state_merge_")
def _(acc, acc_lse, outs, lses):
    return None


@_custom_op("quantumattention_amd::fp8_rope_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_rope_attention_forward(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    cos_k: Optional[torch.Tensor] = None,
    sin_k: Optional[torch.Tensor] = None,
    interleaved: bool = False,
    is_causal: bool = False,
    scaling_method: str = "head-wise",
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    precision: str = "auto",
    pv_16bit: bool = False,
    return_lse: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """FP8 attention on UNROTATED 16-bit query / key (include/qattn_rope.h): query [B, Hq, Sq, D], key / value [B, Hkv, Skv, D] bf16 / fp16;
    cos / sin fp32 [T, D/2] or [B, T, D/2] rotate the query, cos_k / sin_k (default: the query's) the key, inside the quant pre-pass;
    interleaved: pairs (2i, 2i+1) instead of (i, i + D/2).  Then the fp8 attention entry on the result (pv_16bit: 16-bit P on the 16-bit
    value).  Returns (out [B, Hq, Sq, D], lse fp32 [B, Hq, Sq] -- or an empty [0] tensor without return_lse).  Reference implementation:
    rope.apply_rope_eager + the separate calls.  Arguments are validated by rope.fp8_attn_rope_func."""
    res = _native.fp8_rope_quant_attention(
        query, key, value, cos, sin, cos if cos_k is None else cos_k, sin if sin_k is None else sin_k, interleaved=interleaved,
        is_causal=is_causal, scaling=scaling_method, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics,
        sm_scale=0.0 if scale is None else float(scale), precision=precision, pv_16bit=pv_16bit, return_lse=return_lse)
    if return_lse:
        return res
    return res, torch.empty((0,), dtype=torch.float32, device=query.device)


@_register_fake("quantumattention_amd::fp8_rope_attention_forward")
def _(query, key, value, cos, sin, cos_k=None, sin_k=None, interleaved=False, is_causal=False, scaling_method="head-wise", fp8_format="e4m3",
      numerics="compiled", precision="auto", pv_16bit=False, return_lse=False, *, scale=None):
    B, Hq, Sq = query.shape[0], query.shape[1], query.shape[2]
    out = query.new_empty((B, Hq, Sq, value.shape[3]), dtype=value.dtype)
    lse = query.new_empty((B, Hq, Sq) if return_lse else (0,), dtype=torch.float32)
    return out, lse


@_custom_op("quantumattention_amd::fp8_splitkv_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_splitkv_attention_forward(
    query: torch.Tensor,
    k_frag: torch.Tensor,
    v_frag: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    seqused_k: Optional[torch.Tensor],
    seqlen_k: int,
    num_splits: int,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    is_causal: bool = False,
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Split-KV FP8 attention of a short query over PREPARED keys / values (include/qattn_splitkv.h): query [B, Hq, Sq, D] bf16 / fp16;
    k_frag / v_frag the KFRAG / VFRAG images (flat uint8) of [B, Hkv, seqlen_k, D] with scale_k / scale_v fp32 [B, Hkv]
    (splitkv.prepare_kv_fp8); seqused_k int32 [B] or None, read on the device; num_splits 1 .. 64 (the caller has resolved the auto rule:
    the partials' shape depends on it).  Returns (out, lse, partial_o, partial_lse, partial_path); what was not asked for, and the
    partials of a one-split call, are empty tensors.  Reference implementation: splitkv._splitkv_eager.  Arguments are validated by
    splitkv.fp8_attn_splitkv_func."""
    res = _native.fp8_attention_splitkv(
        query, k_frag, v_frag, scale_k, scale_v, Skv=seqlen_k, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics,
        is_causal=is_causal, sm_scale=0.0 if scale is None else float(scale), precision=precision, num_splits=num_splits,
        seqused_k=seqused_k, return_lse=return_lse, return_partials=return_partials)
    res = res if isinstance(res, tuple) else (res,)
    none_f = lambda: torch.empty((0,), dtype=torch.float32, device=query.device)
    out = res[0]
    lse = res[1] if return_lse else none_f()
    parts = res[-3:] if return_partials else (none_f(), none_f(), torch.empty((0,), dtype=torch.uint8, device=query.device))
    return (out, lse) + tuple(parts)


@_register_fake("quantumattention_amd::fp8_splitkv_attention_forward")
def _(query, k_frag, v_frag, scale_k, scale_v, seqused_k, seqlen_k, num_splits, fp8_format="e4m3", numerics="compiled", is_causal=False,
      precision="accurate", return_lse=False, return_partials=False, *, scale=None):
    B, Hq, Sq, D = query.shape
    out = query.new_empty((B, Hq, Sq, D))
    lse = query.new_empty((B, Hq, Sq) if return_lse else (0,), dtype=torch.float32)
    n = num_splits if num_splits > 1 else 0
    if return_partials:
        return (out, lse, query.new_empty((n, B, Hq, Sq, D), dtype=torch.float32), query.new_empty((n, B, Hq, Sq), dtype=torch.float32),
                query.new_empty((n, B, Hq, Sq), dtype=torch.uint8))
    return (out, lse, query.new_empty((0,), dtype=torch.float32), query.new_empty((0,), dtype=torch.float32),
            query.new_empty((0,), dtype=torch.uint8))


@_custom_op("quantumattention_amd::fp8_kv_cache_append_", mutates_args=("k_frag", "v_frag", "seqlens"), device_types=("cuda",))
def fp8_kv_cache_append_(
    k_frag: torch.Tensor,
    v_frag: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    seqlens: torch.Tensor,
    k_new: torch.Tensor,
    v_new: torch.Tensor,
    new_lens: Optional[torch.Tensor],
    capacity: int,
    fp8_format: str = "e4m3",
    advance: bool = True,
) -> None:
    """Append to an FP8 K/V cache with fixed scales IN PLACE (include/qattn_kvcache.h): k_new / v_new [B, Hkv, T, D] bf16 / fp16 are
    quantised with scale_k / scale_v fp32 [B, Hkv] and written into the KFRAG / VFRAG images k_frag / v_frag (flat uint8) of
    [B, Hkv, capacity, D] from key seqlens[b] on; seqlens int32 [B] and new_lens (int32 [B] or None) are read on the device, seqlens is
    advanced unless advance is False.  Reference implementation: kvcache._append_eager.  Arguments are validated by
    kvcache.kv_cache_append_fp8."""
    _native.kv_cache_append_fp8(k_frag, v_frag, scale_k, scale_v, seqlens, k_new, v_new, capacity=capacity,
                                fp8_dtype=_native.fp8_dtype_of(fp8_format), new_lens=new_lens, advance=advance)


@_register_fake("quantumattention_amd::fp8_kv_cache_append_")
def _(k_frag, v_frag, scale_k, scale_v, seqlens, k_new, v_new, new_lens, capacity, fp8_format="e4m3", advance=True):
    return None


@_custom_op("quantumattention_amd::fp8_paged_splitkv_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_paged_splitkv_attention_forward(
    query: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqused_k: torch.Tensor,
    seqlen_k: int,
    num_pages: int,
    page_size: int,
    num_splits: int,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    is_causal: bool = False,
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Split-KV FP8 attention of a short query over a PAGED cache (include/qattn_paged.h): fp8_splitkv_attention_forward with the pools
    k_pool / v_pool (flat uint8: the KFRAG / VFRAG images of [num_pages, Hkv, page_size, D]) and block_table int32 [B, max_pages] in place
    of the contiguous images; seqlen_k <= max_pages page_size is the logical bound, seqused_k int32 [B] is required; table and lengths are
    read on the device.  Returns (out, lse, partial_o, partial_lse, partial_path) as that op does.  Reference implementation:
    paged._attend_eager.  Arguments are validated by paged.fp8_attn_paged_func."""
    res = _native.fp8_attention_paged_splitkv(
        query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, Skv=seqlen_k, num_pages=num_pages, page_size=page_size,
        fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics, is_causal=is_causal, sm_scale=0.0 if scale is None else float(scale),
        precision=precision, num_splits=num_splits, return_lse=return_lse, return_partials=return_partials)
    res = res if isinstance(res, tuple) else (res,)
    none_f = lambda: torch.empty((0,), dtype=torch.float32, device=query.device)
    out = res[0]
    lse = res[1] if return_lse else none_f()
    parts = res[-3:] if return_partials else (none_f(), none_f(), torch.empty((0,), dtype=torch.uint8, device=query.device))
    return (out, lse) + tuple(parts)


@_register_fake("quantumattention_amd::fp8_paged_splitkv_attention_forward")
def _(query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, seqlen_k, num_pages, page_size, num_splits, fp8_format="e4m3",
      numerics="compiled", is_causal=False, precision="accurate", return_lse=False, return_partials=False, *, scale=None):
    B, Hq, Sq, D = query.shape
    out = query.new_empty((B, Hq, Sq, D))
    lse = query.new_empty((B, Hq, Sq) if return_lse else (0,), dtype=torch.float32)
    n = num_splits if num_splits > 1 else 0
    if return_partials:
        return (out, lse, query.new_empty((n, B, Hq, Sq, D), dtype=torch.float32), query.new_empty((n, B, Hq, Sq), dtype=torch.float32),
                query.new_empty((n, B, Hq, Sq), dtype=torch.uint8))
    return (out, lse, query.new_empty((0,), dtype=torch.float32), query.new_empty((0,), dtype=torch.float32),
            query.new_empty((0,), dtype=torch.uint8))


@_custom_op("quantumattention_amd::fp8_paged_kv_cache_append_", mutates_args=("k_pool", "v_pool", "seqlens"), device_types=("cuda",))
def fp8_paged_kv_cache_append_(
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqlens: torch.Tensor,
    k_new: torch.Tensor,
    v_new: torch.Tensor,
    new_lens: Optional[torch.Tensor],
    num_pages: int,
    page_size: int,
    fp8_format: str = "e4m3",
    advance: bool = True,
) -> None:
    """Append to a PAGED FP8 K/V cache IN PLACE (include/qattn_paged.h): fp8_kv_cache_append_ into the pools k_pool / v_pool (flat uint8: the
    KFRAG / VFRAG images of [num_pages, Hkv, page_size, D]) through block_table int32 [B, max_pages]; capacity = max_pages page_size.
    Reference implementation: paged._append_eager.  Arguments are validated by paged.paged_kv_cache_append_fp8."""
    _native.paged_kv_cache_append_fp8(k_pool, v_pool, scale_k, scale_v, block_table, seqlens, k_new, v_new, num_pages=num_pages,
                                      page_size=page_size, fp8_dtype=_native.fp8_dtype_of(fp8_format), new_lens=new_lens, advance=advance)


@_register_fake("quantumattention_amd::fp8_paged_kv_cache_append_")
def _(k_pool, v_pool, scale_k, scale_v, block_table, seqlens, k_new, v_new, new_lens, num_pages, page_size, fp8_format="e4m3", advance=True):
    return None


@_custom_op("quantumattention_amd::fp8_paged_varlen_kv_cache_append_", mutates_args=("k_pool", "v_pool", "seqlens"), device_types=("cuda",))
def fp8_paged_varlen_kv_cache_append_(
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqlens: torch.Tensor,
    k_new: torch.Tensor,
    v_new: torch.Tensor,
    cu_seqlens: torch.Tensor,
    num_pages: int,
    page_size: int,
    fp8_format: str = "e4m3",
    advance: bool = True,
) -> None:
    """Append PACKED tokens to a paged FP8 K/V cache IN PLACE (include/qattn_paged_varlen_append.h): fp8_paged_kv_cache_append_ on k_new /
    v_new [total, Hkv, D], slot b owning the rows cu_seqlens[b] .. cu_seqlens[b + 1] (int32 [B + 1], read on the device).
    Reference implementation: paged_varlen._append_varlen_eager.  Arguments are validated by paged_varlen.paged_kv_cache_append_varlen_fp8."""
    _native.paged_kv_cache_append_varlen_fp8(k_pool, v_pool, scale_k, scale_v, block_table, seqlens, k_new, v_new, cu_seqlens,
                                             num_pages=num_pages, page_size=page_size, fp8_dtype=_native.fp8_dtype_of(fp8_format),
                                             advance=advance)


@_register_fake("quantumattention_amd::fp8_paged_varlen_kv_cache_append_")
def _(k_pool, v_pool, scale_k, scale_v, block_table, seqlens, k_new, v_new, cu_seqlens, num_pages, page_size, fp8_format="e4m3", advance=True):
    return None


@_custom_op("quantumattention_amd::fp8_paged_varlen_rope_kv_cache_append_", mutates_args=("k_pool", "v_pool", "seqlens"), device_types=("cuda",))
def fp8_paged_varlen_rope_kv_cache_append_(
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqlens: torch.Tensor,
    k_new: torch.Tensor,
    v_new: torch.Tensor,
    cu_seqlens: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    num_pages: int,
    page_size: int,
    fp8_format: str = "e4m3",
    interleaved: bool = False,
    advance: bool = True,
) -> None:
    """fp8_paged_varlen_kv_cache_append_ with K rotated inside the append (include/qattn_paged_varlen_rope.h): key p + t of a slot rotates
    with row min(p + t, T - 1) of cos / sin (fp32 [T, D/2], read in place) before it is quantised.
    Reference implementation: paged_varlen._append_varlen_rope_eager.  Arguments are validated by
    paged_varlen.paged_kv_cache_append_varlen_rope_fp8."""
    _native.paged_kv_cache_append_varlen_rope_fp8(k_pool, v_pool, scale_k, scale_v, block_table, seqlens, k_new, v_new, cu_seqlens, cos, sin,
                                                  num_pages=num_pages, page_size=page_size, fp8_dtype=_native.fp8_dtype_of(fp8_format),
                                                  interleaved=interleaved, advance=advance)


@_register_fake("quantumattention_amd::fp8_paged_varlen_rope_kv_cache_append_")
def _(k_pool, v_pool, scale_k, scale_v, block_table, seqlens, k_new, v_new, cu_seqlens, cos, sin, num_pages, page_size, fp8_format="e4m3",
      interleaved=False, advance=True):
    return None


@_custom_op("quantumattention_amd::rope_paged_varlen", mutates_args=(), device_types=("cuda",))
def rope_paged_varlen(
    x: torch.Tensor,
    seqlens: torch.Tensor,
    cu_seqlens: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    capacity: int,
    interleaved: bool = False,
    appended: bool = False,
) -> torch.Tensor:
    """Packed rows x [total, H, D] rotated at the positions of a paged cache's slots (include/qattn_paged_varlen_rope.h) -> dense
    [total, H, D]; rows behind cu_seqlens[B] have unspecified contents.  Reference implementation: paged_varlen._rope_paged_varlen_eager.
    Arguments are validated by paged_varlen.apply_rope_paged_varlen."""
    return _native.rope_paged_varlen(x, seqlens, cu_seqlens, cos, sin, capacity=capacity, interleaved=interleaved, appended=appended)


@_register_fake("quantumattention_amd::rope_paged_varlen")
def _(x, seqlens, cu_seqlens, cos, sin, capacity, interleaved=False, appended=False):
    return x.new_empty(x.shape)


@_custom_op("quantumattention_amd::fp8_paged_varlen_splitkv_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_paged_varlen_splitkv_attention_forward(
    query: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqused_k: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    max_seqlen_q: int,
    seqlen_k: int,
    num_pages: int,
    page_size: int,
    num_splits: int,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    is_causal: bool = False,
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Split-KV FP8 attention of PACKED queries over a paged cache (include/qattn_paged_varlen.h): query [total_q, Hq, D] cut by
    cu_seqlens_q int32 [B + 1], a different count per sequence slot; the pools, the table, seqused_k and seqlen_k as
    fp8_paged_splitkv_attention_forward; num_splits >= 1 (resolved by the caller).  Returns (out [total_q, Hq, D], lse [Hq, total_q],
    partial_o [ns, total_q, Hq, D], partial_lse [ns, Hq, total_q], partial_path); what was not asked for is an empty tensor.  Reference
    implementation: paged._attend_varlen_eager.  Arguments are validated by paged.fp8_attn_paged_varlen_func."""
    res = _native.fp8_attention_paged_varlen(
        query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, cu_seqlens_q, max_seqlen_q=max_seqlen_q, Skv=seqlen_k,
        num_pages=num_pages, page_size=page_size, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics, is_causal=is_causal,
        sm_scale=0.0 if scale is None else float(scale), precision=precision, num_splits=num_splits, return_lse=return_lse,
        return_partials=return_partials)
    res = res if isinstance(res, tuple) else (res,)
    none_f = lambda: torch.empty((0,), dtype=torch.float32, device=query.device)
    out = res[0]
    lse = res[1] if return_lse else none_f()
    parts = res[-3:] if return_partials else (none_f(), none_f(), torch.empty((0,), dtype=torch.uint8, device=query.device))
    return (out, lse) + tuple(parts)


@_register_fake("quantumattention_amd::fp8_paged_varlen_splitkv_attention_forward")
def _(query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, cu_seqlens_q, max_seqlen_q, seqlen_k, num_pages, page_size, num_splits,
      fp8_format="e4m3", numerics="compiled", is_causal=False, precision="accurate", return_lse=False, return_partials=False, *, scale=None):
    total_q, Hq, D = query.shape
    out = query.new_empty((total_q, Hq, D))
    lse = query.new_empty((Hq, total_q) if return_lse else (0,), dtype=torch.float32)
    n = num_splits if num_splits > 1 else 0
    if return_partials:
        return (out, lse, query.new_empty((n, total_q, Hq, D), dtype=torch.float32), query.new_empty((n, Hq, total_q), dtype=torch.float32),
                query.new_empty((n, Hq, total_q), dtype=torch.uint8))
    return (out, lse, query.new_empty((0,), dtype=torch.float32), query.new_empty((0,), dtype=torch.float32),
            query.new_empty((0,), dtype=torch.uint8))


# ---- the three split-KV ops under a sliding window (include/qattn_splitkv_window.h): the sibling's arguments with is_causal replaced by
# window_left, window_right (each >= -1).  They always run the window kernels, also for (-1, 0) and (-1, -1).

def _skv_pack(res, query, return_lse, return_partials):
    """(out, lse, partial_o, partial_lse, partial_path) of a _native split-KV result: what was not asked for is an empty tensor."""
    res = res if isinstance(res, tuple) else (res,)
    none_f = lambda: torch.empty((0,), dtype=torch.float32, device=query.device)
    lse = res[1] if return_lse else none_f()
    parts = res[-3:] if return_partials else (none_f(), none_f(), torch.empty((0,), dtype=torch.uint8, device=query.device))
    return (res[0], lse) + tuple(parts)


def _skv_fake(query, rows_o, rows_l, num_splits, return_lse, return_partials):
    """The fake result of a split-KV op: rows_o / rows_l are the shapes of out without D / of lse."""
    D = query.shape[-1]
    out = query.new_empty(tuple(rows_o) + (D,))
    lse = query.new_empty(tuple(rows_l) if return_lse else (0,), dtype=torch.float32)
    n = num_splits if num_splits > 1 else 0
    if return_partials:
        return (out, lse, query.new_empty((n,) + tuple(rows_o) + (D,), dtype=torch.float32),
                query.new_empty((n,) + tuple(rows_l), dtype=torch.float32), query.new_empty((n,) + tuple(rows_l), dtype=torch.uint8))
    return (out, lse, query.new_empty((0,), dtype=torch.float32), query.new_empty((0,), dtype=torch.float32),
            query.new_empty((0,), dtype=torch.uint8))


@_custom_op("quantumattention_amd::fp8_splitkv_window_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_splitkv_window_attention_forward(
    query: torch.Tensor,
    k_frag: torch.Tensor,
    v_frag: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    seqused_k: Optional[torch.Tensor],
    seqlen_k: int,
    num_splits: int,
    window_left: int,
    window_right: int,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8_splitkv_attention_forward under a sliding window (include/qattn_splitkv_window.h).  Reference implementation:
    splitkv._splitkv_eager with window=.  Arguments are validated by splitkv_window.fp8_attn_splitkv_window_func."""
    res = _native.fp8_attention_splitkv(
        query, k_frag, v_frag, scale_k, scale_v, Skv=seqlen_k, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics,
        sm_scale=0.0 if scale is None else float(scale), precision=precision, num_splits=num_splits, seqused_k=seqused_k,
        return_lse=return_lse, return_partials=return_partials, window=(window_left, window_right))
    return _skv_pack(res, query, return_lse, return_partials)


@_register_fake("quantumattention_amd::fp8_splitkv_window_attention_forward")
def _(query, k_frag, v_frag, scale_k, scale_v, seqused_k, seqlen_k, num_splits, window_left, window_right, fp8_format="e4m3",
      numerics="compiled", precision="accurate", return_lse=False, return_partials=False, *, scale=None):
    B, Hq, Sq, _ = query.shape
    return _skv_fake(query, (B, Hq, Sq), (B, Hq, Sq), num_splits, return_lse, return_partials)


@_custom_op("quantumattention_amd::fp8_paged_splitkv_window_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_paged_splitkv_window_attention_forward(
    query: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqused_k: torch.Tensor,
    seqlen_k: int,
    num_pages: int,
    page_size: int,
    num_splits: int,
    window_left: int,
    window_right: int,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8_paged_splitkv_attention_forward under a sliding window (include/qattn_splitkv_window.h).  Reference implementation:
    paged._attend_eager with window=.  Arguments are validated by splitkv_window.fp8_attn_paged_window_func."""
    res = _native.fp8_attention_paged_splitkv(
        query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, Skv=seqlen_k, num_pages=num_pages, page_size=page_size,
        fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics, sm_scale=0.0 if scale is None else float(scale), precision=precision,
        num_splits=num_splits, return_lse=return_lse, return_partials=return_partials, window=(window_left, window_right))
    return _skv_pack(res, query, return_lse, return_partials)


@_register_fake("quantumattention_amd::fp8_paged_splitkv_window_attention_forward")
def _(query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, seqlen_k, num_pages, page_size, num_splits, window_left, window_right,
      fp8_format="e4m3", numerics="compiled", precision="accurate", return_lse=False, return_partials=False, *, scale=None):
    B, Hq, Sq, _ = query.shape
    return _skv_fake(query, (B, Hq, Sq), (B, Hq, Sq), num_splits, return_lse, return_partials)


@_custom_op("quantumattention_amd::fp8_paged_varlen_splitkv_window_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_paged_varlen_splitkv_window_attention_forward(
    query: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqused_k: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    max_seqlen_q: int,
    seqlen_k: int,
    num_pages: int,
    page_size: int,
    num_splits: int,
    window_left: int,
    window_right: int,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8_paged_varlen_splitkv_attention_forward under a sliding window per sequence (include/qattn_splitkv_window.h).  Reference
    implementation: paged._attend_varlen_eager with window=.  Arguments are validated by splitkv_window.fp8_attn_paged_varlen_window_func."""
    res = _native.fp8_attention_paged_varlen(
        query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, cu_seqlens_q, max_seqlen_q=max_seqlen_q, Skv=seqlen_k,
        num_pages=num_pages, page_size=page_size, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics,
        sm_scale=0.0 if scale is None else float(scale), precision=precision, num_splits=num_splits, return_lse=return_lse,
        return_partials=return_partials, window=(window_left, window_right))
    return _skv_pack(res, query, return_lse, return_partials)


@_register_fake("quantumattention_amd::fp8_paged_varlen_splitkv_window_attention_forward")
def _(query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, cu_seqlens_q, max_seqlen_q, seqlen_k, num_pages, page_size, num_splits,
      window_left, window_right, fp8_format="e4m3", numerics="compiled", precision="accurate", return_lse=False, return_partials=False, *,
      scale=None):
    total_q, Hq, _ = query.shape
    return _skv_fake(query, (total_q, Hq), (Hq, total_q), num_splits, return_lse, return_partials)


# ---- learned attention sinks (include/qattn_sinks.h): the three window ops with `sinks`, fp32 [Hq], after window_right -- a logit per query
# head in the softmax denominator; the partials stay free of it -- and the state merge with the sink as one more state.

@_custom_op("quantumattention_amd::fp8_splitkv_sink_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_splitkv_sink_attention_forward(
    query: torch.Tensor,
    k_frag: torch.Tensor,
    v_frag: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    seqused_k: Optional[torch.Tensor],
    seqlen_k: int,
    num_splits: int,
    window_left: int,
    window_right: int,
    sinks: torch.Tensor,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8_splitkv_window_attention_forward with learned sinks (include/qattn_sinks.h).  Reference implementation: splitkv._splitkv_eager
    with sinks=.  Arguments are validated by sinks.fp8_attn_splitkv_sink_func."""
    res = _native.fp8_attention_splitkv(
        query, k_frag, v_frag, scale_k, scale_v, Skv=seqlen_k, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics,
        sm_scale=0.0 if scale is None else float(scale), precision=precision, num_splits=num_splits, seqused_k=seqused_k,
        return_lse=return_lse, return_partials=return_partials, window=(window_left, window_right), sinks=sinks)
    return _skv_pack(res, query, return_lse, return_partials)


@_register_fake("quantumattention_amd::fp8_splitkv_sink_attention_forward")
def _(query, k_frag, v_frag, scale_k, scale_v, seqused_k, seqlen_k, num_splits, window_left, window_right, sinks, fp8_format="e4m3",
      numerics="compiled", precision="accurate", return_lse=False, return_partials=False, *, scale=None):
    B, Hq, Sq, _ = query.shape
    return _skv_fake(query, (B, Hq, Sq), (B, Hq, Sq), num_splits, return_lse, return_partials)


@_custom_op("quantumattention_amd::fp8_paged_splitkv_sink_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_paged_splitkv_sink_attention_forward(
    query: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqused_k: torch.Tensor,
    seqlen_k: int,
    num_pages: int,
    page_size: int,
    num_splits: int,
    window_left: int,
    window_right: int,
    sinks: torch.Tensor,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8_paged_splitkv_window_attention_forward with learned sinks (include/qattn_sinks.h).  Reference implementation:
    paged._attend_eager with sinks=.  Arguments are validated by sinks.fp8_attn_paged_sink_func."""
    res = _native.fp8_attention_paged_splitkv(
        query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, Skv=seqlen_k, num_pages=num_pages, page_size=page_size,
        fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics, sm_scale=0.0 if scale is None else float(scale), precision=precision,
        num_splits=num_splits, return_lse=return_lse, return_partials=return_partials, window=(window_left, window_right), sinks=sinks)
    return _skv_pack(res, query, return_lse, return_partials)


@_register_fake("quantumattention_amd::fp8_paged_splitkv_sink_attention_forward")
def _(query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, seqlen_k, num_pages, page_size, num_splits, window_left, window_right,
      sinks, fp8_format="e4m3", numerics="compiled", precision="accurate", return_lse=False, return_partials=False, *, scale=None):
    B, Hq, Sq, _ = query.shape
    return _skv_fake(query, (B, Hq, Sq), (B, Hq, Sq), num_splits, return_lse, return_partials)


@_custom_op("quantumattention_amd::fp8_paged_varlen_splitkv_sink_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_paged_varlen_splitkv_sink_attention_forward(
    query: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqused_k: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    max_seqlen_q: int,
    seqlen_k: int,
    num_pages: int,
    page_size: int,
    num_splits: int,
    window_left: int,
    window_right: int,
    sinks: torch.Tensor,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8_paged_varlen_splitkv_window_attention_forward with learned sinks (include/qattn_sinks.h).  Reference implementation:
    paged_varlen._attend_varlen_eager with sinks=.  Arguments are validated by sinks.fp8_attn_paged_varlen_sink_func."""
    res = _native.fp8_attention_paged_varlen(
        query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, cu_seqlens_q, max_seqlen_q=max_seqlen_q, Skv=seqlen_k,
        num_pages=num_pages, page_size=page_size, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics,
        sm_scale=0.0 if scale is None else float(scale), precision=precision, num_splits=num_splits, return_lse=return_lse,
        return_partials=return_partials, window=(window_left, window_right), sinks=sinks)
    return _skv_pack(res, query, return_lse, return_partials)


@_register_fake("quantumattention_amd::fp8_paged_varlen_splitkv_sink_attention_forward")
def _(query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, cu_seqlens_q, max_seqlen_q, seqlen_k, num_pages, page_size, num_splits,
      window_left, window_right, sinks, fp8_format="e4m3", numerics="compiled", precision="accurate", return_lse=False, return_partials=False,
      *, scale=None):
    total_q, Hq, _ = query.shape
    return _skv_fake(query, (total_q, Hq), (Hq, total_q), num_splits, return_lse, return_partials)


@_custom_op("quantumattention_amd::attention_state_merge_sink", mutates_args=(), device_types=("cuda",))
def attention_state_merge_sink(outs: Sequence[torch.Tensor], lses: Sequence[torch.Tensor], sinks: torch.Tensor,
                               out_dtype: Optional[torch.dtype] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """attention_state_merge of 1 .. 8 states with the learned sink of every head, fp32 [H], as one more state without an O row
    (include/qattn_sinks.h): a row whose partials are all at -inf is a zero row with LSE sink_h.  Reference implementation:
    merge.merge_attn_states_eager with sinks=.  Arguments are validated by sinks.merge_attn_states_with_sinks."""
    return _native.attention_state_merge_sink(list(outs), list(lses), sinks, out_dtype=out_dtype, return_lse=True)


@_register_fake("quantumattention_amd::attention_state_merge_sink")
def _(outs, lses, sinks, out_dtype=None):
    return (outs[0].new_empty(outs[0].shape, dtype=out_dtype or outs[0].dtype), lses[0].new_empty(lses[0].shape, dtype=torch.float32))


# ---- tree-shaped speculative decoding on the paged cache (include/qattn_paged_varlen_tree.h): the packed paged op under a draft tree --
# tree_mask, int64 [total_q], in is_causal's place (the call is causal) -- and the compaction of the accepted path.

@_custom_op("quantumattention_amd::fp8_paged_varlen_splitkv_tree_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_paged_varlen_splitkv_tree_attention_forward(
    query: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqused_k: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    tree_mask: torch.Tensor,
    max_seqlen_q: int,
    seqlen_k: int,
    num_pages: int,
    page_size: int,
    num_splits: int,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8_paged_varlen_splitkv_attention_forward(is_causal=True) under a draft tree per sequence slot: in a slot with at most 64 queries
    position p attends a draft key j >= L_b - Sq_b only if bit j - (L_b - Sq_b) of tree_mask[token] is set.  Reference implementation:
    paged_varlen._attend_varlen_eager with tree_mask=.  Arguments are validated by tree.fp8_attn_paged_varlen_tree_func."""
    res = _native.fp8_attention_paged_varlen(
        query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, cu_seqlens_q, max_seqlen_q=max_seqlen_q, Skv=seqlen_k,
        num_pages=num_pages, page_size=page_size, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics, is_causal=True,
        sm_scale=0.0 if scale is None else float(scale), precision=precision, num_splits=num_splits, return_lse=return_lse,
        return_partials=return_partials, tree_mask=tree_mask)
    return _skv_pack(res, query, return_lse, return_partials)


@_register_fake("quantumattention_amd::fp8_paged_varlen_splitkv_tree_attention_forward")
def _(query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, cu_seqlens_q, tree_mask, max_seqlen_q, seqlen_k, num_pages, page_size,
      num_splits, fp8_format="e4m3", numerics="compiled", precision="accurate", return_lse=False, return_partials=False, *, scale=None):
    total_q, Hq, _ = query.shape
    return _skv_fake(query, (total_q, Hq), (Hq, total_q), num_splits, return_lse, return_partials)


@_custom_op("quantumattention_amd::fp8_paged_kv_cache_compact_", mutates_args=("k_pool", "v_pool", "seqlens"), device_types=("cuda",))
def fp8_paged_kv_cache_compact_(
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    block_table: torch.Tensor,
    seqlens: torch.Tensor,
    cu_seqlens: torch.Tensor,
    accept_index: torch.Tensor,
    accept_lens: torch.Tensor,
    num_kv_heads: int,
    head_dim: int,
    num_pages: int,
    page_size: int,
) -> None:
    """Compact the accepted draft keys of a tree-shaped speculative step IN PLACE (include/qattn_paged_varlen_tree.h): in every slot with
    1 .. 64 draft tokens key base + i takes the bytes of key base + accept_index[cu[b] + i] for i < accept_lens[b], and seqlens[b] becomes
    base + accept_lens[b].  Reference implementation: tree._compact_eager.  Arguments are validated by tree.paged_kv_cache_compact_fp8."""
    _native.paged_kv_cache_compact_fp8(k_pool, v_pool, block_table, seqlens, cu_seqlens, accept_index, accept_lens, Hkv=num_kv_heads,
                                       D=head_dim, num_pages=num_pages, page_size=page_size)


@_register_fake("quantumattention_amd::fp8_paged_kv_cache_compact_")
def _(k_pool, v_pool, block_table, seqlens, cu_seqlens, accept_index, accept_lens, num_kv_heads, head_dim, num_pages, page_size):
    return None


# ---- the tree under a sliding window, optionally with learned sinks (include/qattn_paged_varlen_tree_window.h): the tree op's arguments
# with window_left, window_right after num_splits and `sinks`, fp32 [Hq] or None, after them.

@_custom_op("quantumattention_amd::fp8_paged_varlen_splitkv_tree_window_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_paged_varlen_splitkv_tree_window_attention_forward(
    query: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqused_k: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    tree_mask: torch.Tensor,
    max_seqlen_q: int,
    seqlen_k: int,
    num_pages: int,
    page_size: int,
    num_splits: int,
    window_left: int,
    window_right: int,
    sinks: Optional[torch.Tensor] = None,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8_paged_varlen_splitkv_tree_attention_forward under a sliding window (left, 0), left = -1 or left >= 63, optionally with learned
    sinks: a draft token sits at sequence position L_b - Sq_b + depth, depth = the set bits of its word below its own index, and the
    window's lower edge is taken from there.  Reference implementation: paged_varlen._attend_varlen_eager with tree_mask=, window= and
    sinks=.  Arguments are validated by tree.fp8_attn_paged_varlen_tree_window_func."""
    res = _native.fp8_attention_paged_varlen(
        query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, cu_seqlens_q, max_seqlen_q=max_seqlen_q, Skv=seqlen_k,
        num_pages=num_pages, page_size=page_size, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics, is_causal=True,
        sm_scale=0.0 if scale is None else float(scale), precision=precision, num_splits=num_splits, return_lse=return_lse,
        return_partials=return_partials, window=(window_left, window_right), sinks=sinks, tree_mask=tree_mask)
    return _skv_pack(res, query, return_lse, return_partials)


@_register_fake("quantumattention_amd::fp8_paged_varlen_splitkv_tree_window_attention_forward")
def _(query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, cu_seqlens_q, tree_mask, max_seqlen_q, seqlen_k, num_pages, page_size,
      num_splits, window_left, window_right, sinks=None, fp8_format="e4m3", numerics="compiled", precision="accurate", return_lse=False,
      return_partials=False, *, scale=None):
    total_q, Hq, _ = query.shape
    return _skv_fake(query, (total_q, Hq), (Hq, total_q), num_splits, return_lse, return_partials)


# ---- the rotary embedding at the caller's positions (include/qattn_paged_varlen_rope_pos.h): the rotating packed append and the packed
# rotation with `positions`, int64 [total] -- a tree node sits at base + depth.

@_custom_op("quantumattention_amd::fp8_paged_varlen_rope_pos_kv_cache_append_", mutates_args=("k_pool", "v_pool", "seqlens"), device_types=("cuda",))
def fp8_paged_varlen_rope_pos_kv_cache_append_(
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqlens: torch.Tensor,
    k_new: torch.Tensor,
    v_new: torch.Tensor,
    cu_seqlens: torch.Tensor,
    positions: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    num_pages: int,
    page_size: int,
    fp8_format: str = "e4m3",
    interleaved: bool = False,
    advance: bool = True,
) -> None:
    """fp8_paged_varlen_rope_kv_cache_append_ with token t rotated with row clamp(positions[t], 0, T - 1) of cos / sin instead of the row of
    its key's index; where the key is stored is unchanged.  Reference implementation: paged_varlen._append_varlen_rope_pos_eager.
    Arguments are validated by paged_varlen.paged_kv_cache_append_varlen_rope_pos_fp8."""
    _native.paged_kv_cache_append_varlen_rope_pos_fp8(k_pool, v_pool, scale_k, scale_v, block_table, seqlens, k_new, v_new, cu_seqlens, positions,
                                                      cos, sin, num_pages=num_pages, page_size=page_size,
                                                      fp8_dtype=_native.fp8_dtype_of(fp8_format), interleaved=interleaved, advance=advance)


@_register_fake("quantumattention_amd::fp8_paged_varlen_rope_pos_kv_cache_append_")
def _(k_pool, v_pool, scale_k, scale_v, block_table, seqlens, k_new, v_new, cu_seqlens, positions, cos, sin, num_pages, page_size,
      fp8_format="e4m3", interleaved=False, advance=True):
    return None


@_custom_op("quantumattention_amd::rope_packed_positions", mutates_args=(), device_types=("cuda",))
def rope_packed_positions(
    x: torch.Tensor,
    positions: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    interleaved: bool = False,
) -> torch.Tensor:
    """Packed rows x [total, H, D], row t rotated with row clamp(positions[t], 0, T - 1) of cos / sin (include/qattn_paged_varlen_rope_pos.h)
    -> dense [total, H, D].  Reference implementation: rope.apply_rope_eager at those positions.  Arguments are validated by
    paged_varlen.apply_rope_positions."""
    return _native.rope_packed_positions(x, positions, cos, sin, interleaved=interleaved)


@_register_fake("quantumattention_amd::rope_packed_positions")
def _(x, positions, cos, sin, interleaved=False):
    return x.new_empty(x.shape)


# ---- logit soft-capping (include/qattn_softcap.h): the three window ops with the host float `softcap` after window_right --
# y = softcap tanh(x / softcap) on the scaled scores, before the mask.  A model constant: it is baked into a traced or captured graph.

@_custom_op("quantumattention_amd::fp8_splitkv_softcap_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_splitkv_softcap_attention_forward(
    query: torch.Tensor,
    k_frag: torch.Tensor,
    v_frag: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    seqused_k: Optional[torch.Tensor],
    seqlen_k: int,
    num_splits: int,
    window_left: int,
    window_right: int,
    softcap: float,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8_splitkv_window_attention_forward with soft-capped scores (include/qattn_softcap.h).  Reference implementation:
    splitkv._splitkv_eager with softcap=.  Arguments are validated by softcap.fp8_attn_splitkv_softcap_func."""
    res = _native.fp8_attention_splitkv(
        query, k_frag, v_frag, scale_k, scale_v, Skv=seqlen_k, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics,
        sm_scale=0.0 if scale is None else float(scale), precision=precision, num_splits=num_splits, seqused_k=seqused_k,
        return_lse=return_lse, return_partials=return_partials, window=(window_left, window_right), softcap=softcap)
    return _skv_pack(res, query, return_lse, return_partials)


@_register_fake("quantumattention_amd::fp8_splitkv_softcap_attention_forward")
def _(query, k_frag, v_frag, scale_k, scale_v, seqused_k, seqlen_k, num_splits, window_left, window_right, softcap, fp8_format="e4m3",
      numerics="compiled", precision="accurate", return_lse=False, return_partials=False, *, scale=None):
    B, Hq, Sq, _ = query.shape
    return _skv_fake(query, (B, Hq, Sq), (B, Hq, Sq), num_splits, return_lse, return_partials)


@_custom_op("quantumattention_amd::fp8_paged_splitkv_softcap_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_paged_splitkv_softcap_attention_forward(
    query: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqused_k: torch.Tensor,
    seqlen_k: int,
    num_pages: int,
    page_size: int,
    num_splits: int,
    window_left: int,
    window_right: int,
    softcap: float,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8_paged_splitkv_window_attention_forward with soft-capped scores (include/qattn_softcap.h).  Reference implementation:
    paged._attend_eager with softcap=.  Arguments are validated by softcap.fp8_attn_paged_softcap_func."""
    res = _native.fp8_attention_paged_splitkv(
        query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, Skv=seqlen_k, num_pages=num_pages, page_size=page_size,
        fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics, sm_scale=0.0 if scale is None else float(scale), precision=precision,
        num_splits=num_splits, return_lse=return_lse, return_partials=return_partials, window=(window_left, window_right), softcap=softcap)
    return _skv_pack(res, query, return_lse, return_partials)


@_register_fake("quantumattention_amd::fp8_paged_splitkv_softcap_attention_forward")
def _(query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, seqlen_k, num_pages, page_size, num_splits, window_left, window_right,
      softcap, fp8_format="e4m3", numerics="compiled", precision="accurate", return_lse=False, return_partials=False, *, scale=None):
    B, Hq, Sq, _ = query.shape
    return _skv_fake(query, (B, Hq, Sq), (B, Hq, Sq), num_splits, return_lse, return_partials)


@_custom_op("quantumattention_amd::fp8_paged_varlen_splitkv_softcap_attention_forward", mutates_args=(), device_types=("cuda",))
def fp8_paged_varlen_splitkv_softcap_attention_forward(
    query: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    scale_k: torch.Tensor,
    scale_v: torch.Tensor,
    block_table: torch.Tensor,
    seqused_k: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    max_seqlen_q: int,
    seqlen_k: int,
    num_pages: int,
    page_size: int,
    num_splits: int,
    window_left: int,
    window_right: int,
    softcap: float,
    fp8_format: str = "e4m3",
    numerics: str = "compiled",
    precision: str = "accurate",
    return_lse: bool = False,
    return_partials: bool = False,
    *,
    scale: Optional[float] = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8_paged_varlen_splitkv_window_attention_forward with soft-capped scores (include/qattn_softcap.h).  Reference implementation:
    paged_varlen._attend_varlen_eager with softcap=.  Arguments are validated by softcap.fp8_attn_paged_varlen_softcap_func."""
    res = _native.fp8_attention_paged_varlen(
        query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, cu_seqlens_q, max_seqlen_q=max_seqlen_q, Skv=seqlen_k,
        num_pages=num_pages, page_size=page_size, fp8_dtype=_native.fp8_dtype_of(fp8_format), numerics=numerics,
        sm_scale=0.0 if scale is None else float(scale), precision=precision, num_splits=num_splits, return_lse=return_lse,
        return_partials=return_partials, window=(window_left, window_right), softcap=softcap)
    return _skv_pack(res, query, return_lse, return_partials)


@_register_fake("quantumattention_amd::fp8_paged_varlen_splitkv_softcap_attention_forward")
def _(query, k_pool, v_pool, scale_k, scale_v, block_table, seqused_k, cu_seqlens_q, max_seqlen_q, seqlen_k, num_pages, page_size, num_splits,
      window_left, window_right, softcap, fp8_format="e4m3", numerics="compiled", precision="accurate", return_lse=False, return_partials=False,
      *, scale=None):
    total_q, Hq, _ = query.shape
    return _skv_fake(query, (total_q, Hq), (Hq, total_q), num_splits, return_lse, return_partials)

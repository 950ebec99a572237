"""Rotary position embedding (RoPE) fused into the FP8 quant pre-pass (include/qattn_rope.h).

Every model this library serves rotates q and k immediately before attention.  Here the caller hands over the UNROTATED 16-bit q and k
with their cos / sin tables; the pre-pass rotates the values it already holds in registers, and the rotated 16-bit tensors never exist.

The contract (one definition, `apply_rope_eager`, which the HIP kernels reproduce bit for bit): row x[b,h,s,:] is rotated with row s of
fp32 tables cos, sin [T, D/2] (T >= S; or [B, T, D/2], one table per batch element).  `interleaved` is flash-attn's apply_rotary_emb flag:
False pairs (i, i + D/2) (GPT-NeoX / HF rotate_half), True pairs (2i, 2i + 1) (GPT-J; the complex-pair form of Wan and Flux).  For a
pair (a, b) with table entry (c, s):

    y_first  = round16( fl(a c) - fl(b s) )       three separately rounded fp32 operations, no fused multiply-add;
    y_second = round16( fl(b c) + fl(a s) )       round16 = round to nearest even to x's dtype

and the quantiser then sees y.  Rounding through 16 bits is deliberate: the fused path equals "rotate in torch, then call the existing
entries" bit for bit, so it changes time and nothing else.  Only the full head dim is rotated (no partial rotary_dim).  A -0 input may
come out +0; a non-finite input poisons its head's (token-wise: its row's) scale as it does without RoPE.

Package attributes, not names of `__all__` (that list mirrors the reference)."""
import math
from typing import Optional, Tuple

import torch

from . import _native, nn
from .nn import _cfg

_TABLE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_HEAD_DIMS = (64, 128, 256)


def _check_tables(x: torch.Tensor, cos, sin, what: str = "cos / sin") -> Tuple[torch.Tensor, torch.Tensor]:
    """Validate a table pair against x [..., S, D]; returns the pair as fp32 (16-bit tables are up-cast, which is exact)."""
    if not isinstance(cos, torch.Tensor) or not isinstance(sin, torch.Tensor):
        raise ValueError(f"{what} must be tensors")
    if x.dim() < 2:
        raise ValueError(f"the rotated tensor must be [..., S, D], got {x.dim()} dimension(s)")
    S, D = x.shape[-2], x.shape[-1]
    if D % 2 != 0:
        raise ValueError(f"head_dim must be even to be rotated in pairs, got {D}")
    if cos.shape != sin.shape:
        raise ValueError(f"{what} must have the same shape, got {tuple(cos.shape)} and {tuple(sin.shape)}")
    if cos.dtype != sin.dtype or cos.dtype not in _TABLE_DTYPES:
        raise ValueError(f"{what} must share a dtype out of float32, bfloat16, float16, got {cos.dtype} and {sin.dtype}")
    if cos.device != x.device or sin.device != x.device:
        raise ValueError(f"{what} must be on the rotated tensor's device {x.device}, got {cos.device} and {sin.device}")
    if cos.dim() not in (2, 3):
        raise ValueError(f"{what} must be [T, D/2] or [B, T, D/2], got {cos.dim()} dimension(s)")
    if cos.shape[-1] != D // 2:
        raise ValueError(f"{what} must hold D/2 = {D // 2} entries per row, one per rotated pair, got {cos.shape[-1]}: a partial "
                         "rotary_dim is not supported (only the full head dim is rotated), nor is the duplicated [T, D] table layout")
    if cos.dim() == 3 and (x.dim() != 4 or cos.shape[0] != x.shape[0]):
        raise ValueError(f"a [B, T, D/2] table needs a 4-D [B, H, S, D] tensor of the same batch size, got {tuple(cos.shape)} for {tuple(x.shape)}")
    if cos.shape[-2] < S:
        raise ValueError(f"{what} hold T = {cos.shape[-2]} positions, fewer than the sequence length S = {S}")
    return cos.to(torch.float32), sin.to(torch.float32)


def _rotate(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, interleaved: bool) -> torch.Tensor:
    S, D = x.shape[-2], x.shape[-1]
    h = D // 2
    c, s = cos[..., :S, :], sin[..., :S, :]
    if c.dim() == 3:
        c, s = c[:, None], s[:, None]                 # [B, 1, S, D/2] over the heads
    xf = x.to(torch.float32)                          # exact
    a, b = (xf[..., 0::2], xf[..., 1::2]) if interleaved else (xf[..., :h], xf[..., h:])
    ac, bs, bc, as_ = a * c, b * s, b * c, a * s      # every product its own op: no fused multiply-add anywhere
    y0 = ac - bs
    y1 = bc + as_
    y = torch.stack((y0, y1), dim=-1).flatten(-2) if interleaved else torch.cat((y0, y1), dim=-1)
    return y.to(x.dtype)                              # round to nearest even


def apply_rope_eager(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *, interleaved: bool = False) -> torch.Tensor:
    """The definition in torch ops, on any device: x [..., S, D] (bf16 / fp16; a [B, T, D/2] table needs [B, H, S, D]) rotated with rows
    0 .. S-1 of cos / sin [T, D/2] or [B, T, D/2] -> a dense tensor of x's shape and dtype.  Reference implementation of the fused kernels
    (they equal it bit for bit) and the CPU path of this module."""
    if not isinstance(x, torch.Tensor) or x.dtype not in nn._HALF_DTYPES:
        raise ValueError(f"the rotated tensor must be bf16 or fp16, got {getattr(x, 'dtype', type(x))}")
    cos, sin = _check_tables(x, cos, sin)
    return _rotate(x, cos, sin, bool(interleaved)).contiguous()


def _hip(x: torch.Tensor) -> bool:
    return x.is_cuda and not _cfg("force_eager_fallback")


def _check_head_dim(D: int) -> None:
    if D not in _HEAD_DIMS:
        raise ValueError(f"head_dim must be one of {list(_HEAD_DIMS)} for the gfx950 RoPE pre-pass, got {D}")


def rope_quantize_fp8(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *, interleaved: bool = False, scaling: str = "head-wise",
                      fp8_dtype=torch.float8_e4m3fn, numerics: str = "compiled") -> Tuple[torch.Tensor, torch.Tensor]:
    """Rotate x [B, H, S, D] (bf16 / fp16) and quantise it to fp8 in the same pass: (x8 row-major fp8 [B, H, S, D], scale fp32 [B, H] for
    scaling="head-wise" or [B, H, S] for "token-wise").  Bit for bit `quantize(apply_rope_eager(x, cos, sin))` with the library's quantiser
    in the chosen `numerics`.  Strided views of x with head_dim innermost (e.g. a transposed [B, S, H, D] projection) and sliced tables
    (cos[off:off + S]) are read in place.  CPU tensors and config.attention.force_eager_fallback run the eager definition followed by the
    torch quantiser; on the device there is no fallback: head_dim must be 64, 128 or 256."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype not in nn._HALF_DTYPES:
        raise ValueError("rope_quantize_fp8 needs a 4-D [B, H, S, D] bf16 / fp16 tensor")
    if scaling not in ("head-wise", "token-wise"):
        raise ValueError(f"Unsupported scaling: {scaling!r} (expected 'head-wise' or 'token-wise')")
    if fp8_dtype not in (torch.float8_e4m3fn, torch.float8_e5m2):
        raise ValueError(f"fp8_dtype must be torch.float8_e4m3fn or torch.float8_e5m2, got {fp8_dtype}")
    if numerics not in _native.NUMERICS:
        raise ValueError(f"Unsupported numerics: {numerics!r} (expected one of {sorted(_native.NUMERICS)})")
    cos, sin = _check_tables(x, cos, sin)
    if not _hip(x):
        y = _rotate(x, cos, sin, bool(interleaved))
        return nn._dynamically_quantize_fp8(y, reduction_dim=[2, 3] if scaling == "head-wise" else [3], fp8_dtype=fp8_dtype)
    _check_head_dim(x.shape[-1])
    return _native.rope_quant_fp8(x, cos, sin, interleaved=bool(interleaved), scaling=scaling, fp8_dtype=fp8_dtype, numerics=numerics)


def _eager_lse(q, k, is_causal, scale):
    s = (q.to(torch.float32) @ nn._expand_kv_heads(k, q.size(-3)).to(torch.float32).transpose(-1, -2)) * (
        1.0 / math.sqrt(q.size(-1)) if scale is None else scale)
    if is_causal:
        i, j = torch.arange(s.shape[-2], device=s.device)[:, None], torch.arange(s.shape[-1], device=s.device)[None, :]
        s = s.masked_fill(j > i, -math.inf)
    return torch.logsumexp(s, dim=-1)


def fp8_attn_rope_func(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *,
                       cos_k: Optional[torch.Tensor] = None, sin_k: Optional[torch.Tensor] = None, interleaved: bool = False,
                       is_causal: bool = False, scale: Optional[float] = None, scaling: str = "head-wise", pv_precision: str = "fp8",
                       precision: str = "auto", return_lse: bool = False):
    """FP8 attention on UNROTATED q [B, Hq, Sq, D], k [B, Hkv, Skv, D] and v [B, Hkv, Skv, D] (bf16 / fp16): q is rotated with cos / sin, k
    with cos_k / sin_k (default: q's tables; cross-attention, or keys at offset positions, pass their own -- cos[off:off + Skv] is read in
    place), both are quantised in the same pass, and the attention kernels run on the result.  One C call
    (qattn_fp8_rope_quant_attention_forward); q and k may be transposed [B, S, H, D]-backed views.

    Bit for bit the composition `apply_rope_eager` on q and k, the quant pre-pass, the fp8 attention entry (include/qattn.h PATH TABLE,
    rows `separate` / `separate16`) -- with strictly fewer bytes moved and fewer launches.
    scaling: "head-wise" or "token-wise" scales of q and k.  pv_precision: "fp8" (v quantised head-wise, both products on the FP8 matrix
    pipe) or "16bit" (16-bit P on the caller's v).  precision: "auto" / "fast" / "accurate" as config.attention.precision.
    scale: the softmax scale (None: 1/sqrt(D)).  The fp8 format and quantiser numerics follow config.attention.fp8_format /
    quant_numerics.  Key smoothing is not combined with RoPE: config.attention.smooth_k is ignored here.
    Returns out [B, Hq, Sq, D], or (out, lse fp32 [B, Hq, Sq]) with return_lse=True.
    CPU tensors and config.attention.force_eager_fallback: the eager rotation followed by torch SDPA."""
    if not all(isinstance(t, torch.Tensor) for t in (q, k, v)) or not (q.dim() == k.dim() == v.dim() == 4):
        raise ValueError("query, key and value must be 4-D [B, H, S, D] tensors")
    if q.dtype not in nn._HALF_DTYPES or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"query, key and value must share bf16 or fp16, got {q.dtype}, {k.dtype}, {v.dtype}")
    if not (q.device == k.device == v.device):
        raise ValueError("query, key and value must be on the same device")
    B, Hq, Sq, D = q.shape
    if k.shape != v.shape or k.shape[0] != B or k.shape[3] != D:
        raise ValueError(f"key {tuple(k.shape)} / value {tuple(v.shape)} do not match query {tuple(q.shape)} (same batch and head_dim; "
                         "key and value the same shape)")
    if k.shape[1] == 0 or Hq % k.shape[1] != 0:
        raise ValueError(f"Hq={Hq} is not a multiple of Hkv={k.shape[1]}")
    if (cos_k is None) != (sin_k is None):
        raise ValueError("cos_k and sin_k must be both provided or both not provided")
    if scaling not in ("head-wise", "token-wise"):
        raise ValueError(f"Unsupported scaling: {scaling!r} (expected 'head-wise' or 'token-wise')")
    if pv_precision not in ("fp8", "16bit"):
        raise ValueError(f"Unsupported pv_precision: {pv_precision!r} (expected 'fp8' or '16bit')")
    if precision not in _native.PRECISION:
        raise ValueError(f"Unsupported precision: {precision!r} (expected one of {sorted(_native.PRECISION)})")
    if scale is not None and not scale > 0:
        raise ValueError(f"scale must be positive (None: 1/sqrt(head_dim)), got {scale}")
    cq, sq = _check_tables(q, cos, sin, "cos / sin")
    ck, sk = _check_tables(k, cos if cos_k is None else cos_k, sin if sin_k is None else sin_k, "cos / sin" if cos_k is None else "cos_k / sin_k")
    il = bool(interleaved)
    if not _hip(q):
        qr, kr = _rotate(q, cq, sq, il).contiguous(), _rotate(k, ck, sk, il).contiguous()
        out = nn._eager_attention(qr, kr, v, is_causal, scale)
        return (out, _eager_lse(qr, kr, is_causal, scale)) if return_lse else out
    _check_head_dim(D)
    out, lse = nn._ops().fp8_rope_attention_forward(
        q, k, v, cq, sq, ck, sk, il, is_causal, scaling, _cfg("fp8_format"), _cfg("quant_numerics"), precision, pv_precision == "16bit",
        return_lse, scale=scale)
    return (out, lse) if return_lse else out

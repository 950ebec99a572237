"""An appendable FP8 K/V cache with FIXED scales for `fp8_attn_splitkv_func`: `alloc_kv_cache_fp8`, `kv_cache_from_prefill_fp8`,
`kv_cache_append_fp8` and the `KVCacheFP8` they share (include/qattn_kvcache.h).

`prepare_kv_fp8` scales each head over the whole tensor, so nothing can be appended to what it returns.  A decode loop needs the opposite:
scales fixed once -- calibrated, or taken from the prefill with headroom, as deployed FP8 KV caches do -- and new tokens quantised with
them.  A value above scale * qmax saturates: its byte is +-qmax and its error the excess, never a NaN.  The attention side needs nothing
new: `fp8_attn_splitkv_func(q, cache, seqused_k=cache.seqlens, causal=True)` reads the lengths on the device and ignores every byte
behind them.

    cache = kv_cache_from_prefill_fp8(k, v, capacity)                  # or alloc_kv_cache_fp8(..., scale_k=..., scale_v=...)
    for step in ...:
        kv_cache_append_fp8(cache, k_new, v_new)                       # [B, Hkv, T, D]; cache.seqlens += T on the device
        out = fp8_attn_splitkv_func(q, cache, seqused_k=cache.seqlens, causal=True)

Rollback (speculative decoding: the rejected tokens of a draft) is `cache.seqlens.sub_(n)`: legal because bytes behind `seqlens` influence
no output bit of the attention entry, and the next append overwrites them.

Package attributes, not names of `__all__` (that list mirrors the reference).  A paged cache (a pool of pages behind a block table) is
paged.py's (alloc_paged_kv_cache_fp8, paged_kv_cache_append_fp8, fp8_attn_paged_func).  Not offered: re-scaling a
live cache, token-wise K or chunk-wise V scales, key smoothing on cached keys."""
import math
from typing import Optional

import torch
from torch import Tensor

from . import _native, nn
from .splitkv import PreparedKV, _kv_reason
from .utils import checks


class KVCacheFP8(PreparedKV):
    """A `PreparedKV` that can grow: shape is (B, Hkv, capacity, D), scale_k / scale_v are FIXED, and
      seqlens   int32 [B] on the cache's device: the keys batch element b holds.  Pass it to the attention call as seqused_k.
    Bytes of the images behind seqlens are unspecified (zero in a fresh cache) and influence no result."""

    __slots__ = ("seqlens",)

    def __init__(self, k, v, scale_k, scale_v, shape, fp8_format, dtype, numerics, layout, seqlens):
        super().__init__(k, v, scale_k, scale_v, shape, fp8_format, dtype, numerics, layout)
        self.seqlens = seqlens

    @property
    def capacity(self) -> int:
        return self.shape[2]

    def __repr__(self):
        return (f"KVCacheFP8(shape={self.shape}, fp8_format={self.fp8_format!r}, dtype={self.dtype}, numerics={self.numerics!r}, "
                f"layout={self.layout!r}, device={self.device})")


def _is_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


def _scale_reason(name, s, B, Hkv) -> Optional[str]:
    if isinstance(s, (int, float)) and not isinstance(s, bool):
        ok = math.isfinite(s) and s > 0
    elif isinstance(s, Tensor):
        if tuple(s.shape) not in ((Hkv,), (B, Hkv)) or not s.dtype.is_floating_point:
            return f"Expected {name} to be a float or a floating-point tensor of shape [{Hkv}] or [{B}, {Hkv}], but got {s.dtype} {list(s.shape)}."
        ok = bool(torch.isfinite(s).all()) and bool((s > 0).all())   # (reads the tensor on the host: once, when the cache is made)
    else:
        return f"Expected {name} to be a float or a tensor of shape [{Hkv}] or [{B}, {Hkv}], but got {type(s).__name__}."
    return None if ok else f"{name} must be finite and > 0 everywhere (values above {name} * qmax saturate)"


def alloc_kv_cache_input_reason(B, Hkv, capacity, D, scale_k, scale_v, dtype) -> Optional[str]:
    """The first rule the arguments of `alloc_kv_cache_fp8` break, or None."""
    if not all(_is_int(x) and x > 0 for x in (B, Hkv, capacity)):
        return f"Expected a positive batch size, head count and capacity, but got B={B!r}, Hkv={Hkv!r}, capacity={capacity!r}"
    if D not in nn._HIP_SUPPORTED_HEAD_DIMS:
        return f"Unsupported head dimension: {D}"
    if dtype not in (torch.float16, torch.bfloat16):
        return f"Expected dtype to be torch.float16 or torch.bfloat16 (the dtype of the tokens to append), but got {dtype} instead."
    return _scale_reason("scale_k", scale_k, B, Hkv) or _scale_reason("scale_v", scale_v, B, Hkv)


def _new_cache(B, Hkv, capacity, D, scale_k, scale_v, dtype, device, fp8_format, numerics) -> KVCacheFP8:
    """scale_k / scale_v: fp32 [B, Hkv] on `device`, taken as they are"""
    device = torch.device(device)
    fp8_dtype = _native.fp8_dtype_of(fp8_format)
    if numerics not in _native.NUMERICS:
        raise ValueError(f"Unsupported quant_numerics: {numerics!r} (expected one of {sorted(_native.NUMERICS)})")
    seqlens = torch.zeros((B,), dtype=torch.int32, device=device)
    if device.type != "cuda" or checks.config_value("attention.force_eager_fallback"):
        k8, v8 = (torch.zeros((B, Hkv, capacity, D), dtype=torch.uint8, device=device).view(fp8_dtype) for _ in range(2))
        return KVCacheFP8(k8, v8, scale_k, scale_v, (B, Hkv, capacity, D), fp8_format, dtype, numerics, "rowmajor", seqlens)
    ok, why = nn._pre_check_can_use_hip_attention(device=device)
    if not ok:
        raise ValueError(why)
    L = _native.lib()
    kf, vf = (torch.zeros((L.qattn_fp8_tensor_bytes(layout, B, Hkv, capacity, D),), dtype=torch.uint8, device=device)
              for layout in (_native.LAYOUT_KFRAG, _native.LAYOUT_VFRAG))
    return KVCacheFP8(kf, vf, scale_k, scale_v, (B, Hkv, capacity, D), fp8_format, dtype, numerics, "frag", seqlens)


def alloc_kv_cache_fp8(B: int, Hkv: int, capacity: int, D: int, *, scale_k, scale_v, dtype, device, fp8_format: Optional[str] = None,
                       numerics: Optional[str] = None) -> KVCacheFP8:
    """An empty cache for `capacity` keys per (batch element, kv head): zero-filled images, seqlens = 0.
    scale_k / scale_v: the FIXED quantisation scales, a float, a tensor [Hkv] or a tensor [B, Hkv]; finite and > 0 (a tensor is checked
    on the host, once, here); kept as fp32 [B, Hkv].  An appended element x becomes fp8(clamp(round(x / scale), +-qmax)): choose
    scale >= the largest |x| to come / qmax, or accept that larger values saturate at scale * qmax.
    dtype: bf16 / fp16, the dtype of the tokens that will be appended (and of the attention output).  fp8_format defaults to
    config.attention.fp8_format; numerics (config.attention.quant_numerics) is what the attention call quantises q with -- the cache's
    bytes do not depend on it.  A CPU device (and config.attention.force_eager_fallback) gives row-major fp8 tensors for the eager
    definitions."""
    reason = alloc_kv_cache_input_reason(B, Hkv, capacity, D, scale_k, scale_v, dtype)
    if reason:
        raise ValueError(reason)
    fp8_format = checks.config_value("attention.fp8_format") if fp8_format is None else fp8_format
    numerics = checks.config_value("attention.quant_numerics") if numerics is None else numerics
    full = lambda s: (torch.as_tensor(s, dtype=torch.float32, device=device) if isinstance(s, Tensor)
                      else torch.full((), float(s), dtype=torch.float32, device=device)).expand(B, Hkv).contiguous()
    return _new_cache(B, Hkv, capacity, D, full(scale_k), full(scale_v), dtype, device, fp8_format, numerics)


def _prefill_scale(x: Tensor, fp8_dtype, numerics: str, rowmajor: bool) -> Tensor:
    """The head-wise scale `prepare_kv_fp8` gives x [B, H, S, D]: fp32 [B, H], computed where x lives (csrc/qattn_common.h make_scale;
    row-major caches: nn._dynamically_quantize_fp8's expression)."""
    eps = torch.finfo(torch.float32).eps
    inv_qmax = 1.0 / torch.finfo(fp8_dtype).max
    # one read of x and no |x| copy of it, in two steps -- per row, then over the rows -- so that the first runs as B H S reductions side by
    # side (one reduction per head over S D elements runs on B H workgroups: measured 30 x prepare_kv_fp8 at S = 32768); any view with
    # head_dim innermost is read in place; a NaN comes through as it does through the abs-max
    lo, hi = torch.aminmax(x, dim=3)
    amax = torch.maximum(hi.amax(2), -lo.amin(2))
    if rowmajor:
        return amax.mul(inv_qmax).clamp_min(eps).to(torch.float32)
    s = amax.to(torch.float32).mul(inv_qmax)
    if numerics == "eager":   # the scale and eps rounded to the input dtype
        s = s.to(x.dtype).to(torch.float32)
        eps = float(torch.tensor(eps, dtype=torch.float32).to(x.dtype))
    return s.clamp_min(eps)


def kv_cache_from_prefill_fp8(k: Tensor, v: Tensor, capacity: int, *, headroom: float = 2.0, fp8_format: Optional[str] = None,
                              numerics: Optional[str] = None) -> KVCacheFP8:
    """A cache for `capacity` >= Skv keys that holds k, v [B, Hkv, Skv, D] (bf16 / fp16) as its first Skv keys, with the scales
    `prepare_kv_fp8(k, v)` would compute times `headroom` (finite, >= 1): later tokens up to headroom times the prefill's largest
    magnitude still fit, larger ones saturate.  The scales are computed on the device; nothing is read on the host.
    headroom = 1.0 with capacity = Skv reproduces `prepare_kv_fp8(k, v)`'s images and scales bit for bit.  V must be finite."""
    reason = _kv_reason(k, v)
    if reason is None and not (_is_int(capacity) and capacity >= k.shape[2]):
        reason = f"capacity must be an integer >= the prefill's {k.shape[2]} keys, got {capacity!r}"
    if reason is None and not (isinstance(headroom, (int, float)) and not isinstance(headroom, bool) and math.isfinite(headroom) and headroom >= 1):
        reason = f"headroom must be a finite number >= 1, got {headroom!r}"
    if reason:
        raise ValueError(reason)
    fp8_format = checks.config_value("attention.fp8_format") if fp8_format is None else fp8_format
    numerics = checks.config_value("attention.quant_numerics") if numerics is None else numerics
    fp8_dtype = _native.fp8_dtype_of(fp8_format)
    if numerics not in _native.NUMERICS:
        raise ValueError(f"Unsupported quant_numerics: {numerics!r} (expected one of {sorted(_native.NUMERICS)})")
    rowmajor = not k.is_cuda or bool(checks.config_value("attention.force_eager_fallback"))
    sk, sv = (_prefill_scale(x, fp8_dtype, numerics, rowmajor).mul(float(headroom)).contiguous() for x in (k, v))
    B, Hkv, _, D = k.shape
    cache = _new_cache(B, Hkv, capacity, D, sk, sv, k.dtype, k.device, fp8_format, numerics)
    return kv_cache_append_fp8(cache, k, v)


def _rows_addressable(t: Tensor) -> bool:
    """head_dim innermost and dense, every other stride of a dimension longer than 1 a non-negative multiple of 8 elements, the first
    element 16-byte aligned in its storage (torch allocations are): the rows the kernel loads 16 bytes at a time"""
    # (while Dynamo traces, the storage offset is not to be had: the op's binding checks the real pointer)
    aligned = torch.compiler.is_dynamo_compiling() or t.storage_offset() % 8 == 0
    return (t.stride(3) == 1 and aligned
            and all(t.shape[i] == 1 or (t.stride(i) >= 0 and t.stride(i) % 8 == 0) for i in (0, 1, 2)))


def kv_cache_append_input_reason(cache, k_new, v_new, new_lens=None) -> Optional[str]:
    """The first rule the arguments of `kv_cache_append_fp8` break, or None.  Shapes, dtypes, devices and strides only: the CONTENTS of
    seqlens / new_lens are read on the device."""
    if not isinstance(cache, KVCacheFP8):
        return "Expected cache to be a KVCacheFP8 (alloc_kv_cache_fp8 / kv_cache_from_prefill_fp8)"
    if not isinstance(k_new, Tensor) or not isinstance(v_new, Tensor) or k_new.dim() != 4 or v_new.dim() != 4:
        return "NYI: k_new and v_new must be 4-D tensors [B, Hkv, T, head_dim]"
    if k_new.requires_grad or v_new.requires_grad:
        return "NYI: k_new and v_new must be leaf tensors (no backward)"
    if k_new.dtype != cache.dtype or v_new.dtype != cache.dtype:
        return f"Expected k_new and v_new to have the cache's dtype {cache.dtype}, but got {k_new.dtype} and {v_new.dtype} instead."
    B, Hkv, _, D = cache.shape
    if k_new.shape != v_new.shape:
        return f"Expect k_new and v_new to have the same shape but got {tuple(k_new.shape)} and {tuple(v_new.shape)}."
    if (k_new.shape[0], k_new.shape[1], k_new.shape[3]) != (B, Hkv, D) or k_new.shape[2] == 0:
        return f"Expected k_new and v_new to have shape [{B}, {Hkv}, T >= 1, {D}], but got {list(k_new.shape)}."
    if k_new.device != cache.device or v_new.device != cache.device:
        return f"Expected k_new and v_new to be on the cache's device {cache.device}, but got {k_new.device} and {v_new.device} instead."
    for name, t in (("k_new", k_new), ("v_new", v_new)):
        if not _rows_addressable(t):
            return (f"Expected {name} to have head_dim innermost and 16-byte-aligned rows (strides that are multiples of 8 elements), but got "
                    f"strides {tuple(t.stride())} at storage offset {t.storage_offset()}; pass {name}.contiguous()")
    if cache.fp8_format not in _native.FP8_DTYPE:
        return f"Unsupported fp8_format of the cache: {cache.fp8_format!r}"
    if cache.k.dtype != (torch.uint8 if cache.layout == "frag" else _native.FP8_DTYPE[cache.fp8_format]):
        return f"The cache holds {cache.k.dtype} data, which is not its format {cache.fp8_format!r} in layout {cache.layout!r}"
    for name, t in (("cache.seqlens", cache.seqlens), ("new_lens", new_lens)):
        if t is None and name == "new_lens":
            continue
        if not isinstance(t, Tensor) or t.dtype != torch.int32:
            return f"Expected {name} to be a torch.int32 tensor, but got {getattr(t, 'dtype', type(t))}"
        if tuple(t.shape) != (B,):
            return f"Expected {name} to have shape [{B}], but got {list(t.shape)}."
        if t.device != cache.device:
            return f"Expected {name} to be on {cache.device}, but got {t.device} instead."
    return None


def _append_eager(cache: KVCacheFP8, k_new: Tensor, v_new: Tensor, new_lens: Optional[Tensor], advance: bool) -> None:
    """CPU tensors and config.attention.force_eager_fallback: the torch definition on row-major fp8 tensors -- the formula of
    include/qattn_kvcache.h plus an indexed copy.  (This path reads seqlens / new_lens on the host.)"""
    fp8_dtype = _native.fp8_dtype_of(cache.fp8_format)
    qmax = torch.finfo(fp8_dtype).max
    B, _, capacity, _ = cache.shape
    T = k_new.shape[2]
    pos = [min(max(int(x), 0), capacity) for x in cache.seqlens.tolist()]
    cnt = [T] * B if new_lens is None else [min(max(int(x), 0), T) for x in new_lens.tolist()]
    for b in range(B):
        n = min(cnt[b], capacity - pos[b])   # tokens at or beyond the capacity are dropped
        for img, x, s in ((cache.k, k_new, cache.scale_k), (cache.v, v_new, cache.scale_v)):
            if n > 0:
                q = (x[b, :, :n].float() / s[b, :, None, None]).to(x.dtype).clamp(-qmax, qmax).to(fp8_dtype)
                img[b, :, pos[b]:pos[b] + n] = q
        pos[b] += n
    if advance:
        cache.seqlens.copy_(torch.tensor(pos, dtype=torch.int32))


def kv_cache_append_fp8(cache: KVCacheFP8, k_new: Tensor, v_new: Tensor, *, new_lens: Optional[Tensor] = None, advance: bool = True) -> KVCacheFP8:
    """Append T tokens per (batch element, kv head) to `cache`, in place; returns `cache`.

    k_new, v_new [B, Hkv, T, D] in cache.dtype: dense, or any view with head_dim innermost and 16-byte-aligned rows -- the transposed view
    of a [B, T, Hkv, D] projection output goes to the kernel without a copy.  Token t < n_b of batch element b becomes key p_b + t of every
    kv head, p_b = clamp(cache.seqlens[b], 0, capacity), n_b = T or clamp(new_lens[b], 0, T) (new_lens: int32 [B] on the cache's device);
    a token whose position is >= capacity is dropped.  With `advance` seqlens[b] becomes min(p_b + n_b, capacity): a full cache
    saturates there.  Everything is read on the device: no host synchronisation, no allocation, graph-capture safe, and a captured call
    follows the later contents of seqlens / new_lens.
    Bytes: fp8(clamp(round_to_dtype(fp32(x) / scale), +-qmax)) with the cache's fixed scales -- a larger value saturates (+-inf too: it becomes
    +-qmax), a NaN in K stays a NaN byte, V must be finite.  Exactly the bytes of the appended keys change; no result depends on what the cache held.
    Rollback: `cache.seqlens.sub_(n)` -- bytes behind seqlens influence no output bit, and the next append overwrites them.
    CPU tensors and config.attention.force_eager_fallback run the eager definition (`_append_eager`); on the device there is no fallback.
    Invalid input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = kv_cache_append_input_reason(cache, k_new, v_new, new_lens)
        if reason:
            raise ValueError(reason)
    eager = (not k_new.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if cache.layout != "rowmajor":
            raise ValueError("the eager definition needs a cache made on a CPU device or under config.attention.force_eager_fallback")
        _append_eager(cache, k_new, v_new, new_lens, bool(advance))
        return cache
    if cache.layout != "frag":
        raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                         "config.attention.force_eager_fallback")
    ok, why = nn._pre_check_can_use_hip_attention(device=k_new.device)
    if not ok:
        raise ValueError(why)
    if torch.compiler.is_compiling():
        nn._ops().fp8_kv_cache_append_(cache.k, cache.v, cache.scale_k, cache.scale_v, cache.seqlens, k_new, v_new, new_lens, cache.shape[2],
                                       cache.fp8_format, bool(advance))
    else:
        # outside a trace: the op's own body, without the dispatcher's bookkeeping for a mutating op -- a decode step appends one token, and
        # the host's path to the launch is most of what that costs
        _native.kv_cache_append_fp8(cache.k, cache.v, cache.scale_k, cache.scale_v, cache.seqlens, k_new, v_new, capacity=cache.shape[2],
                                    fp8_dtype=_native.fp8_dtype_of(cache.fp8_format), new_lens=new_lens, advance=bool(advance))
    return cache

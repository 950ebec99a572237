"""A PAGED FP8 K/V cache (a pool of fixed-size pages and a per-sequence block table) for split-KV decode: `alloc_paged_kv_cache_fp8`,
`paged_kv_cache_append_fp8`, `fp8_attn_paged_func` and the `PagedKVCacheFP8` they share (include/qattn_paged.h).

A contiguous `KVCacheFP8` [B, Hkv, capacity, D] reserves `capacity` keys for every sequence, cannot share a prompt prefix between
sequences and cannot hand a finished sequence's memory to a new one without a copy.  Here the keys live in pages of `page_size` keys (a
multiple of 64) in one pool, and sequence b finds key j in page `block_table[b, j // page_size]` at key `j % page_size` -- the convention
of vLLM, SGLang and flash-attn's `flash_attn_with_kvcache(block_table=...)` (INTEGRATION.md maps them).  Only WHICH 64-key chunk a kernel
fetches or stores changes: the sweep, the numerics and every output bit are those of `fp8_attn_splitkv_func` / `kv_cache_append_fp8` on
the cache gathered through the table.

    cache = alloc_paged_kv_cache_fp8(num_pages, Hkv, page_size, D, batch_size=B, max_pages_per_seq=M, scale_k=..., scale_v=...,
                                     dtype=torch.bfloat16, device="cuda")
    cache.block_table[b, i] = page          # the CALLER's allocator writes the table, in place; the library allocates no pages
    for step in ...:
        paged_kv_cache_append_fp8(cache, k_new, v_new)          # [B, Hkv, T, D]; the pages that cover the new keys are assigned already
        out = fp8_attn_paged_func(q, cache, causal=True, max_seqlen_k=longest_live_sequence)

The table's entries are clamped into [0, num_pages - 1] on the device before they form an address; entries that no used key needs may
hold anything.  A page shared by several sequences (a common prefix) needs equal scales in all of them: the caller's responsibility.  Two
sequences that append into the same page in one call have two writers: undefined.

Package attributes, not names of `__all__` (that list mirrors the reference).  Not offered: page allocation, copy-on-write, re-scaling,
a per-call table whose batch differs from the cache's slots.  Sliding windows: splitkv_window.fp8_attn_paged_window_func.  Queries of a different count per sequence slot (packed
[total_q, Hq, D] under cu_seqlens_q): `fp8_attn_paged_varlen_func`, and the append of packed [total, Hkv, D] tokens under the same
cu_seqlens: `paged_kv_cache_append_varlen_fp8`, both paged_varlen.py."""
import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native, nn
from .kvcache import _is_int, _rows_addressable, _scale_reason
from .splitkv import MAX_SPLITS, PreparedKV, _resolve_splits, _splitkv_eager
from .utils import checks


class PagedKVCacheFP8:
    """A pool of pages and the table that maps sequences onto it.
      k, v             the pools.  Device tensors: the KFRAG / VFRAG images of [num_pages, Hkv, page_size, D] (flat uint8) -- byte for
                       byte a KVCacheFP8 of that shape whose "batch element" p is page p; CPU tensors (and
                       config.attention.force_eager_fallback): row-major fp8 [num_pages, Hkv, page_size, D] for the eager definitions
      scale_k, scale_v fp32 [B, Hkv], FIXED, per sequence slot (not per page)
      block_table      int32 [B, max_pages_per_seq], zero-filled when made; written in place by the caller's allocator
      seqlens          int32 [B]: the keys sequence slot b holds; the default seqused_k of the attention call
      shape            (num_pages, Hkv, page_size, D);  page_size, num_pages, fp8_format, dtype, numerics, layout ("frag" / "rowmajor")"""

    __slots__ = ("k", "v", "scale_k", "scale_v", "block_table", "seqlens", "shape", "page_size", "num_pages", "fp8_format", "dtype",
                 "numerics", "layout")

    def __init__(self, k, v, scale_k, scale_v, block_table, seqlens, shape, fp8_format, dtype, numerics, layout):
        self.k, self.v, self.scale_k, self.scale_v, self.block_table, self.seqlens = k, v, scale_k, scale_v, block_table, seqlens
        self.shape = tuple(shape)
        self.num_pages, self.page_size = self.shape[0], self.shape[2]
        self.fp8_format, self.dtype, self.numerics, self.layout = fp8_format, dtype, numerics, layout

    @property
    def device(self):
        return self.k.device

    @property
    def batch_size(self) -> int:
        return self.block_table.shape[0]

    @property
    def max_pages_per_seq(self) -> int:
        return self.block_table.shape[1]

    @property
    def capacity(self) -> int:
        """keys a sequence can hold: max_pages_per_seq * page_size"""
        return self.block_table.shape[1] * self.page_size

    def __repr__(self):
        return (f"PagedKVCacheFP8(shape={self.shape}, batch_size={self.batch_size}, max_pages_per_seq={self.max_pages_per_seq}, "
                f"fp8_format={self.fp8_format!r}, dtype={self.dtype}, numerics={self.numerics!r}, layout={self.layout!r}, device={self.device})")


def paged_alloc_input_reason(num_pages, Hkv, page_size, D, batch_size, max_pages_per_seq, scale_k, scale_v, dtype) -> Optional[str]:
    """The first rule the arguments of `alloc_paged_kv_cache_fp8` break, or None."""
    if not all(_is_int(x) and x > 0 for x in (num_pages, Hkv, batch_size, max_pages_per_seq)):
        return (f"Expected a positive page count, head count, batch size and table width, but got num_pages={num_pages!r}, Hkv={Hkv!r}, "
                f"batch_size={batch_size!r}, max_pages_per_seq={max_pages_per_seq!r}")
    if not (_is_int(page_size) and page_size >= 64 and page_size % 64 == 0):
        return f"page_size must be a positive multiple of 64 (a page holds whole 64-key chunks), got {page_size!r}"
    if D not in nn._HIP_SUPPORTED_HEAD_DIMS:
        return f"Unsupported head dimension: {D}"
    if num_pages * Hkv * (page_size // 64) > 2 ** 31 - 1:
        return f"num_pages * Hkv * (page_size / 64) must stay below 2^31 (the physical chunk index), got {num_pages * Hkv * (page_size // 64)}"
    if max_pages_per_seq * page_size > 2 ** 31 - 65:
        return f"max_pages_per_seq * page_size must stay below 2^31 - 64, got {max_pages_per_seq * page_size}"
    if dtype not in (torch.float16, torch.bfloat16):
        return f"Expected dtype to be torch.float16 or torch.bfloat16 (the dtype of the tokens to append), but got {dtype} instead."
    return _scale_reason("scale_k", scale_k, batch_size, Hkv) or _scale_reason("scale_v", scale_v, batch_size, Hkv)


def alloc_paged_kv_cache_fp8(num_pages: int, Hkv: int, page_size: int, D: int, *, batch_size: int, max_pages_per_seq: int, scale_k, scale_v,
                             dtype, device, fp8_format: Optional[str] = None, numerics: Optional[str] = None) -> PagedKVCacheFP8:
    """An empty paged cache: zero-filled pools of `num_pages` pages of `page_size` keys (a multiple of 64) per kv head, a zero-filled
    block table int32 [batch_size, max_pages_per_seq] and seqlens = 0.  scale_k / scale_v, dtype, fp8_format and numerics: as
    `alloc_kv_cache_fp8` (FIXED scales, a float or a tensor [Hkv] or [batch_size, Hkv], finite and > 0, kept as fp32 [batch_size, Hkv]).
    A CPU device (and config.attention.force_eager_fallback) gives row-major fp8 pools for the eager definitions."""
    reason = paged_alloc_input_reason(num_pages, Hkv, page_size, D, batch_size, max_pages_per_seq, scale_k, scale_v, dtype)
    if reason:
        raise ValueError(reason)
    fp8_format = checks.config_value("attention.fp8_format") if fp8_format is None else fp8_format
    numerics = checks.config_value("attention.quant_numerics") if numerics is None else numerics
    fp8_dtype = _native.fp8_dtype_of(fp8_format)
    if numerics not in _native.NUMERICS:
        raise ValueError(f"Unsupported quant_numerics: {numerics!r} (expected one of {sorted(_native.NUMERICS)})")
    device = torch.device(device)
    full = lambda s: (torch.as_tensor(s, dtype=torch.float32, device=device) if isinstance(s, Tensor)
                      else torch.full((), float(s), dtype=torch.float32, device=device)).expand(batch_size, Hkv).contiguous()
    table = torch.zeros((batch_size, max_pages_per_seq), dtype=torch.int32, device=device)
    seqlens = torch.zeros((batch_size,), dtype=torch.int32, device=device)
    shape = (num_pages, Hkv, page_size, D)
    if device.type != "cuda" or checks.config_value("attention.force_eager_fallback"):
        k8, v8 = (torch.zeros(shape, dtype=torch.uint8, device=device).view(fp8_dtype) for _ in range(2))
        return PagedKVCacheFP8(k8, v8, full(scale_k), full(scale_v), table, seqlens, shape, fp8_format, dtype, numerics, "rowmajor")
    ok, why = nn._pre_check_can_use_hip_attention(device=device)
    if not ok:
        raise ValueError(why)
    L = _native.lib()
    kf, vf = (torch.zeros((L.qattn_fp8_tensor_bytes(layout, num_pages, Hkv, page_size, D),), dtype=torch.uint8, device=device)
              for layout in (_native.LAYOUT_KFRAG, _native.LAYOUT_VFRAG))
    return PagedKVCacheFP8(kf, vf, full(scale_k), full(scale_v), table, seqlens, shape, fp8_format, dtype, numerics, "frag")


def _cache_reason(cache) -> Optional[str]:
    """what every call checks of the cache itself: shapes, dtypes and devices only -- the CONTENTS of the table and of seqlens are read on
    the device"""
    if not isinstance(cache, PagedKVCacheFP8):
        return "Expected cache to be a PagedKVCacheFP8 (alloc_paged_kv_cache_fp8)"
    if cache.fp8_format not in _native.FP8_DTYPE:
        return f"Unsupported fp8_format of the cache: {cache.fp8_format!r}"
    if cache.k.dtype != (torch.uint8 if cache.layout == "frag" else _native.FP8_DTYPE[cache.fp8_format]):
        return f"The cache holds {cache.k.dtype} data, which is not its format {cache.fp8_format!r} in layout {cache.layout!r}"
    t = cache.block_table
    if not isinstance(t, Tensor) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] == 0 or t.shape[1] == 0:
        return f"Expected cache.block_table to be a torch.int32 tensor [B, max_pages_per_seq], but got {getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', ()))}"
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        return f"Expected cache.block_table to have dense rows (a row stride >= max_pages_per_seq), but got strides {tuple(t.stride())}"
    if t.device != cache.device:
        return f"Expected cache.block_table to be on the cache's device {cache.device}, but got {t.device} instead."
    B, Hkv = t.shape[0], cache.shape[1]
    for name, s in (("scale_k", cache.scale_k), ("scale_v", cache.scale_v)):
        if not isinstance(s, Tensor) or s.dtype != torch.float32 or tuple(s.shape) != (B, Hkv) or s.device != cache.device:
            return f"Expected cache.{name} to be a torch.float32 tensor [{B}, {Hkv}] on {cache.device}"
    return None


def _lens_reason(name, t, B, device) -> Optional[str]:
    if not isinstance(t, Tensor) or t.dtype != torch.int32:
        return f"Expected {name} to be a torch.int32 tensor, but got {getattr(t, 'dtype', type(t))}"
    if tuple(t.shape) != (B,):
        return f"Expected {name} to have shape [{B}], but got {list(t.shape)}."
    if t.device != device:
        return f"Expected {name} to be on {device}, but got {t.device} instead."
    return None


def paged_append_input_reason(cache, k_new, v_new, new_lens=None) -> Optional[str]:
    """The first rule the arguments of `paged_kv_cache_append_fp8` break, or None.  Shapes, dtypes, devices and strides only: the CONTENTS
    of block_table / seqlens / new_lens are read on the device."""
    reason = _cache_reason(cache)
    if reason:
        return reason
    if not isinstance(k_new, Tensor) or not isinstance(v_new, Tensor) or k_new.dim() != 4 or v_new.dim() != 4:
        return "NYI: k_new and v_new must be 4-D tensors [B, Hkv, T, head_dim]"
    if k_new.requires_grad or v_new.requires_grad:
        return "NYI: k_new and v_new must be leaf tensors (no backward)"
    if k_new.dtype != cache.dtype or v_new.dtype != cache.dtype:
        return f"Expected k_new and v_new to have the cache's dtype {cache.dtype}, but got {k_new.dtype} and {v_new.dtype} instead."
    B = cache.batch_size
    _, Hkv, _, D = cache.shape
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
    reason = _lens_reason("cache.seqlens", cache.seqlens, B, cache.device)
    if reason is None and new_lens is not None:
        reason = _lens_reason("new_lens", new_lens, B, cache.device)
    return reason


def paged_attn_input_reason(q, cache, seqused_k=None, scale=None, num_splits=0, max_seqlen_k=None) -> Optional[str]:
    """The first rule the arguments of `fp8_attn_paged_func` break, or None.  Shapes, dtypes and devices only."""
    if not isinstance(q, Tensor) or q.dim() != 4:
        return "NYI: query must be a 4-D tensor [B, Hq, Sq, head_dim]"
    if q.requires_grad:
        return "NYI: query must be a leaf tensor (no backward)"
    if q.dtype not in (torch.float16, torch.bfloat16):
        return f"Expected query to have dtype torch.float16 or torch.bfloat16, but got query.dtype: {q.dtype} instead."
    reason = _cache_reason(cache)
    if reason:
        return reason
    B = cache.batch_size
    _, Hkv, _, D = cache.shape
    if cache.dtype != q.dtype:
        return f"Expected query to have the cache's dtype, but got {q.dtype} and {cache.dtype} instead."
    if q.shape[-1] != D:
        return f"Expect query, key and value to have the same head dimension but got {q.shape[-1]} and {D}."
    if q.shape[0] != B:
        return f"Expect query and the cache's block table to have the same batch size but got {q.shape[0]} and {B}."
    if q.shape[1] == 0 or q.shape[2] == 0:
        return "Expected a non-empty head count and query sequence"
    if q.shape[1] % Hkv != 0:
        return f"Expect the number of query heads to be a multiple of the key/value heads but got Hq={q.shape[1]} and Hkv={Hkv}."
    if q.device != cache.device:
        return f"Expected query and the cache to be on the same device, but got {q.device} and {cache.device} instead."
    reason = _lens_reason("seqused_k" if seqused_k is not None else "cache.seqlens", cache.seqlens if seqused_k is None else seqused_k, B, q.device)
    if reason:
        return reason
    if max_seqlen_k is not None and not (_is_int(max_seqlen_k) and 1 <= max_seqlen_k <= cache.capacity):
        return f"max_seqlen_k must be None or an integer in 1 .. max_pages_per_seq * page_size = {cache.capacity}, got {max_seqlen_k!r}"
    if isinstance(num_splits, bool) or not isinstance(num_splits, int) or not 0 <= num_splits <= MAX_SPLITS:
        return f"num_splits must be 0 (choose) or an integer in 1 .. {MAX_SPLITS}, got {num_splits!r}"
    if scale is not None and not (isinstance(scale, (int, float)) and not isinstance(scale, bool) and math.isfinite(scale) and scale > 0):
        return f"scale must be a finite number > 0 (or None for 1/sqrt(head_dim)), got {scale!r}"
    return None


def _append_eager(cache: PagedKVCacheFP8, k_new: Tensor, v_new: Tensor, new_lens: Optional[Tensor], advance: bool) -> None:
    """CPU tensors and config.attention.force_eager_fallback: the torch definition on row-major fp8 pools -- kvcache._append_eager's
    formula, each key stored through the (clamped) table.  (This path reads block_table / seqlens / new_lens on the host.)"""
    fp8_dtype = _native.fp8_dtype_of(cache.fp8_format)
    qmax = torch.finfo(fp8_dtype).max
    ps, capacity, B = cache.page_size, cache.capacity, cache.batch_size
    T = k_new.shape[2]
    table = cache.block_table.clamp(0, cache.num_pages - 1).tolist()
    pos = [min(max(int(x), 0), capacity) for x in cache.seqlens.tolist()]
    cnt = [T] * B if new_lens is None else [min(max(int(x), 0), T) for x in new_lens.tolist()]
    for b in range(B):
        n = min(cnt[b], capacity - pos[b])   # tokens at or beyond the capacity are dropped
        if n > 0:
            keys = torch.arange(pos[b], pos[b] + n)
            page = torch.tensor(table[b], dtype=torch.long)[keys // ps].to(cache.k.device)
            slot = (keys % ps).to(cache.k.device)
            for pool, x, s in ((cache.k, k_new, cache.scale_k), (cache.v, v_new, cache.scale_v)):
                q = (x[b, :, :n].float() / s[b, :, None, None]).to(x.dtype).clamp(-qmax, qmax).to(fp8_dtype)   # [Hkv, n, D]
                pool.view(torch.uint8)[page, :, slot] = q.view(torch.uint8).transpose(0, 1)
        pos[b] += n
    if advance:
        cache.seqlens.copy_(torch.tensor(pos, dtype=torch.int32))


def gather_paged_eager(cache: PagedKVCacheFP8, Skv: Optional[int] = None) -> PreparedKV:
    """The contiguous row-major PreparedKV [B, Hkv, Skv, D] a row-major paged cache holds, gathered through the (clamped) table: what the
    eager definition attends.  Skv defaults to max_pages_per_seq * page_size."""
    if cache.layout != "rowmajor":
        raise ValueError("gather_paged_eager needs a cache made on a CPU device or under config.attention.force_eager_fallback")
    Skv = cache.capacity if Skv is None else Skv
    B, M = cache.block_table.shape
    _, Hkv, ps, D = cache.shape
    idx = cache.block_table.clamp(0, cache.num_pages - 1).long()                                      # [B, M]
    gather = lambda pool: pool[idx].permute(0, 2, 1, 3, 4).reshape(B, Hkv, M * ps, D)[:, :, :Skv].contiguous()
    return PreparedKV(gather(cache.k), gather(cache.v), cache.scale_k, cache.scale_v, (B, Hkv, Skv, D), cache.fp8_format, cache.dtype,
                      cache.numerics, "rowmajor")


def _attend_eager(q, cache, causal, scale, seqused_k, Skv, ns, precision, softcap=None, sinks=None, window=None):
    """CPU tensors and config.attention.force_eager_fallback: splitkv._splitkv_eager on the cache gathered through the table."""
    return _splitkv_eager(q, gather_paged_eager(cache, Skv), causal, scale, seqused_k, ns, precision, sinks=sinks, softcap=softcap, window=window)


def paged_kv_cache_append_fp8(cache: PagedKVCacheFP8, k_new: Tensor, v_new: Tensor, *, new_lens: Optional[Tensor] = None,
                              advance: bool = True) -> PagedKVCacheFP8:
    """Append T tokens per (sequence slot, kv head) to the paged `cache`, in place; returns `cache`.

    `kv_cache_append_fp8` with capacity = max_pages_per_seq * page_size: positions p_b = clamp(seqlens[b], 0, capacity), n_b = T or
    clamp(new_lens[b], 0, T), tokens at or beyond the capacity dropped, seqlens advanced to min(p_b + n_b, capacity) unless
    advance=False, the same bytes (fixed scales, saturation, a NaN in K stays a NaN byte, V must be finite), the same views of k_new / v_new
    accepted, everything read on the device (graph-capture safe; a captured call follows the later contents of block_table, seqlens and
    new_lens).  Key j of slot b is stored at key j % page_size of page clamp(block_table[b, j // page_size], 0, num_pages - 1): the pages
    that cover [p_b, p_b + n_b) must have been assigned BEFORE the call, and only those entries are read.  Exactly the bytes of the
    appended keys change.  Two slots that append into the same page in one call have two writers: undefined.
    CPU tensors and config.attention.force_eager_fallback run the eager definition (`_append_eager`); on the device there is no fallback.
    Invalid input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_append_input_reason(cache, k_new, v_new, new_lens)
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
        nn._ops().fp8_paged_kv_cache_append_(cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, cache.seqlens, k_new, v_new,
                                             new_lens, cache.num_pages, cache.page_size, cache.fp8_format, bool(advance))
    else:
        # outside a trace: the op's own body, without the dispatcher's bookkeeping for a mutating op (as kv_cache_append_fp8)
        _native.paged_kv_cache_append_fp8(cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, cache.seqlens, k_new, v_new,
                                          num_pages=cache.num_pages, page_size=cache.page_size,
                                          fp8_dtype=_native.fp8_dtype_of(cache.fp8_format), new_lens=new_lens, advance=bool(advance))
    return cache


def fp8_attn_paged_func(q, cache: PagedKVCacheFP8, *, causal: bool = False, scale: Optional[float] = None, seqused_k: Optional[Tensor] = None,
                        max_seqlen_k: Optional[int] = None, num_splits: int = 0, precision: str = "accurate", return_lse: bool = False,
                        return_partials: bool = False):
    """`fp8_attn_splitkv_func` over a paged cache: the same arguments, split plan, masks, precision rule, outputs and BITS as that call on
    the cache gathered through the block table.

    q [B, Hq, Sq, D] in cache.dtype, B = the table's rows.  seqused_k: int32 [B] on the device, default cache.seqlens (a paged call always
    has one); sequence b uses its first L_b = clamp(seqused_k[b], 0, Skv) keys.
    max_seqlen_k: a host int, optional: the logical key bound Skv of the call.  Default max_pages_per_seq * page_size -- in a serving
    table far more than any live sequence holds, which makes the num_splits = 0 rule over-split and the workspace large: pass the longest
    live sequence.  Keys at or beyond max_seqlen_k are not attended (L_b is clamped to it).
    Only the table entries below ceil(L_b / page_size) are read (causal: up to the last page a row attends), each clamped into
    [0, num_pages - 1] before it forms an address; the others may hold anything.  Table and lengths are read on the device: no host
    synchronisation, graph-capture safe, and a captured call follows their later contents.
    causal, scale, num_splits, precision ("auto" raises ValueError), return_lse, return_partials: as `fp8_attn_splitkv_func`.
    CPU tensors and config.attention.force_eager_fallback run the eager definition (`_attend_eager`); on the device there is no fallback.
    Unsupported input raises ValueError(reason)."""
    if precision not in ("accurate", "fast"):
        raise ValueError(f"Unsupported precision: {precision!r} (expected 'accurate' or 'fast'; 'auto' is not offered by the split-KV entries)")
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_attn_input_reason(q, cache, seqused_k, scale, num_splits, max_seqlen_k)
        if reason:
            raise ValueError(reason)
    B, Hq, Sq, D = q.shape
    Hkv = cache.shape[1]
    Skv = cache.capacity if max_seqlen_k is None else int(max_seqlen_k)
    used = cache.seqlens if seqused_k is None else seqused_k
    ns = _resolve_splits(num_splits, B, Hq, Hkv, Sq, Skv, D, q.device)
    eager = (not q.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if cache.layout != "rowmajor":
            raise ValueError("the eager definition needs a cache made on a CPU device or under config.attention.force_eager_fallback")
        out, lse, po, plse, ppath = _attend_eager(q, cache, causal, scale, used, Skv, ns, precision)
    else:
        if cache.layout != "frag":
            raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        out, lse, po, plse, ppath = nn._ops().fp8_paged_splitkv_attention_forward(
            q.contiguous(), cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, used, Skv, cache.num_pages, cache.page_size, ns,
            cache.fp8_format, cache.numerics, bool(causal), precision, bool(return_lse), bool(return_partials), scale=scale)
    res: Tuple = (out,)
    if return_lse:
        res += (lse,)
    if return_partials:
        res += (po, plse, ppath)
    return res if len(res) > 1 else out

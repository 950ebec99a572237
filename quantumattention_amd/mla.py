"""FP8 multi-head latent attention (MLA: DeepSeek-V2 / V3 / R1, Kimi-K2) in its ABSORBED decode form over a paged latent cache:
`alloc_paged_mla_cache_fp8`, `paged_mla_cache_append_fp8`, `fp8_mla_paged_func` and the `PagedMLACacheFP8` they share (include/qattn_mla.h,
DESIGN.md section 4.30).

Every query head of a token attends ONE shared vector per key: 512 latent channels (`kv_c`) followed by 64 rotary channels (`k_pe`, rotated
by the caller).  Scores are 576-channel dot products; the value of a key is the first 512 channels of the same vector, so the cache is ONE
image -- the kernel transposes each 64-key chunk on the chip for the value product instead of keeping a second copy.

    cache = alloc_paged_mla_cache_fp8(num_pages, page_size, batch_size=B, max_pages_per_seq=M, scale=0.05, dtype=torch.bfloat16, device="cuda")
    cache.block_table[b, i] = page          # the CALLER's allocator writes the table, in place
    for step in ...:
        paged_mla_cache_append_fp8(cache, kv[..., :512], kv[..., 512:])          # [B, T, 512], [B, T, 64]: views of one projection tensor
        out = fp8_mla_paged_func(q, cache, scale=model_softmax_scale, max_seqlen_k=longest_live_sequence)     # q [B, Hq, Sq, 576]

The cache has ONE fixed fp32 scale per slot for all 576 channels.  A caller whose k_pe range differs from the latent's may pre-multiply k_pe by
a constant and q_pe by its inverse.  `scale` of the attention call is REQUIRED: MLA's softmax scale is the model's (1/sqrt(192) times its
YaRN factor), never 1/sqrt(576).  q is quantised inside the kernel, token-wise, always to e4m3.  Table, lengths and clamping: paged.py.

Package attributes, not names of `__all__`.  Not offered: windows, sinks, soft cap or trees on MLA; RoPE inside the
append; precision "fast" / "auto"; per-token cache scales.  (Packed variable-length q: mla_varlen.py.  The indexer of DeepSeek-V3.2's sparse attention -- its scores and the top-k
selection -- is mla_index.py; the attention over the selected keys is below.  The non-absorbed prefill form -- ordinary MHA at D 192 / 128 --
is mla_prefill.py)

SPARSE (top-k indexed) decode, the attention of DeepSeek-V3.2-style layers (include/qattn_mla_sparse.h):
`alloc_paged_mla_row_cache_fp8`, `paged_mla_row_cache_append_fp8`, `fp8_mla_paged_sparse_func`.  The cache is ROW-MAJOR -- a key is one
contiguous 576-byte row, any page_size -- and `indices` int32 [B, Sq, topk] names the LOGICAL key positions each query token attends, shared
by all its heads; the kernel resolves them through the block table and gathers exactly those rows."""
import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native, nn
from .kvcache import _is_int
from .paged import _lens_reason
from .utils import checks

D, D_LATENT, D_ROPE, MAX_SPLITS = _native.MLA_D, _native.MLA_D_LATENT, _native.MLA_D_ROPE, _native.MLA_MAX_SPLITS
SPLIT_ENTRIES, MAX_TOPK = _native.MLA_SPARSE_SPLIT_ENTRIES, _native.MLA_SPARSE_MAX_TOPK
_CHUNK = 64 * D
_CPU_NUM_CUS = 256   # the CU count the split rule assumes where there is no device to ask (CPU tensors: the eager definition)


def chunk_byte_offset(key: int, d: int) -> int:
    """include/qattn_mla.h's byte map: where byte (key < 64, channel d < 576) of a 64-key chunk lies in its 36 864 bytes."""
    return (((key >> 5) * 9 + (d >> 6)) << 11) + (((d >> 5) & 1) << 10) + (((d >> 4) & 1) << 9) + ((key & 31) << 4) + (d & 15)


def pool_rowmajor(pool: Tensor, num_pages: int, page_size: int) -> Tensor:
    """The bytes of a device pool (flat uint8) as row-major uint8 [num_pages, page_size, 576], by the header's byte map."""
    k, d = torch.arange(64, device=pool.device)[:, None], torch.arange(D, device=pool.device)[None, :]
    off = ((((k >> 5) * 9 + (d >> 6)) << 11) + (((d >> 5) & 1) << 10) + (((d >> 4) & 1) << 9) + ((k & 31) << 4) + (d & 15)).reshape(-1)
    return pool.view(num_pages * (page_size // 64), _CHUNK)[:, off].reshape(num_pages, page_size, D)


class PagedMLACacheFP8:
    """A pool of latent pages and the table that maps sequence slots onto it.
      pool          device tensors: flat uint8, the one-image chunk order of include/qattn_mla.h; CPU tensors (and
                    config.attention.force_eager_fallback): row-major fp8 [num_pages, page_size, 576] for the eager definitions
      scale         fp32 [B], FIXED, one per slot for all 576 channels
      block_table   int32 [B, max_pages_per_seq], zero-filled when made; written in place by the caller's allocator
      seqlens       int32 [B]: the keys slot b holds; the default seqused_k of the attention call
      num_pages, page_size, fp8_format, dtype, layout ("frag" / "rowmajor")"""

    __slots__ = ("pool", "scale", "block_table", "seqlens", "num_pages", "page_size", "fp8_format", "dtype", "layout")

    def __init__(self, pool, scale, block_table, seqlens, num_pages, page_size, fp8_format, dtype, layout):
        self.pool, self.scale, self.block_table, self.seqlens = pool, scale, block_table, seqlens
        self.num_pages, self.page_size, self.fp8_format, self.dtype, self.layout = num_pages, page_size, fp8_format, dtype, layout

    @property
    def device(self):
        return self.pool.device

    @property
    def batch_size(self) -> int:
        return self.block_table.shape[0]

    @property
    def capacity(self) -> int:
        """keys a slot can hold: max_pages_per_seq * page_size"""
        return self.block_table.shape[1] * self.page_size

    def __repr__(self):
        return (f"PagedMLACacheFP8(num_pages={self.num_pages}, page_size={self.page_size}, batch_size={self.batch_size}, "
                f"max_pages_per_seq={self.block_table.shape[1]}, fp8_format={self.fp8_format!r}, dtype={self.dtype}, layout={self.layout!r}, "
                f"device={self.device})")


def _alloc_reason(num_pages, page_size, batch_size, max_pages_per_seq, scale, dtype) -> Optional[str]:
    if not all(_is_int(x) and x > 0 for x in (num_pages, batch_size, max_pages_per_seq)):
        return (f"Expected a positive page count, batch size and table width, but got num_pages={num_pages!r}, batch_size={batch_size!r}, "
                f"max_pages_per_seq={max_pages_per_seq!r}")
    if not (_is_int(page_size) and page_size >= 64 and page_size % 64 == 0):
        return f"page_size must be a positive multiple of 64 (a page holds whole 64-key chunks), got {page_size!r}"
    if num_pages * (page_size // 64) > 2 ** 31 - 1 or max_pages_per_seq * page_size > 2 ** 31 - 65:
        return "num_pages * (page_size / 64) and max_pages_per_seq * page_size must stay below 2^31"
    if dtype not in (torch.float16, torch.bfloat16):
        return f"Expected dtype to be torch.float16 or torch.bfloat16 (the dtype of the tokens to append), but got {dtype} instead."
    if scale is None:
        return "scale is required: ONE fixed scale per slot for all 576 channels (a float, or a tensor [batch_size])"
    s = scale if isinstance(scale, Tensor) else torch.tensor(float(scale))
    if s.dim() > 1 or (s.dim() == 1 and s.shape[0] != batch_size) or not bool((torch.isfinite(s.float()) & (s.float() > 0)).all()):
        return f"scale must be finite and > 0, a float or a tensor [{batch_size}]"
    return None


def alloc_paged_mla_cache_fp8(num_pages: int, page_size: int, *, batch_size: int, max_pages_per_seq: int, scale, dtype, device,
                              fp8_format: Optional[str] = None) -> PagedMLACacheFP8:
    """An empty paged latent cache: a zero-filled pool of `num_pages` pages of `page_size` keys (a multiple of 64) of 576 bytes, a zero-filled
    block table int32 [batch_size, max_pages_per_seq] and seqlens = 0.  scale: the FIXED quantisation scale, a float or a tensor
    [batch_size], finite and > 0, kept as fp32 [batch_size]; dtype: of the tokens to append and of q.  A CPU device (and
    config.attention.force_eager_fallback) gives a row-major fp8 pool for the eager definitions."""
    reason = _alloc_reason(num_pages, page_size, batch_size, max_pages_per_seq, scale, dtype)
    if reason:
        raise ValueError(reason)
    fp8_format = checks.config_value("attention.fp8_format") if fp8_format is None else fp8_format
    fp8_dtype = _native.fp8_dtype_of(fp8_format)
    device = torch.device(device)
    sc = (torch.as_tensor(scale, dtype=torch.float32, device=device) if isinstance(scale, Tensor)
          else torch.full((), float(scale), dtype=torch.float32, device=device)).expand(batch_size).contiguous()
    table = torch.zeros((batch_size, max_pages_per_seq), dtype=torch.int32, device=device)
    seqlens = torch.zeros((batch_size,), dtype=torch.int32, device=device)
    if device.type != "cuda" or checks.config_value("attention.force_eager_fallback"):
        pool = torch.zeros((num_pages, page_size, D), dtype=torch.uint8, device=device).view(fp8_dtype)
        return PagedMLACacheFP8(pool, sc, table, seqlens, num_pages, page_size, fp8_format, dtype, "rowmajor")
    ok, why = nn._pre_check_can_use_hip_attention(device=device)
    if not ok:
        raise ValueError(why)
    pool = torch.zeros((_native.lib().qattn_mla_pool_bytes(num_pages, page_size),), dtype=torch.uint8, device=device)
    return PagedMLACacheFP8(pool, sc, table, seqlens, num_pages, page_size, fp8_format, dtype, "frag")


def _cache_reason(cache, row: bool = False) -> Optional[str]:
    """row: the rules of the row-major cache of the sparse call (any page_size >= 1) instead of the chunk image's"""
    if not isinstance(cache, PagedMLACacheFP8):
        return "Expected cache to be a PagedMLACacheFP8 (alloc_paged_mla_cache_fp8)"
    if row and not (_is_int(cache.page_size) and cache.page_size >= 1):
        return f"page_size must be a positive integer, got {cache.page_size!r}"
    if not row and not (_is_int(cache.page_size) and cache.page_size >= 64 and cache.page_size % 64 == 0):
        return f"page_size must be a positive multiple of 64 (a page holds whole 64-key chunks), got {cache.page_size!r}"
    t = cache.block_table
    if not isinstance(t, Tensor) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] == 0 or t.shape[1] == 0 or t.stride(1) != 1:
        return "Expected cache.block_table to be a torch.int32 tensor [B, max_pages_per_seq] with dense rows"
    if t.device != cache.device:
        return f"Expected cache.block_table to be on the cache's device {cache.device}, but got {t.device} instead."
    s = cache.scale
    if not isinstance(s, Tensor) or s.dtype != torch.float32 or tuple(s.shape) != (t.shape[0],) or s.device != cache.device:
        return f"Expected cache.scale to be a torch.float32 tensor [{t.shape[0]}] on {cache.device}"
    return None


def _append_reason(cache, ckv_new, kpe_new, new_lens) -> Optional[str]:
    B = cache.batch_size
    for name, t, ch in (("ckv_new", ckv_new, D_LATENT), ("kpe_new", kpe_new, D_ROPE)):
        if not isinstance(t, Tensor) or t.dim() != 3 or t.shape[0] != B or t.shape[1] == 0 or t.shape[2] != ch:
            return f"Expected {name} to be a tensor [{B}, T >= 1, {ch}], but got {list(getattr(t, 'shape', ()))}"
        if t.dtype != cache.dtype or t.requires_grad:
            return f"Expected {name} to be a leaf tensor of the cache's dtype {cache.dtype}, but got {t.dtype}"
        if t.device != cache.device:
            return f"Expected {name} to be on the cache's device {cache.device}, but got {t.device} instead."
        if not _native.mla_rows_addressable(t):
            return f"Expected {name} to have dense channels and 16-byte-aligned rows, but got strides {tuple(t.stride())}; pass {name}.contiguous()"
    if ckv_new.shape[1] != kpe_new.shape[1]:
        return f"Expect ckv_new and kpe_new to hold the same tokens but got T = {ckv_new.shape[1]} and {kpe_new.shape[1]}."
    reason = _lens_reason("cache.seqlens", cache.seqlens, B, cache.device)
    return reason if reason or new_lens is None else _lens_reason("new_lens", new_lens, B, cache.device)


def _query_reason(q, cache, scale, seqused_k) -> Optional[str]:
    B = cache.batch_size
    if not isinstance(q, Tensor) or q.dim() != 4:
        return "NYI: query must be a 4-D tensor [B, Hq, Sq, 576]"
    if q.requires_grad:
        return "NYI: query must be a leaf tensor (no backward)"
    if q.dtype not in (torch.float16, torch.bfloat16) or q.dtype != cache.dtype:
        return f"Expected query to have the cache's dtype {cache.dtype} (torch.float16 or torch.bfloat16), but got {q.dtype} instead."
    if q.shape[-1] != D:
        return f"Expected the query's head dimension to be {D} (512 latent + 64 rotary channels, absorbed form), but got {q.shape[-1]}."
    if q.shape[0] != B or q.shape[1] == 0 or q.shape[2] == 0 or q.shape[1] * q.shape[2] > 2 ** 20:
        return f"Expected query to have shape [{B}, Hq >= 1, Sq >= 1, {D}] with Hq * Sq <= 2^20, but got {list(q.shape)}."
    if q.device != cache.device:
        return f"Expected query and the cache to be on the same device, but got {q.device} and {cache.device} instead."
    if not _native.mla_rows_addressable(q):
        return f"Expected query to have dense channels and 16-byte-aligned rows, but got strides {tuple(q.stride())}; pass query.contiguous()"
    if scale is None:
        return "scale is required: MLA's softmax scale is the model's (1/sqrt(192) times its YaRN factor), not 1/sqrt(576)"
    if not (isinstance(scale, (int, float)) and not isinstance(scale, bool) and math.isfinite(scale) and scale > 0):
        return f"scale must be a finite number > 0, got {scale!r}"
    return _lens_reason("seqused_k" if seqused_k is not None else "cache.seqlens", cache.seqlens if seqused_k is None else seqused_k, B, q.device)


def mla_input_reason(q, cache, *, scale=None, seqused_k=None, max_seqlen_k=None, num_splits=0, ckv_new=None, kpe_new=None,
                     new_lens=None) -> Optional[str]:
    """The first rule the arguments of `fp8_mla_paged_func` (q given) or `paged_mla_cache_append_fp8` (q None; ckv_new, kpe_new given) break,
    or None.  Shapes, dtypes, devices and strides only: the CONTENTS of block_table / seqlens are read on the device."""
    reason = _cache_reason(cache)
    if reason:
        return reason
    if q is None:
        return _append_reason(cache, ckv_new, kpe_new, new_lens)
    reason = _query_reason(q, cache, scale, seqused_k)
    if reason:
        return reason
    if max_seqlen_k is not None and not (_is_int(max_seqlen_k) and 1 <= max_seqlen_k <= cache.capacity):
        return f"max_seqlen_k must be None or an integer in 1 .. max_pages_per_seq * page_size = {cache.capacity}, got {max_seqlen_k!r}"
    if isinstance(num_splits, bool) or not isinstance(num_splits, int) or not 0 <= num_splits <= MAX_SPLITS:
        return f"num_splits must be 0 (choose) or an integer in 1 .. {MAX_SPLITS}, got {num_splits!r}"
    return None


# ---- the eager definitions (CPU tensors, config.attention.force_eager_fallback): the specification -------------------------------------------
def _append_eager(cache, ckv_new, kpe_new, new_lens, advance) -> None:
    """paged._append_eager's formula on the concatenated [ckv | kpe] rows: fp8(clamp(round16(x / scale), +-qmax)) stored through the
    (clamped) table.  (Reads block_table / seqlens / new_lens on the host.)"""
    fp8_dtype = _native.fp8_dtype_of(cache.fp8_format)
    qmax = torch.finfo(fp8_dtype).max
    ps, capacity, B, T = cache.page_size, cache.capacity, cache.batch_size, ckv_new.shape[1]
    table = cache.block_table.clamp(0, cache.num_pages - 1).tolist()
    pos = [min(max(int(x), 0), capacity) for x in cache.seqlens.tolist()]
    cnt = [T] * B if new_lens is None else [min(max(int(x), 0), T) for x in new_lens.tolist()]
    x = torch.cat([ckv_new, kpe_new], dim=-1)
    for b in range(B):
        n = min(cnt[b], capacity - pos[b])   # tokens at or beyond the capacity are dropped
        if n > 0:
            keys = torch.arange(pos[b], pos[b] + n)
            page = torch.tensor(table[b], dtype=torch.long)[keys // ps].to(cache.device)
            q = (x[b, :n].float() / cache.scale[b]).to(x.dtype).clamp(-qmax, qmax).to(fp8_dtype)
            cache.pool.view(torch.uint8)[page, (keys % ps).to(cache.device)] = q.view(torch.uint8)
        pos[b] += n
    if advance:
        cache.seqlens.copy_(torch.tensor(pos, dtype=torch.int32))


def quantize_q_eager(q: Tensor) -> Tuple[Tensor, Tensor]:
    """the kernel's q quantiser: scale_q = max(amax / 448, 2^-23) per row, q8 = e4m3(clamp(fp32(q) * (1 / scale_q), +-448))"""
    qf = q.float()
    scale_q = (qf.abs().amax(dim=-1) / 448.0).clamp_min(2.0 ** -23)
    q8 = (qf * (1.0 / scale_q)[..., None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q8, scale_q


def split_plan(L: int, num_splits: int):
    """Key ranges [lo, hi) of the splits of a slot with L used keys: ceil(L / 64) chunks, per = ceil(chunks / ns) per split."""
    nch = -(-L // 64)
    per = -(-nch // num_splits)
    return [(min(64 * s * per, L), min(64 * (s + 1) * per, L)) for s in range(num_splits)]


def combine_eager(po: Tensor, plse: Tensor, dtype) -> Tuple[Tensor, Tensor]:
    """the combine kernel's formula: L = log sum exp(lse_i), O = sum_i exp(lse_i - L) O_i in fp32 in the order of i, one rounding"""
    L = torch.logsumexp(plse, dim=0)
    acc = torch.zeros_like(po[0])
    for i in range(po.shape[0]):
        w = torch.where(torch.isneginf(plse[i]), torch.zeros_like(L), torch.exp(plse[i] - L))
        acc = acc + w[..., None] * po[i]
    return acc.to(dtype), L


def _attend_eager(q, cache, causal, scale, seqused_k, Skv, ns):
    """de-quantise the bytes, fp32 softmax per split, values = the first 512 channels; the partials are merged by `combine_eager`.
    (Reads block_table / seqused_k on the host.)"""
    B, Hq, Sq, _ = q.shape
    q8, scale_q = quantize_q_eager(q)
    idx = cache.block_table.clamp(0, cache.num_pages - 1).long()
    lat = cache.pool[idx].reshape(B, -1, D)[:, :Skv].float() * cache.scale[:, None, None]     # [B, Skv, 576]
    qd = q8.float() * scale_q[..., None]
    po = torch.zeros((ns, B, Hq, Sq, D_LATENT), dtype=torch.float32, device=q.device)
    plse = torch.full((ns, B, Hq, Sq), -math.inf, dtype=torch.float32, device=q.device)
    for b, Lb in enumerate(seqused_k.tolist()):
        Lb = min(max(int(Lb), 0), Skv)
        for s, (lo, hi) in enumerate(split_plan(Lb, ns)):
            if hi <= lo:
                continue
            sc = torch.einsum("hqd,kd->hqk", qd[b], lat[b, lo:hi]) * scale
            if causal:
                keys, rows = torch.arange(lo, hi, device=q.device)[None, :], torch.arange(Sq, device=q.device)[:, None]
                sc = sc.masked_fill(keys > Lb - Sq + rows, -math.inf)
            lse = torch.logsumexp(sc, dim=-1)
            p = torch.where(torch.isneginf(lse)[..., None], torch.zeros_like(sc), torch.exp(sc - lse[..., None]))
            po[s, b] = torch.einsum("hqk,kd->hqd", p, lat[b, lo:hi, :D_LATENT])
            plse[s, b] = lse
    out, lse = combine_eager(po, plse, q.dtype)
    empty = torch.empty((0,), dtype=torch.float32, device=q.device)
    return out, lse, (po if ns > 1 else empty), (plse if ns > 1 else empty), q8, scale_q


# ---- the calls -----------------------------------------------------------------------------------------------------------------------------------
def _eager(t: Tensor) -> bool:
    return (not t.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()


def _layout_check(cache, eager: bool) -> None:
    if eager and cache.layout != "rowmajor":
        raise ValueError("the eager definition needs a cache made on a CPU device or under config.attention.force_eager_fallback")
    if not eager and cache.layout != "frag":
        raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                         "config.attention.force_eager_fallback")


def paged_mla_cache_append_fp8(cache: PagedMLACacheFP8, ckv_new: Tensor, kpe_new: Tensor, *, new_lens: Optional[Tensor] = None,
                               advance: bool = True) -> PagedMLACacheFP8:
    """Append T tokens per slot to the paged latent `cache`, in place; returns `cache`.

    ckv_new [B, T, 512] and kpe_new [B, T, 64] in cache.dtype -- the two slices of the model's projection; views with dense channels and
    16-byte-aligned rows are read through their strides, nothing is copied; k_pe is ALREADY rotated.  Token t of slot b becomes key
    seqlens[b] + t, quantised with the slot's scale (`paged_kv_cache_append_fp8`'s quantiser: saturating, a NaN stays a NaN byte) and
    stored through the (clamped) table; n_b = T or clamp(new_lens[b], 0, T); tokens at or beyond the capacity are dropped; seqlens advances
    unless advance=False.  Exactly the bytes of the appended keys change.  Everything is read on the device: graph-capture safe.
    CPU tensors and config.attention.force_eager_fallback run the eager definition (`_append_eager`); on the device there is no fallback.
    Invalid input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = mla_input_reason(None, cache, ckv_new=ckv_new, kpe_new=kpe_new, new_lens=new_lens)
        if reason:
            raise ValueError(reason)
    eager = _eager(ckv_new)
    _layout_check(cache, eager)
    if eager:
        _append_eager(cache, ckv_new, kpe_new, new_lens, bool(advance))
        return cache
    ok, why = nn._pre_check_can_use_hip_attention(device=ckv_new.device)
    if not ok:
        raise ValueError(why)
    if torch.compiler.is_compiling():
        nn._ops().fp8_paged_mla_cache_append_(cache.pool, cache.scale, cache.block_table, cache.seqlens, ckv_new, kpe_new, new_lens,
                                              cache.num_pages, cache.page_size, cache.fp8_format, bool(advance))
    else:
        _native.paged_mla_cache_append_fp8(cache.pool, cache.scale, cache.block_table, cache.seqlens, ckv_new, kpe_new,
                                           num_pages=cache.num_pages, page_size=cache.page_size,
                                           fp8_dtype=_native.fp8_dtype_of(cache.fp8_format), new_lens=new_lens, advance=bool(advance))
    return cache


@torch.compiler.assume_constant_result
def _resolve_splits(num_splits: int, B: int, Hq: int, Sq: int, Skv: int, device) -> int:
    if num_splits:
        return num_splits
    cus = torch.cuda.get_device_properties(device).multi_processor_count if torch.device(device).type == "cuda" else _CPU_NUM_CUS
    return _native.mla_auto_splits(B, Hq, Sq, Skv, cus)


def fp8_mla_paged_func(q: Tensor, cache: PagedMLACacheFP8, *, scale: Optional[float] = None, causal: bool = True,
                       seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, num_splits: int = 0, return_lse: bool = False,
                       return_partials: bool = False, return_q8: bool = False):
    """Absorbed MLA decode: q [B, Hq, Sq, 576] (the absorbed q_nope | the rotated q_pe, in cache.dtype) over the paged latent cache; returns
    out [B, Hq, Sq, 512] in q's dtype (the caller applies W_UV).

    scale         REQUIRED: the model's softmax scale (1/sqrt(192) times its YaRN factor for DeepSeek-V3); there is no 1/sqrt(576) default.
    causal        bottom-right over Sq: position i attends keys j <= L_b - Sq + i.
    seqused_k     int32 [B] on the device, default cache.seqlens; slot b uses its first L_b = clamp(seqused_k[b], 0, max_seqlen_k) keys.  A row
                  without a key is a zero row with LSE -inf.
    max_seqlen_k  a host int: the logical key bound of the call, default max_pages_per_seq * page_size.  Pass the longest live sequence or
                  the num_splits = 0 rule over-splits.
    num_splits    0: `qattn_mla_auto_splits` on max_seqlen_k; one split rounds into out, more are merged by ONE combine launch.
    return_lse / return_partials / return_q8 append lse [B, Hq, Sq] (natural log of the scaled scores), (partial_o [ns, B, Hq, Sq, 512],
    partial_lse [ns, B, Hq, Sq]) in fp32 (empty with one split), and (q8 [B, Hq, Sq, 576] e4m3, scale_q [B, Hq, Sq]) -- what the kernel's
    own token-wise quantiser made of q.
    Table and lengths are read on the device: no host synchronisation, graph-capture safe.  CPU tensors and
    config.attention.force_eager_fallback run the eager definition (`_attend_eager`); on the device there is no fallback.  Unsupported input
    raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = mla_input_reason(q, cache, scale=scale, seqused_k=seqused_k, max_seqlen_k=max_seqlen_k, num_splits=num_splits)
        if reason:
            raise ValueError(reason)
    B, Hq, Sq, _ = q.shape
    Skv = cache.capacity if max_seqlen_k is None else int(max_seqlen_k)
    used = cache.seqlens if seqused_k is None else seqused_k
    ns = _resolve_splits(num_splits, B, Hq, Sq, Skv, q.device)
    eager = _eager(q)
    _layout_check(cache, eager)
    if eager:
        out, lse, po, plse, q8, sq = _attend_eager(q, cache, bool(causal), float(scale), used, Skv, ns)
    else:
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        out, lse, po, plse, q8, sq = nn._ops().fp8_paged_mla_attention_forward(
            q, cache.pool, cache.scale, cache.block_table, used, Skv, cache.num_pages, cache.page_size, ns, float(scale), cache.fp8_format,
            bool(causal), bool(return_partials), bool(return_q8))
    res: Tuple = (out,)
    if return_lse:
        res += (lse,)
    if return_partials:
        res += (po, plse)
    if return_q8:
        res += (q8, sq)
    return res if len(res) > 1 else out


# ---- sparse (top-k indexed) decode on a row-major cache (include/qattn_mla_sparse.h) -------------------------------------------------------------
def alloc_paged_mla_row_cache_fp8(num_pages: int, page_size: int, *, batch_size: int, max_pages_per_seq: int, scale, dtype, device,
                                  fp8_format: Optional[str] = None) -> PagedMLACacheFP8:
    """An empty ROW-MAJOR paged latent cache for `fp8_mla_paged_sparse_func`: a zero-filled fp8 pool [num_pages, page_size, 576] (a key is one
    contiguous row; page_size is any integer >= 1), a zero-filled block table int32 [batch_size, max_pages_per_seq] and seqlens = 0, on
    any device.  num_pages * page_size <= 2^31 - 1 and max_pages_per_seq * page_size <= 2^31 - 65; scale and dtype as
    `alloc_paged_mla_cache_fp8`.  layout = "rowmajor"."""
    reason = _alloc_reason(num_pages, 64, batch_size, max_pages_per_seq, scale, dtype)
    if not reason and not (_is_int(page_size) and page_size >= 1):
        reason = f"page_size must be a positive integer, got {page_size!r}"
    if not reason and (num_pages * page_size > 2 ** 31 - 1 or max_pages_per_seq * page_size > 2 ** 31 - 65):
        reason = "num_pages * page_size and max_pages_per_seq * page_size must stay below 2^31"
    if reason:
        raise ValueError(reason)
    fp8_format = checks.config_value("attention.fp8_format") if fp8_format is None else fp8_format
    fp8_dtype = _native.fp8_dtype_of(fp8_format)
    device = torch.device(device)
    if device.type == "cuda" and not checks.config_value("attention.force_eager_fallback"):
        ok, why = nn._pre_check_can_use_hip_attention(device=device)
        if not ok:
            raise ValueError(why)
    sc = (torch.as_tensor(scale, dtype=torch.float32, device=device) if isinstance(scale, Tensor)
          else torch.full((), float(scale), dtype=torch.float32, device=device)).expand(batch_size).contiguous()
    table = torch.zeros((batch_size, max_pages_per_seq), dtype=torch.int32, device=device)
    seqlens = torch.zeros((batch_size,), dtype=torch.int32, device=device)
    pool = torch.zeros((num_pages, page_size, D), dtype=torch.uint8, device=device).view(fp8_dtype)
    return PagedMLACacheFP8(pool, sc, table, seqlens, num_pages, page_size, fp8_format, dtype, "rowmajor")


def mla_sparse_input_reason(q, cache, indices=None, *, scale=None, seqused_k=None, num_splits=0, ckv_new=None, kpe_new=None,
                            new_lens=None) -> Optional[str]:
    """The first rule the arguments of `fp8_mla_paged_sparse_func` (q, indices given) or `paged_mla_row_cache_append_fp8` (q None; ckv_new,
    kpe_new given) break, or None.  Shapes, dtypes, devices and strides only: the CONTENTS of indices / block_table / seqlens are read on
    the device."""
    reason = _cache_reason(cache, row=True)
    if reason:
        return reason
    p = cache.pool
    if cache.layout != "rowmajor" or not isinstance(p, Tensor) or tuple(p.shape) != (cache.num_pages, cache.page_size, D) or not p.is_contiguous():
        return (f"Expected a row-major cache (alloc_paged_mla_row_cache_fp8) with a dense pool [num_pages, page_size, {D}]; "
                "a chunk-image cache (alloc_paged_mla_cache_fp8) serves fp8_mla_paged_func")
    if q is None:
        return _append_reason(cache, ckv_new, kpe_new, new_lens)
    reason = _query_reason(q, cache, scale, seqused_k)
    if reason:
        return reason
    B, Sq = q.shape[0], q.shape[2]
    if (not isinstance(indices, Tensor) or indices.dtype != torch.int32 or indices.dim() != 3 or tuple(indices.shape[:2]) != (B, Sq)
            or not 1 <= indices.shape[2] <= MAX_TOPK):
        return (f"Expected indices to be a torch.int32 tensor [{B}, {Sq}, 1 <= topk <= {MAX_TOPK}] of logical key positions, but got "
                f"{getattr(indices, 'dtype', None)} {list(getattr(indices, 'shape', ()))}")
    if indices.device != q.device:
        return f"Expected indices to be on the query's device {q.device}, but got {indices.device} instead."
    if (indices.shape[2] > 1 and indices.stride(2) != 1) or any(indices.shape[i] > 1 and indices.stride(i) < 0 for i in (0, 1)):
        return f"Expected indices to have a dense last dimension, but got strides {tuple(indices.stride())}; pass indices.contiguous()"
    least = -(-indices.shape[2] // SPLIT_ENTRIES)
    if isinstance(num_splits, bool) or not isinstance(num_splits, int) or not (num_splits == 0 or least <= num_splits <= MAX_SPLITS):
        return (f"num_splits must be 0 (choose) or an integer in ceil(topk / {SPLIT_ENTRIES}) = {least} .. {MAX_SPLITS} (a split resolves at "
                f"most {SPLIT_ENTRIES} entries), got {num_splits!r}")
    return None


def sparse_split_plan(topk: int, num_splits: int):
    """Entry ranges [lo, hi) of the splits of a list of topk entries: ceil(topk / 64) groups, per = ceil(groups / ns) per split."""
    per = -(-(-(-topk // 64)) // num_splits)
    return [(min(64 * s * per, topk), min(64 * (s + 1) * per, topk)) for s in range(num_splits)]


def _attend_sparse_eager(q, cache, indices, causal, scale, seqused_k, ns):
    """gather the listed valid rows through the (clamped) table, de-quantise, fp32 softmax per split over the entries in list order, values =
    the first 512 channels; the partials are merged by `combine_eager`.  (Reads indices / block_table / seqused_k on the host.)"""
    B, Hq, Sq, _ = q.shape
    topk, ps = indices.shape[2], cache.page_size
    q8, scale_q = quantize_q_eager(q)
    qd = q8.float() * scale_q[..., None]
    table = cache.block_table.clamp(0, cache.num_pages - 1).long()
    po = torch.zeros((ns, B, Hq, Sq, D_LATENT), dtype=torch.float32, device=q.device)
    plse = torch.full((ns, B, Hq, Sq), -math.inf, dtype=torch.float32, device=q.device)
    for b, Lb in enumerate(seqused_k.tolist()):
        Lb = min(max(int(Lb), 0), cache.capacity)
        for i in range(Sq):
            kend = max(Lb - Sq + i + 1, 0) if causal else Lb
            for s, (lo, hi) in enumerate(sparse_split_plan(topk, ns)):
                j = indices[b, i, lo:hi].long()
                j = j[(j >= 0) & (j < kend)]
                if j.numel() == 0:
                    continue
                lat = cache.pool[table[b][j // ps], j % ps].float() * cache.scale[b]          # [n, 576]
                sc = qd[b, :, i] @ lat.T * scale
                lse = torch.logsumexp(sc, dim=-1)
                po[s, b, :, i] = torch.exp(sc - lse[:, None]) @ lat[:, :D_LATENT]
                plse[s, b, :, i] = lse
    out, lse = combine_eager(po, plse, q.dtype)
    empty = torch.empty((0,), dtype=torch.float32, device=q.device)
    return out, lse, (po if ns > 1 else empty), (plse if ns > 1 else empty), q8, scale_q


def paged_mla_row_cache_append_fp8(cache: PagedMLACacheFP8, ckv_new: Tensor, kpe_new: Tensor, *, new_lens: Optional[Tensor] = None,
                                   advance: bool = True) -> PagedMLACacheFP8:
    """Append T tokens per slot to the ROW-MAJOR paged latent `cache` (alloc_paged_mla_row_cache_fp8), in place; returns `cache`.  The contract
    of `paged_mla_cache_append_fp8` word for word -- views read through their strides, the same quantiser, tokens at or beyond the capacity
    dropped, every table entry clamped, exactly the bytes of the appended keys change, everything read on the device -- with key j of slot
    b stored as row j % page_size of page block_table[b, j // page_size].  CPU tensors and config.attention.force_eager_fallback run the
    eager definition (`_append_eager`); on the device there is no fallback.  Invalid input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = mla_sparse_input_reason(None, cache, ckv_new=ckv_new, kpe_new=kpe_new, new_lens=new_lens)
        if reason:
            raise ValueError(reason)
    if _eager(ckv_new):
        _append_eager(cache, ckv_new, kpe_new, new_lens, bool(advance))
        return cache
    ok, why = nn._pre_check_can_use_hip_attention(device=ckv_new.device)
    if not ok:
        raise ValueError(why)
    if torch.compiler.is_compiling():
        nn._ops().fp8_paged_mla_row_cache_append_(cache.pool, cache.scale, cache.block_table, cache.seqlens, ckv_new, kpe_new, new_lens,
                                                  cache.num_pages, cache.page_size, cache.fp8_format, bool(advance))
    else:
        _native.paged_mla_row_cache_append_fp8(cache.pool, cache.scale, cache.block_table, cache.seqlens, ckv_new, kpe_new,
                                               num_pages=cache.num_pages, page_size=cache.page_size,
                                               fp8_dtype=_native.fp8_dtype_of(cache.fp8_format), new_lens=new_lens, advance=bool(advance))
    return cache


@torch.compiler.assume_constant_result
def _resolve_sparse_splits(num_splits: int, B: int, Hq: int, Sq: int, topk: int, device) -> int:
    if num_splits:
        return num_splits
    cus = torch.cuda.get_device_properties(device).multi_processor_count if torch.device(device).type == "cuda" else _CPU_NUM_CUS
    return _native.mla_sparse_auto_splits(B, Hq, Sq, topk, cus)


def fp8_mla_paged_sparse_func(q: Tensor, cache: PagedMLACacheFP8, indices: Tensor, *, scale: Optional[float] = None, causal: bool = True,
                              seqused_k: Optional[Tensor] = None, num_splits: int = 0, return_lse: bool = False,
                              return_partials: bool = False, return_q8: bool = False):
    """Sparse absorbed MLA decode (DeepSeek-V3.2-style layers): q [B, Hq, Sq, 576] attends only the keys `indices` names in the row-major
    paged latent cache; returns out [B, Hq, Sq, 512] in q's dtype.

    indices       int32 [B, Sq, topk] on q's device, last dimension dense, topk >= 1 arbitrary: LOGICAL key positions of slot b, shared by
                  all Hq heads of (b, i) and resolved through cache.block_table on the device.  An entry j is VALID iff 0 <= j < kend(b, i),
                  kend = L_b (causal=False) or L_b - Sq + i + 1 (causal=True), L_b = clamp(seqused_k[b], 0, capacity).  Everything else
                  (-1, padding, positions at or behind the limit) contributes nothing, whatever bytes it points at.  Entries count as often
                  as they are listed; a row without a valid entry is a zero row with LSE -inf.
    scale         REQUIRED: the model's softmax scale, as in `fp8_mla_paged_func`.
    seqused_k     int32 [B] on the device, default cache.seqlens.
    num_splits    0: `qattn_mla_sparse_auto_splits`; else ceil(topk / 2048) .. 64 splits of the LIST (64-entry groups), merged by ONE
                  combine launch.
    return_lse / return_partials / return_q8 as in `fp8_mla_paged_func`.  Numerics are that call's: q quantised in the kernel (token-wise
    e4m3), two-term e4m3 P, both products on the FP8 matrix instructions.
    Indices, table and lengths are read on the device: no host synchronisation, graph-capture safe.  CPU tensors and
    config.attention.force_eager_fallback run the eager definition (`_attend_sparse_eager`); on the device there is no fallback.
    Unsupported input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = mla_sparse_input_reason(q, cache, indices, scale=scale, seqused_k=seqused_k, num_splits=num_splits)
        if reason:
            raise ValueError(reason)
    B, Hq, Sq, _ = q.shape
    used = cache.seqlens if seqused_k is None else seqused_k
    ns = _resolve_sparse_splits(num_splits, B, Hq, Sq, indices.shape[2], q.device)
    if _eager(q):
        out, lse, po, plse, q8, sq = _attend_sparse_eager(q, cache, indices, bool(causal), float(scale), used, ns)
    else:
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        out, lse, po, plse, q8, sq = nn._ops().fp8_paged_mla_sparse_attention_forward(
            q, cache.pool, cache.scale, cache.block_table, used, indices, cache.num_pages, cache.page_size, ns, float(scale), cache.fp8_format,
            bool(causal), bool(return_partials), bool(return_q8))
    res: Tuple = (out,)
    if return_lse:
        res += (lse,)
    if return_partials:
        res += (po, plse)
    if return_q8:
        res += (q8, sq)
    return res if len(res) > 1 else out

"""Absorbed FP8 MLA on PACKED variable-length queries over the one-image paged latent cache: `fp8_mla_paged_func` for a continuous-batching
step whose slots carry different numbers of new tokens -- one decode token, a few speculative drafts, a prompt chunk attended in absorbed form
(include/qattn_mla_varlen.h):

    paged_mla_cache_append_fp8(cache, ckv, kpe, new_lens=n)                       # the step's own keys first: L_b includes them
    out = fp8_mla_paged_varlen_func(q, cache, cu_seqlens_q, max_seqlen_q, scale=model_softmax_scale)     # q [total_q, Hq, 576]

Token i of slot b (packed row cu[b] + i) attends the keys j <= L_b - n_b + i (bottom-right causal) or all L_b (causal=False); everything else
is `fp8_mla_paged_func`'s rule word for word, and out, lse, q8, scale_q and the partials of a slot equal that call on the slot's tokens as
[1, Hq, n_b, 576] with the same num_splits bit for bit.  On the device one 8-wave workgroup serves a 128-row tile of ONE slot's (head, token)
rows and a key split: half the chunk reads and transpositions per row of the 64-row dense kernel.

Package attributes, not names of `__all__`.  Not offered: the row-major cache; a 64-row instance for slots of <= 64 rows (a pure decode step
keeps `fp8_mla_paged_func`); per-slot split counts; windows, sinks, soft cap or trees on MLA."""
import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native, mla as _mla, nn
from .kvcache import _is_int
from .mla import D, D_LATENT, MAX_SPLITS, PagedMLACacheFP8
from .paged import _lens_reason
from .utils import checks


def mla_varlen_input_reason(q, cache, cu_seqlens_q, max_seqlen_q, *, scale=None, seqused_k=None, max_seqlen_k=None,
                            num_splits=0) -> Optional[str]:
    """The first rule the arguments of `fp8_mla_paged_varlen_func` break, or None.  Shapes, dtypes, devices and strides only: the CONTENTS of
    cu_seqlens_q / block_table / seqlens are read on the device."""
    reason = _mla._cache_reason(cache)
    if reason:
        return reason
    B = cache.batch_size
    if cache.device.type == "cuda" and not checks.config_value("attention.force_eager_fallback") and cache.layout != "frag":
        return ("Expected the chunk-image cache of alloc_paged_mla_cache_fp8; a row-major cache (alloc_paged_mla_row_cache_fp8) serves "
                "fp8_mla_paged_sparse_varlen_func")
    if not isinstance(q, Tensor) or q.dim() != 3:
        return "NYI: the packed query must be a 3-D tensor [total_q, Hq, 576]"
    if q.requires_grad:
        return "NYI: query must be a leaf tensor (no backward)"
    if q.dtype not in (torch.float16, torch.bfloat16) or q.dtype != cache.dtype:
        return f"Expected query to have the cache's dtype {cache.dtype} (torch.float16 or torch.bfloat16), but got {q.dtype} instead."
    if q.shape[-1] != D:
        return f"Expected the query's head dimension to be {D} (512 latent + 64 rotary channels, absorbed form), but got {q.shape[-1]}."
    total_q, Hq = q.shape[0], q.shape[1]
    if total_q < 1 or not 1 <= Hq <= 2 ** 20 or total_q * Hq + 128 * (B + 1) > 2 ** 31 - 1:
        return f"Expected the packed query to have shape [total_q >= 1, 1 <= Hq <= 2^20, {D}] with total_q * Hq below 2^31, but got {list(q.shape)}."
    if q.device != cache.device:
        return f"Expected query and the cache to be on the same device, but got {q.device} and {cache.device} instead."
    if not _native.mla_rows_addressable(q):
        return f"Expected query to have dense channels and 16-byte-aligned rows, but got strides {tuple(q.stride())}; pass query.contiguous()"
    if not isinstance(cu_seqlens_q, Tensor) or cu_seqlens_q.dtype != torch.int32 or tuple(cu_seqlens_q.shape) != (B + 1,):
        return f"Expected cu_seqlens_q to be a torch.int32 tensor [B + 1 = {B + 1}], but got {getattr(cu_seqlens_q, 'dtype', None)} {list(getattr(cu_seqlens_q, 'shape', ()))}"
    if cu_seqlens_q.device != q.device:
        return f"Expected cu_seqlens_q to be on {q.device}, but got {cu_seqlens_q.device} instead."
    if not (_is_int(max_seqlen_q) and 1 <= max_seqlen_q <= total_q):
        return f"max_seqlen_q must be an integer in 1 .. total_q = {total_q} (the host bound of a slot's tokens), got {max_seqlen_q!r}"
    if scale is None:
        return "scale is required: MLA's softmax scale is the model's (1/sqrt(192) times its YaRN factor), not 1/sqrt(576)"
    if not (isinstance(scale, (int, float)) and not isinstance(scale, bool) and math.isfinite(scale) and scale > 0):
        return f"scale must be a finite number > 0, got {scale!r}"
    if max_seqlen_k is not None and not (_is_int(max_seqlen_k) and 1 <= max_seqlen_k <= cache.capacity):
        return f"max_seqlen_k must be None or an integer in 1 .. max_pages_per_seq * page_size = {cache.capacity}, got {max_seqlen_k!r}"
    if isinstance(num_splits, bool) or not isinstance(num_splits, int) or not 0 <= num_splits <= MAX_SPLITS:
        return f"num_splits must be 0 (choose) or an integer in 1 .. {MAX_SPLITS}, got {num_splits!r}"
    return _lens_reason("seqused_k" if seqused_k is not None else "cache.seqlens", cache.seqlens if seqused_k is None else seqused_k, B, q.device)


def _varlen_eager(q, cache, cu, causal, scale, used, Skv, ns):
    """the definition: per slot, `mla._attend_eager` on the slot's tokens with Sq = n_b.  (Reads cu_seqlens_q on the host.)"""
    total_q, Hq, _ = q.shape
    out = torch.zeros((total_q, Hq, D_LATENT), dtype=q.dtype, device=q.device)
    lse = torch.full((Hq, total_q), -math.inf, dtype=torch.float32, device=q.device)
    po = torch.zeros((ns, total_q, Hq, D_LATENT), dtype=torch.float32, device=q.device)
    plse = torch.full((ns, total_q, Hq), -math.inf, dtype=torch.float32, device=q.device)
    q8 = torch.zeros((total_q, Hq, D), dtype=torch.uint8, device=q.device).view(torch.float8_e4m3fn)
    sq = torch.zeros((total_q, Hq), dtype=torch.float32, device=q.device)
    ends = [min(max(int(x), 0), total_q) for x in cu.tolist()]
    for b in range(cache.batch_size):
        lo, hi = ends[b], max(ends[b + 1], ends[b])
        if hi == lo:
            continue
        one = PagedMLACacheFP8(cache.pool, cache.scale[b:b + 1], cache.block_table[b:b + 1], used[b:b + 1], cache.num_pages, cache.page_size,
                               cache.fp8_format, cache.dtype, cache.layout)
        o, l, pob, plb, q8b, sqb = _mla._attend_eager(q[lo:hi].transpose(0, 1)[None], one, causal, scale, used[b:b + 1], Skv, ns)
        out[lo:hi], lse[:, lo:hi], sq[lo:hi] = o[0].transpose(0, 1), l[0], sqb[0].transpose(0, 1)
        q8.view(torch.uint8)[lo:hi] = q8b[0].transpose(0, 1).view(torch.uint8)
        if ns > 1:
            po[:, lo:hi], plse[:, lo:hi] = pob[:, 0].transpose(1, 2), plb[:, 0].transpose(1, 2)
    empty = torch.empty((0,), dtype=torch.float32, device=q.device)
    return out, lse, (po if ns > 1 else empty), (plse if ns > 1 else empty), q8, sq


@torch.compiler.assume_constant_result
def _resolve_splits(num_splits: int, B: int, total_q: int, Hq: int, Skv: int, device) -> int:
    if num_splits:
        return num_splits
    cus = torch.cuda.get_device_properties(device).multi_processor_count if torch.device(device).type == "cuda" else _mla._CPU_NUM_CUS
    return _native.mla_varlen_auto_splits(_native.mla_varlen_tile_slots(B, total_q, Hq), Skv, cus)


def fp8_mla_paged_varlen_func(q: Tensor, cache: PagedMLACacheFP8, cu_seqlens_q: Tensor, max_seqlen_q: int, *, scale: Optional[float] = None,
                              causal: bool = True, seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None,
                              num_splits: int = 0, return_lse: bool = False, return_partials: bool = False, return_q8: bool = False):
    """Absorbed MLA on packed queries over the paged latent cache: returns out [total_q, Hq, 512] in q's dtype (the caller applies W_UV).

    q             [total_q, Hq, 576] in cache.dtype (the absorbed q_nope | the rotated q_pe; a view with dense channels and 16-byte-aligned
                  rows -- a slice of a wider projection -- is read through its strides); quantised in the kernel per (token, head) row.
    cache         the chunk-image paged latent cache of `alloc_paged_mla_cache_fp8`.
    cu_seqlens_q  int32 [B + 1] on the device, B = cache.batch_size, cu[0] = 0, non-decreasing: slot b owns the rows cu[b] .. cu[b+1] - 1
                  (n_b of them, 0 allowed).  Rows at or behind cu[B] -- a padded token bucket -- are never read from q: zero rows, LSE -inf.
    max_seqlen_q  a host int in 1 .. total_q that bounds n_b; never read back from the device.
    scale         REQUIRED: the model's softmax scale, as in `fp8_mla_paged_func`.
    causal        token i of slot b attends keys j <= L_b - n_b + i (bottom-right: append the step's own keys first); False: all L_b keys.
                  L_b = clamp(seqused_k[b], 0, max_seqlen_k).  A row without a key is a zero row with LSE -inf.
    seqused_k     int32 [B] on the device, default cache.seqlens.   max_seqlen_k: the logical key bound, default the capacity.
    num_splits    ONE count for all slots; slot b uses `fp8_mla_paged_func`'s plan on its own L_b.  0: `qattn_mla_varlen_auto_splits` on
                  ceil(total_q Hq / 128) + B tile slots and max_seqlen_k.  More than one split is merged by ONE combine launch.
    return_lse appends lse fp32 [Hq, total_q] (the packed convention `merge_attn_states` takes); return_partials appends (partial_o
    [ns, total_q, Hq, 512], partial_lse [ns, total_q, Hq]) in fp32 (empty with one split); return_q8 appends (q8 [total_q, Hq, 576] e4m3,
    scale_q [total_q, Hq]).
    Everything is read on the device: no host synchronisation, graph-capture safe.  CPU tensors and config.attention.force_eager_fallback
    run the eager definition (`_varlen_eager`); on the device there is no fallback.  Unsupported input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = mla_varlen_input_reason(q, cache, cu_seqlens_q, max_seqlen_q, scale=scale, seqused_k=seqused_k, max_seqlen_k=max_seqlen_k,
                                         num_splits=num_splits)
        if reason:
            raise ValueError(reason)
    total_q, Hq, _ = q.shape
    Skv = cache.capacity if max_seqlen_k is None else int(max_seqlen_k)
    used = cache.seqlens if seqused_k is None else seqused_k
    ns = _resolve_splits(num_splits, cache.batch_size, total_q, Hq, Skv, q.device)
    eager = _mla._eager(q)
    _mla._layout_check(cache, eager)
    if eager:
        out, lse, po, plse, q8, sq = _varlen_eager(q, cache, cu_seqlens_q, bool(causal), float(scale), used, Skv, ns)
    else:
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        out, lse, po, plse, q8, sq = nn._ops().fp8_mla_paged_varlen_attention_forward(
            q, cache.pool, cache.scale, cache.block_table, used, cu_seqlens_q, int(max_seqlen_q), Skv, cache.num_pages, cache.page_size, ns,
            float(scale), cache.fp8_format, bool(causal), bool(return_partials), bool(return_q8))
    res: Tuple = (out,)
    if return_lse:
        res += (lse,)
    if return_partials:
        res += (po, plse)
    if return_q8:
        res += (q8, sq)
    return res if len(res) > 1 else out

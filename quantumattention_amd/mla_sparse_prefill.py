"""Sparse (top-k indexed) FP8 MLA on PACKED variable-length queries: the prompt's form of `fp8_mla_paged_sparse_func`
(include/qattn_mla_sparse_prefill.h).  It takes the lists `fp8_mla_index_topk_varlen_func` returns as they are:

    paged_mla_row_cache_append_fp8(row_cache, ckv, kpe, new_lens=n)                          # the chunk's own keys first: L_b includes them
    indices = fp8_mla_index_topk_varlen_func(q_idx, weights, icache, cu_seqlens_q, 2048)     # int32 [total_q, topk]
    out = fp8_mla_paged_sparse_varlen_func(q, row_cache, indices, cu_seqlens_q, scale=model_softmax_scale)   # q [total_q, Hq, 576]

Token i of slot b (packed row cu[b] + i) attends the listed positions j with 0 <= j < kend = L_b (causal=False) or L_b - n_b + i + 1
(bottom-right causal); everything else is `fp8_mla_paged_sparse_func`'s rule word for word, and out, lse, q8 and scale_q of a slot equal that
call on the slot's tokens (num_splits=1) bit for bit.  On the device one 8-wave workgroup serves a token and up to 128 of its heads: one
resolve, one gather and one transposition per 64-entry group instead of one per 64 heads.

Package attributes, not names of `__all__`.  Not offered: key splits (a step of a handful of tokens keeps `fp8_mla_paged_sparse_func`); a
64-row instance for Hq <= 64; physical indices; a packed row-cache append."""
import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import mla as _mla, nn
from .mla import D, D_LATENT, MAX_TOPK, PagedMLACacheFP8
from .paged import _lens_reason
from .utils import checks


def mla_sparse_varlen_input_reason(q, cache, indices, cu_seqlens_q, *, scale=None, seqused_k=None) -> Optional[str]:
    """The first rule the arguments of `fp8_mla_paged_sparse_varlen_func` break, or None.  Shapes, dtypes, devices and strides only: the
    CONTENTS of indices / cu_seqlens_q / block_table / seqlens are read on the device."""
    reason = _mla._cache_reason(cache, row=True)
    if reason:
        return reason
    p, B = cache.pool, cache.batch_size
    if cache.layout != "rowmajor" or not isinstance(p, Tensor) or tuple(p.shape) != (cache.num_pages, cache.page_size, D) or not p.is_contiguous():
        return f"Expected a row-major cache (alloc_paged_mla_row_cache_fp8) with a dense pool [num_pages, page_size, {D}]"
    if not isinstance(q, Tensor) or q.dim() != 3:
        return "NYI: the packed query must be a 3-D tensor [total_q, Hq, 576]"
    if q.requires_grad:
        return "NYI: query must be a leaf tensor (no backward)"
    if q.dtype not in (torch.float16, torch.bfloat16) or q.dtype != cache.dtype:
        return f"Expected query to have the cache's dtype {cache.dtype} (torch.float16 or torch.bfloat16), but got {q.dtype} instead."
    if q.shape[-1] != D:
        return f"Expected the query's head dimension to be {D} (512 latent + 64 rotary channels, absorbed form), but got {q.shape[-1]}."
    if q.shape[0] < 1 or not 1 <= q.shape[1] <= 2 ** 20:
        return f"Expected the packed query to have shape [total_q >= 1, 1 <= Hq <= 2^20, {D}], but got {list(q.shape)}."
    if q.device != cache.device:
        return f"Expected query and the cache to be on the same device, but got {q.device} and {cache.device} instead."
    if not _mla._native.mla_rows_addressable(q):
        return f"Expected query to have dense channels and 16-byte-aligned rows, but got strides {tuple(q.stride())}; pass query.contiguous()"
    total_q = q.shape[0]
    if (not isinstance(indices, Tensor) or indices.dtype != torch.int32 or indices.dim() != 2 or indices.shape[0] != total_q
            or not 1 <= indices.shape[1] <= MAX_TOPK):
        return (f"Expected indices to be a torch.int32 tensor [{total_q}, 1 <= topk <= {MAX_TOPK}] of logical key positions, but got "
                f"{getattr(indices, 'dtype', None)} {list(getattr(indices, 'shape', ()))}")
    if indices.device != q.device:
        return f"Expected indices to be on the query's device {q.device}, but got {indices.device} instead."
    if (indices.shape[1] > 1 and indices.stride(1) != 1) or (total_q > 1 and indices.stride(0) < 0):
        return f"Expected indices to have a dense last dimension, but got strides {tuple(indices.stride())}; pass indices.contiguous()"
    if not isinstance(cu_seqlens_q, Tensor) or cu_seqlens_q.dtype != torch.int32 or tuple(cu_seqlens_q.shape) != (B + 1,):
        return f"Expected cu_seqlens_q to be a torch.int32 tensor [B + 1 = {B + 1}], but got {getattr(cu_seqlens_q, 'dtype', None)} {list(getattr(cu_seqlens_q, 'shape', ()))}"
    if cu_seqlens_q.device != q.device:
        return f"Expected cu_seqlens_q to be on {q.device}, but got {cu_seqlens_q.device} instead."
    if scale is None:
        return "scale is required: MLA's softmax scale is the model's (1/sqrt(192) times its YaRN factor), not 1/sqrt(576)"
    if not (isinstance(scale, (int, float)) and not isinstance(scale, bool) and math.isfinite(scale) and scale > 0):
        return f"scale must be a finite number > 0, got {scale!r}"
    return _lens_reason("seqused_k" if seqused_k is not None else "cache.seqlens", cache.seqlens if seqused_k is None else seqused_k, B, q.device)


def _varlen_eager(q, cache, indices, cu, causal, scale, used) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """the definition: per slot, `mla._attend_sparse_eager` with one split on the slot's tokens.  (Reads cu_seqlens_q on the host.)"""
    total_q, Hq, _ = q.shape
    out = torch.zeros((total_q, Hq, D_LATENT), dtype=q.dtype, device=q.device)
    lse = torch.full((Hq, total_q), -math.inf, dtype=torch.float32, device=q.device)
    q8 = torch.zeros((total_q, Hq, D), dtype=torch.uint8, device=q.device).view(torch.float8_e4m3fn)
    sq = torch.zeros((total_q, Hq), dtype=torch.float32, device=q.device)
    ends = [min(max(int(x), 0), total_q) for x in cu.tolist()]
    for b in range(cache.batch_size):
        lo, hi = ends[b], max(ends[b + 1], ends[b])
        if hi == lo:
            continue
        one = PagedMLACacheFP8(cache.pool, cache.scale[b:b + 1], cache.block_table[b:b + 1], used[b:b + 1], cache.num_pages, cache.page_size,
                               cache.fp8_format, cache.dtype, cache.layout)
        o, l, _, _, q8b, sqb = _mla._attend_sparse_eager(q[lo:hi].transpose(0, 1)[None], one, indices[None, lo:hi], causal, scale,
                                                         used[b:b + 1], 1)
        out[lo:hi], lse[:, lo:hi], sq[lo:hi] = o[0].transpose(0, 1), l[0], sqb[0].transpose(0, 1)
        q8.view(torch.uint8)[lo:hi] = q8b[0].transpose(0, 1).view(torch.uint8)
    return out, lse, q8, sq


def fp8_mla_paged_sparse_varlen_func(q: Tensor, cache: PagedMLACacheFP8, indices: Tensor, cu_seqlens_q: Tensor, *,
                                     scale: Optional[float] = None, causal: bool = True, seqused_k: Optional[Tensor] = None,
                                     return_lse: bool = False, return_q8: bool = False):
    """Sparse absorbed MLA on packed queries: returns out [total_q, Hq, 512] in q's dtype.

    q             [total_q, Hq, 576] in cache.dtype (a view with dense channels and 16-byte-aligned rows -- a slice of a wider projection --
                  is read through its strides); quantised in the kernel per (token, head) row, always to e4m3.
    cache         a ROW-MAJOR paged latent cache (`alloc_paged_mla_row_cache_fp8`).
    indices       int32 [total_q, topk] on q's device, last dimension dense, any row stride, 1 <= topk <= 2048 * 64: LOGICAL key positions
                  of the token's slot, shared by all its heads.  An entry j is VALID iff 0 <= j < kend; everything else (-1, padding,
                  positions at or behind the limit) contributes nothing, whatever bytes it points at.  Entries count as often as listed.
    cu_seqlens_q  int32 [B + 1] on the device, B = cache.batch_size, cu[0] = 0, non-decreasing: slot b owns the rows cu[b] .. cu[b+1] - 1
                  (n_b of them, 0 allowed).  Rows at or behind cu[B] -- a padded token bucket -- read neither q nor their list: zero rows,
                  LSE -inf, q8 / scale_q 0.
    scale         REQUIRED: the model's softmax scale, as in `fp8_mla_paged_func`.
    causal        token i of slot b has kend = L_b - n_b + i + 1 (bottom-right: append the chunk's own keys first); False: kend = L_b.
                  L_b = clamp(seqused_k[b], 0, capacity).  A token without a valid entry is a zero row with LSE -inf.
    seqused_k     int32 [B] on the device, default cache.seqlens.
    return_lse appends lse fp32 [Hq, total_q] (the packed convention `merge_attn_states` takes); return_q8 appends (q8 [total_q, Hq, 576]
    e4m3, scale_q [total_q, Hq]).
    One launch, no workspace; everything is read on the device: no host synchronisation, graph-capture safe.
    CPU tensors and config.attention.force_eager_fallback run the eager definition (`_varlen_eager`); on the device there is no fallback.
    Unsupported input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = mla_sparse_varlen_input_reason(q, cache, indices, cu_seqlens_q, scale=scale, seqused_k=seqused_k)
        if reason:
            raise ValueError(reason)
    used = cache.seqlens if seqused_k is None else seqused_k
    if _mla._eager(q):
        out, lse, q8, sq = _varlen_eager(q, cache, indices, cu_seqlens_q, bool(causal), float(scale), used)
    else:
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        out, lse, q8, sq = nn._ops().fp8_mla_paged_sparse_varlen_attention_forward(
            q, cache.pool, cache.scale, cache.block_table, used, indices, cu_seqlens_q, cache.num_pages, cache.page_size, float(scale),
            cache.fp8_format, bool(causal), bool(return_q8))
    res: Tuple = (out,)
    if return_lse:
        res += (lse,)
    if return_q8:
        res += (q8, sq)
    return res if len(res) > 1 else out

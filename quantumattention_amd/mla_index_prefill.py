"""The FP8 lightning indexer on PACKED variable-length queries: the prompt's form of `fp8_mla_index_topk_func` (include/qattn_mla_index_prefill.h,
DESIGN.md section 4.35).  One call scores several prompts or prompt chunks of different lengths, each over its own cached keys:

    paged_mla_index_cache_append_fp8(icache, k_idx, new_lens=n)                              # the chunk's own keys first: L_b includes them
    indices = fp8_mla_index_topk_varlen_func(q_idx, weights, icache, cu_seqlens_q, 2048)     # q_idx [total_q, Hi, 128], weights [total_q, Hi]
    out_b = fp8_mla_paged_sparse_func(q_b, row_cache, indices[cu[b]:cu[b+1]][None], ...)     # per sequence (or directly at B = 1)

Token i of slot b (packed row cu[b] + i) scores the keys j < kend = L_b (causal=False) or max(L_b - n_b + i + 1, 0) (bottom-right causal),
L_b = clamp(seqused_k[b], 0, max_seqlen_k); everything else is `fp8_mla_index_topk_func`'s rule word for word, and the logits, indices, q8
and scale_q equal that call on the slot's tokens bit for bit.  On the device the score sweep shares every 128-key tile among 8 tokens
through LDS, where the dense entry's sweep pulls the keys once per token.

Package attributes, not names of `__all__`.  (Packed q for the sparse attention: mla_sparse_prefill.py.)  Not offered: the first selection histogram fused into
the sweep; per-key index scales."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native, mla as _mla, nn
from .kvcache import _is_int
from .mla_index import D, MAX_HEADS, MAX_TOPK, PagedMLAIndexCacheFP8, _scores_eager, _select_eager
from .paged import _lens_reason
from .utils import checks

TOKENS, KEYS, WG_KEYS = _native.MLA_INDEX_PREFILL_TOKENS, _native.MLA_INDEX_PREFILL_KEYS, _native.MLA_INDEX_PREFILL_WG_KEYS


def mla_index_varlen_input_reason(q, weights, icache, cu_seqlens_q, topk, *, seqused_k=None, max_seqlen_k=None) -> Optional[str]:
    """The first rule the arguments of `fp8_mla_index_topk_varlen_func` break, or None.  Shapes, dtypes, devices and strides only: the
    CONTENTS of cu_seqlens_q / block_table / seqlens are read on the device."""
    if not isinstance(icache, PagedMLAIndexCacheFP8):
        return "Expected icache to be a PagedMLAIndexCacheFP8 (alloc_paged_mla_index_cache_fp8)"
    reason = _mla._cache_reason(icache, row=True)
    if reason:
        return reason
    p, B = icache.pool, icache.batch_size
    if not isinstance(p, Tensor) or tuple(p.shape) != (icache.num_pages, icache.page_size, D) or not p.is_contiguous():
        return f"Expected icache.pool to be a dense fp8 tensor [num_pages, page_size, {D}]"
    if not isinstance(q, Tensor) or q.dim() != 3:
        return "NYI: the packed index query must be a 3-D tensor [total_q, Hi, 128]"
    if q.requires_grad:
        return "NYI: the index query must be a leaf tensor (no backward)"
    if q.dtype not in (torch.float16, torch.bfloat16) or q.dtype != icache.dtype:
        return f"Expected the index query to have the cache's dtype {icache.dtype} (torch.float16 or torch.bfloat16), but got {q.dtype} instead."
    if q.shape[-1] != D:
        return f"Expected the index query's head dimension to be {D}, but got {q.shape[-1]}."
    if q.shape[0] < 1 or not 1 <= q.shape[1] <= MAX_HEADS:
        return f"Expected the packed index query to have shape [total_q >= 1, 1 <= Hi <= {MAX_HEADS}, {D}], but got {list(q.shape)}."
    if q.device != icache.device:
        return f"Expected the index query and the cache to be on the same device, but got {q.device} and {icache.device} instead."
    if not _native.mla_rows_addressable(q):
        return f"Expected the index query to have dense channels and 16-byte-aligned rows, but got strides {tuple(q.stride())}; pass q.contiguous()"
    total_q, Hi = q.shape[:2]
    if not isinstance(weights, Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != (total_q, Hi) or weights.requires_grad:
        return f"Expected weights to be a torch.float32 leaf tensor [{total_q}, {Hi}], but got {getattr(weights, 'dtype', None)} {list(getattr(weights, 'shape', ()))}"
    if weights.device != q.device:
        return f"Expected weights to be on the query's device {q.device}, but got {weights.device} instead."
    if (Hi > 1 and weights.stride(1) != 1) or (total_q > 1 and weights.stride(0) <= 0):
        return f"Expected weights to have dense heads, but got strides {tuple(weights.stride())}; pass weights.contiguous()"
    if not isinstance(cu_seqlens_q, Tensor) or cu_seqlens_q.dtype != torch.int32 or tuple(cu_seqlens_q.shape) != (B + 1,):
        return f"Expected cu_seqlens_q to be a torch.int32 tensor [B + 1 = {B + 1}], but got {getattr(cu_seqlens_q, 'dtype', None)} {list(getattr(cu_seqlens_q, 'shape', ()))}"
    if cu_seqlens_q.device != q.device:
        return f"Expected cu_seqlens_q to be on {q.device}, but got {cu_seqlens_q.device} instead."
    if not (_is_int(topk) and 1 <= topk <= MAX_TOPK):
        return f"topk must be an integer in 1 .. {MAX_TOPK}, got {topk!r}"
    if max_seqlen_k is not None and not (_is_int(max_seqlen_k) and 1 <= max_seqlen_k <= min(icache.capacity, 2 ** 30)):
        return f"max_seqlen_k must be None or an integer in 1 .. max_pages_per_seq * page_size = {icache.capacity} (at most 2^30), got {max_seqlen_k!r}"
    if max_seqlen_k is None and icache.capacity > 2 ** 30:
        return "max_seqlen_k is required for a capacity above 2^30 keys"
    return _lens_reason("seqused_k" if seqused_k is not None else "icache.seqlens", icache.seqlens if seqused_k is None else seqused_k, B, q.device)


def _varlen_eager(q, weights, icache, cu, causal, used, Skv, topk) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """the definition: per slot, the dense entry's eager definitions on the slot's tokens.  (Reads cu_seqlens_q on the host.)"""
    total_q, Hi, _ = q.shape
    indices = torch.full((total_q, topk), -1, dtype=torch.int32, device=q.device)
    logits = torch.full((total_q, Skv), -torch.inf, dtype=torch.float32, device=q.device)
    q8 = torch.zeros((total_q, Hi, D), dtype=torch.uint8, device=q.device).view(torch.float8_e4m3fn)
    sq = torch.zeros((total_q, Hi), dtype=torch.float32, device=q.device)
    ends = [min(max(int(x), 0), total_q) for x in cu.tolist()]
    for b in range(icache.batch_size):
        lo, hi = ends[b], max(ends[b + 1], ends[b])
        if hi == lo:
            continue
        one = PagedMLAIndexCacheFP8(icache.pool, icache.scale[b:b + 1], icache.block_table[b:b + 1], used[b:b + 1], icache.num_pages,
                                    icache.page_size, icache.fp8_format, icache.dtype, "index")
        lg, q8b, sqb = _scores_eager(q[lo:hi].transpose(0, 1)[None], weights[None, lo:hi], one, causal, used[b:b + 1], Skv)
        indices[lo:hi] = _select_eager(lg, used[b:b + 1], topk, causal)[0]
        logits[lo:hi], sq[lo:hi] = lg[0], sqb[0].transpose(0, 1)
        q8.view(torch.uint8)[lo:hi] = q8b[0].transpose(0, 1).view(torch.uint8)
    return indices, logits, q8, sq


def fp8_mla_index_topk_varlen_func(q_idx: Tensor, weights: Tensor, icache: PagedMLAIndexCacheFP8, cu_seqlens_q: Tensor, topk: int, *,
                                   causal: bool = True, seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None,
                                   return_logits: bool = False, return_q8: bool = False):
    """The lightning indexer on packed queries: returns indices int32 [total_q, topk].

    q_idx         [total_q, Hi <= 64, 128] in icache.dtype (a view with dense channels and 16-byte-aligned rows is read through its
                  strides); quantised in the kernel per (token, head) row as in `fp8_mla_index_topk_func`.
    weights       fp32 [total_q, Hi], heads dense.
    cu_seqlens_q  int32 [B + 1] on the device, B = icache.batch_size, cu[0] = 0, non-decreasing: slot b owns the rows cu[b] .. cu[b+1] - 1
                  (n_b of them, 0 allowed: an idle slot).  Rows at or behind cu[B] -- a padded token bucket -- are not read: their indices
                  are all -1, their logits -inf, their q8 / scale_q 0.
    topk          as `fp8_mla_index_topk_func`: the positions of the min(topk, kend) largest logits among j < kend in ASCENDING order, then
                  -1; ties to the lower position.  Token i of slot b has kend = L_b (causal=False) or max(L_b - n_b + i + 1, 0)
                  (causal=True: bottom-right -- the slot's last token sees all L_b keys, so append the chunk's own keys first),
                  L_b = clamp(seqused_k[b], 0, max_seqlen_k).
    seqused_k     int32 [B] on the device, default icache.seqlens.  max_seqlen_k: a host int, default the capacity; pass the longest L_b.
    return_logits appends logits fp32 [total_q, max_seqlen_k], -inf at j >= kend; return_q8 appends (q8 [total_q, Hi, 128] e4m3, scale_q
                  [total_q, Hi]).
    One score launch and ceil(total_q / 65535) selection launches, their number a function of the shapes alone; cu_seqlens_q, table, lengths,
    weights and q are read on the device: no host synchronisation, graph-capture safe.  Logits, indices, q8 and scale_q of a slot equal
    `fp8_mla_index_topk_func` on that slot's tokens bit for bit.
    CPU tensors and config.attention.force_eager_fallback run the eager definition (`_varlen_eager`); on the device there is no fallback.
    Unsupported input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = mla_index_varlen_input_reason(q_idx, weights, icache, cu_seqlens_q, topk, seqused_k=seqused_k, max_seqlen_k=max_seqlen_k)
        if reason:
            raise ValueError(reason)
    Skv = icache.capacity if max_seqlen_k is None else int(max_seqlen_k)
    used = icache.seqlens if seqused_k is None else seqused_k
    if _mla._eager(q_idx):
        indices, logits, q8, sq = _varlen_eager(q_idx, weights, icache, cu_seqlens_q, bool(causal), used, Skv, int(topk))
    else:
        ok, why = nn._pre_check_can_use_hip_attention(device=q_idx.device)
        if not ok:
            raise ValueError(why)
        indices, logits, q8, sq = nn._ops().fp8_mla_index_topk_varlen_forward(
            q_idx, weights, icache.pool, icache.scale, icache.block_table, cu_seqlens_q, used, Skv, int(topk), icache.num_pages,
            icache.page_size, icache.fp8_format, bool(causal), bool(return_logits), bool(return_q8))
    res: Tuple = (indices,)
    if return_logits:
        res += (logits,)
    if return_q8:
        res += (q8, sq)
    return res if len(res) > 1 else indices

"""The FP8 LIGHTNING INDEXER of sparse multi-head latent attention (DeepSeek-V3.2-style layers; include/qattn_mla_index.h, DESIGN.md section
4.32): the paged FP8 index-key cache, its append, and `fp8_mla_index_topk_func`, which scores every cached key of a slot against the index
query of a token and returns the `indices` that `fp8_mla_paged_sparse_func` (mla.py) attends.

    icache = alloc_paged_mla_index_cache_fp8(num_pages, page_size, batch_size=B, max_pages_per_seq=M, scale=0.05, dtype=torch.bfloat16,
                                             device="cuda", block_table=row_cache.block_table, seqlens=row_cache.seqlens)   # ONE table, ONE length vector
    for step in ...:
        paged_mla_index_cache_append_fp8(icache, k_idx, advance=False)                     # k_idx [B, T, 128]: after the model's LayerNorm and RoPE
        paged_mla_row_cache_append_fp8(row_cache, ckv, kpe)                                # advances the shared lengths
        indices = fp8_mla_index_topk_func(q_idx, weights, icache, 2048)                    # q_idx [B, Hi, Sq, 128], weights fp32 [B, Sq, Hi]
        out = fp8_mla_paged_sparse_func(q, row_cache, indices, scale=model_softmax_scale)

    logit[b, i, j] = scale_k[b] sum_h w[b, i, h] scale_q[b, h, i] ReLU(sum_c q8[b, h, i, c] k8[b, j, c])          (no softmax)
    indices[b, i]  = the positions of the min(topk, kend) largest logits among j < kend(b, i), ASCENDING, then -1; ties to the lower position

The selection of a row runs on one workgroup or, for few rows over many keys, cut across up to 256 workgroups (include/qattn_mla_index_split.h,
DESIGN.md section 4.33): `select_splits=` / `num_splits=`, 0 = `qattn_mla_index_select_auto_splits` on the device's CU count, resolved on
the host by `_native.mla_index_resolve_splits` (1 unless the row has 16 384 keys or more and B Sq is at most an eighth of the CU count; the
ops and the library take the resolved count, 1 .. 256).  The indices are the same bit for bit for every value.

Package attributes, not names of `__all__`.  Not offered: per-key cache scales (DeepSeek's own 132-byte index row); RoPE or the LayerNorm of
the index key; the first selection histogram fused into the score sweep.  (Packed variable-length q -- a prompt -- is
`fp8_mla_index_topk_varlen_func`, mla_index_prefill.py.)"""
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native, mla as _mla, nn
from .kvcache import _is_int
from .paged import _lens_reason
from .utils import checks

D, MAX_HEADS, MAX_TOPK = _native.MLA_INDEX_D, _native.MLA_INDEX_MAX_HEADS, _native.MLA_SPARSE_MAX_TOPK
WG_KEYS, LDS_CANDIDATES = _native.MLA_INDEX_WG_KEYS, _native.MLA_INDEX_LDS_CANDIDATES
MAX_SELECT_SPLITS = _native.MLA_INDEX_MAX_SELECT_SPLITS


class PagedMLAIndexCacheFP8(_mla.PagedMLACacheFP8):
    """`PagedMLACacheFP8`'s fields with pool fp8 [num_pages, page_size, 128], row-major on every device: ONE index key per position, shared by
    all index heads; layout = "index"."""
    __slots__ = ()


def alloc_paged_mla_index_cache_fp8(num_pages: int, page_size: int, *, batch_size: int, max_pages_per_seq: int, scale, dtype, device,
                                    fp8_format: Optional[str] = None, block_table: Optional[Tensor] = None,
                                    seqlens: Optional[Tensor] = None) -> PagedMLAIndexCacheFP8:
    """An empty paged index-key cache: a zero-filled fp8 pool [num_pages, page_size, 128] (page_size any integer >= 1), ONE fixed fp32 scale
    per slot (a float or a tensor [batch_size]; the selection does not depend on it), a zero-filled block table int32 [batch_size,
    max_pages_per_seq] and seqlens = 0, on any device.  block_table= / seqlens= make the cache ALIAS the given tensors instead -- a row-major
    latent cache and its index cache then share one table and one length vector, and the caller appends one of the two with advance=False."""
    reason = _mla._alloc_reason(num_pages, 64, batch_size, max_pages_per_seq, scale, dtype)
    if not reason and not (_is_int(page_size) and page_size >= 1):
        reason = f"page_size must be a positive integer, got {page_size!r}"
    if not reason and (num_pages * page_size > 2 ** 31 - 1 or max_pages_per_seq * page_size > 2 ** 31 - 65):
        reason = "num_pages * page_size and max_pages_per_seq * page_size must stay below 2^31"
    device = torch.device(device)
    if not reason and block_table is not None and not (isinstance(block_table, Tensor) and block_table.dtype == torch.int32
                                                       and tuple(block_table.shape) == (batch_size, max_pages_per_seq)
                                                       and block_table.stride(1) == 1 and block_table.device.type == device.type):
        reason = f"Expected block_table to be a torch.int32 tensor [{batch_size}, {max_pages_per_seq}] with dense rows on {device}"
    if not reason and seqlens is not None:
        reason = _lens_reason("seqlens", seqlens, batch_size, seqlens.device if isinstance(seqlens, Tensor) and seqlens.device.type == device.type else device)
    if reason:
        raise ValueError(reason)
    fp8_format = checks.config_value("attention.fp8_format") if fp8_format is None else fp8_format
    fp8_dtype = _native.fp8_dtype_of(fp8_format)
    if block_table is not None:
        device = block_table.device
    if device.type == "cuda" and not checks.config_value("attention.force_eager_fallback"):
        ok, why = nn._pre_check_can_use_hip_attention(device=device)
        if not ok:
            raise ValueError(why)
    sc = (torch.as_tensor(scale, dtype=torch.float32, device=device) if isinstance(scale, Tensor)
          else torch.full((), float(scale), dtype=torch.float32, device=device)).expand(batch_size).contiguous()
    table = torch.zeros((batch_size, max_pages_per_seq), dtype=torch.int32, device=device) if block_table is None else block_table
    lens = torch.zeros((batch_size,), dtype=torch.int32, device=device) if seqlens is None else seqlens
    pool = torch.zeros((num_pages, page_size, D), dtype=torch.uint8, device=device).view(fp8_dtype)
    return PagedMLAIndexCacheFP8(pool, sc, table, lens, num_pages, page_size, fp8_format, dtype, "index")


def select_splits_reason(name: str, value, B: int, Sq: int) -> Optional[str]:
    """The rule a `num_splits` / `select_splits` value breaks, or None: an integer, 0 (the auto rule) .. MAX_SELECT_SPLITS; more than one
    split needs B, Sq <= 65535 (grid axes)."""
    if not (_is_int(value) and 0 <= value <= MAX_SELECT_SPLITS):
        return f"{name} must be an integer in 0 .. {MAX_SELECT_SPLITS} (0: chosen from the shape), got {value!r}"
    if value > 1 and (B > 65535 or Sq > 65535):
        return f"{name} > 1 needs B, Sq <= 65535, got B {B}, Sq {Sq}"
    return None


def mla_index_input_reason(q, weights, icache, topk=None, *, seqused_k=None, max_seqlen_k=None, k_new=None, new_lens=None,
                           select_splits=0) -> Optional[str]:
    """The first rule the arguments of `fp8_mla_index_topk_func` (q, weights, topk given) or `paged_mla_index_cache_append_fp8` (q None; k_new
    given) break, or None.  Shapes, dtypes, devices and strides only: the CONTENTS of block_table / seqlens are read on the device."""
    if not isinstance(icache, PagedMLAIndexCacheFP8):
        return "Expected icache to be a PagedMLAIndexCacheFP8 (alloc_paged_mla_index_cache_fp8)"
    reason = _mla._cache_reason(icache, row=True)
    if reason:
        return reason
    p, B = icache.pool, icache.batch_size
    if not isinstance(p, Tensor) or tuple(p.shape) != (icache.num_pages, icache.page_size, D) or not p.is_contiguous():
        return f"Expected icache.pool to be a dense fp8 tensor [num_pages, page_size, {D}]"
    if q is None:
        t = k_new
        if not isinstance(t, Tensor) or t.dim() != 3 or t.shape[0] != B or t.shape[1] == 0 or t.shape[2] != D:
            return f"Expected k_new to be a tensor [{B}, T >= 1, {D}], but got {list(getattr(t, 'shape', ()))}"
        if t.dtype != icache.dtype or t.requires_grad:
            return f"Expected k_new to be a leaf tensor of the cache's dtype {icache.dtype}, but got {t.dtype}"
        if t.device != icache.device:
            return f"Expected k_new to be on the cache's device {icache.device}, but got {t.device} instead."
        if not _native.mla_rows_addressable(t):
            return f"Expected k_new to have dense channels and 16-byte-aligned rows, but got strides {tuple(t.stride())}; pass k_new.contiguous()"
        reason = _lens_reason("icache.seqlens", icache.seqlens, B, icache.device)
        return reason if reason or new_lens is None else _lens_reason("new_lens", new_lens, B, icache.device)
    if not isinstance(q, Tensor) or q.dim() != 4:
        return "NYI: the index query must be a 4-D tensor [B, Hi, Sq, 128]"
    if q.requires_grad:
        return "NYI: the index query must be a leaf tensor (no backward)"
    if q.dtype not in (torch.float16, torch.bfloat16) or q.dtype != icache.dtype:
        return f"Expected the index query to have the cache's dtype {icache.dtype} (torch.float16 or torch.bfloat16), but got {q.dtype} instead."
    if q.shape[-1] != D:
        return f"Expected the index query's head dimension to be {D}, but got {q.shape[-1]}."
    if q.shape[0] != B or not 1 <= q.shape[1] <= MAX_HEADS or not 1 <= q.shape[2] <= 65535:
        return f"Expected the index query to have shape [{B}, 1 <= Hi <= {MAX_HEADS}, Sq >= 1, {D}], but got {list(q.shape)}."
    if q.device != icache.device:
        return f"Expected the index query and the cache to be on the same device, but got {q.device} and {icache.device} instead."
    if not _native.mla_rows_addressable(q):
        return f"Expected the index query to have dense channels and 16-byte-aligned rows, but got strides {tuple(q.stride())}; pass q.contiguous()"
    Hi, Sq = q.shape[1], q.shape[2]
    if not isinstance(weights, Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != (B, Sq, Hi) or weights.requires_grad:
        return f"Expected weights to be a torch.float32 leaf tensor [{B}, {Sq}, {Hi}], but got {getattr(weights, 'dtype', None)} {list(getattr(weights, 'shape', ()))}"
    if weights.device != q.device:
        return f"Expected weights to be on the query's device {q.device}, but got {weights.device} instead."
    if (Hi > 1 and weights.stride(2) != 1) or any(weights.shape[i] > 1 and weights.stride(i) < 0 for i in (0, 1)):
        return f"Expected weights to have dense heads, but got strides {tuple(weights.stride())}; pass weights.contiguous()"
    if not (_is_int(topk) and 1 <= topk <= MAX_TOPK):
        return f"topk must be an integer in 1 .. {MAX_TOPK}, got {topk!r}"
    if max_seqlen_k is not None and not (_is_int(max_seqlen_k) and 1 <= max_seqlen_k <= min(icache.capacity, 2 ** 30)):
        return f"max_seqlen_k must be None or an integer in 1 .. max_pages_per_seq * page_size = {icache.capacity} (at most 2^30), got {max_seqlen_k!r}"
    if max_seqlen_k is None and icache.capacity > 2 ** 30:
        return "max_seqlen_k is required for a capacity above 2^30 keys"
    reason = select_splits_reason("select_splits", select_splits, B, Sq)
    if reason:
        return reason
    return _lens_reason("seqused_k" if seqused_k is not None else "icache.seqlens", icache.seqlens if seqused_k is None else seqused_k, B, q.device)


# ---- the eager definitions (CPU tensors, config.attention.force_eager_fallback): the specification -------------------------------------------
def _kends(used: Tensor, N: int, Sq: int, causal: bool):
    """kend(b, i) as nested lists.  (Reads the lengths on the host.)"""
    lens = [min(max(int(x), 0), N) for x in used.tolist()]
    return [[max(L - Sq + i + 1, 0) if causal else L for i in range(Sq)] for L in lens]


def _scores_eager(q, weights, icache, causal, used, Skv) -> Tuple[Tensor, Tensor, Tensor]:
    """de-quantise nothing: the fp32 products of the e4m3 q8 and the cache bytes, ReLU, the head sum with w scale_q, the slot's scale; -inf at
    j >= kend.  Returns (logits [B, Sq, Skv], q8, scale_q)."""
    B, Hi, Sq, _ = q.shape
    q8, scale_q = _mla.quantize_q_eager(q)
    idx = icache.block_table.clamp(0, icache.num_pages - 1).long()
    k = icache.pool[idx].reshape(B, -1, D)[:, :Skv].float()                                   # [B, Skv, 128]
    s = torch.relu(torch.einsum("bhic,bjc->bihj", q8.float(), k))                             # [B, Sq, Hi, Skv]
    logits = (s * (weights * scale_q.transpose(1, 2))[..., None]).sum(dim=2) * icache.scale[:, None, None]
    kend = torch.tensor(_kends(used, Skv, Sq, causal), device=q.device)
    return torch.where(torch.arange(Skv, device=q.device)[None, None, :] < kend[..., None], logits, torch.full_like(logits, -torch.inf)), q8, scale_q


def _select_eager(logits: Tensor, used: Tensor, topk: int, causal: bool) -> Tensor:
    """the selection rule: a stable descending sort of the canonical row (NaN -> -inf, -0.0 -> +0.0) below kend, its first topk positions in
    ascending order, then -1"""
    B, Sq, N = logits.shape
    out = torch.full((B, Sq, topk), -1, dtype=torch.int32, device=logits.device)
    for b, row_ends in enumerate(_kends(used, N, Sq, causal)):
        for i, kend in enumerate(row_ends):
            row = torch.nan_to_num(logits[b, i, :kend].float(), nan=-torch.inf, posinf=torch.inf, neginf=-torch.inf) + 0.0
            order = torch.sort(row, descending=True, stable=True).indices[:topk]
            out[b, i, : order.numel()] = torch.sort(order).values.to(torch.int32)
    return out


# ---- the calls -----------------------------------------------------------------------------------------------------------------------------------
def paged_mla_index_cache_append_fp8(icache: PagedMLAIndexCacheFP8, k_new: Tensor, *, new_lens: Optional[Tensor] = None,
                                     advance: bool = True) -> PagedMLAIndexCacheFP8:
    """Append T index keys per slot to the paged index-key `icache`, in place; returns `icache`.  k_new [B, T, 128] in icache.dtype, a view
    with dense channels and 16-byte-aligned rows is read through its strides.  The contract of `paged_mla_row_cache_append_fp8` word for
    word: the same quantiser with the slot's scale, n_b = T or clamp(new_lens[b], 0, T), tokens at or beyond the capacity dropped, every
    table entry clamped, exactly the bytes of the appended keys change, seqlens advances unless advance=False (a cache that aliases a latent
    cache's seqlens appends one of the two with advance=False), everything read on the device: graph-capture safe.  CPU tensors and
    config.attention.force_eager_fallback run the eager definition; on the device there is no fallback.  Invalid input raises
    ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = mla_index_input_reason(None, None, icache, k_new=k_new, new_lens=new_lens)
        if reason:
            raise ValueError(reason)
    if _mla._eager(k_new):
        _mla._append_eager(icache, k_new, k_new[..., :0], new_lens, bool(advance))   # (the latent caches' definition on 128-channel rows)
        return icache
    ok, why = nn._pre_check_can_use_hip_attention(device=k_new.device)
    if not ok:
        raise ValueError(why)
    if torch.compiler.is_compiling():
        nn._ops().fp8_paged_mla_index_cache_append_(icache.pool, icache.scale, icache.block_table, icache.seqlens, k_new, new_lens,
                                                    icache.num_pages, icache.page_size, icache.fp8_format, bool(advance))
    else:
        _native.paged_mla_index_cache_append_fp8(icache.pool, icache.scale, icache.block_table, icache.seqlens, k_new,
                                                 num_pages=icache.num_pages, page_size=icache.page_size,
                                                 fp8_dtype=_native.fp8_dtype_of(icache.fp8_format), new_lens=new_lens, advance=bool(advance))
    return icache


def fp8_mla_index_topk_func(q_idx: Tensor, weights: Tensor, icache: PagedMLAIndexCacheFP8, topk: int, *, causal: bool = True,
                            seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, return_logits: bool = False,
                            return_q8: bool = False, select_splits: int = 0):
    """The lightning indexer: returns indices int32 [B, Sq, topk] for `fp8_mla_paged_sparse_func`.

    q_idx         [B, Hi <= 64, Sq, 128] in icache.dtype (a view with dense channels and 16-byte-aligned rows is read through its strides);
                  quantised in the kernel per (token, head) row to e4m3 with scale_q = amax / 448, as the MLA kernels' q.
    weights       fp32 [B, Sq, Hi]: the head weights, with the model's d^-1/2 and Hi^-1/2 folded in by the caller.
    topk          1 .. 131 072.  indices[b, i] holds the positions of the min(topk, kend) largest logits among j < kend(b, i) in ASCENDING
                  position order, then -1; a larger logit wins, equal logits are won by the lower position (-0.0 equals +0.0), a NaN logit
                  ranks as -inf.  kend = L_b (causal=False) or L_b - Sq + i + 1 (causal=True: bottom-right, the sparse call's rule),
                  L_b = clamp(seqused_k[b], 0, max_seqlen_k).  Keys at or behind kend and never-written pages influence nothing.
    seqused_k     int32 [B] on the device, default icache.seqlens.
    max_seqlen_k  a host int: bounds the grid and the logits row; default the capacity.  Pass the longest live sequence.
    return_logits appends logits fp32 [B, Sq, max_seqlen_k], -inf at j >= kend; return_q8 appends (q8 [B, Hi, Sq, 128] e4m3, scale_q
                  [B, Hi, Sq]).
    select_splits 0: `qattn_mla_index_select_auto_splits` on the device's CU count; 1: one workgroup selects a row; 2 .. 256: the row is cut
                  across that many workgroups (include/qattn_mla_index_split.h).  The indices are the same bit for bit.
    The scores launch and the selection (one launch, or six with a split row), their number a function of the shapes alone; table, lengths,
    weights and q are read on the device: no host synchronisation, graph-capture safe.
    CPU tensors and config.attention.force_eager_fallback run the eager definitions (`_scores_eager`, `_select_eager`); on the device there
    is no fallback.  Unsupported input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = mla_index_input_reason(q_idx, weights, icache, topk, seqused_k=seqused_k, max_seqlen_k=max_seqlen_k, select_splits=select_splits)
        if reason:
            raise ValueError(reason)
    Skv = icache.capacity if max_seqlen_k is None else int(max_seqlen_k)
    used = icache.seqlens if seqused_k is None else seqused_k
    if _mla._eager(q_idx):
        logits, q8, sq = _scores_eager(q_idx, weights, icache, bool(causal), used, Skv)
        indices = _select_eager(logits, used, int(topk), bool(causal))
    else:
        ok, why = nn._pre_check_can_use_hip_attention(device=q_idx.device)
        if not ok:
            raise ValueError(why)
        ns = _native.mla_index_resolve_splits(int(select_splits), q_idx.shape[0] * q_idx.shape[2], Skv, int(topk), q_idx.device)
        if ns == 1:
            indices, logits, q8, sq = nn._ops().fp8_mla_index_topk_forward(
                q_idx, weights, icache.pool, icache.scale, icache.block_table, used, Skv, int(topk), icache.num_pages, icache.page_size,
                icache.fp8_format, bool(causal), bool(return_logits), bool(return_q8))
        else:
            indices, logits, q8, sq = nn._ops().fp8_mla_index_topk_split_forward(
                q_idx, weights, icache.pool, icache.scale, icache.block_table, used, Skv, int(topk), icache.num_pages, icache.page_size, ns,
                icache.fp8_format, bool(causal), bool(return_logits), bool(return_q8))
    res: Tuple = (indices,)
    if return_logits:
        res += (logits,)
    if return_q8:
        res += (q8, sq)
    return res if len(res) > 1 else indices


def mla_index_select(logits: Tensor, topk: int, *, seqused_k: Tensor, causal: bool = True, num_splits: int = 0) -> Tensor:
    """The selection of `fp8_mla_index_topk_func` alone, on the caller's logits fp32 [B, Sq, N] (last dimension dense): indices int32
    [B, Sq, topk] by the same rule, with L_b = clamp(seqused_k[b], 0, N).  num_splits: `select_splits` of that call -- one launch for 1,
    six for a split row; the same indices bit for bit.  Graph-capture safe; CPU tensors and config.attention.force_eager_fallback run
    `_select_eager` (num_splits is validated and ignored)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = None
        if not isinstance(logits, Tensor) or logits.dtype != torch.float32 or logits.dim() != 3 or logits.numel() == 0 or logits.requires_grad:
            reason = f"Expected logits to be a torch.float32 leaf tensor [B, Sq, N >= 1], but got {getattr(logits, 'dtype', None)} {list(getattr(logits, 'shape', ()))}"
        elif logits.shape[2] > 2 ** 30 or (logits.shape[2] > 1 and logits.stride(2) != 1) or any(logits.shape[i] > 1 and logits.stride(i) < 0 for i in (0, 1)):
            reason = f"Expected logits to have a dense last dimension of at most 2^30 elements, but got strides {tuple(logits.stride())}"
        elif not (_is_int(topk) and 1 <= topk <= MAX_TOPK):
            reason = f"topk must be an integer in 1 .. {MAX_TOPK}, got {topk!r}"
        else:
            reason = _lens_reason("seqused_k", seqused_k, logits.shape[0], logits.device) or select_splits_reason("num_splits", num_splits, *logits.shape[:2])
        if reason:
            raise ValueError(reason)
    if _mla._eager(logits):
        return _select_eager(logits, seqused_k, int(topk), bool(causal))
    ok, why = nn._pre_check_can_use_hip_attention(device=logits.device)
    if not ok:
        raise ValueError(why)
    ns = _native.mla_index_resolve_splits(int(num_splits), logits.shape[0] * logits.shape[1], logits.shape[2], int(topk), logits.device)
    if ns == 1:
        return nn._ops().mla_index_select_forward(logits, seqused_k, int(topk), bool(causal))
    return nn._ops().mla_index_select_split_forward(logits, seqused_k, int(topk), ns, bool(causal))

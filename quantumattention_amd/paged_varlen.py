"""PACKED variable-length queries over the paged FP8 K/V cache: `fp8_attn_paged_varlen_func` (include/qattn_paged_varlen.h, DESIGN.md
section 4.20) -- one call for a serving step that mixes chunked prefill, decode and idle slots.

`fp8_attn_paged_func` takes q [B, Hq, Sq, D]: every sequence slot has Sq queries.  A continuous-batching step does not: a few slots are
in chunked prefill with hundreds of queries, many decode one token (or a few speculative ones), some are idle.  Here q is
[total_q, Hq, D], slot b owns the tokens cu_seqlens_q[b] .. cu_seqlens_q[b + 1] -- the call shape of flash-attn's / vLLM's
`flash_attn_varlen_func(q, ..., cu_seqlens_q, max_seqlen_q, seqused_k, block_table, causal=True)`.

    cu = torch.tensor([0, 512, 513, 513, 514], dtype=torch.int32, device="cuda")     # a prefill chunk, a decode, an idle slot, a decode
    out = fp8_attn_paged_varlen_func(q, cache, cu, 512, causal=True, max_seqlen_k=longest_live_sequence)   # [total_q, Hq, D]

The rule: for every slot with queries, the rows of every output are, bit for bit, those of `fp8_attn_paged_func` on that slot alone.

The append half of the same step, on the same packed tensor and the same cu_seqlens: `paged_kv_cache_append_varlen_fp8`
(include/qattn_paged_varlen_append.h) -- the K and V slices of the QKV projection go into the cache as they are,
no padding to the longest chunk, no new_lens beside cu_seqlens.

    qkv = proj(x).view(total, Hq + 2 * Hkv, D)
    paged_kv_cache_append_varlen_fp8(cache, qkv[:, Hq:Hq + Hkv], qkv[:, Hq + Hkv:], cu)
    out = fp8_attn_paged_varlen_func(qkv[:, :Hq], cache, cu, max_seqlen_q, causal=True, max_seqlen_k=longest_live_sequence)

With the rotary embedding (include/qattn_paged_varlen_rope.h): `paged_kv_cache_append_varlen_rope_fp8` rotates K
inside the append -- key p_b + t of slot b with row p_b + t of one cos / sin table pair, a key's index in its sequence being its position
-- and `apply_rope_paged_varlen` rotates q at the positions of the keys the same tokens become.  No positions tensor, no rotated K in
memory:

    q = apply_rope_paged_varlen(qkv[:, :Hq], cache, cu, cos, sin)                      # before the append: the default appended=False
    paged_kv_cache_append_varlen_rope_fp8(cache, qkv[:, Hq:Hq + Hkv], qkv[:, Hq + Hkv:], cu, cos, sin)
    out = fp8_attn_paged_varlen_func(q, cache, cu, max_seqlen_q, causal=True, max_seqlen_k=longest_live_sequence)

At the CALLER's positions instead (include/qattn_paged_varlen_rope_pos.h; vLLM's `positions`, and the base + depth
of a draft tree's tokens, `tree.tree_positions`): `paged_kv_cache_append_varlen_rope_pos_fp8` and `apply_rope_positions`.

Package attributes, not names of `__all__`.  Not offered: RoPE fused into the attention's q pre-pass, per-slot position offsets, a partial
rotary_dim, multi-axis (M-RoPE) positions, scaled / YaRN tables beyond what the caller puts into cos / sin, RoPE in the padded and the
contiguous appends, a per-token slot_mapping form, a per-call table whose batch differs from the cache's slots, the contiguous
`KVCacheFP8`, page allocation.  Sliding windows: splitkv_window.fp8_attn_paged_varlen_window_func."""
import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native, nn
from .kvcache import _is_int
from .paged import PagedKVCacheFP8, _append_eager, _cache_reason, _lens_reason, gather_paged_eager
from .rope import _TABLE_DTYPES, apply_rope_eager
from .splitkv import _CPU_NUM_CUS, MAX_SPLITS, PreparedKV, _splitkv_eager_depth
from .utils import checks


def _q_rows_addressable(q: Tensor) -> bool:
    """head_dim innermost and dense, token and head strides of a dimension longer than 1 non-negative multiples of 8 elements, the first
    element 16-byte aligned in its storage: the rows the pre-pass loads 16 bytes at a time"""
    # (while Dynamo traces, the storage offset is not to be had: the op's binding checks the real pointer)
    aligned = torch.compiler.is_dynamo_compiling() or q.storage_offset() % 8 == 0
    return ((q.shape[2] == 1 or q.stride(2) == 1) and aligned
            and all(q.shape[i] == 1 or (q.stride(i) >= 0 and q.stride(i) % 8 == 0) for i in (0, 1)))


def paged_varlen_attn_input_reason(q, cache, cu_seqlens_q, max_seqlen_q, seqused_k=None, scale=None, num_splits=0,
                                   max_seqlen_k=None) -> Optional[str]:
    """The first rule the arguments of `fp8_attn_paged_varlen_func` break, or None.  Shapes, dtypes, devices and strides only: the CONTENTS
    of cu_seqlens_q, seqused_k and the block table are read on the device."""
    if not isinstance(q, Tensor) or q.dim() != 3:
        return "NYI: query must be a 3-D tensor [total_q, Hq, head_dim]"
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
    if q.shape[1] == 0:
        return "Expected a non-empty head count"
    if q.shape[1] % Hkv != 0:
        return f"Expect the number of query heads to be a multiple of the key/value heads but got Hq={q.shape[1]} and Hkv={Hkv}."
    if (q.shape[1] // Hkv) * q.shape[0] > 2 ** 31 - 1:
        return f"(Hq / Hkv) * total_q must stay below 2^31 (the packed row index), got {(q.shape[1] // Hkv) * q.shape[0]}"
    if q.device != cache.device:
        return f"Expected query and the cache to be on the same device, but got {q.device} and {cache.device} instead."
    if q.shape[0] > 0 and not _q_rows_addressable(q):
        return (f"Expected query to have head_dim innermost and 16-byte-aligned rows (strides that are multiples of 8 elements), but got "
                f"strides {tuple(q.stride())} at storage offset {q.storage_offset()}; pass query.contiguous()")
    if not isinstance(cu_seqlens_q, Tensor) or cu_seqlens_q.dtype != torch.int32:
        return f"Expected cu_seqlens_q to be a torch.int32 tensor, but got {getattr(cu_seqlens_q, 'dtype', type(cu_seqlens_q))}"
    if tuple(cu_seqlens_q.shape) != (B + 1,):
        return f"Expected cu_seqlens_q to have shape [{B + 1}] (the cache's slots + 1), but got {list(cu_seqlens_q.shape)}."
    if cu_seqlens_q.device != q.device:
        return f"Expected cu_seqlens_q to be on {q.device}, but got {cu_seqlens_q.device} instead."
    if not cu_seqlens_q.is_contiguous():
        return "Expected cu_seqlens_q to be contiguous"
    if not (_is_int(max_seqlen_q) and max_seqlen_q >= 1):
        return f"max_seqlen_q must be an integer >= 1 (the most queries of a sequence), got {max_seqlen_q!r}"
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


@torch.compiler.assume_constant_result
def _resolve_varlen_splits(num_splits: int, B: int, Hq: int, Hkv: int, total_q: int, max_seqlen_q: int, Skv: int, D: int, device) -> int:
    """num_splits = 0 -> qattn_paged_varlen_auto_splits on the device's CU count: a pure function of host ints (it reads neither
    cu_seqlens_q nor seqused_k), so a trace-time constant."""
    if num_splits:
        return num_splits
    cus = torch.cuda.get_device_properties(device).multi_processor_count if torch.device(device).type == "cuda" else _CPU_NUM_CUS
    return _native.paged_varlen_auto_splits(B, Hq, Hkv, total_q, max_seqlen_q, Skv, D, cus)


def _attend_varlen_eager(q, cache, cu_seqlens_q, causal, scale, seqused_k, Skv, ns, precision, tree_mask=None, softcap=None, sinks=None,
                         window=None):
    """CPU tensors and config.attention.force_eager_fallback: per sequence slot, splitkv._splitkv_eager on the slot's queries and on its
    keys gathered through the table, scattered into the packed outputs.  Rows of tokens that belong to no sequence: zeros.  (This path
    reads cu_seqlens_q, seqused_k and the table on the host.)
    tree_mask = int64 [total_q] (None: none; with causal): the draft tree of include/qattn_paged_varlen_tree.h -- in a slot with at most 64
    queries position p keeps key j >= max(delta, 0), delta = L_b - Sq_b, only if bit j - delta of the token's word is set.
    tree_mask with window = (left, 0) (and, optionally, sinks): the definition of include/qattn_paged_varlen_tree_window.h -- in such a
    slot the window's lower edge is taken from the token's DEPTH (the set bits of its word below its own index) and cuts committed keys
    only; a slot with more than 64 queries is the window rule.
    softcap = a float > 0 (None: none; with window): the scaled scores capped before the mask, as splitkv._splitkv_eager defines it."""
    total_q, Hq, D = q.shape
    B = cache.batch_size
    n = ns if ns > 1 else 0
    out = torch.zeros((total_q, Hq, D), dtype=q.dtype, device=q.device)
    lse = torch.zeros((Hq, total_q), dtype=torch.float32, device=q.device)
    po = torch.zeros((n, total_q, Hq, D), dtype=torch.float32, device=q.device) if n else torch.empty((0,), dtype=torch.float32, device=q.device)
    plse = torch.zeros((n, Hq, total_q), dtype=torch.float32, device=q.device) if n else torch.empty((0,), dtype=torch.float32, device=q.device)
    ppath = torch.zeros((n, Hq, total_q), dtype=torch.uint8, device=q.device) if n else torch.empty((0,), dtype=torch.uint8, device=q.device)
    if total_q == 0:
        return out, lse, po, plse, ppath
    kv = gather_paged_eager(cache, Skv)
    cu = cu_seqlens_q.tolist()
    for b in range(B):
        start = min(max(int(cu[b]), 0), total_q)
        end = min(max(int(cu[b + 1]), start), total_q)
        if end == start:
            continue
        one = PreparedKV(kv.k[b:b + 1], kv.v[b:b + 1], kv.scale_k[b:b + 1], kv.scale_v[b:b + 1], (1,) + tuple(kv.shape[1:]), kv.fp8_format,
                         kv.dtype, kv.numerics, "rowmajor")
        also = depth = None
        if tree_mask is not None and end - start <= 64:
            if window is not None:   # depth_p = popcount(w_p & (2^p - 1)): the set bits below p (an arithmetic shift: the low bits are the word's)
                p = torch.arange(end - start, device=q.device)
                below = ((tree_mask[start:end, None] >> torch.arange(64, device=q.device)) & 1).bool() & (torch.arange(64, device=q.device) < p[:, None])
                depth = [below.sum(1)]
            delta = min(max(int(seqused_k[b]), 0), Skv) - (end - start)
            bits = ((tree_mask[start:end, None] >> torch.arange(64, device=q.device)) & 1).bool()           # [Sq_b, 64]: bit i of word p
            j0, j1 = max(delta, 0), max(min(delta + 64, Skv), 0)
            also = torch.ones((1, end - start, Skv), dtype=torch.bool, device=q.device)
            if j1 > j0:
                also[0, :, j0:j1] = bits[:, j0 - delta:j1 - delta]
        o, l, p_o, p_l, p_p = _splitkv_eager_depth(q[start:end].transpose(0, 1)[None], one, causal, scale, seqused_k[b:b + 1], ns, precision,
                                                   also, sinks, window, depth, softcap=softcap)
        out[start:end] = o[0].transpose(0, 1)
        lse[:, start:end] = l[0]
        if n:
            po[:, start:end] = p_o[:, 0].transpose(1, 2)
            plse[:, :, start:end] = p_l[:, 0]
            ppath[:, :, start:end] = p_p[:, 0]
    return out, lse, po, plse, ppath


def fp8_attn_paged_varlen_func(q, cache: PagedKVCacheFP8, cu_seqlens_q: Tensor, max_seqlen_q: int, *, causal: bool = False,
                               scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None,
                               num_splits: int = 0, precision: str = "accurate", return_lse: bool = False, return_partials: bool = False):
    """`fp8_attn_paged_func` for PACKED queries, a different count per sequence slot.

    q [total_q, Hq, D] in cache.dtype; a view with D innermost and 16-byte-aligned rows (a slice of a packed QKV projection) goes in as it
    is.  cu_seqlens_q: int32 [cache.batch_size + 1] on the device; slot b owns the tokens clamp(cu[b], 0, total_q) .. clamp(cu[b + 1],
    that, total_q), Sq_b of them (0: an idle slot), and attends the first L_b = clamp(seqused_k[b], 0, Skv) keys of slot b.  causal:
    bottom-right per sequence -- position p attends the keys j <= p + L_b - Sq_b.  max_seqlen_q: a host int >= 1, the most queries of a
    slot: read by the num_splits = 0 rule only.  seqused_k (default cache.seqlens), max_seqlen_k, scale, num_splits, precision: as
    `fp8_attn_paged_func`.

    Returns out [total_q, Hq, D]; with return_lse, lse fp32 [Hq, total_q] (flash-attn's packed layout); with return_partials, partial_o fp32
    [ns, total_q, Hq, D], partial_lse [ns, Hq, total_q] and partial_path uint8 [ns, Hq, total_q] (three empty tensors with one split).
    For every slot with Sq_b > 0 these rows are, bit for bit, `fp8_attn_paged_func` on that slot alone (q[cu[b]:cu[b+1]] as
    [1, Hq, Sq_b, D], a one-slot cache on the same pools) with the same max_seqlen_k and num_splits > 0.  Rows of tokens that belong to
    no slot (cu[B] < total_q: a padded token bucket) have unspecified contents.  total_q = 0 returns empty tensors.
    Everything is read on the device: no host synchronisation, graph-capture safe, and a captured call follows the later contents of
    cu_seqlens_q, seqused_k and the table.  CPU tensors and config.attention.force_eager_fallback run the eager definition
    (`_attend_varlen_eager`); on the device there is no fallback.  Unsupported input raises ValueError(reason)."""
    if precision not in ("accurate", "fast"):
        raise ValueError(f"Unsupported precision: {precision!r} (expected 'accurate' or 'fast'; 'auto' is not offered by the split-KV entries)")
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_varlen_attn_input_reason(q, cache, cu_seqlens_q, max_seqlen_q, seqused_k, scale, num_splits, max_seqlen_k)
        if reason:
            raise ValueError(reason)
    total_q, Hq, D = q.shape
    B, Hkv = cache.batch_size, cache.shape[1]
    Skv = cache.capacity if max_seqlen_k is None else int(max_seqlen_k)
    used = cache.seqlens if seqused_k is None else seqused_k
    ns = _resolve_varlen_splits(num_splits, B, Hq, Hkv, total_q, max_seqlen_q, Skv, D, q.device)
    eager = (not q.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if cache.layout != "rowmajor":
            raise ValueError("the eager definition needs a cache made on a CPU device or under config.attention.force_eager_fallback")
        out, lse, po, plse, ppath = _attend_varlen_eager(q, cache, cu_seqlens_q, causal, scale, used, Skv, ns, precision)
    else:
        if cache.layout != "frag":
            raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        out, lse, po, plse, ppath = nn._ops().fp8_paged_varlen_splitkv_attention_forward(
            q, cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, used, cu_seqlens_q, int(max_seqlen_q), Skv, cache.num_pages,
            cache.page_size, ns, cache.fp8_format, cache.numerics, bool(causal), precision, bool(return_lse), bool(return_partials), scale=scale)
    res: Tuple = (out,)
    if return_lse:
        res += (lse,)
    if return_partials:
        res += (po, plse, ppath)
    return res if len(res) > 1 else out


def paged_varlen_append_input_reason(cache, k_new, v_new, cu_seqlens) -> Optional[str]:
    """The first rule the arguments of `paged_kv_cache_append_varlen_fp8` break, or None.  Shapes, dtypes, devices and strides only: the
    CONTENTS of cu_seqlens, cache.seqlens and the block table are read on the device."""
    reason = _cache_reason(cache)
    if reason:
        return reason
    if not isinstance(k_new, Tensor) or not isinstance(v_new, Tensor) or k_new.dim() != 3 or v_new.dim() != 3:
        return "NYI: k_new and v_new must be 3-D tensors [total, Hkv, head_dim]"
    if k_new.requires_grad or v_new.requires_grad:
        return "NYI: k_new and v_new must be leaf tensors (no backward)"
    if k_new.dtype != cache.dtype or v_new.dtype != cache.dtype:
        return f"Expected k_new and v_new to have the cache's dtype {cache.dtype}, but got {k_new.dtype} and {v_new.dtype} instead."
    B = cache.batch_size
    _, Hkv, _, D = cache.shape
    if k_new.shape != v_new.shape:
        return f"Expect k_new and v_new to have the same shape but got {tuple(k_new.shape)} and {tuple(v_new.shape)}."
    if tuple(k_new.shape[1:]) != (Hkv, D):
        return f"Expected k_new and v_new to have shape [total, {Hkv}, {D}], but got {list(k_new.shape)}."
    if (2 * B + k_new.shape[0] // 64) * Hkv > 2 ** 31 - 1:
        return f"(2 * batch_size + total // 64) * Hkv must stay below 2^31 (the grid), got {(2 * B + k_new.shape[0] // 64) * Hkv}"
    if k_new.device != cache.device or v_new.device != cache.device:
        return f"Expected k_new and v_new to be on the cache's device {cache.device}, but got {k_new.device} and {v_new.device} instead."
    for name, t in (("k_new", k_new), ("v_new", v_new)):
        if t.shape[0] > 0 and not _q_rows_addressable(t):
            return (f"Expected {name} to have head_dim innermost and 16-byte-aligned rows (strides that are multiples of 8 elements), but got "
                    f"strides {tuple(t.stride())} at storage offset {t.storage_offset()}; pass {name}.contiguous()")
    if not isinstance(cu_seqlens, Tensor) or cu_seqlens.dtype != torch.int32:
        return f"Expected cu_seqlens to be a torch.int32 tensor, but got {getattr(cu_seqlens, 'dtype', type(cu_seqlens))}"
    if tuple(cu_seqlens.shape) != (B + 1,):
        return f"Expected cu_seqlens to have shape [{B + 1}] (the cache's slots + 1), but got {list(cu_seqlens.shape)}."
    if cu_seqlens.device != cache.device:
        return f"Expected cu_seqlens to be on {cache.device}, but got {cu_seqlens.device} instead."
    if not cu_seqlens.is_contiguous():
        return "Expected cu_seqlens to be contiguous"
    return _lens_reason("cache.seqlens", cache.seqlens, B, cache.device)


def _append_varlen_eager(cache: PagedKVCacheFP8, k_new: Tensor, v_new: Tensor, cu_seqlens: Tensor, advance: bool) -> None:
    """CPU tensors and config.attention.force_eager_fallback: the torch definition on row-major fp8 pools -- paged._append_eager on each
    slot's own rows of the packed tokens, the counts taken from cu_seqlens.  (This path reads cu_seqlens, seqlens and the table on the
    host.)"""
    total, Hkv, D = k_new.shape
    B = cache.batch_size
    cu = cu_seqlens.tolist()
    start = [min(max(int(cu[b]), 0), total) for b in range(B)]
    cnt = [min(max(int(cu[b + 1]), start[b]), total) - start[b] for b in range(B)]
    T = max(max(cnt), 1)
    # the padded tokens of the rule: slot b's rows, then zeros that new_lens keeps out of the cache
    pad = lambda x: torch.stack([torch.cat([x[start[b]:start[b] + cnt[b]], x.new_zeros((T - cnt[b], Hkv, D))]).transpose(0, 1)
                                 for b in range(B)])
    _append_eager(cache, pad(k_new), pad(v_new), torch.tensor(cnt, dtype=torch.int32), advance)


def paged_kv_cache_append_varlen_fp8(cache: PagedKVCacheFP8, k_new: Tensor, v_new: Tensor, cu_seqlens: Tensor, *,
                                     advance: bool = True) -> PagedKVCacheFP8:
    """`paged_kv_cache_append_fp8` for PACKED tokens, a different count per sequence slot; in place, returns `cache`.

    k_new, v_new [total, Hkv, D] in cache.dtype, read through their strides: head_dim innermost, token and head strides non-negative
    multiples of 8 elements, the base 16-byte aligned -- the K and V slices of a packed QKV projection go in as they are.  cu_seqlens:
    int32 [cache.batch_size + 1] on the device, the tensor `fp8_attn_paged_varlen_func` takes as cu_seqlens_q; slot b owns the tokens
    start_b = clamp(cu[b], 0, total) .. clamp(cu[b + 1], start_b, total), n_b of them (0: an idle slot).  With p_b = clamp(seqlens[b], 0,
    capacity), token start_b + t becomes key p_b + t of slot b; tokens at or beyond the capacity are dropped; seqlens[b] becomes
    min(p_b + n_b, capacity) unless advance=False.
    The rule: pools and seqlens end, byte for byte, as `paged_kv_cache_append_fp8(cache, pad(k_new), pad(v_new), new_lens=n)` leaves
    them (the same quantiser bytes, saturation, NaN handling, store schemes, table entries read and clamped); exactly the bytes of the
    appended keys change.  Rows behind cu[B] (a padded token bucket) are not read.  A cu_seqlens that is not non-decreasing gives
    unspecified pool contents in the slots concerned, and nothing worse.  Two slots that append into one page: undefined.
    Everything is read on the device: no host synchronisation, no allocation, graph-capture safe, and a captured call follows the later
    contents of cu_seqlens, seqlens and the table.  total = 0 returns at once.  CPU tensors and config.attention.force_eager_fallback run
    the eager definition (`_append_varlen_eager`); on the device there is no fallback.  Invalid input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_varlen_append_input_reason(cache, k_new, v_new, cu_seqlens)
        if reason:
            raise ValueError(reason)
    if k_new.shape[0] == 0:
        return cache
    eager = (not k_new.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if cache.layout != "rowmajor":
            raise ValueError("the eager definition needs a cache made on a CPU device or under config.attention.force_eager_fallback")
        _append_varlen_eager(cache, k_new, v_new, cu_seqlens, bool(advance))
        return cache
    if cache.layout != "frag":
        raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                         "config.attention.force_eager_fallback")
    ok, why = nn._pre_check_can_use_hip_attention(device=k_new.device)
    if not ok:
        raise ValueError(why)
    if torch.compiler.is_compiling():
        nn._ops().fp8_paged_varlen_kv_cache_append_(cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, cache.seqlens, k_new, v_new,
                                                    cu_seqlens, cache.num_pages, cache.page_size, cache.fp8_format, bool(advance))
    else:
        # outside a trace: the op's own body, without the dispatcher's bookkeeping for a mutating op (as paged_kv_cache_append_fp8)
        _native.paged_kv_cache_append_varlen_fp8(cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, cache.seqlens, k_new, v_new,
                                                 cu_seqlens, num_pages=cache.num_pages, page_size=cache.page_size,
                                                 fp8_dtype=_native.fp8_dtype_of(cache.fp8_format), advance=bool(advance))
    return cache


# ---- the rotary embedding at the cache's positions (include/qattn_paged_varlen_rope.h) ----------------------------------------------------
def _rope_tables_reason(cos, sin, D: int, capacity: int, device) -> Optional[str]:
    """The first rule a cos / sin pair breaks for a cache of head_dim D and `capacity` keys per slot, or None.  Host ints only."""
    if not isinstance(cos, Tensor) or not isinstance(sin, Tensor):
        return "cos / sin must be tensors"
    if cos.shape != sin.shape:
        return f"cos / sin must have the same shape, got {tuple(cos.shape)} and {tuple(sin.shape)}"
    if cos.dtype != sin.dtype or cos.dtype not in _TABLE_DTYPES:
        return f"cos / sin must share a dtype out of float32, bfloat16, float16, got {cos.dtype} and {sin.dtype}"
    if cos.device != device or sin.device != device:
        return f"cos / sin must be on the cache's device {device}, got {cos.device} and {sin.device}"
    if cos.dim() != 2:
        return (f"cos / sin must be [T, D/2], one table pair for every slot, got {cos.dim()} dimension(s): the [B, T, D/2] form (a table per "
                "slot) is not offered here, nor are per-slot position offsets")
    if cos.shape[1] != D // 2:
        return (f"cos / sin must hold D/2 = {D // 2} entries per row, one per rotated pair, got {cos.shape[1]}: a partial rotary_dim is not "
                "supported (only the full head dim is rotated), nor is the duplicated [T, D] table layout")
    if cos.shape[0] < capacity:
        return (f"cos / sin hold T = {cos.shape[0]} positions, fewer than the cache's capacity max_pages_per_seq * page_size = {capacity}: "
                "a key's index in its sequence is its position")
    if cos.dtype == torch.float32:   # read in place (16-bit tables are up-cast into dense ones)
        for name, t in (("cos", cos), ("sin", sin)):
            aligned = torch.compiler.is_dynamo_compiling() or t.storage_offset() % 4 == 0
            if not (t.stride(1) == 1 and aligned and (t.shape[0] == 1 or (t.stride(0) >= 0 and t.stride(0) % 4 == 0))):
                return (f"Expected {name} to have dense rows, a 16-byte-aligned base and a row stride that is a non-negative multiple of 4 "
                        f"floats (rows are read 16 bytes at a time), but got strides {tuple(t.stride())} at storage offset "
                        f"{t.storage_offset()}; pass {name}.contiguous()")
        if cos.shape[0] > 1 and cos.stride(0) != sin.stride(0):
            return f"Expected cos and sin to have the same row stride, but got {cos.stride(0)} and {sin.stride(0)}"
    return None


def paged_varlen_rope_append_input_reason(cache, k_new, v_new, cu_seqlens, cos, sin) -> Optional[str]:
    """The first rule the arguments of `paged_kv_cache_append_varlen_rope_fp8` break, or None: `paged_varlen_append_input_reason`, then
    the table rules -- cos / sin [T, D/2] of one dtype out of float32 / bfloat16 / float16 on the cache's device, T >= cache.capacity,
    float32 tables addressable as rows of float4.  Shapes, dtypes, devices and strides only: nothing is read on the device."""
    reason = paged_varlen_append_input_reason(cache, k_new, v_new, cu_seqlens)
    if reason:
        return reason
    return _rope_tables_reason(cos, sin, cache.shape[3], cache.capacity, cache.device)


def _fp32_tables(cos: Tensor, sin: Tensor) -> Tuple[Tensor, Tensor]:
    """16-bit tables are up-cast (exact), as rope._check_tables does; float32 tables go as they are"""
    if cos.dtype == torch.float32:
        return cos, sin
    return cos.to(torch.float32).contiguous(), sin.to(torch.float32).contiguous()


def _rope_positions_host(cache: PagedKVCacheFP8, cu_seqlens: Tensor, total: int, T: int, appended: bool):
    """(rows, positions): the rows of the packed tokens that a slot owns and the table row each is rotated with, as host lists.  (Reads
    cu_seqlens and seqlens on the host: the eager definitions only.)"""
    cu, lens, cap = cu_seqlens.tolist(), cache.seqlens.tolist(), cache.capacity
    rows, pos = [], []
    for b in range(cache.batch_size):
        start = min(max(int(cu[b]), 0), total)
        n = min(max(int(cu[b + 1]), start), total) - start
        base = max(min(max(int(lens[b]), 0), cap) - (n if appended else 0), 0)
        rows += range(start, start + n)
        pos += [min(base + t, T - 1) for t in range(n)]
    return rows, pos


def _rope_rows_eager(x: Tensor, rows, pos, cos: Tensor, sin: Tensor, interleaved: bool) -> Tensor:
    """apply_rope_eager on the rows `rows` of x [total, H, D], row rows[j] with table row pos[j] -> [len(rows), H, D]"""
    at = torch.tensor(pos, dtype=torch.long, device=cos.device)
    return apply_rope_eager(x[rows].transpose(0, 1)[None], cos[at], sin[at], interleaved=interleaved)[0].transpose(0, 1)


def _append_varlen_rope_eager(cache: PagedKVCacheFP8, k_new: Tensor, v_new: Tensor, cu_seqlens: Tensor, cos: Tensor, sin: Tensor,
                              interleaved: bool, advance: bool) -> None:
    """CPU tensors and config.attention.force_eager_fallback: the rule's composition -- `apply_rope_eager` on the owned rows of k_new at
    their keys' positions, then `_append_varlen_eager`.  (This path reads cu_seqlens and seqlens on the host.)"""
    rows, pos = _rope_positions_host(cache, cu_seqlens, k_new.shape[0], cos.shape[0], False)
    k_rot = torch.zeros(k_new.shape, dtype=k_new.dtype, device=k_new.device)      # (rows nobody owns are not read by the append)
    if rows:
        k_rot[rows] = _rope_rows_eager(k_new, rows, pos, cos, sin, interleaved)
    _append_varlen_eager(cache, k_rot, v_new, cu_seqlens, advance)


def paged_kv_cache_append_varlen_rope_fp8(cache: PagedKVCacheFP8, k_new: Tensor, v_new: Tensor, cu_seqlens: Tensor, cos: Tensor, sin: Tensor, *,
                                          interleaved: bool = False, advance: bool = True) -> PagedKVCacheFP8:
    """`paged_kv_cache_append_varlen_fp8` with the rotary embedding of K inside the append; in place, returns `cache`.

    cache, k_new, v_new, cu_seqlens, advance: exactly those of `paged_kv_cache_append_varlen_fp8` (strided slices of the packed
    projection, clamps, dropped tail, idle slots, rows behind cu[B] not read).  k_new is the UNROTATED K.  cos, sin: [T, D/2], one table
    pair for every slot, T >= cache.capacity; float32 tables are read in place as rows of float4 (base 16-byte aligned, row stride a
    non-negative multiple of 4 floats: a slice cos[:, :D/2] of a wider table is fine), bfloat16 / float16 tables are up-cast.
    `interleaved` as `fp8_attn_rope_func`: False pairs (i, i + D/2), True pairs (2i, 2i + 1).  Key p_b + t of slot b,
    p_b = clamp(seqlens[b], 0, capacity), is rotated with table row p_b + t: a key's index in its sequence is its position.  V is not
    rotated.
    The rule: pools and seqlens end, byte for byte, as `paged_kv_cache_append_varlen_fp8(cache, k_rot, v_new, cu_seqlens)` leaves them
    with k_rot = `apply_rope_eager` of every token at its key's position -- the rotated value rounded to the input dtype before the
    quantiser, non-finite values handled as the composition handles them; exactly the bytes of the appended keys change.
    Everything is read on the device: no host synchronisation, no allocation (16-bit tables excepted), graph-capture safe, and a
    captured call follows the later contents of cu_seqlens, seqlens, the table and cos / sin.  total = 0 returns at once.  CPU tensors
    and config.attention.force_eager_fallback run the eager definition (`_append_varlen_rope_eager`); on the device there is no
    fallback.  Invalid input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_varlen_rope_append_input_reason(cache, k_new, v_new, cu_seqlens, cos, sin)
        if reason:
            raise ValueError(reason)
    if k_new.shape[0] == 0:
        return cache
    cos, sin = _fp32_tables(cos, sin)
    il = bool(interleaved)
    eager = (not k_new.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if cache.layout != "rowmajor":
            raise ValueError("the eager definition needs a cache made on a CPU device or under config.attention.force_eager_fallback")
        _append_varlen_rope_eager(cache, k_new, v_new, cu_seqlens, cos, sin, il, bool(advance))
        return cache
    if cache.layout != "frag":
        raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                         "config.attention.force_eager_fallback")
    ok, why = nn._pre_check_can_use_hip_attention(device=k_new.device)
    if not ok:
        raise ValueError(why)
    if torch.compiler.is_compiling():
        nn._ops().fp8_paged_varlen_rope_kv_cache_append_(cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, cache.seqlens, k_new,
                                                         v_new, cu_seqlens, cos, sin, cache.num_pages, cache.page_size, cache.fp8_format, il,
                                                         bool(advance))
    else:
        # outside a trace: the op's own body, without the dispatcher's bookkeeping for a mutating op (as paged_kv_cache_append_varlen_fp8)
        _native.paged_kv_cache_append_varlen_rope_fp8(cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, cache.seqlens, k_new,
                                                      v_new, cu_seqlens, cos, sin, num_pages=cache.num_pages, page_size=cache.page_size,
                                                      fp8_dtype=_native.fp8_dtype_of(cache.fp8_format), interleaved=il, advance=bool(advance))
    return cache


def paged_varlen_rope_input_reason(x, cache, cu_seqlens, cos, sin, out=None) -> Optional[str]:
    """The first rule the arguments of `apply_rope_paged_varlen` break, or None.  Shapes, dtypes, devices and strides only."""
    reason = _cache_reason(cache)
    if reason:
        return reason
    if not isinstance(x, Tensor) or x.dim() != 3:
        return "NYI: x must be a 3-D tensor [total, H, head_dim]"
    if x.requires_grad:
        return "NYI: x must be a leaf tensor (no backward)"
    if x.dtype != cache.dtype:
        return f"Expected x to have the cache's dtype {cache.dtype}, but got {x.dtype} instead."
    B, D = cache.batch_size, cache.shape[3]
    if x.shape[2] != D:
        return f"Expect x to have the cache's head dimension but got {x.shape[2]} and {D}."
    if x.shape[1] == 0:
        return "Expected a non-empty head count"
    if x.device != cache.device:
        return f"Expected x to be on the cache's device {cache.device}, but got {x.device} instead."
    if x.shape[0] > 0 and not _q_rows_addressable(x):
        return (f"Expected x to have head_dim innermost and 16-byte-aligned rows (strides that are multiples of 8 elements), but got "
                f"strides {tuple(x.stride())} at storage offset {x.storage_offset()}; pass x.contiguous()")
    if not isinstance(cu_seqlens, Tensor) or cu_seqlens.dtype != torch.int32:
        return f"Expected cu_seqlens to be a torch.int32 tensor, but got {getattr(cu_seqlens, 'dtype', type(cu_seqlens))}"
    if tuple(cu_seqlens.shape) != (B + 1,):
        return f"Expected cu_seqlens to have shape [{B + 1}] (the cache's slots + 1), but got {list(cu_seqlens.shape)}."
    if cu_seqlens.device != cache.device:
        return f"Expected cu_seqlens to be on {cache.device}, but got {cu_seqlens.device} instead."
    if not cu_seqlens.is_contiguous():
        return "Expected cu_seqlens to be contiguous"
    reason = _lens_reason("cache.seqlens", cache.seqlens, B, cache.device)
    if reason:
        return reason
    if out is not None:
        if not isinstance(out, Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
            return f"Expected out to have x's shape {list(x.shape)}, dtype and device"
        if not out.is_contiguous() or (not torch.compiler.is_dynamo_compiling() and out.storage_offset() % 8 != 0):
            return "Expected out to be contiguous and 16-byte aligned"
    return _rope_tables_reason(cos, sin, D, cache.capacity, cache.device)


def _rope_paged_varlen_eager(x: Tensor, cache: PagedKVCacheFP8, cu_seqlens: Tensor, cos: Tensor, sin: Tensor, interleaved: bool,
                             appended: bool, out: Tensor) -> None:
    """CPU tensors and config.attention.force_eager_fallback: `apply_rope_eager` on the owned rows at host-computed positions, written
    into `out`; other rows of `out` are left alone.  (Reads cu_seqlens and seqlens on the host.)"""
    rows, pos = _rope_positions_host(cache, cu_seqlens, x.shape[0], cos.shape[0], appended)
    if rows:
        out[rows] = _rope_rows_eager(x, rows, pos, cos, sin, interleaved)


def apply_rope_paged_varlen(x: Tensor, cache: PagedKVCacheFP8, cu_seqlens: Tensor, cos: Tensor, sin: Tensor, *, interleaved: bool = False,
                            appended: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """Rotate packed rows -- q, or anything packed under cu_seqlens -- at the positions of the paged cache's slots.

    x [total, H, D] in cache.dtype, read through its {token, head} strides under the packed append's stride rules: the q slice of the
    projection goes in as it is.  Returns dense [total, H, D] in x.dtype (`out`, if given: contiguous, 16-byte aligned).  cu_seqlens, cos,
    sin, interleaved: as `paged_kv_cache_append_varlen_rope_fp8`.  Row start_b + t is rotated with table row max(base_b, 0) + t,
    base_b = clamp(seqlens[b], 0, capacity) - (n_b if appended else 0): appended=False for a call made BEFORE the step's append -- a
    query then gets the position of the key the same token becomes -- appended=True for one made after an advancing append.
    Bit for bit `apply_rope_eager` at these positions.  Rows behind cu[B] are neither read nor written (unspecified in a new tensor).
    One launch; everything is read on the device: no host synchronisation, no allocation beyond the result (16-bit tables excepted),
    graph-capture safe.  CPU tensors and config.attention.force_eager_fallback run the eager definition; on the device there is no
    fallback.  Invalid input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_varlen_rope_input_reason(x, cache, cu_seqlens, cos, sin, out)
        if reason:
            raise ValueError(reason)
    cos, sin = _fp32_tables(cos, sin)
    il, ap = bool(interleaved), bool(appended)
    eager = (not x.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        res = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
        _rope_paged_varlen_eager(x, cache, cu_seqlens, cos, sin, il, ap, res)
        return res
    ok, why = nn._pre_check_can_use_hip_attention(device=x.device)
    if not ok:
        raise ValueError(why)
    if torch.compiler.is_compiling():
        res = nn._ops().rope_paged_varlen(x, cache.seqlens, cu_seqlens, cos, sin, cache.capacity, il, ap)
        return res if out is None else out.copy_(res)
    return _native.rope_paged_varlen(x, cache.seqlens, cu_seqlens, cos, sin, capacity=cache.capacity, interleaved=il, appended=ap, out=out)


# ---- the rotary embedding at the CALLER's positions (include/qattn_paged_varlen_rope_pos.h) ------------------------------------------------
def _positions_reason(positions, total: int, device) -> Optional[str]:
    if not isinstance(positions, Tensor) or positions.dtype != torch.int64:
        return f"Expected positions to be a torch.int64 tensor [total], but got {getattr(positions, 'dtype', type(positions))}"
    if tuple(positions.shape) != (total,):
        return f"Expected positions to have shape [{total}] (one position per packed token), but got {list(positions.shape)}."
    if positions.device != device:
        return f"Expected positions to be on {device}, but got {positions.device} instead."
    if not positions.is_contiguous():
        return "Expected positions to be contiguous"
    return None


def paged_varlen_rope_pos_append_input_reason(cache, k_new, v_new, cu_seqlens, positions, cos, sin) -> Optional[str]:
    """The first rule the arguments of `paged_kv_cache_append_varlen_rope_pos_fp8` break, or None: `paged_varlen_append_input_reason`,
    then positions int64 [total], contiguous, on the cache's device, then the table rules of `paged_varlen_rope_append_input_reason`
    with any T >= 1 (positions are clamped into the tables).  Shapes, dtypes, devices and strides only: nothing is read on the device."""
    reason = paged_varlen_append_input_reason(cache, k_new, v_new, cu_seqlens)
    if reason:
        return reason
    reason = _positions_reason(positions, k_new.shape[0], cache.device)
    if reason:
        return reason
    return _rope_tables_reason(cos, sin, cache.shape[3], 1, cache.device)


def _clamped_rows(positions: Tensor, rows, T: int):
    """the table rows of the packed rows `rows`: clamp(positions[row], 0, T - 1), as a host list (the eager definitions only)"""
    at = positions.tolist()
    return [min(max(int(at[r]), 0), T - 1) for r in rows]


def _append_varlen_rope_pos_eager(cache: PagedKVCacheFP8, k_new: Tensor, v_new: Tensor, cu_seqlens: Tensor, positions: Tensor, cos: Tensor,
                                  sin: Tensor, interleaved: bool, advance: bool) -> None:
    """CPU tensors and config.attention.force_eager_fallback: the rule's composition -- `apply_rope_eager` on the owned rows of k_new at
    the caller's (clamped) positions, then `_append_varlen_eager`.  (This path reads cu_seqlens and positions on the host.)"""
    rows, _ = _rope_positions_host(cache, cu_seqlens, k_new.shape[0], cos.shape[0], False)
    k_rot = torch.zeros(k_new.shape, dtype=k_new.dtype, device=k_new.device)      # (rows nobody owns are not read by the append)
    if rows:
        k_rot[rows] = _rope_rows_eager(k_new, rows, _clamped_rows(positions, rows, cos.shape[0]), cos, sin, interleaved)
    _append_varlen_eager(cache, k_rot, v_new, cu_seqlens, advance)


def paged_kv_cache_append_varlen_rope_pos_fp8(cache: PagedKVCacheFP8, k_new: Tensor, v_new: Tensor, cu_seqlens: Tensor, positions: Tensor,
                                              cos: Tensor, sin: Tensor, *, interleaved: bool = False, advance: bool = True) -> PagedKVCacheFP8:
    """`paged_kv_cache_append_varlen_rope_fp8` at the CALLER's positions (vLLM's `positions`); in place, returns `cache`.

    cache, k_new, v_new, cu_seqlens, cos, sin, interleaved, advance: those of `paged_kv_cache_append_varlen_rope_fp8`, except that the
    tables may hold any T >= 1 rows.  positions: int64 [total] on the device.  Token t is rotated with table row
    clamp(positions[t], 0, T - 1).  WHERE the key is stored is unchanged: token start_b + t becomes key seqlens[b] + t of slot b.  Under
    tree-shaped speculative decoding a draft token's position is base + depth (`tree_positions`): siblings share a position while their
    keys lie next to each other.  Rows behind cu[B] are not read.
    The rule: pools and seqlens end, byte for byte, as `apply_rope_eager` on K at those positions followed by
    `paged_kv_cache_append_varlen_fp8` leaves them; with positions[start_b + t] = seqlens[b] + t the bits are those of
    `paged_kv_cache_append_varlen_rope_fp8`.  Exactly the bytes of the appended keys change.
    Everything is read on the device: no host synchronisation, no allocation (16-bit tables excepted), graph-capture safe, and a
    captured call follows the later contents of positions, cu_seqlens, seqlens, the table and cos / sin.  total = 0 returns at once.
    CPU tensors and config.attention.force_eager_fallback run the eager definition (`_append_varlen_rope_pos_eager`); on the device
    there is no fallback.  Invalid input raises ValueError(reason).  Not offered: a partial rotary_dim, multi-axis (M-RoPE) positions,
    positions in the padded and the contiguous appends."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_varlen_rope_pos_append_input_reason(cache, k_new, v_new, cu_seqlens, positions, cos, sin)
        if reason:
            raise ValueError(reason)
    if k_new.shape[0] == 0:
        return cache
    cos, sin = _fp32_tables(cos, sin)
    il = bool(interleaved)
    eager = (not k_new.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if cache.layout != "rowmajor":
            raise ValueError("the eager definition needs a cache made on a CPU device or under config.attention.force_eager_fallback")
        _append_varlen_rope_pos_eager(cache, k_new, v_new, cu_seqlens, positions, cos, sin, il, bool(advance))
        return cache
    if cache.layout != "frag":
        raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                         "config.attention.force_eager_fallback")
    ok, why = nn._pre_check_can_use_hip_attention(device=k_new.device)
    if not ok:
        raise ValueError(why)
    if torch.compiler.is_compiling():
        nn._ops().fp8_paged_varlen_rope_pos_kv_cache_append_(cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, cache.seqlens,
                                                             k_new, v_new, cu_seqlens, positions, cos, sin, cache.num_pages, cache.page_size,
                                                             cache.fp8_format, il, bool(advance))
    else:
        # outside a trace: the op's own body, without the dispatcher's bookkeeping for a mutating op (as paged_kv_cache_append_varlen_fp8)
        _native.paged_kv_cache_append_varlen_rope_pos_fp8(cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, cache.seqlens,
                                                          k_new, v_new, cu_seqlens, positions, cos, sin, num_pages=cache.num_pages,
                                                          page_size=cache.page_size, fp8_dtype=_native.fp8_dtype_of(cache.fp8_format),
                                                          interleaved=il, advance=bool(advance))
    return cache


def rope_positions_input_reason(x, positions, cos, sin, out=None) -> Optional[str]:
    """The first rule the arguments of `apply_rope_positions` break, or None.  Shapes, dtypes, devices and strides only."""
    if not isinstance(x, Tensor) or x.dim() != 3:
        return "NYI: x must be a 3-D tensor [total, H, head_dim]"
    if x.requires_grad:
        return "NYI: x must be a leaf tensor (no backward)"
    if x.dtype not in (torch.float16, torch.bfloat16):
        return f"Expected x to have dtype torch.float16 or torch.bfloat16, but got x.dtype: {x.dtype} instead."
    D = x.shape[2]
    if D not in (64, 128, 256):
        return f"head_dim must be one of [64, 128, 256], got {D}"
    if x.shape[1] == 0:
        return "Expected a non-empty head count"
    if x.shape[0] > 0 and not _q_rows_addressable(x):
        return (f"Expected x to have head_dim innermost and 16-byte-aligned rows (strides that are multiples of 8 elements), but got "
                f"strides {tuple(x.stride())} at storage offset {x.storage_offset()}; pass x.contiguous()")
    reason = _positions_reason(positions, x.shape[0], x.device)
    if reason:
        return reason
    if out is not None:
        if not isinstance(out, Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
            return f"Expected out to have x's shape {list(x.shape)}, dtype and device"
        if not out.is_contiguous() or (not torch.compiler.is_dynamo_compiling() and out.storage_offset() % 8 != 0):
            return "Expected out to be contiguous and 16-byte aligned"
    return _rope_tables_reason(cos, sin, D, 1, x.device)


def apply_rope_positions(x: Tensor, positions: Tensor, cos: Tensor, sin: Tensor, *, interleaved: bool = False,
                         out: Optional[Tensor] = None) -> Tensor:
    """Rotate packed rows -- q, any strided q slice of a packed projection -- at the CALLER's positions.

    x [total, H, D] bf16 / fp16, D in {64, 128, 256}, read through its {token, head} strides under the packed append's stride rules.
    positions: int64 [total] on x's device; row t is rotated with table row clamp(positions[t], 0, T - 1) of cos / sin [T, D/2] (as
    `paged_kv_cache_append_varlen_rope_pos_fp8` takes them).  Returns dense [total, H, D] in x.dtype (`out`, if given: contiguous,
    16-byte aligned).  Every row is read and written: there is no cu_seqlens here.  Bit for bit `apply_rope_eager` at these positions,
    and with the positions of `apply_rope_paged_varlen` its bits.
    One launch; everything is read on the device: no host synchronisation, no allocation beyond the result (16-bit tables excepted),
    graph-capture safe.  CPU tensors and config.attention.force_eager_fallback run the eager definition; on the device there is no
    fallback.  Invalid input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = rope_positions_input_reason(x, positions, cos, sin, out)
        if reason:
            raise ValueError(reason)
    cos, sin = _fp32_tables(cos, sin)
    il = bool(interleaved)
    eager = (not x.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        res = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
        rows = list(range(x.shape[0]))
        if rows:
            res[rows] = _rope_rows_eager(x, rows, _clamped_rows(positions, rows, cos.shape[0]), cos, sin, il)
        return res
    ok, why = nn._pre_check_can_use_hip_attention(device=x.device)
    if not ok:
        raise ValueError(why)
    if torch.compiler.is_compiling():
        res = nn._ops().rope_packed_positions(x, positions, cos, sin, il)
        return res if out is None else out.copy_(res)
    return _native.rope_packed_positions(x, positions, cos, sin, interleaved=il, out=out)

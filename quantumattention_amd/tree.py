"""Tree-shaped speculative decoding on the paged FP8 K/V cache (include/qattn_paged_varlen_tree.h): the verify
pass under a draft TREE per sequence slot, `fp8_attn_paged_varlen_tree_func`, and the compaction of the accepted root-to-leaf path into
the contiguous tail of the slot's keys, `paged_kv_cache_compact_fp8`.

`fp8_attn_paged_varlen_func(causal=True)` lets draft token p see every earlier draft, siblings included: that verifies a LINEAR draft.
A tree verifier (EAGLE, Medusa, SpecInfer) lets a draft token see the committed keys plus its own ancestors.  The step:

    paged_kv_cache_append_varlen_fp8(cache, k_draft, v_draft, cu)                      # the drafts become the slots' last keys
    words = tree_mask_from_parents(parents, cu)                                        # int64 [total_q]: bit i = draft i is an ancestor (or self)
    out = fp8_attn_paged_varlen_tree_func(q_draft, cache, cu, max_seqlen_q, words, max_seqlen_k=longest)
    ...                                                                                # the caller verifies: accept_index, accept_lens
    paged_kv_cache_compact_fp8(cache, cu, accept_index, accept_lens)                   # the accepted path becomes the tail; seqlens follow

Package attributes, not names of `__all__`.  Not offered: sliding windows under a tree mask; sinks folded into the tree call (compose:
return_lse=True, then `merge_attn_states_with_sinks([out], [lse], sinks)`); trees above 64 tokens per slot (such a slot is plain causal);
a positions tensor for the fused RoPE append (a tree node's position is base + depth, not base + index: rotate the drafts with
`apply_rope_eager` at the caller's positions, then use the plain packed append); the contiguous `KVCacheFP8`; masks for the dense, 16-bit
and block-sparse entries."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native, nn
from .paged import PagedKVCacheFP8, _cache_reason, _lens_reason
from .paged_varlen import _attend_varlen_eager, _resolve_varlen_splits, paged_varlen_attn_input_reason
from .utils import checks

TREE_MAX_TOKENS = 64   # draft tokens of a slot that a mask word covers


def _packed_ints_reason(name, t, n, device, dtype=torch.int32) -> Optional[str]:
    if not isinstance(t, Tensor) or t.dtype != dtype:
        return f"Expected {name} to be a {dtype} tensor, but got {getattr(t, 'dtype', type(t))}"
    if tuple(t.shape) != (n,):
        return f"Expected {name} to have shape [{n}], but got {list(t.shape)}."
    if t.device != device:
        return f"Expected {name} to be on {device}, but got {t.device} instead."
    if not t.is_contiguous():
        return f"Expected {name} to be contiguous"
    return None


def tree_mask_from_parents(parents: Tensor, cu_seqlens_q: Tensor) -> Tensor:
    """The mask words of draft trees given by parent pointers -> int64 [total_q].

    parents: int32 [total_q], the in-slot index of each draft token's parent, -1 for a root; a parent's index is below its child's.
    cu_seqlens_q: int32 [B + 1], the packing of the tokens.  The word of token p of a slot has bit p and the bits of all its ancestors
    set (bits 0 .. 63: meaningful for slots with at most 64 tokens; others are plain causal in the attention and their words are not
    read).  Torch ops on the input's device, nothing read on the host: 6 doubling steps cover every depth below 64."""
    if not isinstance(parents, Tensor) or parents.dtype != torch.int32 or parents.dim() != 1:
        raise ValueError("Expected parents to be a 1-D torch.int32 tensor [total_q]")
    if not isinstance(cu_seqlens_q, Tensor) or cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or cu_seqlens_q.shape[0] < 2:
        raise ValueError("Expected cu_seqlens_q to be a 1-D torch.int32 tensor [B + 1]")
    if cu_seqlens_q.device != parents.device:
        raise ValueError(f"Expected cu_seqlens_q to be on {parents.device}, but got {cu_seqlens_q.device} instead.")
    total = parents.shape[0]
    if total == 0:
        return torch.zeros((0,), dtype=torch.int64, device=parents.device)
    tok = torch.arange(total, device=parents.device)
    cu = cu_seqlens_q.long().clamp(0, total)
    slot = (tok[:, None] >= cu[None, 1:]).sum(1).clamp(max=cu.shape[0] - 2)   # the slot that owns the token (tokens behind cu[B]: the last)
    start = cu[slot]
    p = tok - start                                                        # the in-slot index
    par = parents.long()
    has = (par >= 0) & (par < p)
    # anc: the packed token of the 2^k-th ancestor (the token itself once the root is passed: its bits are already in)
    anc = torch.where(has, (start + par).clamp(0, total - 1), tok)
    word = torch.ones_like(tok) << (p & 63)
    for _ in range(6):
        word = word | word[anc]
        anc = anc[anc]
    return word


def paged_varlen_tree_input_reason(q, cache, cu_seqlens_q, max_seqlen_q, tree_mask, seqused_k=None, scale=None, num_splits=0,
                                   max_seqlen_k=None) -> Optional[str]:
    """The first rule the arguments of `fp8_attn_paged_varlen_tree_func` break, or None: `paged_varlen_attn_input_reason`, then tree_mask
    int64 [total_q], contiguous, on q's device.  Shapes, dtypes, devices and strides only: the words are read on the device."""
    reason = paged_varlen_attn_input_reason(q, cache, cu_seqlens_q, max_seqlen_q, seqused_k, scale, num_splits, max_seqlen_k)
    if reason:
        return reason
    return _packed_ints_reason("tree_mask", tree_mask, q.shape[0], q.device, torch.int64)


def fp8_attn_paged_varlen_tree_func(q, cache: PagedKVCacheFP8, cu_seqlens_q: Tensor, max_seqlen_q: int, tree_mask: Tensor, *,
                                    scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None,
                                    num_splits: int = 0, precision: str = "accurate", return_lse: bool = False,
                                    return_partials: bool = False):
    """`fp8_attn_paged_varlen_func(causal=True)` under a draft TREE per sequence slot: the verify pass of tree speculative decoding.

    Arguments and outputs are those of `fp8_attn_paged_varlen_func(..., causal=True)`, plus tree_mask: int64 [total_q] on the device,
    read as an unsigned 64-bit word per token.  Slot b has Sq_b queries and L_b keys, delta = L_b - Sq_b; its draft tokens are its LAST
    Sq_b keys (already appended, as for the causal call).  Position p attends key j iff j <= min(L_b - 1, p + delta) -- the causal rule
    -- and, for j >= max(delta, 0), bit j - delta of tree_mask[cu[b] + p] is set.  Bits above p are ignored; the self bit p is honoured
    as given; committed keys (j < delta) are always attended.  A slot with Sq_b > 64 (a prefill chunk of a mixed step) ignores its words
    and is plain causal.  A row whose mask leaves no key is a zero row with LSE -inf.  The word belongs to the token: all heads read it.
    The split plan, the chunks swept and the merge are the causal call's, so a chain (`tree_mask_from_parents` of parents p - 1) gives
    `fp8_attn_paged_varlen_func(causal=True)` bit for bit: out, lse and the partials.
    Everything is read on the device: no host synchronisation, graph-capture safe, and a captured call follows the later contents of
    tree_mask, cu_seqlens_q, seqused_k and the table.  CPU tensors and config.attention.force_eager_fallback run the eager definition
    (`paged_varlen._attend_varlen_eager` with tree_mask=); on the device there is no fallback.  Unsupported input raises
    ValueError(reason)."""
    if precision not in ("accurate", "fast"):
        raise ValueError(f"Unsupported precision: {precision!r} (expected 'accurate' or 'fast'; 'auto' is not offered by the split-KV entries)")
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_varlen_tree_input_reason(q, cache, cu_seqlens_q, max_seqlen_q, tree_mask, seqused_k, scale, num_splits, max_seqlen_k)
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
        out, lse, po, plse, ppath = _attend_varlen_eager(q, cache, cu_seqlens_q, True, scale, used, Skv, ns, precision, tree_mask=tree_mask)
    else:
        if cache.layout != "frag":
            raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        out, lse, po, plse, ppath = nn._ops().fp8_paged_varlen_splitkv_tree_attention_forward(
            q, cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, used, cu_seqlens_q, tree_mask, int(max_seqlen_q), Skv,
            cache.num_pages, cache.page_size, ns, cache.fp8_format, cache.numerics, precision, bool(return_lse), bool(return_partials),
            scale=scale)
    res: Tuple = (out,)
    if return_lse:
        res += (lse,)
    if return_partials:
        res += (po, plse, ppath)
    return res if len(res) > 1 else out


def paged_compact_input_reason(cache, cu_seqlens, accept_index, accept_lens) -> Optional[str]:
    """The first rule the arguments of `paged_kv_cache_compact_fp8` break, or None.  Shapes, dtypes, devices and strides only: the
    CONTENTS of cu_seqlens, accept_index, accept_lens, cache.seqlens and the block table are read on the device."""
    reason = _cache_reason(cache)
    if reason:
        return reason
    B = cache.batch_size
    reason = _packed_ints_reason("cu_seqlens", cu_seqlens, B + 1, cache.device)
    if reason:
        return reason
    if not isinstance(accept_index, Tensor) or accept_index.dim() != 1:
        return "Expected accept_index to be a 1-D torch.int32 tensor [total], packed like the step's tokens"
    reason = _packed_ints_reason("accept_index", accept_index, accept_index.shape[0], cache.device)
    if reason:
        return reason
    reason = _packed_ints_reason("accept_lens", accept_lens, B, cache.device)
    if reason:
        return reason
    reason = _lens_reason("cache.seqlens", cache.seqlens, B, cache.device)
    if reason:
        return reason
    if B * cache.shape[1] > 2 ** 31 - 1:
        return f"batch_size * Hkv must stay below 2^31 (the grid), got {B * cache.shape[1]}"
    return None


def _compact_eager(cache: PagedKVCacheFP8, cu_seqlens: Tensor, accept_index: Tensor, accept_lens: Tensor) -> None:
    """CPU tensors and config.attention.force_eager_fallback: the rule of include/qattn_paged_varlen_tree.h on row-major fp8 pools --
    per compactable slot, the source keys' bytes gathered through the (clamped) table, then stored at the destination keys.  (This path
    reads cu_seqlens, accept_index, accept_lens, seqlens and the table on the host.)"""
    total = accept_index.shape[0]
    ps, capacity, B = cache.page_size, cache.capacity, cache.batch_size
    cu, idx, cnt, lens = cu_seqlens.tolist(), accept_index.tolist(), accept_lens.tolist(), cache.seqlens.tolist()
    table = cache.block_table.clamp(0, cache.num_pages - 1).tolist()
    for b in range(B):
        start = min(max(int(cu[b]), 0), total)
        Sq = min(max(int(cu[b + 1]), start), total) - start
        L = min(max(int(lens[b]), 0), capacity)
        if not (1 <= Sq <= TREE_MAX_TOKENS and L >= Sq):
            continue
        base = L - Sq
        n = min(max(int(cnt[b]), 0), Sq)
        if n:
            src = torch.tensor([base + min(max(int(idx[start + i]), 0), Sq - 1) for i in range(n)], dtype=torch.long)
            dst = torch.arange(base, base + n)
            pages = torch.tensor(table[b], dtype=torch.long)
            for pool in (cache.k, cache.v):
                u8 = pool.view(torch.uint8)
                held = u8[pages[src // ps].to(u8.device), :, (src % ps).to(u8.device)].clone()    # every read before every write
                u8[pages[dst // ps].to(u8.device), :, (dst % ps).to(u8.device)] = held
        lens[b] = base + n
    cache.seqlens.copy_(torch.tensor(lens, dtype=torch.int32))


def paged_kv_cache_compact_fp8(cache: PagedKVCacheFP8, cu_seqlens: Tensor, accept_index: Tensor, accept_lens: Tensor) -> PagedKVCacheFP8:
    """After a tree-shaped speculative step: the accepted root-to-leaf path of every slot becomes the contiguous tail of its keys; in
    place, returns `cache`.

    cu_seqlens: the verify step's int32 [cache.batch_size + 1].  accept_index: int32 [total], packed like the step's tokens; slot b's
    entries cu[b] .. cu[b] + n_b - 1 are in-slot draft indices.  accept_lens: int32 [batch_size].  All on the device.
    A slot is compactable iff 1 <= Sq_b <= 64 and L_b = clamp(seqlens[b], 0, capacity) >= Sq_b.  Then base = L_b - Sq_b,
    n_b = clamp(accept_lens[b], 0, Sq_b), idx_i = clamp(accept_index[cu[b] + i], 0, Sq_b - 1); for i < n_b key base + i receives the K and
    V bytes key base + idx_i held BEFORE the call (all reads happen before all writes: any index list is well defined), and seqlens[b]
    becomes base + n_b.  Other slots keep their bytes and their seqlens.  Exactly the bytes of the keys base + i, i < n_b, may change.
    The scales are fixed per (slot, head), so the bytes move unchanged: the cache ends as if only the accepted tokens had been
    appended.  Two slots whose draft regions share a page: undefined, as for the append.
    Everything is read on the device: no host synchronisation, no allocation, graph-capture safe, and a captured call follows the later
    contents of its index tensors, seqlens and the table.  total = 0 returns at once.  CPU tensors and
    config.attention.force_eager_fallback run the eager definition (`_compact_eager`); on the device there is no fallback.  Invalid
    input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_compact_input_reason(cache, cu_seqlens, accept_index, accept_lens)
        if reason:
            raise ValueError(reason)
    if accept_index.shape[0] == 0:
        return cache
    eager = (not cache.k.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if cache.layout != "rowmajor":
            raise ValueError("the eager definition needs a cache made on a CPU device or under config.attention.force_eager_fallback")
        _compact_eager(cache, cu_seqlens, accept_index, accept_lens)
        return cache
    if cache.layout != "frag":
        raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                         "config.attention.force_eager_fallback")
    ok, why = nn._pre_check_can_use_hip_attention(device=cache.device)
    if not ok:
        raise ValueError(why)
    Hkv, D = cache.shape[1], cache.shape[3]
    if torch.compiler.is_compiling():
        nn._ops().fp8_paged_kv_cache_compact_(cache.k, cache.v, cache.block_table, cache.seqlens, cu_seqlens, accept_index, accept_lens, Hkv, D,
                                              cache.num_pages, cache.page_size)
    else:
        # outside a trace: the op's own body, without the dispatcher's bookkeeping for a mutating op (as paged_kv_cache_append_varlen_fp8)
        _native.paged_kv_cache_compact_fp8(cache.k, cache.v, cache.block_table, cache.seqlens, cu_seqlens, accept_index, accept_lens, Hkv=Hkv,
                                           D=D, num_pages=cache.num_pages, page_size=cache.page_size)
    return cache

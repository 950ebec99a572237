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

On windowed layers and layers with learned sinks (gpt-oss, Mistral, Gemma-2/3, Phi-3; include/qattn_paged_varlen_tree_window.h, DESIGN.md
section 4.28) the attend is `fp8_attn_paged_varlen_tree_window_func(..., words, (127, 0), sinks=s)`, and with the rotary embedding the
drafts are rotated at the tree's positions, base + depth (include/qattn_paged_varlen_rope_pos.h), nothing read on the host:

    pos = tree_positions(words, cu, cache.seqlens)                                     # before the append: base_b + depth_p, siblings share one
    q = apply_rope_positions(q_draft, pos, cos, sin)
    paged_kv_cache_append_varlen_rope_pos_fp8(cache, k_draft, v_draft, cu, pos, cos, sin)
    out = fp8_attn_paged_varlen_tree_window_func(q, cache, cu, max_seqlen_q, words, (127, 0), sinks=s, max_seqlen_k=longest)

Package attributes, not names of `__all__`.  Not offered: a window with left < 63 under a tree (an ancestor could fall out of it); trees
above 64 tokens per slot (such a slot is plain causal, under a window the window entry's slot); a partial rotary_dim; multi-axis (M-RoPE)
positions; positions in the padded and the contiguous appends; the contiguous `KVCacheFP8`; masks for the dense, 16-bit and block-sparse
entries."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native, nn
from .paged import PagedKVCacheFP8, _cache_reason, _lens_reason
from .paged_varlen import _attend_varlen_eager, _resolve_varlen_splits, paged_varlen_attn_input_reason
from .sinks import _sinks_f32, sinks_input_reason
from .splitkv_window import _resolve_varlen_window_splits
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


def tree_positions(tree_mask: Tensor, cu_seqlens_q: Tensor, seqlens: Tensor, *, appended: bool = False) -> Tensor:
    """The rotary positions of a step's draft tokens -> int64 [total]: what `paged_kv_cache_append_varlen_rope_pos_fp8` and
    `apply_rope_positions` take.

    tree_mask: int64 [total], the step's words; cu_seqlens_q: int32 [B + 1]; seqlens: int32 [B], the cache's lengths -- BEFORE the step's
    append (appended=False) or after an advancing one (appended=True).  Token p of slot b gets base_b + depth_p with base_b =
    clamp(seqlens[b], 0) - (Sq_b if appended else 0) and, in a slot with 1 <= Sq_b <= 64, depth_p = popcount(w_p & (2^p - 1)): the set
    bits of its word below p, the depth `fp8_attn_paged_varlen_tree_window_func` places it at; in a longer slot depth_p = p.  Siblings
    share a position.  Tokens behind cu[B] get unspecified values.  Torch ops on the inputs' device, nothing read on the host."""
    if not isinstance(tree_mask, Tensor) or tree_mask.dtype != torch.int64 or tree_mask.dim() != 1:
        raise ValueError("Expected tree_mask to be a 1-D torch.int64 tensor [total]")
    if not isinstance(cu_seqlens_q, Tensor) or cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or cu_seqlens_q.shape[0] < 2:
        raise ValueError("Expected cu_seqlens_q to be a 1-D torch.int32 tensor [B + 1]")
    if not isinstance(seqlens, Tensor) or seqlens.dtype != torch.int32 or tuple(seqlens.shape) != (cu_seqlens_q.shape[0] - 1,):
        raise ValueError(f"Expected seqlens to be a torch.int32 tensor [{cu_seqlens_q.shape[0] - 1}]")
    if cu_seqlens_q.device != tree_mask.device or seqlens.device != tree_mask.device:
        raise ValueError(f"Expected cu_seqlens_q and seqlens to be on {tree_mask.device}")
    total = tree_mask.shape[0]
    if total == 0:
        return torch.zeros((0,), dtype=torch.int64, device=tree_mask.device)
    tok = torch.arange(total, device=tree_mask.device)
    cu = cu_seqlens_q.long().clamp(0, total)
    slot = (tok[:, None] >= cu[None, 1:]).sum(1).clamp(max=cu.shape[0] - 2)   # the slot that owns the token (tokens behind cu[B]: the last)
    start = cu[slot]
    n = (cu[slot + 1] - start).clamp(min=0)
    p = tok - start
    bit = torch.arange(TREE_MAX_TOKENS, device=tree_mask.device)
    below = ((tree_mask[:, None] >> bit) & 1).bool() & (bit[None, :] < p[:, None])   # (an arithmetic shift: the bits read are the word's)
    depth = torch.where(n <= TREE_MAX_TOKENS, below.sum(1), p)
    base = seqlens.long().clamp(min=0)[slot] - (n if appended else 0)
    return base + depth


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


TREE_WINDOW_MIN_LEFT = TREE_MAX_TOKENS - 1   # the least window_left >= 0 under a tree: every ancestor of a draft lies inside the window


def _tree_window_reason(window_size) -> Optional[str]:
    """Why window_size cannot be the window of a tree call, or None: (left, 0) with left = -1 or left >= 63."""
    ok = (isinstance(window_size, (tuple, list)) and len(window_size) == 2
          and all(isinstance(w, int) and not isinstance(w, bool) for w in window_size))
    if not ok:
        return f"window_size must be a pair of integers (left, right), got {window_size!r}"
    left, right = window_size
    if right != 0:
        return f"window_size[1] must be 0 under a draft tree (the tree is causal: a right window has no meaning), got {right}"
    if left != -1 and left < TREE_WINDOW_MIN_LEFT:
        return (f"window_size[0] must be -1 (unbounded) or >= {TREE_WINDOW_MIN_LEFT} under a draft tree, got {left}: a narrower window could "
                "cut an ancestor of a draft token, which is not offered")
    if left > 2 ** 31 - 1:
        return f"window_size[0] must fit a 32-bit integer, got {left}"
    return None


def paged_varlen_tree_window_input_reason(q, cache, cu_seqlens_q, max_seqlen_q, tree_mask, window_size, sinks=None, seqused_k=None, scale=None,
                                          num_splits=0, max_seqlen_k=None) -> Optional[str]:
    """The first rule the arguments of `fp8_attn_paged_varlen_tree_window_func` break, or None: `paged_varlen_tree_input_reason`, then
    window_size = (left, 0) with left = -1 or left >= 63, then -- if given -- sinks [Hq] fp32 / bf16 / fp16 on q's device
    (`sinks.sinks_input_reason`).  Shapes, dtypes, devices and strides only."""
    reason = paged_varlen_tree_input_reason(q, cache, cu_seqlens_q, max_seqlen_q, tree_mask, seqused_k, scale, num_splits, max_seqlen_k)
    if reason:
        return reason
    reason = _tree_window_reason(window_size)
    if reason:
        return reason
    if sinks is not None:
        return sinks_input_reason(sinks, q.shape[1], q.device)
    return None


def fp8_attn_paged_varlen_tree_window_func(q, cache: PagedKVCacheFP8, cu_seqlens_q: Tensor, max_seqlen_q: int, tree_mask: Tensor, window_size, *,
                                           sinks: Optional[Tensor] = None, scale: Optional[float] = None,
                                           seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, num_splits: int = 0,
                                           precision: str = "accurate", return_lse: bool = False, return_partials: bool = False):
    """`fp8_attn_paged_varlen_tree_func` on a WINDOWED layer and / or a layer with learned SINKS: the tree verify of gpt-oss, Mistral,
    Gemma-2/3 and Phi-3 layers (include/qattn_paged_varlen_tree_window.h).

    The arguments and outputs are those of `fp8_attn_paged_varlen_tree_func`, plus window_size = (left, right) and sinks: [Hq] fp32 / bf16
    / fp16 on the device, one logit per query head as `fp8_attn_paged_varlen_sink_func` takes them, or None.

        out = fp8_attn_paged_varlen_tree_window_func(q, cache, cu, max_q, words, (127, 0), sinks=s, max_seqlen_k=longest)   # gpt-oss, windowed
        out = fp8_attn_paged_varlen_tree_window_func(q, cache, cu, max_q, words, (-1, 0), sinks=s, max_seqlen_k=longest)    # gpt-oss, full

    Slot b has Sq_b queries and L_b keys, delta = L_b - Sq_b; w_p is the word of position p, unsigned.  In a slot with 1 <= Sq_b <= 64,
    depth_p = popcount(w_p & (2^p - 1)) -- the set bits below p; the self bit does not count -- and the query sits at sequence position
    delta + depth_p.  It attends key j iff the tree rule holds (j <= min(L_b - 1, p + delta), and for j >= max(delta, 0) bit j - delta of
    w_p is set) and, for left >= 0 and a committed key j < delta, j >= delta + depth_p - left.  Draft keys get no window test.  A slot
    with Sq_b > 64 reads no word: depth_p = p, and it is the window entry's slot.  Accepted windows: right == 0 and left == -1 or
    left >= 63 (every ancestor then lies inside the window: depths within a slot differ by at most 63; real windows are 127 and
    larger); anything else raises ValueError.  A row without a key is a zero row with LSE -inf, with a sink LSE sink_h.  With sinks,
    L = log(exp(sink_h) + sum_j exp(x_j)) as the sink entries define it: -inf is no sink, +inf and NaN poison their head alone, the
    byte-exponential sweep is never taken, and `return_partials` returns the sink-free partials:
    out, lse = merge_attn_states_with_sinks(list(po), list(plse), sinks, out_dtype=q.dtype), bit for bit.
    Bit for bit (out, lse, the partials; both precisions, every num_splits): left = -1 without sinks is `fp8_attn_paged_varlen_tree_func`;
    a chain is `fp8_attn_paged_varlen_window_func` under (left, 0), with sinks `fp8_attn_paged_varlen_sink_func`; every slot's rows are
    those of the call on that slot alone.  num_splits = 0 is the window entries' rule.
    Everything is read on the device: no host synchronisation, graph-capture safe, and a captured call follows the later contents of
    tree_mask, cu_seqlens_q, seqused_k, the table and sinks.  CPU tensors and config.attention.force_eager_fallback run the eager
    definition (`paged_varlen._attend_varlen_eager` with tree_mask=, window= and sinks=); on the device there is no fallback.
    Unsupported input raises ValueError(reason)."""
    if precision not in ("accurate", "fast"):
        raise ValueError(f"Unsupported precision: {precision!r} (expected 'accurate' or 'fast'; 'auto' is not offered by the split-KV entries)")
    reason = _tree_window_reason(window_size)   # (always: the kernels take no other window)
    if reason:
        raise ValueError(reason)
    if not checks.config_value("attention.skip_supported_check"):
        reason = paged_varlen_tree_window_input_reason(q, cache, cu_seqlens_q, max_seqlen_q, tree_mask, window_size, sinks, seqused_k, scale,
                                                       num_splits, max_seqlen_k)
        if reason:
            raise ValueError(reason)
    left, right = int(window_size[0]), int(window_size[1])
    total_q, Hq, D = q.shape
    B, Hkv = cache.batch_size, cache.shape[1]
    if sinks is not None:
        sinks = _sinks_f32(sinks, Hq, q.device)
    Skv = cache.capacity if max_seqlen_k is None else int(max_seqlen_k)
    used = cache.seqlens if seqused_k is None else seqused_k
    ns = _resolve_varlen_window_splits(num_splits, B, Hq, Hkv, total_q, int(max_seqlen_q), Skv, D, left, q.device)
    eager = (not q.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if cache.layout != "rowmajor":
            raise ValueError("the eager definition needs a cache made on a CPU device or under config.attention.force_eager_fallback")
        out, lse, po, plse, ppath = _attend_varlen_eager(q, cache, cu_seqlens_q, True, scale, used, Skv, ns, precision, tree_mask=tree_mask,
                                                         sinks=sinks, window=(left, right))
    else:
        if cache.layout != "frag":
            raise ValueError("this cache holds row-major bytes for the eager definition; make it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        out, lse, po, plse, ppath = nn._ops().fp8_paged_varlen_splitkv_tree_window_attention_forward(
            q, cache.k, cache.v, cache.scale_k, cache.scale_v, cache.block_table, used, cu_seqlens_q, tree_mask, int(max_seqlen_q), Skv,
            cache.num_pages, cache.page_size, ns, left, right, sinks, cache.fp8_format, cache.numerics, precision, bool(return_lse),
            bool(return_partials), scale=scale)
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

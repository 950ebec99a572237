"""What tests/test_cpu_mla_index_prefill.py and tests/test_gpu_mla_index_prefill.py share (include/qattn_mla_index_prefill.h), on top of
tests/mla_index_cases.py: packed token counts and key lengths that straddle the token tile, the key tile and the key range of the prefill
sweep, and the check both devices run -- the packed call against the dense entry on every slot's tokens (bit for bit) and against fp64."""
import numpy as np
import torch

import quantumattention_amd as qa
from quantumattention_amd import mla_index_prefill as P
from tests import mla_cases as C
from tests import mla_index_cases as X

TQ, KT, WGK = P.TOKENS, P.KEYS, P.WG_KEYS
CAP = WGK + KT + 70                               # the seam of two key ranges and a partial last key tile
# (token counts n_b, key lengths L_b) of the four slots
SHAPES = {
    # pure prefill | a chunk whose kends cross the first key-tile edge by +1 | an idle slot over live keys | one token over the whole cache
    "a": ((2 * TQ + 3, TQ, 0, 1), (2 * TQ + 3, KT + 1, 500, CAP)),
    # L < n: leading rows with kend 0 | kends ending one below the tile edge | kends across the key-range seam | an empty cache slot
    "b": ((TQ + 1, TQ - 1, 2 * TQ + 3, TQ), (3, KT - 1, WGK + 2, 0)),
}
TOTAL = max(sum(n) for n, _ in SHAPES.values()) + 5   # one token bucket for both: 5 or more rows behind cu[B] are padding
CASES = [("a", 64, 16, True, "e4m3", torch.bfloat16), ("b", 33, 1, True, "e4m3", torch.bfloat16), ("b", 64, 64, False, "e4m3", torch.bfloat16),
         ("a", 20, 64, False, "e5m2", torch.float16), ("b", 20, 16, True, "e4m3", torch.float16)]


def make_packed(shape, Hi, dtype, device, exact=True, seed=0):
    """(q [TOTAL, Hi, 128] -- a strided view --, weights [TOTAL, Hi], cu_seqlens_q int32 [B + 1])"""
    counts, total = SHAPES[shape][0], TOTAL
    q = X.make_q(Hi, total, dtype, seed=seed, exact=exact)[0].to(device).transpose(0, 1)
    w = (C.draw((total, Hi), 50 + seed) if exact else torch.randn((total, Hi), generator=torch.Generator().manual_seed(seed))).to(device)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=device)
    return q, w, cu


def check(shape, Hi, page, causal, fmt, dtype, device, exact=True, topk=24):
    """Returns the worst error / bound against fp64 (0 on exact inputs, where the logits must equal fp64 bit for bit)."""
    counts, lens = SHAPES[shape]
    icache = X.make_icache(page, lens, dtype, fmt, device, exact=exact, cap=CAP)
    q, w, cu = make_packed(shape, Hi, dtype, device, exact)
    idx, logits, q8, sq = qa.fp8_mla_index_topk_varlen_func(q, w, icache, cu, topk, causal=causal, max_seqlen_k=CAP, return_logits=True, return_q8=True)
    plain = qa.fp8_mla_index_topk_varlen_func(q, w, icache, cu, topk, causal=causal, max_seqlen_k=CAP)   # the rows in the workspace
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (q.shape[0], topk) and torch.equal(plain, idx)
    worst, lo = 0.0, 0
    for b, n in enumerate(counts):
        if n == 0:
            continue
        # the only form there was: the dense entry on the slot's tokens, Sq = n_b (every slot of the call gets them; row b counts)
        qd, wd = q[lo:lo + n].transpose(0, 1)[None].expand(X.B, -1, -1, -1), w[lo:lo + n][None].expand(X.B, -1, -1)
        d_idx, d_logits, d_q8, d_sq = qa.fp8_mla_index_topk_func(qd, wd, icache, topk, causal=causal, max_seqlen_k=CAP, return_logits=True, return_q8=True)
        rows = slice(lo, lo + n)
        what = (shape, Hi, page, causal, fmt, b)
        assert torch.equal(logits[rows].view(torch.int32), d_logits[b].view(torch.int32)), what          # -inf at j >= kend included
        assert torch.equal(idx[rows], d_idx[b]), what
        assert torch.equal(q8[rows].view(torch.uint8), d_q8[b].transpose(0, 1).view(torch.uint8)) and torch.equal(sq[rows], d_sq[b].t()), what
        # ... and a plain fp64 reference on the slot's tokens
        ref, bound = X.ref_logits(q8[rows].transpose(0, 1)[None].expand(X.B, -1, -1, -1), sq[rows].t()[None].expand(X.B, -1, -1), wd, icache, lens, causal, CAP)
        ref, bound, got = ref[b], bound[b], logits[rows].double().cpu().numpy()
        live = np.isfinite(ref)
        assert np.array_equal(np.isneginf(got), ~live), what
        if exact:
            assert np.array_equal(got[live], ref[live]), what
        elif live.any():
            worst = max(worst, float((np.abs(got[live] - ref[live]) / (256 * 2.0 ** -24 * bound[live])).max()))
        lo += n
    # the padded bucket: not read, kend 0
    assert (idx[lo:] == -1).all() and torch.isneginf(logits[lo:]).all() and not q8[lo:].view(torch.uint8).any() and not sq[lo:].any()
    return worst

#!/usr/bin/env python3
"""Time the two calls of tree-shaped speculative decoding on the paged FP8 K/V cache (include/qattn_paged_varlen_tree.h, DESIGN.md section
4.27) against what the library offered before them, in the same process.  As tools/time_paged_varlen_append.py (whose helpers this
imports): HIP events around blocks of `--iters` back-to-back replays of ONE captured graph per candidate, the candidates interleaved block
by block over `--rounds` rounds, median over the rounds, min .. max as the spread; ratios are taken within one run only.

Hq 32, Hkv 8, D 128, page size 128; shapes: 32 slots x 16 drafts over 8192 keys, 4 slots x 64 drafts over 32768 keys (the drafts are the
slots' last keys).
  (a) tree     fp8_attn_paged_varlen_tree_func under a binary tree against fp8_attn_paged_varlen_func(causal=True) on the same cache --
               the code of the parent commit.  The baseline is timed twice (first and last candidate): `causal_again_over_causal` and the
               min .. max spread over the rounds are the margin the ratio is held to.
  (b) compact  paged_kv_cache_compact_fp8 accepting 4 of the drafts of every slot, against the composition a caller needed before: keep the
               16-bit draft K / V, roll back (seqlens.sub_), index_select the accepted rows, paged_kv_cache_append_varlen_fp8.  Both end
               in the same cache state (checked before anything is timed); every call shortens the slots by the rejected drafts on both paths alike, and a reset
               outside the timed region puts the lengths back before each block."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import quantumattention_amd as qa  # noqa: E402
import time_kvcache as TK  # noqa: E402
import time_paged as TP  # noqa: E402
from quantumattention_amd import _native  # noqa: E402

DEV, BF16 = TK.DEV, TK.BF16
PAGE, HQ, HKV, D = 128, 32, 8, 128
SHAPES = {"b32_d16_k8192": (32, 16, 8192), "b4_d64_k32768": (4, 64, 32768)}   # slots, drafts per slot, keys per slot (drafts included)
ACCEPT = 4


def summarise(t, baseline, others):
    base = t[baseline]["median_ms"]
    s = {f"{baseline}_ms": base, f"{baseline}_spread_pct": TK.spread_pct(t[baseline]),
         f"{baseline}_again_over_{baseline}": t[baseline + "_again"]["median_ms"] / base}
    for k in others:
        s[f"{k}_ms"] = t[k]["median_ms"]
        s[f"{k}_spread_pct"] = TK.spread_pct(t[k])
        s[f"{k}_over_{baseline}"] = t[k]["median_ms"] / base
    return s


def measure(name, iters, rounds):
    B, n, Skv = SHAPES[name]
    total = B * n
    cc = qa.kv_cache_from_prefill_fp8(TK.rand(B, HKV, Skv - n, D), TK.rand(B, HKV, Skv - n, D), Skv + 256)
    c = TP.paged_from(cc, PAGE, "shuffled")
    del cc
    cu = torch.arange(0, total + 1, n, dtype=torch.int32, device=DEV)
    kd, vd, q = TK.rand(total, HKV, D), TK.rand(total, HKV, D), TK.rand(total, HQ, D)
    qa.paged_kv_cache_append_varlen_fp8(c, kd, vd, cu)                       # the drafts are the slots' last keys
    assert c.seqlens.tolist() == [Skv] * B
    parents = torch.tensor([(p - 1) // 2 if p else -1 for p in range(n)] * B, dtype=torch.int32, device=DEV)
    words = qa.tree_mask_from_parents(parents, cu)
    chain = qa.tree_mask_from_parents(torch.tensor(list(range(-1, n - 1)) * B, dtype=torch.int32, device=DEV), cu)
    causal = lambda: qa.fp8_attn_paged_varlen_func(q, c, cu, n, causal=True, max_seqlen_k=Skv)
    tree = lambda w: (lambda: qa.fp8_attn_paged_varlen_tree_func(q, c, cu, n, w, max_seqlen_k=Skv))
    assert torch.equal(causal(), tree(chain)())                              # the same bits under a chain, before anything is timed
    out = []
    cands, keep = {}, []
    for k, fn in (("causal", causal), ("tree", tree(words)), ("tree_chain", tree(chain)), ("causal_again", causal)):
        g, _ = TK.graph_of(fn)
        keep.append(g)
        cands[k] = ((lambda g: lambda i: g.replay())(g), TK.nothing)
    t = TK.timed(cands, iters, rounds)
    out.append({"measure": "tree_attention", "shape": name, "B": B, "drafts": n, "Skv": Skv, "Hq": HQ, "Hkv": HKV, "D": D, "page_size": PAGE,
                "iters": iters, "rounds": rounds, "times": t, "summary": summarise(t, "causal", ("tree", "tree_chain"))})

    # (b) the accepted path: the root, its first child and two later drafts of every slot
    path = [0, 1, n // 2, n - 1]
    assert len(path) == ACCEPT
    ai = torch.zeros(total, dtype=torch.int32, device=DEV)
    ai.view(B, n)[:, :ACCEPT] = torch.tensor(path, dtype=torch.int32, device=DEV)
    al = torch.full((B,), ACCEPT, dtype=torch.int32, device=DEV)
    rows = (torch.arange(B, device=DEV)[:, None] * n + torch.tensor(path, device=DEV)[None, :]).reshape(-1)
    cu4 = torch.arange(0, B * ACCEPT + 1, ACCEPT, dtype=torch.int32, device=DEV)

    def compact():
        qa.paged_kv_cache_compact_fp8(c, cu, ai, al)

    def reappend():
        c.seqlens.sub_(n)
        qa.paged_kv_cache_append_varlen_fp8(c, kd.index_select(0, rows), vd.index_select(0, rows), cu4)

    def fresh():                                                             # the drafts in place behind Skv - n committed keys
        c.seqlens.fill_(Skv - n)
        qa.paged_kv_cache_append_varlen_fp8(c, kd, vd, cu)

    states = []
    for fn in (compact, reappend):                                           # the same cache state either way, before anything is timed
        fresh()
        fn()
        states.append((c.k.clone(), c.v.clone(), c.seqlens.tolist()))
    assert states[0][2] == states[1][2] == [Skv - n + ACCEPT] * B
    assert torch.equal(states[0][0], states[1][0]) and torch.equal(states[0][1], states[1][1])
    del states
    fresh()
    # every call shortens the slots by n - ACCEPT keys, the same on both paths; the lengths go back to Skv before each block
    reset = lambda: c.seqlens.fill_(Skv)
    cands, keep = {}, []
    for k, fn in (("reappend", reappend), ("compact", compact), ("reappend_again", reappend)):
        reset()
        g, _ = TK.graph_of(fn)
        keep.append(g)
        cands[k] = ((lambda g: lambda i: g.replay())(g), reset)
    t = TK.timed(cands, iters, rounds)
    out.append({"measure": "tree_compaction", "shape": name, "B": B, "drafts": n, "accepted": ACCEPT, "Skv": Skv, "Hkv": HKV, "D": D,
                "page_size": PAGE, "iters": iters, "rounds": rounds, "workgroups": {"compact": 2 * B * HKV, "reappend": 2 * HKV * (2 * B + B * ACCEPT // 64)},
                "times": t, "summary": summarise(t, "reappend", ("compact",))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--only", default=",".join(SHAPES))
    args = ap.parse_args()
    assert args.rounds >= 1 and args.iters >= 1
    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    torch.manual_seed(0)
    for name in args.only.split(","):
        for r in measure(name, args.iters, args.rounds):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()

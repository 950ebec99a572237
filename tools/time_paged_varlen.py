#!/usr/bin/env python3
"""Time packed variable-length queries over the paged FP8 K/V cache (include/qattn_paged_varlen.h) against what a
caller of the dense paged entry can do, in the same process.  As tools/time_paged.py (whose helpers this imports): HIP events around
blocks of `--iters` back-to-back calls, the candidates interleaved block by block over `--rounds` rounds, median over the rounds, min ..
max as the spread; ratios are taken within one run only.  Attention calls only (no append), eager over `copies` cold copies of the pools
and as ONE replayed graph per candidate on the first copy.

  mixed step   Hq 32, Hkv 8, D 128, page size 128: one sequence with 512 queries over 8192 keys beside 31 sequences with 1 query over 8192
               keys, causal.  `varlen`: fp8_attn_paged_varlen_func on the 543 packed tokens.  `padded`: the only single-call form the dense
               entry has -- fp8_attn_paged_func on q [32, Hq, 512, D], every sequence's queries right-aligned (the bottom-right causal mask
               then fits; the padding rows are computed and thrown away).  `per_sequence`: 32 calls of fp8_attn_paged_func, one per sequence
               on a one-slot cache (the graph holds all 32).  All three with num_splits = 0 and the same max_seqlen_k.
  pure decode  all Sq_i = 1: B 1 / Skv 32768 and B 4 / Skv 8192.  `varlen` against `dense` = fp8_attn_paged_func on the same bytes; both
               pick the same split count.
  yardstick    the baseline of each comparison timed twice (first and last candidate): `<baseline>_again_over_<baseline>` and the min ..
               max spread over the rounds are the margin a ratio is held to"""
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
PAGE = 128


def paged_cache(B, Hkv, Skv, D, seed=0):
    """a paged cache of B sequences with Skv random keys each, pages shuffled"""
    cc = qa.kv_cache_from_prefill_fp8(TK.rand(B, Hkv, Skv, D), TK.rand(B, Hkv, Skv, D), Skv)
    return TP.paged_from(cc, PAGE, "shuffled", seed)


def one_slot(c, b):
    return qa.PagedKVCacheFP8(c.k, c.v, c.scale_k[b:b + 1].contiguous(), c.scale_v[b:b + 1].contiguous(), c.block_table[b:b + 1].contiguous(),
                              c.seqlens[b:b + 1].contiguous(), c.shape, c.fp8_format, c.dtype, c.numerics, c.layout)


def copies_of(first):
    set_bytes = 2 * first.k.numel()
    n = max(2, min(8, -(-2 * TK.LLC_BYTES // set_bytes)))
    return [first] + [TP.clone_paged(first) for _ in range(n - 1)]


def run(fams, baseline, iters, rounds):
    """fams: {name: fn(copy index)}; eager over the cold copies and one replayed graph (copy 0) per candidate, the baseline once more last"""
    cands, graphs = {}, []
    for k in list(fams) + [baseline + "_again"]:
        fn = fams[k.replace("_again", "")]
        cands[f"cold_{k}"] = ((lambda fn: lambda i: fn(i))(fn), TK.nothing)
        g, _ = TK.graph_of((lambda fn: lambda: fn(0))(fn))
        graphs.append(g)
        cands[f"graph_{k}"] = ((lambda g: lambda i: g.replay())(g), TK.nothing)
    t = TK.timed(cands, iters, rounds)
    summary = {}
    for kind in ("cold", "graph"):
        base = t[f"{kind}_{baseline}"]["median_ms"]
        summary[f"{kind}_{baseline}_ms"] = base
        summary[f"{kind}_{baseline}_spread_pct"] = TK.spread_pct(t[f"{kind}_{baseline}"])
        summary[f"{kind}_{baseline}_again_over_{baseline}"] = t[f"{kind}_{baseline}_again"]["median_ms"] / base
        for k in fams:
            if k != baseline:
                summary[f"{kind}_{k}_ms"] = t[f"{kind}_{k}"]["median_ms"]
                summary[f"{kind}_{k}_spread_pct"] = TK.spread_pct(t[f"{kind}_{k}"])
                summary[f"{kind}_{k}_over_{baseline}"] = t[f"{kind}_{k}"]["median_ms"] / base
    return t, summary


def mixed(iters, rounds):
    B, Hq, Hkv, D, Skv, big = 32, 32, 8, 128, 8192, 512
    sq = [big] + [1] * (B - 1)
    total = sum(sq)
    cs = copies_of(paged_cache(B, Hkv, Skv, D))
    n = len(cs)
    q = TK.rand(total, Hq, D)
    cu = torch.tensor([0] + torch.tensor(sq).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    cul = cu.tolist()
    padded = torch.zeros(B, Hq, big, D, dtype=BF16, device=DEV)
    for b in range(B):
        padded[b, :, big - sq[b]:] = q[cul[b]:cul[b + 1]].transpose(0, 1)
    alone = [q[cul[b]:cul[b + 1]].transpose(0, 1)[None].contiguous() for b in range(B)]
    slots = [[one_slot(c, b) for b in range(B)] for c in cs]
    fams = {
        "padded": lambda i: qa.fp8_attn_paged_func(padded, cs[i % n], causal=True, max_seqlen_k=Skv),
        "varlen": lambda i: qa.fp8_attn_paged_varlen_func(q, cs[i % n], cu, big, causal=True, max_seqlen_k=Skv),
        "per_sequence": lambda i: [qa.fp8_attn_paged_func(alone[b], slots[i % n][b], causal=True, max_seqlen_k=Skv) for b in range(B)],
    }
    # the same rows on every path, before anything is timed: bit for bit against the per-sequence calls; the padded call composes its
    # tiles differently (the rescale decision of the sweep is wave-wide), so its rows agree to rounding only
    # (with a split count fixed: num_splits = 0 picks another count for one sequence alone than for the batch)
    v = qa.fp8_attn_paged_varlen_func(q, cs[0], cu, big, causal=True, max_seqlen_k=Skv, num_splits=4)
    p = qa.fp8_attn_paged_func(padded, cs[0], causal=True, max_seqlen_k=Skv, num_splits=4)
    for b in range(B):
        rows = v[cul[b]:cul[b + 1]].transpose(0, 1)
        assert torch.equal(rows, qa.fp8_attn_paged_func(alone[b], slots[0][b], causal=True, max_seqlen_k=Skv, num_splits=4)[0]), b
        assert torch.allclose(rows.float(), p[b, :, big - sq[b]:].float(), atol=2.0 ** -6, rtol=2.0 ** -6), b
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    splits = {"varlen": _native.paged_varlen_auto_splits(B, Hq, Hkv, total, big, Skv, D, cus),
              "padded": _native.splitkv_auto_splits(B, Hq, Hkv, big, Skv, D, cus),
              "per_sequence_prefill": _native.splitkv_auto_splits(1, Hq, Hkv, big, Skv, D, cus),
              "per_sequence_decode": _native.splitkv_auto_splits(1, Hq, Hkv, 1, Skv, D, cus)}
    t, summary = run(fams, "padded", iters, rounds)
    return {"measure": "paged_varlen_mixed_step", "B": B, "Hq": Hq, "Hkv": Hkv, "Skv": Skv, "D": D, "page_size": PAGE, "queries": f"{big} + {B - 1} x 1",
            "copies": n, "iters": iters, "rounds": rounds, "num_splits": splits, "times": t, "summary": summary}


def decode(name, iters, rounds):
    B, Hq, Hkv, Skv, D = TK.DECODE[name]
    cs = copies_of(paged_cache(B, Hkv, Skv, D))
    n = len(cs)
    q = TK.rand(B, Hq, D)
    qd = q[:, :, None]
    cu = torch.arange(B + 1, dtype=torch.int32, device=DEV)
    fams = {
        "dense": lambda i: qa.fp8_attn_paged_func(qd, cs[i % n], causal=True, max_seqlen_k=Skv),
        "varlen": lambda i: qa.fp8_attn_paged_varlen_func(q, cs[i % n], cu, 1, causal=True, max_seqlen_k=Skv),
    }
    assert torch.equal(fams["varlen"](0), fams["dense"](0)[:, :, 0])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    splits = {"varlen": _native.paged_varlen_auto_splits(B, Hq, Hkv, B, 1, Skv, D, cus), "dense": _native.splitkv_auto_splits(B, Hq, Hkv, 1, Skv, D, cus)}
    t, summary = run(fams, "dense", iters, rounds)
    return {"measure": "paged_varlen_pure_decode", "shape": name, "B": B, "Hq": Hq, "Hkv": Hkv, "Skv": Skv, "D": D, "page_size": PAGE, "copies": n,
            "iters": iters, "rounds": rounds, "num_splits": splits, "times": t, "summary": summary}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--only", default="mixed,decode")
    args = ap.parse_args()
    assert args.rounds >= 1 and args.iters >= 1
    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    only = args.only.split(",")
    torch.manual_seed(0)
    if "mixed" in only:
        print(json.dumps(mixed(args.iters, args.rounds)), flush=True)
    if "decode" in only:
        for s in TK.DECODE:
            print(json.dumps(decode(s, args.iters, args.rounds)), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the packed variable-length append to the paged FP8 K/V cache (include/qattn_paged_varlen_append.h) against
what a caller of the padded append can do, in the same process.  As tools/time_paged_varlen.py (whose helpers this imports): HIP events
around blocks of `--iters` back-to-back calls, the candidates interleaved block by block over `--rounds` rounds, median over the rounds,
min .. max as the spread; ratios are taken within one run only; eager over `copies` cold copies of the pools and as ONE replayed graph per
candidate on the first copy.  Every call advances seqlens; a reset outside the timed region puts the lengths back before each block.

  mixed step   Hq 32, Hkv 8, D 128, page size 128, 8192 keys of history per slot: one slot appends 512 tokens, 31 slots one token each.  The
               tokens are the K and V slices of one packed projection tensor [543, (Hq + 2 Hkv), D].
               `packed`        paged_kv_cache_append_varlen_fp8 on the slices as they are.
               `pad_then_padded`  what a caller of the padded entry does: scatter the slices into [32, 512, Hkv, D] tensors (torch.empty +
                               index_copy_, the destination rows precomputed from cu_seqlens and not timed: generous to this baseline),
                               then paged_kv_cache_append_fp8(new_lens=).
               `padded_given`  that append alone, the padded tensors given for free.
  whole step   the three forms each followed by fp8_attn_paged_varlen_func on the query slice, as ONE replayed graph.
  pure decode  all counts 1: B 1 at 32768 keys and B 4 at 8192 keys.  `packed` against `padded` = paged_kv_cache_append_fp8 with T = 1 on
               [B, Hkv, 1, D] views of the same tensor (no copy, no new_lens).
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


def caches(B, Hkv, Skv, cap, D):
    """cold copies of a paged cache of B sequences with Skv random keys each and room for `cap`, pages shuffled"""
    cc = qa.kv_cache_from_prefill_fp8(TK.rand(B, Hkv, Skv, D), TK.rand(B, Hkv, Skv, D), cap)
    first = TP.paged_from(cc, PAGE, "shuffled")
    del cc
    n = max(2, min(8, -(-2 * TK.LLC_BYTES // (2 * first.k.numel()))))
    return [first] + [TP.clone_paged(first) for _ in range(n - 1)]


def run(fams, baseline, cs, Skv, iters, rounds, kinds=("cold", "graph")):
    """fams: {name: fn(cache)}; eager over the cold copies and one replayed graph (copy 0) per candidate, the baseline once more last"""
    n = len(cs)
    reset = lambda: [c.seqlens.fill_(Skv) for c in cs]
    cands, graphs = {}, []
    for k in list(fams) + [baseline + "_again"]:
        fn = fams[k.replace("_again", "")]
        reset()
        if "cold" in kinds:
            cands[f"cold_{k}"] = ((lambda fn: lambda i: fn(cs[i % n]))(fn), reset)
        if "graph" in kinds:
            g, _ = TK.graph_of((lambda fn: lambda: fn(cs[0]))(fn))
            graphs.append(g)
            cands[f"graph_{k}"] = ((lambda g: lambda i: g.replay())(g), reset)
    t = TK.timed(cands, iters, rounds)
    summary = {}
    for kind in kinds:
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


def same_state(a, b):
    return torch.equal(a.k, b.k) and torch.equal(a.v, b.v) and torch.equal(a.seqlens, b.seqlens)


def mixed(iters, rounds):
    B, Hq, Hkv, D, Skv, big = 32, 32, 8, 128, 8192, 512
    counts = [big] + [1] * (B - 1)
    total = sum(counts)
    cap = -(-(Skv + big * (iters + 4)) // 256) * 256
    cs = caches(B, Hkv, Skv, cap, D)
    qkv = TK.rand(total, Hq + 2 * Hkv, D)
    q, ks, vs = qkv[:, :Hq], qkv[:, Hq:Hq + Hkv], qkv[:, Hq + Hkv:]
    cul = [0] + torch.tensor(counts).cumsum(0).tolist()
    cu = torch.tensor(cul, dtype=torch.int32, device=DEV)
    nl = torch.tensor(counts, dtype=torch.int32, device=DEV)
    # token cu[b] + t -> row b big + t of the padded [B, big, Hkv, D] tensor
    dest = torch.cat([torch.arange(counts[b]) + b * big for b in range(B)]).to(DEV)

    def pad(x):
        p = torch.empty((B * big, Hkv, D), dtype=BF16, device=DEV)
        p.index_copy_(0, dest, x)
        return p.view(B, big, Hkv, D).transpose(1, 2)

    kp, vp = pad(ks), pad(vs)
    appends = {
        "padded_given": lambda c: qa.paged_kv_cache_append_fp8(c, kp, vp, new_lens=nl),
        "pad_then_padded": lambda c: qa.paged_kv_cache_append_fp8(c, pad(ks), pad(vs), new_lens=nl),
        "packed": lambda c: qa.paged_kv_cache_append_varlen_fp8(c, ks, vs, cu),
    }
    # the same bytes on every path, before anything is timed
    states = []
    for fn in appends.values():
        c = TP.clone_paged(cs[0])
        fn(c)
        states.append(c)
    assert same_state(states[0], states[1]) and same_state(states[0], states[2]) and states[0].seqlens.tolist() == [Skv + n for n in counts]
    del states
    t, summary = run(appends, "padded_given", cs, Skv, iters, rounds)
    out = [{"measure": "paged_varlen_append_mixed_step", "B": B, "Hq": Hq, "Hkv": Hkv, "Skv": Skv, "capacity": cap, "D": D, "page_size": PAGE,
            "tokens": f"{big} + {B - 1} x 1", "copies": len(cs), "iters": iters, "rounds": rounds,
            "workgroups": {"packed": 2 * Hkv * (2 * B + total // 64), "padded": 2 * B * Hkv * (-(-big // 64) + 1)}, "times": t, "summary": summary}]
    attend = lambda c: qa.fp8_attn_paged_varlen_func(q, c, cu, big, causal=True, max_seqlen_k=cap)
    steps = {k: (lambda fn: lambda c: (fn(c), attend(c))[1])(fn) for k, fn in appends.items()}
    t, summary = run(steps, "padded_given", cs, Skv, iters, rounds, kinds=("graph",))
    out.append({"measure": "paged_varlen_append_whole_step", "B": B, "Hq": Hq, "Hkv": Hkv, "Skv": Skv, "capacity": cap, "D": D, "page_size": PAGE,
                "tokens": f"{big} + {B - 1} x 1", "iters": iters, "rounds": rounds, "times": t, "summary": summary})
    return out


def decode(name, iters, rounds):
    B, Hq, Hkv, Skv, D = TK.DECODE[name]
    cap = -(-(Skv + 64 * (iters + 4)) // 256) * 256
    cs = caches(B, Hkv, Skv, cap, D)
    qkv = TK.rand(B, Hq + 2 * Hkv, D)
    ks, vs = qkv[:, Hq:Hq + Hkv], qkv[:, Hq + Hkv:]
    cu = torch.arange(B + 1, dtype=torch.int32, device=DEV)
    appends = {
        "padded": lambda c: qa.paged_kv_cache_append_fp8(c, ks[:, :, None], vs[:, :, None]),
        "packed": lambda c: qa.paged_kv_cache_append_varlen_fp8(c, ks, vs, cu),
    }
    a, b = TP.clone_paged(cs[0]), TP.clone_paged(cs[0])
    appends["padded"](a)
    appends["packed"](b)
    assert same_state(a, b) and a.seqlens.tolist() == [Skv + 1] * B
    del a, b
    t, summary = run(appends, "padded", cs, Skv, iters, rounds)
    return {"measure": "paged_varlen_append_pure_decode", "shape": name, "B": B, "Hq": Hq, "Hkv": Hkv, "Skv": Skv, "capacity": cap, "D": D,
            "page_size": PAGE, "copies": len(cs), "iters": iters, "rounds": rounds,
            "workgroups": {"packed": 2 * Hkv * 2 * B, "padded": 2 * B * Hkv * 2}, "times": t, "summary": summary}


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
        for r in mixed(args.iters, args.rounds):
            print(json.dumps(r), flush=True)
    if "decode" in only:
        for s in TK.DECODE:
            print(json.dumps(decode(s, args.iters, args.rounds)), flush=True)


if __name__ == "__main__":
    main()

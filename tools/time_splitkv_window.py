#!/usr/bin/env python3
"""Time sliding-window attention over the paged FP8 K/V cache (include/qattn_splitkv_window.h) against what a
caller had before and against the floor, in the same process.  As tools/time_paged.py (whose helpers this imports): HIP events around
blocks of `--iters` back-to-back calls, the candidates interleaved block by block over `--rounds` rounds, median over the rounds, min ..
max as the spread; ratios are taken within one run only; eager over `copies` cold copies of the pools, and as ONE replayed graph per
candidate on the first copy.  The code under test is never its own baseline.

  decode step  "append T = 1, then attend (num_splits = 0)", page size 128: B 1 / Hq 32 / Hkv 8 / 32768 keys under (4095, 0) and B 4 / 8192 keys
               under (1023, 0).
  mixed step   tools/time_paged_varlen.py's: one sequence with 512 queries beside 31 with one, 8192 keys each, under (4095, 0); attention only.
  window       the window entry on the full cache
  causal       (a) the sibling with causal=True on the same cache: what a caller had to run before (the wrong result for such a layer, and
               every key streamed).  The window call must not be slower than this beyond its own spread.
  floor        (b) the sibling with causal=True on a cache that holds ONLY the window's keys (left + Sq per sequence): the least a window
               call could cost.  Its expected excess over this: one partly masked chunk step per workgroup, and the full cache's table.
  yardstick    `causal` timed twice (first and last candidate): `causal_again_over_causal` and the min .. max spreads are the margin"""
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
WINDOW = {"decode_b1": (4095, 0), "decode_b4": (1023, 0)}


def copies_of(first, most=8):
    n = max(2, min(most, -(-2 * TK.LLC_BYTES // (2 * first.k.numel()))))
    return [first] + [TP.clone_paged(first) for _ in range(n - 1)]


def summarise(t, names):
    summary = {}
    for kind in ("cold", "graph"):
        base = t[f"{kind}_causal"]["median_ms"]
        summary[f"{kind}_causal_again_over_causal"] = t[f"{kind}_causal_again"]["median_ms"] / base
        for k in names:
            summary[f"{kind}_{k}_ms"] = t[f"{kind}_{k}"]["median_ms"]
            summary[f"{kind}_{k}_spread_pct"] = TK.spread_pct(t[f"{kind}_{k}"])
        summary[f"{kind}_window_over_causal"] = t[f"{kind}_window"]["median_ms"] / base
        summary[f"{kind}_window_over_floor"] = t[f"{kind}_window"]["median_ms"] / t[f"{kind}_floor"]["median_ms"]
    return summary


def decode(name, iters, rounds):
    B, Hq, Hkv, Skv, D = TK.DECODE[name]
    window = WINDOW[name]
    grow = 64 * (iters + 4)
    cap = -(-(Skv + grow) // 256) * 256
    few = window[0]                                        # the floor's cache: after the append it holds left + 1 keys, the query's whole window
    cap_f = -(-(few + grow) // 256) * 256
    q, kn, vn = TK.rand(B, Hq, 1, D), TK.rand(B, Hkv, 1, D), TK.rand(B, Hkv, 1, D)
    full = copies_of(TP.paged_from(qa.kv_cache_from_prefill_fp8(TK.rand(B, Hkv, Skv, D), TK.rand(B, Hkv, Skv, D), cap), PAGE, "shuffled"))
    floor = copies_of(TP.paged_from(qa.kv_cache_from_prefill_fp8(TK.rand(B, Hkv, few, D), TK.rand(B, Hkv, few, D), cap_f), PAGE, "shuffled"),
                      most=len(full))

    def step(attend):
        def f(c):
            qa.paged_kv_cache_append_fp8(c, kn, vn)
            return attend(c)
        return f

    fams = {
        "causal": (full, Skv, step(lambda c: qa.fp8_attn_paged_func(q, c, causal=True, max_seqlen_k=cap))),
        "window": (full, Skv, step(lambda c: qa.fp8_attn_paged_window_func(q, c, window, max_seqlen_k=cap))),
        "floor": (floor, few, step(lambda c: qa.fp8_attn_paged_func(q, c, causal=True, max_seqlen_k=cap_f))),
    }
    cands, graphs = {}, []
    for k in list(fams) + ["causal_again"]:
        cs, start, fn = fams[k.replace("_again", "")]
        reset = (lambda cs, start: lambda: [c.seqlens.fill_(start) for c in cs])(cs, start)
        reset()
        assert torch.isfinite(fn(cs[0]).float()).all(), k
        reset()
        cands[f"cold_{k}"] = ((lambda cs, fn: lambda i: fn(cs[i % len(cs)]))(cs, fn), reset)
        g, _ = TK.graph_of((lambda c, fn: lambda: fn(c))(cs[0], fn))
        graphs.append(g)
        cands[f"graph_{k}"] = ((lambda g: lambda i: g.replay())(g), reset)
    t = TK.timed(cands, iters, rounds)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    splits = {"causal": _native.splitkv_auto_splits(B, Hq, Hkv, 1, cap, D, cus),
              "window": _native.splitkv_window_auto_splits(B, Hq, Hkv, 1, cap, D, window[0], cus),
              "floor": _native.splitkv_auto_splits(B, Hq, Hkv, 1, cap_f, D, cus)}
    return {"measure": "window_decode_step", "shape": name, "B": B, "Hq": Hq, "Hkv": Hkv, "Skv": Skv, "D": D, "window": window, "page_size": PAGE,
            "copies": len(full), "iters": iters, "rounds": rounds, "num_splits": splits, "times": t, "summary": summarise(t, list(fams))}


def mixed(iters, rounds):
    B, Hq, Hkv, D, Skv, big, window = 32, 32, 8, 128, 8192, 512, (4095, 0)
    sq = [big] + [1] * (B - 1)
    total = sum(sq)
    few = -(-(window[0] + big) // PAGE) * PAGE             # the floor's cache: every sequence holds left + Sq_i keys
    mk = lambda S: TP.paged_from(qa.kv_cache_from_prefill_fp8(TK.rand(B, Hkv, S, D), TK.rand(B, Hkv, S, D), S), PAGE, "shuffled")
    full = copies_of(mk(Skv))
    first = mk(few)
    first.seqlens.copy_(torch.tensor([window[0] + n for n in sq], dtype=torch.int32, device=DEV))
    floor = copies_of(first, most=len(full))
    q = TK.rand(total, Hq, D)
    cu = torch.tensor([0] + torch.tensor(sq).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    fams = {
        "causal": (full, lambda c: qa.fp8_attn_paged_varlen_func(q, c, cu, big, causal=True, max_seqlen_k=Skv)),
        "window": (full, lambda c: qa.fp8_attn_paged_varlen_window_func(q, c, cu, big, window, max_seqlen_k=Skv)),
        "floor": (floor, lambda c: qa.fp8_attn_paged_varlen_func(q, c, cu, big, causal=True, max_seqlen_k=few)),
    }
    cands, graphs = {}, []
    for k in list(fams) + ["causal_again"]:
        cs, fn = fams[k.replace("_again", "")]
        assert torch.isfinite(fn(cs[0]).float()).all(), k
        cands[f"cold_{k}"] = ((lambda cs, fn: lambda i: fn(cs[i % len(cs)]))(cs, fn), TK.nothing)
        g, _ = TK.graph_of((lambda c, fn: lambda: fn(c))(cs[0], fn))
        graphs.append(g)
        cands[f"graph_{k}"] = ((lambda g: lambda i: g.replay())(g), TK.nothing)
    t = TK.timed(cands, iters, rounds)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    splits = {"causal": _native.paged_varlen_auto_splits(B, Hq, Hkv, total, big, Skv, D, cus),
              "window": _native.paged_varlen_window_auto_splits(B, Hq, Hkv, total, big, Skv, D, window[0], cus),
              "floor": _native.paged_varlen_auto_splits(B, Hq, Hkv, total, big, few, D, cus)}
    return {"measure": "window_mixed_step", "B": B, "Hq": Hq, "Hkv": Hkv, "Skv": Skv, "D": D, "window": window, "page_size": PAGE,
            "queries": f"{big} + {B - 1} x 1", "copies": len(full), "iters": iters, "rounds": rounds, "num_splits": splits, "times": t,
            "summary": summarise(t, list(fams))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--only", default="decode,mixed")
    args = ap.parse_args()
    assert args.rounds >= 1 and args.iters >= 1
    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    only = args.only.split(",")
    torch.manual_seed(0)
    if "decode" in only:
        for s in TK.DECODE:
            print(json.dumps(decode(s, args.iters, args.rounds)), flush=True)
    if "mixed" in only:
        print(json.dumps(mixed(args.iters, args.rounds)), flush=True)


if __name__ == "__main__":
    main()

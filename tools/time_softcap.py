#!/usr/bin/env python3
"""Time the soft-cap entries (include/qattn_softcap.h) against their window siblings on the same cache, in the same
process.  As tools/time_sinks.py (whose helpers this shares): HIP events around blocks of `--iters` back-to-back replays of ONE captured
graph per candidate, the candidates interleaved block by block over `--rounds` rounds, median over the rounds, min .. max as the spread;
ratios are taken within one run only.  The code under test is never its own baseline.

  layers       Gemma-2 9B (Hq 16, Hkv 8, D 256, scale 256^-0.5) and 27B (Hq 32, Hkv 16, D 128, scale 144^-0.5), softcap 50, under
               (4095, 0) -- a window layer -- and (-1, 0) -- a full layer.
  decode step  "append T = 1, then attend (num_splits = 0)", page size 128: B 1 / 32768 keys and B 4 / 8192 keys.
  mixed step   one sequence with 512 queries beside 31 with one, 8192 keys each; attention only.
  window       the window call without a cap on the same cache: the parent's code, instruction for instruction.  THE BASELINE; timed twice
               (first and last candidate): `window_again_over_window` and the min .. max spreads are the margin.
  softcap      the soft-cap entry."""
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

DEV = TK.DEV
PAGE = 128
SOFTCAP = 50.0
LAYERS = {"gemma2_9b": (16, 8, 256, 256.0 ** -0.5), "gemma2_27b": (32, 16, 128, 144.0 ** -0.5)}
DECODE = {"decode_b1": (1, 32768), "decode_b4": (4, 8192)}
WINDOWS = ((4095, 0), (-1, 0))
NAMES = ("window", "softcap")


def summarise(t):
    base = t["graph_window"]["median_ms"]
    s = {"window_again_over_window": t["graph_window_again"]["median_ms"] / base}
    for k in NAMES:
        s[f"{k}_ms"] = t[f"graph_{k}"]["median_ms"]
        s[f"{k}_spread_pct"] = TK.spread_pct(t[f"graph_{k}"])
    s["softcap_over_window"] = t["graph_softcap"]["median_ms"] / base
    return s


def run(fams, reset, iters, rounds):
    cands, graphs = {}, []
    for k in list(NAMES) + ["window_again"]:
        fn = fams[k.replace("_again", "")]
        reset()
        assert torch.isfinite(fn().float()).all(), k
        reset()
        g, _ = TK.graph_of(fn)
        graphs.append(g)
        cands[f"graph_{k}"] = ((lambda g: lambda i: g.replay())(g), reset)
    return TK.timed(cands, iters, rounds)


def decode(layer, name, window, iters, rounds):
    HQ, HKV, D, scale = LAYERS[layer]
    B, Skv = DECODE[name]
    cap = -(-(Skv + 64 * (iters + 4)) // 256) * 256
    q, kn, vn = TK.rand(B, HQ, 1, D), TK.rand(B, HKV, 1, D), TK.rand(B, HKV, 1, D)
    c = TP.paged_from(qa.kv_cache_from_prefill_fp8(TK.rand(B, HKV, Skv, D), TK.rand(B, HKV, Skv, D), cap), PAGE, "shuffled")

    def step(attend):
        def f():
            qa.paged_kv_cache_append_fp8(c, kn, vn)
            return attend()
        return f

    fams = {"window": step(lambda: qa.fp8_attn_paged_window_func(q, c, window, scale=scale, max_seqlen_k=cap)),
            "softcap": step(lambda: qa.fp8_attn_paged_softcap_func(q, c, SOFTCAP, window, scale=scale, max_seqlen_k=cap))}
    t = run(fams, lambda: c.seqlens.fill_(Skv), iters, rounds)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {"measure": "softcap_decode_step", "layer": layer, "shape": name, "B": B, "Hq": HQ, "Hkv": HKV, "Skv": Skv, "D": D, "window": window,
            "softcap": SOFTCAP, "page_size": PAGE, "iters": iters, "rounds": rounds,
            "num_splits": _native.splitkv_window_auto_splits(B, HQ, HKV, 1, cap, D, window[0], cus), "times": t, "summary": summarise(t)}


def mixed(layer, window, iters, rounds):
    HQ, HKV, D, scale = LAYERS[layer]
    B, Skv, big = 32, 8192, 512
    sq = [big] + [1] * (B - 1)
    total = sum(sq)
    c = TP.paged_from(qa.kv_cache_from_prefill_fp8(TK.rand(B, HKV, Skv, D), TK.rand(B, HKV, Skv, D), Skv), PAGE, "shuffled")
    q = TK.rand(total, HQ, D)
    cu = torch.tensor([0] + torch.tensor(sq).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    fams = {"window": lambda: qa.fp8_attn_paged_varlen_window_func(q, c, cu, big, window, scale=scale, max_seqlen_k=Skv),
            "softcap": lambda: qa.fp8_attn_paged_varlen_softcap_func(q, c, cu, big, SOFTCAP, window, scale=scale, max_seqlen_k=Skv)}
    t = run(fams, TK.nothing, iters, rounds)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {"measure": "softcap_mixed_step", "layer": layer, "B": B, "Hq": HQ, "Hkv": HKV, "Skv": Skv, "D": D, "window": window,
            "softcap": SOFTCAP, "page_size": PAGE, "queries": f"{big} + {B - 1} x 1", "iters": iters, "rounds": rounds,
            "num_splits": _native.paged_varlen_window_auto_splits(B, HQ, HKV, total, big, Skv, D, window[0], cus), "times": t,
            "summary": summarise(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--only", default="decode,mixed")
    ap.add_argument("--layers", default=",".join(LAYERS))
    args = ap.parse_args()
    assert args.rounds >= 1 and args.iters >= 1
    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    only = args.only.split(",")
    torch.manual_seed(0)
    for layer in args.layers.split(","):
        for window in WINDOWS:
            if "decode" in only:
                for s in DECODE:
                    print(json.dumps(decode(layer, s, window, args.iters, args.rounds)), flush=True)
            if "mixed" in only:
                print(json.dumps(mixed(layer, window, args.iters, args.rounds)), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time split-KV attention over prepared K / V (include/qattn_splitkv.h) against what a caller has today, in the same
process.  Times are HIP events around blocks of `--iters` back-to-back calls, the candidates interleaved block by block over `--rounds`
rounds (>= 16), median over the rounds (clock and thermal drift hit all alike); min .. max over the rounds is printed as the spread, and
one candidate is listed twice (`auto_again`) so that the run-to-run spread of equal work shows.

Per shape:
  (i)    dense        fp8_attn_func on 16-bit k, v (the fused step: quantises K / V every call)
  (ii)   block_sparse fp8_block_sparse_attn_pv_func(pv_precision="fp8") with an all-true mask (quantises K / V every call)
  (iii)  pair         fp8_attn_splitkv_func on a (k, v) pair, num_splits = auto (prepares K / V every call)
  (iv)   ns1          fp8_attn_splitkv_func on prepared K / V, num_splits = 1
  (v)    auto         ... num_splits = 0 (the rule's choice is printed)
  (vi)   ns<N>        ... num_splits over {1, 2, 4, 8, 16, 32, 64}
and, on ONE set of buffers (cache-warm), (iv) and (v) eager and replayed from a captured graph (`hot_*`).

Cold by default: the calls of a block walk round-robin through `copies` distinct K / V sets sized to exceed the chip's 256 MiB last-level
cache (a decode step walks through its layers' caches the same way); --copies 1 times the cache-warm case.
Next to each shape: the byte floor = prepared K + V bytes / the device-to-device copy rate measured in this run (bytes read + written per
second on a buffer larger than the last-level cache)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import quantumattention_amd as qa  # noqa: E402
from quantumattention_amd import _native  # noqa: E402

SHAPES = {   # B, Hq, Hkv, Sq, Skv, D
    "decode_b1": (1, 32, 8, 1, 32768, 128),
    "decode_b4": (4, 32, 8, 1, 8192, 128),
    "chunk8": (1, 32, 8, 8, 32768, 128),
    "wan_sq64": (1, 40, 40, 64, 32760, 128),
    "c2": (4, 32, 32, 4096, 4096, 128),
}
SWEEP = (1, 2, 4, 8, 16, 32, 64)
LLC_BYTES = 256 << 20


def block_ms(fns, iters, rounds, warmup=2):
    """fns: callables of the call's index within the run (round-robin over the K / V copies)"""
    n = 0
    for fn in fns:
        for _ in range(warmup):
            fn(n)
            n += 1
    torch.cuda.synchronize()
    laps = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn(n)
                n += 1
            e1.record()
            laps[i].append((e0, e1))
    torch.cuda.synchronize()
    times = [sorted(a.elapsed_time(b) / iters for a, b in lap) for lap in laps]
    return [{"median_ms": t[rounds // 2], "min_ms": t[0], "max_ms": t[-1]} for t in times]


def copy_rate(iters, rounds):
    """bytes moved (read + written) per second by a device-to-device copy of 1 GiB"""
    n = 1 << 30
    a, b = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    a.zero_()
    t = block_ms([lambda i: b.copy_(a)], iters, rounds)[0]
    return 2.0 * n / (t["median_ms"] * 1e-3), t


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def run_shape(name, iters, rounds, copies, rate):
    B, Hq, Hkv, Sq, Skv, D = SHAPES[name]
    torch.manual_seed(0)
    dev = "cuda"
    q = torch.randn(B, Hq, Sq, D, dtype=torch.bfloat16, device=dev)
    kv_bytes = 2 * B * Hkv * ((Skv + 63) // 64 * 64) * D
    if copies <= 0:   # enough sets that the 16-bit K / V of consecutive calls cannot stay in the last-level cache (at least 2, at most 16)
        copies = max(2, min(16, -(-2 * LLC_BYTES // kv_bytes)))
    sets = []
    for _ in range(copies):
        k, v = (torch.randn(B, Hkv, Skv, D, dtype=torch.bfloat16, device=dev) for _ in range(2))
        sets.append((k, v, qa.prepare_kv_fp8(k, v)))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    auto = _native.splitkv_auto_splits(B, Hq, Hkv, Sq, Skv, D, cus)
    G = Hq // Hkv
    tiles = B * Hkv * -(-G * Sq // 128)
    mask = torch.ones(1, 1, -(-Sq // 128), -(-Skv // 128), dtype=torch.bool, device=dev)
    pick = lambda i: sets[i % copies]
    fns = {
        "dense": lambda i: qa.fp8_attn_func(q, *pick(i)[:2]),
        "block_sparse": lambda i: qa.fp8_block_sparse_attn_pv_func(q, *pick(i)[:2], mask, pv_precision="fp8", precision="accurate"),
        "pair": lambda i: qa.fp8_attn_splitkv_func(q, pick(i)[:2]),
        "ns1": lambda i: qa.fp8_attn_splitkv_func(q, pick(i)[2], num_splits=1),
        "auto": lambda i: qa.fp8_attn_splitkv_func(q, pick(i)[2]),
    }
    # the pre-passes alone, for attention-only estimates by subtraction: (ii) - quant_q - quant_kv against (iv) - quant_q
    fns["quant_q"] = lambda i: _native.quant_fp8(q, scaling="head-wise")
    fns["quant_kv"] = lambda i: (_native.quant_fp8(pick(i)[0], scaling="head-wise", layout=_native.LAYOUT_KFRAG),
                                 _native.quant_fp8(pick(i)[1], scaling="head-wise", layout=_native.LAYOUT_VFRAG))
    sweep_ns = [n for n in SWEEP if n * B * Hq * Sq * D * 4 <= (2 << 30)]   # (the fp32 partials of a call: at most 2 GiB)
    for n in sweep_ns:
        if n > 1:
            fns[f"ns{n}"] = (lambda n: lambda i: qa.fp8_attn_splitkv_func(q, pick(i)[2], num_splits=n))(n)
    fns["auto_again"] = fns["auto"]
    # cache-warm, eager and replayed from a captured graph
    kv0 = sets[0][2]
    g1, _ = graph_of(lambda: qa.fp8_attn_splitkv_func(q, kv0, num_splits=1))
    ga, _ = graph_of(lambda: qa.fp8_attn_splitkv_func(q, kv0))
    fns["hot_ns1"] = lambda i: qa.fp8_attn_splitkv_func(q, kv0, num_splits=1)
    fns["hot_auto"] = lambda i: qa.fp8_attn_splitkv_func(q, kv0)
    fns["hot_ns1_graph"] = lambda i: g1.replay()
    fns["hot_auto_graph"] = lambda i: ga.replay()
    # faster and different is not faster: the split result against the one-split result on the same inputs
    a, b = qa.fp8_attn_splitkv_func(q, kv0, num_splits=1).float(), qa.fp8_attn_splitkv_func(q, kv0).float()
    skipped = {}
    for k_ in list(fns):   # a candidate that refuses the shape is named, not timed
        try:
            fns[k_](0)
        except (ValueError, RuntimeError) as ex:
            skipped[k_] = f"{type(ex).__name__}: {str(ex)[:160]}"
            del fns[k_]
    torch.cuda.synchronize()
    t = block_ms(list(fns.values()), iters, rounds)
    res = {"skipped": skipped, "shape": name, "B": B, "Hq": Hq, "Hkv": Hkv, "Sq": Sq, "Skv": Skv, "D": D, "iters": iters, "rounds": rounds, "copies": copies,
           "cus": cus, "unsplit_workgroups": tiles, "auto_splits": auto, "prepared_kv_mbytes": kv_bytes / 1e6,
           "byte_floor_ms": kv_bytes / rate * 1e3, "max_abs_auto_vs_ns1": float((a - b).abs().max()),
           "launches": {"ns1": "quant of q + 1 sweep", "auto": "quant of q + 1 sweep" + ("" if auto == 1 else f" + {1 if auto <= 8 else 1 + -(-(auto - 8) // 7)} merge")}}
    res["times"] = dict(zip(fns, t))
    m = lambda k: res["times"][k]["median_ms"] if k in res["times"] else float("nan")
    sweep = {n: m("ns1" if n == 1 else f"ns{n}") for n in sweep_ns}
    best = min(sweep, key=sweep.get)
    res["summary"] = {
        "auto_over_ns1": m("auto") / m("ns1"), "auto_over_block_sparse": m("auto") / m("block_sparse"), "auto_over_dense": m("auto") / m("dense"),
        "auto_over_floor": m("auto") / res["byte_floor_ms"], "best_ns": best, "best_ms": sweep[best], "auto_over_best": m("auto") / sweep[best],
        "auto_again_over_auto": m("auto_again") / m("auto"),
        "auto_spread_pct": (res["times"]["auto"]["max_ms"] / res["times"]["auto"]["min_ms"] - 1.0) * 100.0,
        "block_sparse_attention_only_ms": m("block_sparse") - m("quant_q") - m("quant_kv"), "ns1_attention_only_ms": m("ns1") - m("quant_q"),
        "auto_attention_only_ms": m("auto") - m("quant_q"),
        "hot_graph_over_eager_ns1": m("hot_ns1_graph") / m("hot_ns1"), "hot_graph_over_eager_auto": m("hot_auto_graph") / m("hot_auto"),
    }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--copies", type=int, default=0, help="distinct K / V sets walked round-robin (0: enough to exceed the last-level cache; 1: cache-warm)")
    args = ap.parse_args()
    assert args.rounds >= 1 and args.iters >= 1
    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    rate, t = copy_rate(args.iters, args.rounds)
    print(json.dumps({"copy_1GiB": t, "bytes_moved_per_s": rate}), flush=True)
    for s in args.shapes.split(","):
        print(json.dumps(run_shape(s, args.iters, args.rounds, args.copies, rate)), flush=True)


if __name__ == "__main__":
    main()

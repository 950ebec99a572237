#!/usr/bin/env python3
"""Time the appendable FP8 K/V cache (include/qattn_kvcache.h) against what a caller had before it, in the same
process.  As tools/time_splitkv.py: HIP events around blocks of `--iters` back-to-back calls, the candidates interleaved block by block over
`--rounds` rounds (>= 16), median over the rounds, min .. max printed as the spread; ratios are taken within one run only.

  (i)   decode step   "append T = 1, then fp8_attn_splitkv_func(causal, seqused_k = cache.seqlens)" against "prepare_kv_fp8 of the whole K / V,
                      then the same attention call" (the parent's only way to add a key), eager over `copies` cold K / V sets, and eager
                      and as ONE replayed graph on one warm set
  (ii)  append alone  T = 1, 8, 64 against its launch floor: the same call with new_lens = 0 -- the same two launches, every workgroup
                      exits after reading its two lengths (the library ships no empty kernel); and at T = 1 the host's path three ways:
                      the function, the ctypes binding alone, the torch.library op
  (iii) prefill       one append of T tokens into an empty cache, and kv_cache_from_prefill_fp8 (scales + zero-filled images + that append),
                      against prepare_kv_fp8 on the same tensors: eager over cold sets, and as replayed graphs on one set (device time
                      without the host's launch path)
  (iv)  views         appending the transposed view of a [B, T, H, D] tensor against appending its .contiguous() copy, copy included

Before a timed block seqlens is reset (one tiny fill per block of `iters` calls, outside the timed region), so the cache does not run
full, and the device is drained: an eager figure is the larger of the host's launch path and the device's work, a graph figure the device's."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import quantumattention_amd as qa  # noqa: E402
from quantumattention_amd import _native  # noqa: E402

DECODE = {"decode_b1": (1, 32, 8, 32768, 128), "decode_b4": (4, 32, 8, 8192, 128)}   # B, Hq, Hkv, Skv, D
PREFILL = {"prefill_b4_t4096": (4, 8, 4096, 128), "prefill_b1_t32768": (1, 8, 32768, 128)}   # B, Hkv, T, D
LLC_BYTES = 256 << 20
DEV = "cuda"
BF16 = torch.bfloat16


def block_ms(fns, resets, iters, rounds, warmup=2):
    """fns: callables of the call's running index; resets[i]: called before each block of fns[i], outside the timed region.  Every block
    starts on an idle device (these calls are tens of microseconds: behind a backlog a block would show device time, on an idle device the
    larger of host and device time -- the order of the candidates would decide which)"""
    n = 0
    for fn, rs in zip(fns, resets):
        rs()
        for _ in range(warmup):
            fn(n)
            n += 1
    torch.cuda.synchronize()
    laps = [[] for _ in fns]
    for _ in range(rounds):
        for i, (fn, rs) in enumerate(zip(fns, resets)):
            rs()
            torch.cuda.synchronize()
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


def timed(cands, iters, rounds):
    """cands: {name: (fn, reset)} -> {name: times}"""
    names = list(cands)
    t = block_ms([cands[k][0] for k in names], [cands[k][1] for k in names], iters, rounds)
    return dict(zip(names, t))


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


def rand(*shape):
    return torch.randn(*shape, dtype=BF16, device=DEV)


def nothing():
    pass


def spread_pct(t):
    return (t["max_ms"] / t["min_ms"] - 1.0) * 100.0


def decode(name, iters, rounds):
    B, Hq, Hkv, Skv, D = DECODE[name]
    cap = Skv + 64 * (iters + 4)
    set_bytes = 2 * 2 * B * Hkv * Skv * D
    copies = max(2, min(8, -(-2 * LLC_BYTES // set_bytes)))
    q, kn, vn = rand(B, Hq, 1, D), rand(B, Hkv, 1, D), rand(B, Hkv, 1, D)
    sets = []
    for _ in range(copies):
        k, v = rand(B, Hkv, Skv + 1, D), rand(B, Hkv, Skv + 1, D)          # the parent's caller holds the 16-bit K / V, the new key included
        sets.append((k, v, qa.kv_cache_from_prefill_fp8(k[:, :, :Skv], v[:, :, :Skv], cap)))
    attend = lambda kv, su: qa.fp8_attn_splitkv_func(q, kv, causal=True, seqused_k=su)

    def step_new(c):
        qa.kv_cache_append_fp8(c, kn, vn)
        return attend(c, c.seqlens)

    def step_old(k, v):
        return attend(qa.prepare_kv_fp8(k, v), None)

    def reset_all():
        for s in sets:
            s[2].seqlens.fill_(Skv)

    c0, k0, v0 = sets[0][2], sets[0][0], sets[0][1]
    reset0 = lambda: c0.seqlens.fill_(Skv)
    reset0()
    g_new, _ = graph_of(lambda: step_new(c0))
    g_old, _ = graph_of(lambda: step_old(k0, v0))
    cands = {
        "cold_new": (lambda i: step_new(sets[i % copies][2]), reset_all),
        "cold_reprepare": (lambda i: step_old(*sets[i % copies][:2]), nothing),
        "cold_attention_only": (lambda i: attend(sets[i % copies][2], sets[i % copies][2].seqlens), reset_all),
        "hot_new": (lambda i: step_new(c0), reset0),
        "hot_reprepare": (lambda i: step_old(k0, v0), nothing),
        "hot_new_graph": (lambda i: g_new.replay(), reset0),
        "hot_reprepare_graph": (lambda i: g_old.replay(), nothing),
        "cold_new_again": (lambda i: step_new(sets[i % copies][2]), reset_all),
    }
    t = timed(cands, iters, rounds)
    m = lambda k: t[k]["median_ms"]
    return {"measure": "decode_step", "shape": name, "B": B, "Hq": Hq, "Hkv": Hkv, "Skv": Skv, "D": D, "capacity": cap, "copies": copies,
            "iters": iters, "rounds": rounds, "times": t,
            "summary": {"cold_new_over_reprepare": m("cold_new") / m("cold_reprepare"), "hot_new_over_reprepare": m("hot_new") / m("hot_reprepare"),
                        "graph_new_over_reprepare": m("hot_new_graph") / m("hot_reprepare_graph"),
                        "cold_append_share_ms": m("cold_new") - m("cold_attention_only"), "cold_new_again_over_new": m("cold_new_again") / m("cold_new"),
                        "cold_new_spread_pct": spread_pct(t["cold_new"]), "cold_reprepare_spread_pct": spread_pct(t["cold_reprepare"])}}


def append_alone(iters, rounds):
    B, Hkv, Skv, D = 4, 8, 8192, 128
    cap = Skv + 64 * (iters + 4)
    c = qa.alloc_kv_cache_fp8(B, Hkv, cap, D, scale_k=0.02, scale_v=0.02, dtype=BF16, device=DEV)
    reset = lambda: c.seqlens.fill_(Skv + 61)     # T = 8 and 64 cross a chunk boundary
    zero = torch.zeros(B, dtype=torch.int32, device=DEV)
    cands = {}
    for T in (1, 8, 64):
        kn, vn = rand(B, Hkv, T, D), rand(B, Hkv, T, D)
        cands[f"append_T{T}"] = ((lambda kn, vn: lambda i: qa.kv_cache_append_fp8(c, kn, vn))(kn, vn), reset)
        cands[f"floor_T{T}"] = ((lambda kn, vn: lambda i: qa.kv_cache_append_fp8(c, kn, vn, new_lens=zero))(kn, vn), reset)
        g, _ = graph_of((lambda kn, vn: lambda: qa.kv_cache_append_fp8(c, kn, vn))(kn, vn))
        gf, _ = graph_of((lambda kn, vn: lambda: qa.kv_cache_append_fp8(c, kn, vn, new_lens=zero))(kn, vn))
        cands[f"append_T{T}_graph"] = ((lambda g: lambda i: g.replay())(g), reset)
        cands[f"floor_T{T}_graph"] = ((lambda g: lambda i: g.replay())(gf), reset)
    # the host's path at T = 1: the function (validation + binding), the binding alone, and the torch.library op the function uses in a trace
    kn, vn = rand(B, Hkv, 1, D), rand(B, Hkv, 1, D)
    cands["T1_function"] = (lambda i: qa.kv_cache_append_fp8(c, kn, vn), reset)
    cands["T1_binding"] = (lambda i: _native.kv_cache_append_fp8(c.k, c.v, c.scale_k, c.scale_v, c.seqlens, kn, vn, capacity=cap), reset)
    cands["T1_library_op"] = (lambda i: qa.ops.fp8_kv_cache_append_(c.k, c.v, c.scale_k, c.scale_v, c.seqlens, kn, vn, None, cap, "e4m3", True), reset)
    cands["T1_function_again"] = cands["T1_function"]
    t = timed(cands, iters, rounds)
    m = lambda k: t[k]["median_ms"]
    return {"measure": "append_alone", "B": B, "Hkv": Hkv, "position": Skv + 61, "D": D, "iters": iters, "rounds": rounds, "times": t,
            "summary": dict({f"T{T}{g}_over_floor": m(f"append_T{T}{g}") / m(f"floor_T{T}{g}") for T in (1, 8, 64) for g in ("", "_graph")},
                            library_op_over_binding=m("T1_library_op") / m("T1_binding"), function_over_binding=m("T1_function") / m("T1_binding"),
                            function_again_over_function=m("T1_function_again") / m("T1_function"))}


def prefill(name, iters, rounds):
    B, Hkv, T, D = PREFILL[name]
    set_bytes = 2 * 2 * B * Hkv * T * D
    copies = max(2, min(8, -(-2 * LLC_BYTES // set_bytes)))
    sets = [(rand(B, Hkv, T, D), rand(B, Hkv, T, D)) for _ in range(copies)]
    c = qa.kv_cache_from_prefill_fp8(*sets[0], T, headroom=1.0)
    reset = lambda: c.seqlens.zero_()

    def adv(i):
        qa.kv_cache_append_fp8(c, *sets[i % copies])
        c.seqlens.zero_()

    g_app, _ = graph_of(lambda: qa.kv_cache_append_fp8(c, *sets[0], advance=False))
    g_prep, _ = graph_of(lambda: qa.prepare_kv_fp8(*sets[0]))
    g_from, _ = graph_of(lambda: qa.kv_cache_from_prefill_fp8(*sets[0], T))
    cands = {
        # the function a user calls for a prefill: scales (one more read of k and v), two zero-filled images, then the append
        "from_prefill": (lambda i: qa.kv_cache_from_prefill_fp8(*sets[i % copies], T), nothing),
        "hot_from_prefill_graph": (lambda i: g_from.replay(), nothing),
        "append": (lambda i: qa.kv_cache_append_fp8(c, *sets[i % copies], advance=False), reset),
        "prepare_kv": (lambda i: qa.prepare_kv_fp8(*sets[i % copies]), nothing),
        "append_advance_and_reset": (adv, reset),
        "prepare_kv_again": (lambda i: qa.prepare_kv_fp8(*sets[i % copies]), nothing),
        "append_again": (lambda i: qa.kv_cache_append_fp8(c, *sets[i % copies], advance=False), reset),
        "hot_append_graph": (lambda i: g_app.replay(), reset),
        "hot_prepare_kv_graph": (lambda i: g_prep.replay(), nothing),
        "hot_append_graph_again": (lambda i: g_app.replay(), reset),
    }
    t = timed(cands, iters, rounds)
    m = lambda k: t[k]["median_ms"]
    return {"measure": "prefill_append", "shape": name, "B": B, "Hkv": Hkv, "T": T, "D": D, "copies": copies, "iters": iters, "rounds": rounds, "times": t,
            "summary": {"append_over_prepare": m("append") / m("prepare_kv"), "append_advance_over_prepare": m("append_advance_and_reset") / m("prepare_kv"),
                        "graph_append_over_prepare": m("hot_append_graph") / m("hot_prepare_kv_graph"),
                        "from_prefill_over_prepare": m("from_prefill") / m("prepare_kv"),
                        "graph_from_prefill_over_prepare": m("hot_from_prefill_graph") / m("hot_prepare_kv_graph"),
                        "graph_append_again_over_append": m("hot_append_graph_again") / m("hot_append_graph"),
                        "prepare_again_over_prepare": m("prepare_kv_again") / m("prepare_kv"), "append_again_over_append": m("append_again") / m("append"),
                        "append_spread_pct": spread_pct(t["append"]), "prepare_spread_pct": spread_pct(t["prepare_kv"]),
                        "gbytes_per_s_append": (set_bytes + set_bytes / 2) / (m("append") * 1e-3) / 1e9}}


def views(iters, rounds):
    B, Hkv, D = 4, 8, 128
    out = []
    for T in (1, 64, 4096):
        c = qa.alloc_kv_cache_fp8(B, Hkv, T + 64, D, scale_k=0.02, scale_v=0.02, dtype=BF16, device=DEV)
        reset = lambda: c.seqlens.fill_(3)
        kb, vb = rand(B, T, Hkv, D), rand(B, T, Hkv, D)
        kt, vt = kb.transpose(1, 2), vb.transpose(1, 2)
        kd, vd = kt.contiguous(), vt.contiguous()
        cands = {
            "view": (lambda i: qa.kv_cache_append_fp8(c, kt, vt, advance=False), reset),
            "copy_then_append": (lambda i: qa.kv_cache_append_fp8(c, kt.contiguous(), vt.contiguous(), advance=False), reset),
            "dense": (lambda i: qa.kv_cache_append_fp8(c, kd, vd, advance=False), reset),
            "view_again": (lambda i: qa.kv_cache_append_fp8(c, kt, vt, advance=False), reset),
        }
        t = timed(cands, iters, rounds)
        m = lambda k: t[k]["median_ms"]
        out.append({"measure": "views", "B": B, "Hkv": Hkv, "T": T, "D": D, "iters": iters, "rounds": rounds, "times": t,
                    "summary": {"view_over_copy_then_append": m("view") / m("copy_then_append"), "view_over_dense": m("view") / m("dense"),
                                "view_again_over_view": m("view_again") / m("view")}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--only", default="decode,append,prefill,views")
    args = ap.parse_args()
    assert args.rounds >= 1 and args.iters >= 1
    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    only = args.only.split(",")
    torch.manual_seed(0)
    if "decode" in only:
        for s in DECODE:
            print(json.dumps(decode(s, args.iters, args.rounds)), flush=True)
    if "append" in only:
        print(json.dumps(append_alone(args.iters, args.rounds)), flush=True)
    if "prefill" in only:
        for s in PREFILL:
            print(json.dumps(prefill(s, args.iters, args.rounds)), flush=True)
    if "views" in only:
        for r in views(args.iters, args.rounds):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()

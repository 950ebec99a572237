#!/usr/bin/env python3
"""Time the merge of attention states (quantumattention_amd.merge_attn_states, include/qattn_merge.h) against what a caller writes today:
  merge:N    the HIP kernel on N bf16 states into bf16 (kernel qattn::merge_states_kernel<D, N>)
  torch:N    the torch composition: fp32 up-cast, logsumexp over the stacked LSEs, weighted sum, down-cast (a handful of aten kernels)
  prepass    the quant pre-pass qattn_quant_qkv_fp8 on q, k, v of the same shape -- the bandwidth yardstick of this library: two reads of
             the three 16-bit tensors (abs-max, quantise) and one write of their fp8 images
  multikv    (step times only) fp8_attn_multi_kv_func over 2 x S/2 keys against one fp8_attn_func over S keys
Shapes: c2 = B4 H32 S4096 D128, wan = B1 H40 S32760 D128 (Wan 2.1 14B 480p), bf16.
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_merge.py --calls 16`, no counters in the
same run; then `--summarize DIR --calls 16` prints, per shape and N, the median kernel time of the merge, the median per-call sum of the
composition's kernels, the pre-pass, the bytes each must move and bytes / time.  The phases are told apart by launch order: per shape
[merge:2 x calls][torch:2 x calls][merge:4 x calls][torch:4 x calls][prepass x calls]; kernels that are not this library's and follow a
merge phase are the composition's.  Step times (HIP events, profiler off): the default mode, one JSON line per shape.
Boxes of the pool differ by up to 8 %: only ratios inside one run count."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = {"c2": (4, 32, 4096, 128), "wan": (1, 40, 32760, 128)}
NS = (2, 4)


def merge_bytes(n, B, H, S, D):
    """what the merge must move: N partials in, one state out, 16-bit O and fp32 LSE"""
    return (n + 1) * B * H * S * D * 2 + (n + 1) * B * H * S * 4


def prepass_bytes(B, H, S, D):
    return 2 * 3 * B * H * S * D * 2 + 3 * B * H * S * D


def torch_merge(outs, lses):
    """The composition a user writes today (rows empty in every partial are not handled: it would give NaN there)."""
    import torch

    L = torch.stack(lses)
    lse = torch.logsumexp(L, dim=0)
    w = torch.exp(L - lse)
    out = (torch.stack([o.float() for o in outs]) * w[..., None]).sum(0)
    return out.to(outs[0].dtype), lse


def make_states(B, H, S, D, n, g):
    import torch

    outs = [torch.randn(B, H, S, D, generator=g, device="cuda").to(torch.bfloat16) for _ in range(n)]
    lses = [torch.randn(B, H, S, generator=g, device="cuda") * 3 + 8 for _ in range(n)]
    return outs, lses


def run_shape(name, iters, rounds, calls):
    import torch

    import quantumattention_amd as qa
    from quantumattention_amd import _native
    from time_block_sparse import step_ms

    B, H, S, D = SHAPES[name]
    g = torch.Generator(device="cuda").manual_seed(0)
    outs, lses = make_states(B, H, S, D, max(NS), g)
    q, k, v = outs[0], outs[1], outs[2]
    res = {"shape": name, "B": B, "H": H, "S": S, "D": D}
    fns, names = [], []
    for n in NS:
        fns += [lambda n=n: qa.merge_attn_states(outs[:n], lses[:n]), lambda n=n: torch_merge(outs[:n], lses[:n])]
        names += [f"merge:{n}", f"torch:{n}"]
    fns.append(lambda: _native.quant_qkv_fp8(q, k, v))
    names.append("prepass")
    if calls:   # a kernel-trace run: exactly `calls` calls per phase, one phase after the other
        for fn in fns:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        res["calls"] = calls
        return res
    half = S // 2 // 8 * 8
    k1, k2, v1, v2 = k[:, :, :half], k[:, :, half:], v[:, :, :half], v[:, :, half:]
    fns += [lambda: qa.fp8_attn_multi_kv_func(q, [(k1, v1), (k2, v2)]), lambda: qa.fp8_attn_func(q, k, v)]
    names += ["multikv:2", "fp8_attn_func"]
    for c, ms in zip(names, step_ms(fns, iters, rounds)):
        res[f"step_ms[{c}]"] = ms
    for n in NS:
        res[f"GBps[merge:{n}]"] = merge_bytes(n, B, H, S, D) / res[f"step_ms[merge:{n}]"] / 1e6
    res["GBps[prepass]"] = prepass_bytes(B, H, S, D) / res["step_ms[prepass]"] / 1e6
    return res


def summarize(d, calls, shapes):
    """Per shape and N from the kernel traces under d (see the module docstring for the order the phases were launched in)."""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    kind = lambda name: "merge" if "merge_states_kernel" in name else "prepass" if "qattn" in name else "other"
    phases = []   # (kind, kernel name of its first launch, [durations in us])
    for _, name, us in rows:
        if not phases or phases[-1][0] != kind(name) or (kind(name) == "merge" and phases[-1][1] != name):
            phases.append((kind(name), name, []))
        phases[-1][2].append(us)
    phases = [p for i, p in enumerate(phases) if p[0] != "other" or (i > 0 and phases[i - 1][0] == "merge")]   # (set-up kernels)
    per_call = lambda x: [sum(x[i * (len(x) // calls):(i + 1) * (len(x) // calls)]) for i in range(calls)] if len(x) % calls == 0 else [sum(x) / calls]
    it = iter(phases)
    for s in shapes:
        B, H, S, D = SHAPES[s]
        print(f"== {s}: B{B} H{H} S{S} D{D} bf16, {calls} calls per phase")
        rate = {}
        for n in NS:
            m, t = next(it), next(it)
            assert m[0] == "merge" and any(x in m[1] for x in (f"<{D}, {n}>", f"<{D},{n}>", f"ILi{D}ELi{n}E")) and t[0] == "other", (m[:2], t[:2])
            mus, tus = statistics.median(m[2]), statistics.median(per_call(t[2]))
            rate[n] = merge_bytes(n, B, H, S, D) / mus / 1e6
            print(f"  N={n}: merge kernel median {mus:8.1f} us (min {min(m[2]):8.1f}, n {len(m[2])}) = {rate[n]:5.2f} TB/s of {merge_bytes(n, B, H, S, D) / 1e6:7.1f} MB"
                  f" | torch composition {tus:8.1f} us per call ({len(t[2]) // calls} kernels) = {tus / mus:5.2f} x the kernel")
        p = next(it)
        assert p[0] == "prepass", p[:2]
        pus = statistics.median(per_call(p[2]))
        prate = prepass_bytes(B, H, S, D) / pus / 1e6
        print(f"  quant pre-pass (same run) {pus:8.1f} us per call = {prate:5.2f} TB/s of {prepass_bytes(B, H, S, D) / 1e6:7.1f} MB"
              f" | merge / pre-pass rate: " + ", ".join(f"N={n} {rate[n] / prate:4.2f}" for n in NS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,wan")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--summarize", default="")
    ap.add_argument("--calls", type=int, default=0)
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize, args.calls or 16, args.shapes.split(","))
        return
    from quantumattention_amd import _native

    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    for s in args.shapes.split(","):
        print(json.dumps(run_shape(s, args.iters, args.rounds, args.calls)), flush=True)


if __name__ == "__main__":
    main()

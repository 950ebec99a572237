#!/usr/bin/env python3
"""Time sliding-window attention (quantumattention_amd.fp8_attn_varlen_window_func, include/qattn_window.h) against what a caller had
before it, on the same tensors:
  window:L/R   the window entry (kernel attn_pv16_varlen_window_kernel)
  causal       fp8_attn_varlen_func(causal=True): the full causal sweep (attn_pv16_varlen_kernel)
  plain        fp8_attn_varlen_func(causal=False): the plain packed kernel -- against `window:wide`, a finite window wider than every
               sequence (nothing masked, no chunk skipped, still the window kernel), it is the cost of the interval predicates
  band:L/R     fp8_block_sparse_attn_func with the 128 x 128 band mask that covers the window (shape `long` only: that entry has no
               per-sequence lengths)
--pv fp8 [--precision fast|accurate]: the FP8-PV window entry (fp8_attn_varlen_window_pv_func(pv_precision="fp8"), kernel
attn_vfp8_window_kernel: 128-row tiles, FAST two launches) as `window:L/R`, beside it in the same run `window16:L/R` = the 16-bit window
entry above and `band:L/R` = fp8_block_sparse_attn_pv_func(pv_precision="fp8") on the covering band mask (attn_bs_fp8_kernel); a call's
attention time is the sum over its attention kernels' medians.  The default (--pv 16bit) output is unchanged.
Shapes: long = one sequence of 32768 tokens, H 40, D 128; mixed = the 32 sequences of tools/time_varlen.py (256 .. 4096 tokens, seed 0),
H 24, D 128; bf16.
Step times (the whole call: pre-pass and attention): HIP events around blocks of `--iters` back-to-back calls, the candidates interleaved
block by block over `--rounds` rounds (median).  Kernel times: `--profile DIR` starts, per candidate, one fresh
`rocprofv3 --kernel-trace --stats -d DIR/<n> -- python tools/time_sliding_window.py --shapes S --cands C` and reads the kernel traces:
the median duration of the attention kernel per candidate, its ratio to each alternative, and beside it the ratio of visited 64-key
chunks (counted on the host from the lengths), which is what the time should track.  Prints one JSON line per shape."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS = [(1024, 0), (4096, 0), (512, 512)]
SHAPES = {"long": 40, "mixed": 24}   # heads; D = 128
ATTN_KERNELS = ("attn_pv16_varlen_window_kernel", "attn_pv16_varlen_kernel", "attn_pv16_block_sparse_kernel", "attn_vfp8_window_kernel",
                "attn_bs_fp8_kernel")


def lengths(shape):
    import numpy as np

    return [32768] if shape == "long" else [int(x) for x in np.random.default_rng(0).integers(256, 4097, size=32)]


def all_cands(shape, pv="16bit"):
    if pv == "fp8":
        c = [f"{w}:{l}/{r}" for l, r in WINDOWS for w in ("window", "window16")]
    else:
        c = [f"window:{l}/{r}" for l, r in WINDOWS] + ["window:wide", "causal", "plain"]
    return c + ([f"band:{l}/{r}" for l, r in WINDOWS] if shape == "long" else [])


def window_of(cand, lens):
    w = cand.split(":")[1]
    return (max(lens), max(lens)) if w == "wide" else tuple(int(x) for x in w.split("/"))


def chunks_visited(cand, lens, rows=256):
    """64-key chunks swept per head, summed over the `rows`-row query blocks (self-attention: delta = 0; 128 rows under --pv fp8)"""
    n = 0
    if cand.startswith("window16:"):
        cand, rows = "window:" + cand[9:], 256
    for L in lens:
        for r0 in range(0, L, rows):
            r1 = min(r0 + rows, L) - 1
            if cand.startswith("window:"):
                left, right = window_of(cand, lens)
                n += min(r1 + right, L - 1) // 64 - max(r0 - left, 0) // 64 + 1
            elif cand.startswith("band:"):   # the 128-key blocks either 128-row half lists, two chunks each (the last may hold one)
                left, right = window_of(cand, lens)
                lo, hi = max(r0 - left, 0) // 128, min(r1 + right, L - 1) // 128
                n += sum(min(2, (L - 128 * j + 63) // 64) for j in range(lo, hi + 1))
            elif cand == "causal":
                n += r1 // 64 + 1
            else:
                n += (L + 63) // 64
    return n


def band_mask(S, left, right):
    """tile (i, j) on iff a row of query block i attends a key of key block j under the window"""
    import torch

    nb = (S + 127) // 128
    i, j = torch.arange(nb, device="cuda")[:, None], torch.arange(nb, device="cuda")[None, :]
    return ((128 * j + 127 >= 128 * i - left) & (128 * j <= 128 * i + 127 + right))[None, None]


def step_ms(fns, iters, rounds, warmup=2):
    """ms per call of each of `fns`: blocks of `iters` calls, the candidates interleaved block by block, median over the rounds"""
    import torch

    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    laps = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            laps[i].append((e0, e1))
    torch.cuda.synchronize()
    return [sorted(a.elapsed_time(b) / iters for a, b in lap)[rounds // 2] for lap in laps]


def run_shape(shape, cands, iters, rounds, pv="16bit", precision="fast"):
    import numpy as np
    import torch

    import quantumattention_amd as qa

    lens, H, D = lengths(shape), SHAPES[shape], 128
    total = sum(lens)
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v = (torch.randn(total, H, D, generator=g, device="cuda", dtype=torch.float32).to(torch.bfloat16) for _ in range(3))
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device="cuda")
    dense = lambda t: t.transpose(0, 1)[None]   # [1, H, S, D] view of the one sequence
    fns, res = [], {"shape": shape, "B": len(lens), "H": H, "D": D, "total_tokens": total}
    for c in cands:
        if c.startswith("window:") and pv == "fp8":
            fns.append(lambda w=window_of(c, lens): qa.fp8_attn_varlen_window_pv_func(q, k, v, cu, cu, max(lens), max(lens), w, pv_precision="fp8",
                                                                                      precision=precision))
        elif c.startswith("window:") or c.startswith("window16:"):
            fns.append(lambda w=window_of(c, lens): qa.fp8_attn_varlen_window_func(q, k, v, cu, cu, max(lens), max(lens), w))
        elif c in ("causal", "plain"):
            fns.append(lambda causal=c == "causal": qa.fp8_attn_varlen_func(q, k, v, cu, cu, max(lens), max(lens), causal=causal))
        elif c.startswith("band:") and shape == "long":
            m = band_mask(total, *window_of(c, lens))
            qd, kd, vd = (dense(t).contiguous() for t in (q, k, v))
            if pv == "fp8":
                fns.append(lambda m=m, qd=qd, kd=kd, vd=vd: qa.fp8_block_sparse_attn_pv_func(qd, kd, vd, m, pv_precision="fp8", precision=precision))
            else:
                fns.append(lambda m=m, qd=qd, kd=kd, vd=vd: qa.fp8_block_sparse_attn_func(qd, kd, vd, m))
        else:
            raise SystemExit(f"unknown candidate {c!r} for shape {shape!r}")
        res[f"chunks[{c}]"] = chunks_visited(c, lens, 128 if pv == "fp8" else 256)
    for c, ms in zip(cands, step_ms(fns, iters, rounds)):
        res[f"step_ms[{c}]"] = ms
    return res


def attention_us(d):
    """median duration (us) of the attention kernel in the rocprofv3 kernel traces under d, and its name; a call with several attention
    kernels (FAST under --pv fp8: the one-term and the two-term launch): the sum of their medians"""
    durs = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            durs.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    hits = [(statistics.median(x), a, len(x)) for name, x in sorted(durs.items()) for a in ATTN_KERNELS if a + "<" in name or a + "I" in name]
    if not hits:
        return None, None, 0
    n = hits[0][2] if len(hits) == 1 else "+".join(str(h[2]) for h in hits)   # (launch counts, kernel by kernel)
    return sum(h[0] for h in hits), "+".join(sorted({h[1] for h in hits})), n


def profile(shape, cands, iters, out_dir, timeout, pv="16bit", precision="fast"):
    """one rocprofv3 run per candidate, each a fresh child process; returns the report of the shape"""
    lens = lengths(shape)
    rep = {"shape": shape, "kernel_us": {}, "chunks": {}}
    if pv == "fp8":
        rep["pv"], rep["precision"] = pv, precision
    for n, c in enumerate(cands):
        d = os.path.join(out_dir, f"{shape}_{n}")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--shapes", shape, "--cands", c, "--iters", str(iters), "--rounds", "1", "--pv", pv, "--precision", precision]
        rc = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=timeout)
        if rc.returncode != 0:   # nothing more is started on the GPU after a failed run
            raise SystemExit(f"{' '.join(cmd)} failed ({rc.returncode}):\n{rc.stderr[-2000:]}")
        us, kern, cnt = attention_us(d)
        rep["kernel_us"][c] = us
        rep["chunks"][c] = chunks_visited(c, lens, 128 if pv == "fp8" else 256)
        print(f"  {shape:5s} {c:16s} {kern} n {cnt} median {us:.1f} us, chunks {rep['chunks'][c]}", flush=True)
    for c in [c for c in cands if c.startswith("window:")]:
        for alt in [a for a in cands if not a.startswith("window:")]:
            if alt.startswith("band:") and alt[5:] != c[7:]:
                continue
            if alt.startswith("window16:") and alt[9:] != c[7:]:
                continue
            if (c == "window:wide") != (alt == "plain"):
                continue
            rep[f"{c} / {alt}"] = {"time": rep["kernel_us"][c] / rep["kernel_us"][alt], "chunks": rep["chunks"][c] / rep["chunks"][alt]}
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="long,mixed")
    ap.add_argument("--cands", default="")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile", default="", help="directory for one rocprofv3 kernel trace per candidate")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per rocprofv3 run")
    ap.add_argument("--pv", choices=("16bit", "fp8"), default="16bit", help="P.V path of the window (and band) candidates")
    ap.add_argument("--precision", choices=("fast", "accurate"), default="fast", help="precision of the FP8 P.V path (--pv fp8)")
    args = ap.parse_args()
    for s in args.shapes.split(","):
        cands = args.cands.split(",") if args.cands else all_cands(s, args.pv)
        if args.profile:   # (this process opens no GPU: every measurement is a child of its own)
            print(json.dumps(profile(s, cands, args.iters, args.profile, args.timeout, args.pv, args.precision)), flush=True)
            continue
        from quantumattention_amd import _native

        assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
        print(json.dumps(run_shape(s, cands, args.iters, args.rounds, args.pv, args.precision)), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the packed variable-length entry (quantumattention_amd.fp8_attn_varlen_func, include/qattn_varlen.h) against
  (a) the varlen call itself,
  (b) the per-sequence loop of the bit-identical dense path (dynamically_quantize_fp8 of q and k, then the 16-bit-V fp8 entry: what a
      caller without a varlen entry runs),
  (c) on equal lengths, the dense whole-tensor call with pv_precision = "16bit" on [B, H, S, D] (quantise q and k, then the op).
Step times are HIP events around blocks of `--iters` back-to-back steps, the candidates interleaved block by block (step_ms); kernel times come from a run of this script under
`rocprofv3 --kernel-trace --stats` (the attention kernels: attn_pv16_varlen_kernel, attn_pv16_kernel).  --cases picks the workloads:
  equal    4 x 4096, H 32, D 128, non-causal (the README's dense 16-bit-V step shape)
  mixed    32 sequences drawn from 256 .. 4096 tokens (seed 0), H 24, D 128, causal and non-causal
--pv fp8 --precision fast|accurate: the FP8-PV mode (fp8_attn_varlen_pv_func(..., pv_precision="fp8"), attention kernel attn_vfp8_kernel)
instead, interleaved with the 16-bit-PV packed entry in the same run and -- on equal lengths -- with the dense fused call
fp8_attn_func on 16-bit inputs under config.attention.precision = "fast".  Only same-run ratios count.
Prints one JSON line per case; FLOPs follow bench.py (4 Sq Skv D per head, halved for causal), the attention fraction is against bench.py's
FP8_PEAK_TFLOPS."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import quantumattention_amd as qa  # noqa: E402
from quantumattention_amd import _native  # noqa: E402

FP8_PEAK_TFLOPS = 5000.0   # bench.py


def step_ms(fns, iters, rounds=5, warmup=3, pick=None):
    """ms per step of each of `fns`: blocks of `iters` steps, the candidates interleaved block by block over `rounds` rounds (clock and
    thermal drift hit all of them alike), median over the rounds"""
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
    pick = pick or (lambda xs: sorted(xs)[rounds // 2])
    return [pick([a.elapsed_time(b) / iters for a, b in lap]) for lap in laps]


def flops(lens_q, lens_k, H, D, causal):
    return sum(4.0 * H * a * b * D * (0.5 if causal else 1.0) for a, b in zip(lens_q, lens_k))


def run_case_fp8pv(name, lens, H, D, causal, iters, precision, dense=False):
    """the FP8-PV packed call against the 16-bit-PV packed call (and the dense fused FAST call on equal lengths): medians and minima"""
    torch.manual_seed(0)
    total = int(sum(lens))
    q, k, v = (torch.randn(total, H, D, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device="cuda")
    fns = {"varlen16": lambda: qa.fp8_attn_varlen_func(q, k, v, cu, cu, max(lens), max(lens), causal=causal),
           "varlen_fp8": lambda: qa.fp8_attn_varlen_pv_func(q, k, v, cu, cu, max(lens), max(lens), causal=causal, pv_precision="fp8",
                                                            precision=precision)}
    if dense:
        B, S = len(lens), lens[0]
        qd, kd, vd = (t.view(B, S, H, D).transpose(1, 2) for t in (q, k, v))   # (strided views: read in place)

        def dense_fast():
            with qa.config.patch({"attention.precision": "fast"}):
                return qa.fp8_attn_func(qd, kd, vd, is_causal=causal)

        fns["dense_fast"] = dense_fast
    f = flops(lens, lens, H, D, causal)
    res = {"case": name, "pv": "fp8", "precision": precision, "B": len(lens), "H": H, "D": D, "causal": causal, "total_tokens": total, "flops": f}
    names = list(fns)
    med = step_ms([fns[n] for n in names], iters, rounds=7)
    low = step_ms([fns[n] for n in names], iters, rounds=7, pick=min)
    for n, a, b in zip(names, med, low):
        res[n + "_ms"], res[n + "_min_ms"] = a, b
    res["fp8_over_16bit"] = res["varlen_fp8_ms"] / res["varlen16_ms"]
    if dense:
        res["fp8_over_dense_fast"] = res["varlen_fp8_ms"] / res["dense_fast_ms"]
    res["varlen_fp8_step_TFLOPs"] = f / (res["varlen_fp8_ms"] * 1e-3) / 1e12
    return res


def run_case(name, lens, H, D, causal, iters, dense=False):
    torch.manual_seed(0)
    total = int(sum(lens))
    q, k, v = (torch.randn(total, H, D, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device="cuda")
    starts = [int(x) for x in np.cumsum([0] + list(lens))[:-1]]
    seq = lambda t, a, n: t[a:a + n].transpose(0, 1)[None]

    def varlen():
        return qa.fp8_attn_varlen_func(q, k, v, cu, cu, max(lens), max(lens), causal=causal)

    def loop():
        for a, n in zip(starts, lens):
            q8, sq = qa.dynamically_quantize_fp8(seq(q, a, n), reduction_dim=[2, 3])
            k8, sk = qa.dynamically_quantize_fp8(seq(k, a, n), reduction_dim=[2, 3])
            _native.fp8_attention_forward_rowmajor(q8, k8, seq(v, a, n), sq, sk, is_causal=causal, pv_16bit=True)

    f = flops(lens, lens, H, D, causal)
    res = {"case": name, "B": len(lens), "H": H, "D": D, "causal": causal, "total_tokens": total, "flops": f}
    res["varlen_ms"], res["loop_ms"] = step_ms([varlen, loop], iters)
    res["speedup_vs_loop"] = res["loop_ms"] / res["varlen_ms"]
    res["varlen_step_TFLOPs"] = f / (res["varlen_ms"] * 1e-3) / 1e12
    if dense:
        B, S = len(lens), lens[0]
        qd, kd, vd = (t.view(B, S, H, D).transpose(1, 2).contiguous() for t in (q, k, v))

        def dense16():
            q8, sq = qa.dynamically_quantize_fp8(qd, reduction_dim=[2, 3])
            k8, sk = qa.dynamically_quantize_fp8(kd, reduction_dim=[2, 3])
            return qa.fp8_attn_func(q8, k8, vd, is_causal=causal, scale_q=sq, scale_k=sk)

        with qa.config.patch({"attention.pv_precision": "16bit"}):
            res["varlen_ms_vs_dense"], res["dense16_ms"] = step_ms([varlen, dense16], iters)
            out_d = dense16()
        torch.cuda.synchronize()
        # same numerics: the equal-length varlen output IS the dense one (per-head scales of one sequence = of one batch entry)
        res["varlen_equals_dense16"] = bool(torch.equal(varlen().view(B, S, H, D).transpose(1, 2), out_d))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="equal,mixed")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pv", default="16bit", choices=["16bit", "fp8"])
    ap.add_argument("--precision", default="fast", choices=["fast", "accurate"])
    args = ap.parse_args()
    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    cases = args.cases.split(",")
    if args.pv == "fp8":
        if "equal" in cases:
            print(json.dumps(run_case_fp8pv("equal", [4096] * 4, 32, 128, False, args.iters, args.precision, dense=True)), flush=True)
        if "mixed" in cases:
            lens = [int(x) for x in np.random.default_rng(0).integers(256, 4097, size=32)]
            for causal in (False, True):
                print(json.dumps(run_case_fp8pv("mixed", lens, 24, 128, causal, args.iters, args.precision)), flush=True)
        return
    if "equal" in cases:
        print(json.dumps(run_case("equal", [4096] * 4, 32, 128, False, args.iters, dense=True)), flush=True)
    if "mixed" in cases:
        lens = [int(x) for x in np.random.default_rng(0).integers(256, 4097, size=32)]
        for causal in (False, True):
            r = run_case("mixed", lens, 24, 128, causal, args.iters)
            r["lengths"] = lens
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()

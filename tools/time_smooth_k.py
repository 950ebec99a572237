#!/usr/bin/env python3
"""Time the public fp8 step with key smoothing (config.attention.smooth_k, include/qattn_smooth.h) off and on, in the same process.
Step times are HIP events around blocks of `--iters` back-to-back steps, the two settings interleaved block by block over `--rounds`
rounds, median over the rounds (clock and thermal drift hit both alike); the min .. max over the rounds is printed as the spread.  Kernel
times come from a run of this script under `rocprofv3 --kernel-trace --stats` (the passes of smoothing: kmean_partial_kernel,
kmean_final_kernel, smooth_amax_kernel, smooth_quant_k_kernel; the plain pre-pass: amax_multi_kernel, quant_multi_kernel).
Shapes: bench.py's C2 (B4 H32 S4096 D128 bf16, precision auto), the same causal, and token-wise scales, on bench.py's N(0,1) keys: the
cost of the flag.  c2_offset: C2 on keys with a sigma = 16 channel offset, the keys smoothing is for -- there precision="auto" forecasts
a wide score spread from the unsmoothed K's sum of squares and starts its heads on the precise pass, so flag OFF is the slower one.
What the bytes predict for the flag: one more read of K (B Hkv Skv D 2 bytes) at the pre-pass's 6.0 TB/s.  Prints one JSON line per case."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import quantumattention_amd as qa  # noqa: E402
from quantumattention_amd import _native  # noqa: E402

PREPASS_TBS = 6.0


def step_ms(fns, iters, rounds, warmup=3):
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
    times = [sorted(a.elapsed_time(b) / iters for a, b in lap) for lap in laps]
    return [(t[rounds // 2], t[0], t[-1]) for t in times]


def run_case(name, B, H, S, D, causal, func, sigma, iters, rounds):
    torch.manual_seed(0)
    q, v = (torch.randn(B, H, S, D, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    k = (torch.randn(B, H, S, D, device="cuda") + sigma * torch.randn(B, H, 1, D, device="cuda")).to(torch.bfloat16)
    f = getattr(qa, func)

    def off():
        with qa.config.patch({"attention.smooth_k": False}):
            return f(q, k, v, is_causal=causal)

    def on():
        with qa.config.patch({"attention.smooth_k": True}):
            return f(q, k, v, is_causal=causal)

    (m_off, lo_off, hi_off), (m_on, lo_on, hi_on) = step_ms([off, on], iters, rounds)
    k_bytes = 2.0 * B * H * S * D
    pred_us = k_bytes / (PREPASS_TBS * 1e12) * 1e6
    ref = torch.nn.functional.scaled_dot_product_attention(q[:1, :2].float(), k[:1, :2].float(), v[:1, :2].float(), is_causal=causal)
    rm = lambda o: (o[:1, :2].float() - ref).pow(2).mean().sqrt().item()
    return {"case": name, "func": func, "B": B, "H": H, "S": S, "D": D, "causal": causal, "key_offset_sigma": sigma, "iters": iters, "rounds": rounds,
            "off_ms": m_off, "off_min_max_ms": [lo_off, hi_off], "on_ms": m_on, "on_min_max_ms": [lo_on, hi_on],
            "cost_us": (m_on - m_off) * 1e3, "cost_pct": (m_on / m_off - 1.0) * 100.0, "predicted_us_one_read_of_K": pred_us,
            "rmse_vs_fp32_sdpa_2_heads": {"off": rm(off()), "on": rm(on())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,causal,token,c2_offset")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    cases = {"c2": ("c2", 4, 32, 4096, 128, False, "fp8_attn_func", 0.0), "causal": ("causal", 4, 32, 4096, 128, True, "fp8_attn_func", 0.0),
             "token": ("token", 4, 32, 4096, 128, False, "fp8_token_wise_attn_func", 0.0),
             "c2_offset": ("c2_offset", 4, 32, 4096, 128, False, "fp8_attn_func", 16.0)}
    for c in args.cases.split(","):
        print(json.dumps(run_case(*cases[c], args.iters, args.rounds)), flush=True)


if __name__ == "__main__":
    main()

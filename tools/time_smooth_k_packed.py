#!/usr/bin/env python3
"""Time fp8_attn_varlen_func and fp8_block_sparse_attn_func with key smoothing (config.attention.smooth_k; include/qattn_smooth.h) off and on, in
the same process.  Step times are HIP events around blocks of `--iters` back-to-back steps, the two settings interleaved block by block
over `--rounds` rounds, median over the rounds; the min .. max over the rounds is printed as the spread (tools/time_smooth_k.py).
Kernel times come from a run of this script under `rocprofv3 --kernel-trace --stats` (varlen: varlen_kmean_partial_kernel,
varlen_kmean_final_kernel, varlen_smooth_amax_kernel, varlen_smooth_quant_k_kernel, varlen_smooth_lse_kernel with --lse; block-sparse: the
dense smoothing passes kmean_partial_kernel, kmean_final_kernel, smooth_amax_kernel, smooth_quant_k_kernel).
Cases (DESIGN.md sections 4.7 / 4.8): varlen = 32 sequences drawn from 256 .. 4096 tokens (seed 0), H 24, D 128, bf16; wan_band = B1 H40
S32760 D128 bf16 with the band mask of tools/time_block_sparse.py (+-round(0.07 nKB) key blocks plus two global columns).
What the bytes predict for the flag: one more read of the used K (tokens Hkv D 2 bytes) at the pre-pass's 6.0 TB/s.
Prints one JSON line per case."""
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


def flagged(value, fn):
    def call():
        with qa.config.patch({"attention.smooth_k": value}):
            return fn()
    return call


def report(name, extra, fns, k_bytes, iters, rounds):
    res = step_ms(fns, iters, rounds)
    out = {"case": name, **extra, "iters": iters, "rounds": rounds, "off_ms": res[0][0], "off_min_max_ms": list(res[0][1:]),
           "on_ms": res[1][0], "on_min_max_ms": list(res[1][1:]), "cost_us": (res[1][0] - res[0][0]) * 1e3,
           "cost_pct": (res[1][0] / res[0][0] - 1.0) * 100.0, "predicted_us_one_read_of_K": k_bytes / (PREPASS_TBS * 1e12) * 1e6}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="varlen,varlen_causal,wan_band")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--lse", action="store_true", help="ask for the LSE as well (adds the correction kernel when smoothing)")
    args = ap.parse_args()
    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    torch.manual_seed(0)
    for c in args.cases.split(","):
        if c.startswith("varlen"):
            causal = c == "varlen_causal"
            lens = [int(x) for x in np.random.default_rng(0).integers(256, 4097, size=32)]
            total, H, D = sum(lens), 24, 128
            q, k, v = (torch.randn(total, H, D, device="cuda").to(torch.bfloat16) for _ in range(3))
            cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device="cuda")
            kw = dict(causal=causal, return_lse=args.lse)
            off = flagged(False, lambda: qa.fp8_attn_varlen_func(q, k, v, cu, cu, max(lens), max(lens), **kw))
            on = flagged(True, lambda: qa.fp8_attn_varlen_func(q, k, v, cu, cu, max(lens), max(lens), **kw))
            report(c, {"B": len(lens), "H": H, "D": D, "causal": causal, "total_tokens": total, "lse": args.lse},
                   [off, on], 2.0 * total * H * D, args.iters, args.rounds)
        elif c == "wan_band":
            B, H, S, D = 1, 40, 32760, 128
            q, k, v = (torch.randn(B, H, S, D, device="cuda").to(torch.bfloat16) for _ in range(3))
            nb = (S + 127) // 128
            w = max(1, round(0.07 * nb))
            i, j = torch.arange(nb, device="cuda")[:, None], torch.arange(nb, device="cuda")[None, :]
            mask = (((i - j).abs() <= w) | (j < 2)).expand(B, H, nb, nb).contiguous()
            kw = dict(return_lse=args.lse)
            off = flagged(False, lambda: qa.fp8_block_sparse_attn_func(q, k, v, mask, **kw))
            on = flagged(True, lambda: qa.fp8_block_sparse_attn_func(q, k, v, mask, **kw))
            report(c, {"B": B, "H": H, "S": S, "D": D, "mask_density": float(mask.float().mean()), "lse": args.lse},
                   [off, on], 2.0 * B * H * S * D, max(2, args.iters // 3), args.rounds)
        else:
            raise SystemExit(f"unknown case {c}")


if __name__ == "__main__":
    main()

"""Times the non-absorbed MLA prefill entry (include/qattn_mla_prefill.h) against the only route the library had before it, in ONE run, as
replayed graphs alternated round by round (the method of tools/time_mla_index.py):

  new      fp8_mla_prefill_varlen_func(q [T, 128, 192], k_nope, k_pe [T, 64], v), causal
  padded   fp8_attn_varlen_pv_func(pv_precision="fp8", precision="accurate") at D = 256 on q / k zero-padded from 192 and v from 128, INCLUDING the
           copies the route needs: the broadcast of k_pe over the heads, its concatenation with k_nope, the three zero-paddings and the slice of
           the result

for H = 128 heads, T = 4 096 and 16 384 tokens, as one sequence (B = 1) and as four equal ones (B = 4), bf16, N(0, 1) data.  Every figure is
the median of ROUNDS rounds of REPS replays with its spread (min .. max over the rounds).  The two routes quantise q differently (token-wise
against head-wise), so their outputs are compared by their largest difference, which is printed, not by bits.  Needs the GPU; prints one line
per shape and a JSON line at the end.

    python tools/time_mla_prefill.py [--rounds 5] [--reps 5] [--out FILE] [--tokens 4096,16384] [--batches 1,4]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantumattention_amd as qa  # noqa: E402
from quantumattention_amd import _native  # noqa: E402
from tools.time_mla_index import DEV, captured, timed  # noqa: E402

H = 128
SCALE = 1.0 / math.sqrt(192.0)


def one_shape(T, B, rounds, reps):
    q = torch.randn((T, H, 192), device=DEV).bfloat16()
    kv = torch.randn((T, H, 256), device=DEV).bfloat16()
    k_pe = torch.randn((T, 64), device=DEV).bfloat16()
    L = T // B
    cu = torch.arange(0, T + 1, L, dtype=torch.int32, device=DEV)

    def new():
        return qa.fp8_mla_prefill_varlen_func(q, kv[..., :128], k_pe, kv[..., 128:], cu, cu, L, L, scale=SCALE, causal=True)

    def padded():
        k = torch.cat([kv[..., :128], k_pe[:, None, :].expand(T, H, 64), kv.new_zeros((T, H, 64))], dim=-1)
        out = qa.fp8_attn_varlen_pv_func(F.pad(q, (0, 64)), k, F.pad(kv[..., 128:], (0, 128)), cu, cu, L, L, softmax_scale=SCALE, causal=True,
                                         pv_precision="fp8", precision="accurate")
        return out[..., :128].contiguous()

    diff = (new().float() - padded().float()).abs().max().item()
    cands = {"new": captured(new), "padded": captured(padded)}
    times = {k: [] for k in cands}
    for _ in range(rounds):                    # alternated: one round times every candidate once
        for k, fn in cands.items():
            times[k].append(timed(fn, reps))
    t = {k: (round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)) for k, v in times.items()}
    return {"T": T, "B": B, "H": H, "causal": True, "us_median_min_max": t, "padded_over_new": round(t["padded"][0] / t["new"][0], 3),
            "new_faster_beyond_spread": t["new"][2] < t["padded"][1], "max_abs_diff_of_outputs": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tokens", default="4096,16384")
    ap.add_argument("--batches", default="1,4")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_mla_prefill.py measures on the GPU; none found")
    rows = []
    for T in (int(x) for x in a.tokens.split(",")):
        for B in (int(x) for x in a.batches.split(",")):
            rows.append(one_shape(T, B, a.rounds, a.reps))
            print(rows[-1], flush=True)
    line = json.dumps({"tool": "time_mla_prefill", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps,
                       "library": os.path.basename(_native.LIB_PATH), "rows": rows})
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

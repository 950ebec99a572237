#!/usr/bin/env python3
"""Time the rotary embedding at the paged cache's positions (include/qattn_paged_varlen_rope.h) against the
composition it equals, in the same process.  As tools/time_paged_varlen_append.py (whose helpers this imports): HIP events around blocks
of `--iters` back-to-back replays of ONE captured graph per candidate, the candidates interleaved block by block over `--rounds` rounds,
median over the rounds, min .. max as the spread; ratios are taken within one run only.  Every append advances seqlens; a reset outside
the timed region puts the lengths back before each block.

  shapes    Hq 32, Hkv 8, D 128, page size 128: the mixed step (one slot appends 512 tokens, 31 slots one each, 8192 keys of history)
            and pure decode, B 1 at 32768 keys and B 4 at 8192 keys.  The tokens are slices of one packed projection tensor.
  append    `fused`    (a) paged_kv_cache_append_varlen_rope_fp8 on the K and V slices as they are.
            `composed` (b) what it equals: apply_rope_eager on the K slice with cos[pos] / sin[pos] gathered at a positions tensor (given
                       for free: computing it from seqlens and cu_seqlens is not timed, generous to this baseline), then
                       paged_kv_cache_append_varlen_fp8.
            `plain`    (c) paged_kv_cache_append_varlen_fp8 on the unrotated K: the floor.
  rotate q  `fused_q` apply_rope_paged_varlen on the q slice against `eager_q`, apply_rope_eager with the same gather.
  yardstick the baseline of each comparison timed twice (first and last candidate): `<baseline>_again_over_<baseline>` and the min ..
            max spread over the rounds are the margin a ratio is held to"""
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
import time_paged_varlen_append as TA  # noqa: E402
from quantumattention_amd import _native  # noqa: E402
from quantumattention_amd.rope import apply_rope_eager  # noqa: E402

DEV = TK.DEV
PAGE = TA.PAGE


def tables(T, D):
    h = D // 2
    ang = torch.arange(T, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(h, dtype=torch.float64) / h))[None]
    return ang.cos().float().to(DEV), ang.sin().float().to(DEV)


def shape(name, B, Hq, Hkv, D, Skv, counts, iters, rounds):
    total = sum(counts)
    cap = -(-(Skv + max(max(counts), 64) * (iters + 4)) // 256) * 256
    cs = TA.caches(B, Hkv, Skv, cap, D)
    qkv = TK.rand(total, Hq + 2 * Hkv, D)
    q, ks, vs = qkv[:, :Hq], qkv[:, Hq:Hq + Hkv], qkv[:, Hq + Hkv:]
    cu = torch.tensor([0] + torch.tensor(counts).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    cos, sin = tables(cap, D)
    pos = torch.cat([Skv + torch.arange(n) for n in counts]).to(DEV)      # the positions of the first call of a block

    def rotated(x):
        return apply_rope_eager(x.transpose(0, 1)[None], cos[pos], sin[pos])[0].transpose(0, 1)

    appends = {
        "composed": lambda c: qa.paged_kv_cache_append_varlen_fp8(c, rotated(ks), vs, cu),
        "fused": lambda c: qa.paged_kv_cache_append_varlen_rope_fp8(c, ks, vs, cu, cos, sin),
        "plain": lambda c: qa.paged_kv_cache_append_varlen_fp8(c, ks, vs, cu),
    }
    # the same bytes on both rotating paths, before anything is timed
    a, b = TP.clone_paged(cs[0]), TP.clone_paged(cs[0])
    appends["composed"](a)
    appends["fused"](b)
    assert TA.same_state(a, b) and a.seqlens.tolist() == [Skv + n for n in counts]
    del a, b
    t, summary = TA.run(appends, "composed", cs, Skv, iters, rounds, kinds=("graph",))
    summary["graph_fused_over_plain"] = summary["graph_fused_ms"] / summary["graph_plain_ms"]
    out = [{"measure": "paged_varlen_rope_append", "shape": name, "B": B, "Hq": Hq, "Hkv": Hkv, "Skv": Skv, "capacity": cap, "D": D,
            "page_size": PAGE, "tokens": total, "iters": iters, "rounds": rounds, "times": t, "summary": summary}]
    rots = {
        "eager_q": lambda c: rotated(q),
        "fused_q": lambda c: qa.apply_rope_paged_varlen(q, c, cu, cos, sin),
    }
    for c in cs:
        c.seqlens.fill_(Skv)
    assert torch.equal(rots["eager_q"](cs[0]).view(torch.int16), rots["fused_q"](cs[0]).view(torch.int16))
    t, summary = TA.run(rots, "eager_q", cs, Skv, iters, rounds, kinds=("graph",))
    out.append({"measure": "rope_paged_varlen_q", "shape": name, "B": B, "Hq": Hq, "D": D, "tokens": total, "iters": iters, "rounds": rounds,
                "times": t, "summary": summary})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--only", default="mixed,decode_b1,decode_b4")
    args = ap.parse_args()
    assert args.rounds >= 1 and args.iters >= 1
    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    only = args.only.split(",")
    torch.manual_seed(0)
    shapes = {"mixed": (32, 32, 8, 128, 8192, [512] + [1] * 31)}
    for k, (B, Hq, Hkv, Skv, D) in TK.DECODE.items():
        shapes[k] = (B, Hq, Hkv, D, Skv, [1] * B)
    for name, (B, Hq, Hkv, D, Skv, counts) in shapes.items():
        if name in only:
            for r in shape(name, B, Hq, Hkv, D, Skv, counts, args.iters, args.rounds):
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()

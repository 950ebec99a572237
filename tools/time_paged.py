#!/usr/bin/env python3
"""Time the paged FP8 K/V cache (include/qattn_paged.h) against the contiguous KVCacheFP8 path in the same process.
As tools/time_kvcache.py (whose helpers this imports): HIP events around blocks of `--iters` back-to-back calls, the candidates interleaved
block by block over `--rounds` rounds (>= 16), median over the rounds, min .. max as the spread; ratios are taken within one run only.

  decode step  "append T = 1, then attend (causal, seqused_k = seqlens, num_splits = 0)": the contiguous cache against paged caches that hold
               the SAME bytes -- page sizes 64 and 256, an identity table (page b M + m) and a randomly shuffled one -- eager over `copies`
               cold copies of the images / pools, and as ONE replayed graph per candidate on a warm copy.  Both sides see the same logical
               Skv (max_seqlen_k = the contiguous capacity), so the auto rule picks the same splits and the grids are equal.
  attention    the attention call alone as a replayed graph (the quant pre-pass of q, the sweep, the merge: only the sweep kernel differs
               between the candidates, so the difference of two such figures is the difference of the sweeps)
  yardstick    the contiguous step of the same run, timed twice (first and last candidate): `contiguous_again_over_contiguous` and the
               min .. max spread over the rounds are the margin a paged figure is held to
  auto splits  what the num_splits = 0 rule picks for a table 4 x wider than the live length, with and without max_seqlen_k"""
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
from quantumattention_amd import _native  # noqa: E402

DECODE = TK.DECODE
DEV, BF16 = TK.DEV, TK.BF16
PAGED = [(64, "identity"), (64, "shuffled"), (256, "identity"), (256, "shuffled")]


def paged_from(cc, page_size, order, seed=0):
    """a PagedKVCacheFP8 whose sequences hold the bytes of the contiguous cache cc (capacity a multiple of page_size), every sequence
    owning capacity / page_size pages: page b M + m under `identity`, a random permutation under `shuffled`"""
    B, Hkv, cap, D = cc.shape
    assert cap % page_size == 0
    M, pc, CH = cap // page_size, page_size // 64, 64 * D
    pages = torch.arange(B * M) if order == "identity" else torch.randperm(B * M, generator=torch.Generator().manual_seed(seed))
    c = qa.alloc_paged_kv_cache_fp8(B * M, Hkv, page_size, D, batch_size=B, max_pages_per_seq=M, scale_k=cc.scale_k, scale_v=cc.scale_v,
                                    dtype=cc.dtype, device=cc.device, fp8_format=cc.fp8_format)
    idx = pages.to(cc.device)
    for pool, img in ((c.k, cc.k), (c.v, cc.v)):
        pool.view(B * M, Hkv, pc, CH)[idx] = img.view(B, Hkv, M, pc, CH).permute(0, 2, 1, 3, 4).reshape(B * M, Hkv, pc, CH)
    c.block_table.copy_(pages.view(B, M).to(torch.int32))
    c.seqlens.copy_(cc.seqlens)
    return c


def clone_contig(cc):
    return qa.KVCacheFP8(cc.k.clone(), cc.v.clone(), cc.scale_k, cc.scale_v, cc.shape, cc.fp8_format, cc.dtype, cc.numerics, cc.layout, cc.seqlens.clone())


def clone_paged(c):
    return qa.PagedKVCacheFP8(c.k.clone(), c.v.clone(), c.scale_k, c.scale_v, c.block_table, c.seqlens.clone(), c.shape, c.fp8_format, c.dtype,
                              c.numerics, c.layout)


def decode(name, iters, rounds):
    B, Hq, Hkv, Skv, D = DECODE[name]
    cap = -(-(Skv + 64 * (iters + 4)) // 256) * 256
    set_bytes = 2 * B * Hkv * cap * D
    copies = max(2, min(8, -(-2 * TK.LLC_BYTES // set_bytes)))
    q, kn, vn = TK.rand(B, Hq, 1, D), TK.rand(B, Hkv, 1, D), TK.rand(B, Hkv, 1, D)
    cc = qa.kv_cache_from_prefill_fp8(TK.rand(B, Hkv, Skv, D), TK.rand(B, Hkv, Skv, D), cap)

    def step_c(c):
        qa.kv_cache_append_fp8(c, kn, vn)
        return qa.fp8_attn_splitkv_func(q, c, causal=True, seqused_k=c.seqlens)

    def step_p(c):
        qa.paged_kv_cache_append_fp8(c, kn, vn)
        return qa.fp8_attn_paged_func(q, c, causal=True, max_seqlen_k=cap)

    att_c = lambda c: qa.fp8_attn_splitkv_func(q, c, causal=True, seqused_k=c.seqlens)
    att_p = lambda c: qa.fp8_attn_paged_func(q, c, causal=True, max_seqlen_k=cap)
    fams = {"contiguous": ([clone_contig(cc) for _ in range(copies)], step_c, att_c)}
    for ps, order in PAGED:
        first = paged_from(cc, ps, order)
        fams[f"paged_ps{ps}_{order}"] = ([first] + [clone_paged(first) for _ in range(copies - 1)], step_p, att_p)
    # the same bits on every path, before anything is timed
    want = step_c(fams["contiguous"][0][0])
    for k, (cs, step, _) in fams.items():
        if k != "contiguous":
            assert torch.equal(step(cs[0]), want), k
    cands, graphs = {}, []
    order_names = list(fams) + ["contiguous_again"]
    for k in order_names:
        cs, step, att = fams[k.replace("_again", "")]
        reset = (lambda cs: lambda: [c.seqlens.fill_(Skv) for c in cs])(cs)
        reset()
        cands[f"cold_{k}"] = ((lambda cs, step: lambda i: step(cs[i % copies]))(cs, step), reset)
        g, _ = TK.graph_of((lambda c, step: lambda: step(c))(cs[0], step))
        ga, _ = TK.graph_of((lambda c, att: lambda: att(c))(cs[0], att))
        graphs += [g, ga]
        cands[f"graph_{k}"] = ((lambda g: lambda i: g.replay())(g), reset)
        cands[f"attention_graph_{k}"] = ((lambda g: lambda i: g.replay())(ga), reset)
    t = TK.timed(cands, iters, rounds)
    m = lambda k: t[k]["median_ms"]
    summary = {}
    for kind in ("cold", "graph", "attention_graph"):
        base = m(f"{kind}_contiguous")
        summary[f"{kind}_contiguous_ms"] = base
        summary[f"{kind}_contiguous_spread_pct"] = TK.spread_pct(t[f"{kind}_contiguous"])
        summary[f"{kind}_contiguous_again_over_contiguous"] = m(f"{kind}_contiguous_again") / base
        for ps, order in PAGED:
            summary[f"{kind}_paged_ps{ps}_{order}_over_contiguous"] = m(f"{kind}_paged_ps{ps}_{order}") / base
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {"measure": "paged_decode_step", "shape": name, "B": B, "Hq": Hq, "Hkv": Hkv, "Skv": Skv, "D": D, "capacity": cap, "copies": copies,
            "iters": iters, "rounds": rounds, "num_splits": _native.splitkv_auto_splits(B, Hq, Hkv, 1, cap, D, cus), "times": t, "summary": summary}


def auto_splits():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = []
    for name, (B, Hq, Hkv, Skv, D) in DECODE.items():
        rule = lambda s: _native.splitkv_auto_splits(B, Hq, Hkv, 1, s, D, cus)
        out.append({"measure": "auto_splits", "shape": name, "num_cus": cus, "live_keys": Skv, "table_keys": 4 * Skv,
                    "num_splits_with_max_seqlen_k": rule(Skv), "num_splits_without": rule(4 * Skv)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--only", default="decode,auto")
    args = ap.parse_args()
    assert args.rounds >= 1 and args.iters >= 1
    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    only = args.only.split(",")
    torch.manual_seed(0)
    if "auto" in only:
        for r in auto_splits():
            print(json.dumps(r), flush=True)
    if "decode" in only:
        for s in DECODE:
            print(json.dumps(decode(s, args.iters, args.rounds)), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the tree verify on windowed / sink layers and the rotary embedding at the caller's positions
(include/qattn_paged_varlen_tree_window.h, include/qattn_paged_varlen_rope_pos.h) against what the library
offered before them, in the same process.  As tools/time_tree.py (whose helpers this imports): HIP events around blocks of `--iters`
back-to-back replays of ONE captured graph per candidate, the candidates interleaved block by block over `--rounds` rounds, median over
the rounds, min .. max as the spread; every baseline is timed twice (first and last candidate) for its own same-run repeat; ratios are
taken within one run only.

Hq 64, Hkv 8, D 64, page size 128 (gpt-oss); shapes: 32 slots x 16 drafts over 8192 keys, 4 slots x 64 drafts over 32768 keys (the drafts
are the slots' last keys).
  (a) window   fp8_attn_paged_varlen_tree_window_func on a binary tree under (127, 0) with sinks against fp8_attn_paged_varlen_sink_func
               under the same window on the same cache -- the floor: the same keys swept, no tree; its device code is the parent
               commit's.  A chain under the tree-window call is timed beside it (the same bits as the floor, checked first).
  (b) full     ... under (-1, 0) with sinks against the composition a caller needed before: fp8_attn_paged_varlen_tree_func(return_lse=True)
               + merge_attn_states_with_sinks -- the same math, two launches, two roundings of out.
  (c) append   paged_kv_cache_append_varlen_rope_pos_fp8 at the tree's positions against apply_rope_eager at those positions +
               paged_kv_cache_append_varlen_fp8 (the same bytes, checked before anything is timed), and against the sequential fused
               append paged_kv_cache_append_varlen_rope_fp8: the floor.  No call advances the lengths (advance=False): every replay
               writes the same keys.
  (d) q        apply_rope_positions against apply_rope_eager at the same positions (the same bits, checked first)."""
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
from quantumattention_amd import _native  # noqa: E402
from time_tree import summarise  # noqa: E402

DEV, BF16 = TK.DEV, TK.BF16
PAGE, HQ, HKV, D = 128, 64, 8, 64
SHAPES = {"b32_d16_k8192": (32, 16, 8192), "b4_d64_k32768": (4, 64, 32768)}   # slots, drafts per slot, keys per slot (drafts included)
WINDOW = (127, 0)


def tables(rows):
    h = D // 2
    ang = torch.arange(rows, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(h, dtype=torch.float64) / h))[None]
    return ang.cos().float().to(DEV), ang.sin().float().to(DEV)


def run(cands, iters, rounds, reset=TK.nothing):
    timed, keep = {}, []
    for k, fn in cands:
        g, _ = TK.graph_of(fn)
        keep.append(g)
        timed[k] = ((lambda g: lambda i: g.replay())(g), reset)
    return TK.timed(timed, iters, rounds)


def measure(name, iters, rounds):
    B, n, Skv = SHAPES[name]
    total = B * n
    cc = qa.kv_cache_from_prefill_fp8(TK.rand(B, HKV, Skv - n, D), TK.rand(B, HKV, Skv - n, D), Skv + 256)
    c = TP.paged_from(cc, PAGE, "shuffled")
    del cc
    cu = torch.arange(0, total + 1, n, dtype=torch.int32, device=DEV)
    kd, vd, q = TK.rand(total, HKV, D), TK.rand(total, HKV, D), TK.rand(total, HQ, D)
    parents = torch.tensor([(p - 1) // 2 if p else -1 for p in range(n)] * B, dtype=torch.int32, device=DEV)
    words = qa.tree_mask_from_parents(parents, cu)
    chain = qa.tree_mask_from_parents(torch.tensor(list(range(-1, n - 1)) * B, dtype=torch.int32, device=DEV), cu)
    sinks = torch.randn(HQ, device=DEV)
    cos, sin = tables(c.capacity)
    pos = qa.tree_positions(words, cu, c.seqlens)                            # before the append: base + depth
    seq = qa.tree_positions(chain, cu, c.seqlens)                            # depth = index: the sequential positions
    common = {"shape": name, "B": B, "drafts": n, "Skv": Skv, "Hq": HQ, "Hkv": HKV, "D": D, "page_size": PAGE, "iters": iters, "rounds": rounds}
    out = []

    # (c) the append, on the committed cache (advance=False: the lengths stay at Skv - n)
    at = pos.clamp(0, cos.shape[0] - 1)
    def composed():
        k_rot = qa.apply_rope_eager(kd.transpose(0, 1)[None], cos[at], sin[at])[0].transpose(0, 1)
        qa.paged_kv_cache_append_varlen_fp8(c, k_rot, vd, cu, advance=False)
    fused_pos = lambda: qa.paged_kv_cache_append_varlen_rope_pos_fp8(c, kd, vd, cu, pos, cos, sin, advance=False)
    fused_seq = lambda: qa.paged_kv_cache_append_varlen_rope_fp8(c, kd, vd, cu, cos, sin, advance=False)
    states = []
    for fn in (composed, fused_pos):                                         # the same bytes either way, before anything is timed
        fn()
        states.append((c.k.clone(), c.v.clone()))
    assert torch.equal(states[0][0], states[1][0]) and torch.equal(states[0][1], states[1][1])
    qa.paged_kv_cache_append_varlen_rope_pos_fp8(c, kd, vd, cu, seq, cos, sin, advance=False)
    k_seq = c.k.clone()
    fused_seq()
    assert torch.equal(c.k, k_seq)                                           # sequential positions: the fused entry's bytes
    del states, k_seq
    t = run((("composed", composed), ("positions", fused_pos), ("sequential", fused_seq), ("composed_again", composed)), iters, rounds)
    s = summarise(t, "composed", ("positions", "sequential"))
    s["positions_over_sequential"] = t["positions"]["median_ms"] / t["sequential"]["median_ms"]
    out.append({"measure": "rope_positions_append", **common, "times": t, "summary": s})

    # (d) q's rotation
    at_q = pos.clamp(0, cos.shape[0] - 1)
    eager_q = lambda: qa.apply_rope_eager(q.transpose(0, 1)[None], cos[at_q], sin[at_q])[0].transpose(0, 1).contiguous()
    pos_q = lambda: qa.apply_rope_positions(q, pos, cos, sin)
    assert torch.equal(eager_q().view(torch.int16), pos_q().view(torch.int16))
    t = run((("eager", eager_q), ("positions", pos_q), ("eager_again", eager_q)), iters, rounds)
    out.append({"measure": "rope_positions_q", **common, "times": t, "summary": summarise(t, "eager", ("positions",))})

    # (a), (b) the attention: the drafts are the slots' last keys
    fused_pos()
    c.seqlens.fill_(Skv)
    q_rot = pos_q()
    sink_entry = lambda w: (lambda: qa.fp8_attn_paged_varlen_sink_func(q_rot, c, cu, n, sinks, w, max_seqlen_k=Skv, return_lse=True))
    tree_window = lambda w, m: (lambda: qa.fp8_attn_paged_varlen_tree_window_func(q_rot, c, cu, n, m, w, sinks=sinks, max_seqlen_k=Skv, return_lse=True))
    for x, y in zip(sink_entry(WINDOW)(), tree_window(WINDOW, chain)()):     # the same bits under a chain, before anything is timed
        assert torch.equal(x, y)
    t = run((("sink_window", sink_entry(WINDOW)), ("tree_window", tree_window(WINDOW, words)), ("tree_window_chain", tree_window(WINDOW, chain)),
             ("sink_window_again", sink_entry(WINDOW))), iters, rounds)
    out.append({"measure": "tree_window_sinks", **common, "window": list(WINDOW), "times": t,
                "summary": summarise(t, "sink_window", ("tree_window", "tree_window_chain"))})

    def composed_full():
        o, lse = qa.fp8_attn_paged_varlen_tree_func(q_rot, c, cu, n, words, max_seqlen_k=Skv, return_lse=True)
        return qa.merge_attn_states_with_sinks([o], [lse], sinks)
    full = tree_window((-1, 0), words)
    a, b_ = composed_full(), full()
    worst = float((a[0].float() - b_[0].float()).abs().max())                # the same math; the composition rounds out twice
    assert worst <= 2.0 ** -6 and float((a[1] - b_[1]).abs().max()) <= 1e-4, worst
    t = run((("composed", composed_full), ("tree_full", full), ("sink_full", sink_entry((-1, 0))), ("composed_again", composed_full)), iters, rounds)
    out.append({"measure": "tree_full_sinks", **common, "window": [-1, 0], "max_abs_out_difference": worst, "times": t,
                "summary": summarise(t, "composed", ("tree_full", "sink_full"))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--only", default=",".join(SHAPES))
    args = ap.parse_args()
    assert args.rounds >= 1 and args.iters >= 1
    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    torch.manual_seed(0)
    for name in args.only.split(","):
        for r in measure(name, args.iters, args.rounds):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()

"""Times the exact top-k selection of the lightning indexer with a row on one workgroup (num_splits 1: qattn_mla_index_select) and cut across
2 .. 256 workgroups (include/qattn_mla_index_split.h), as replayed graphs in ONE run, the variants alternated round by round (the method of
tools/time_mla_index.py), and the whole step "index append of 1 token + index top-k" under the auto rule against num_splits 1 and the torch
composition of tools/time_mla_index.py.

  sweep    mla_index_select(logits [B, 1, N], topk 2048, num_splits=s), s in 1, 2, 4, .. 256 and 0 (the auto rule), for B in 1, 4, 32 and N in
           8 192, 16 384, 32 768, 131 072; logits N(0, 1) ("normal") and max(N(0, 1), 0) ("relu": half the row is exactly zero)
  step     B 1 x 32 768, B 1 x 131 072, B 32 x 8 192: append + fp8_mla_index_topk_func with select_splits 0 and 1, and the torch composition

Every figure is the median of ROUNDS rounds of REPS replays with its own spread (min .. max over the rounds).  `beats_s1` of a row names the
split counts whose max lies below the min of s = 1: faster by more than the baseline's spread.  Needs the GPU; prints one line per row and a
JSON line at the end.

    python tools/time_mla_index_select.py [--rounds 7] [--reps 20] [--out FILE] [--batches 1,4,32] [--kinds normal,relu] [--no-steps]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantumattention_amd as qa  # noqa: E402
from quantumattention_amd import _native  # noqa: E402
from tools.time_mla_index import D, DEV, HI, PAGE, TOPK, captured, timed  # noqa: E402

SPLITS = (1, 2, 4, 8, 16, 32, 64, 128, 256)


def measure(cands, rounds, reps):
    times = {k: [] for k in cands}
    for _ in range(rounds):                    # alternated: one round times every candidate once
        for k, fn in cands.items():
            times[k].append(timed(fn, reps))
    return {k: (round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)) for k, v in times.items()}


def sweep_shape(B, N, kind, rounds, reps, cus):
    logits = torch.randn((B, 1, N), device=DEV)
    if kind == "relu":
        logits.clamp_(min=0.0)
    used = torch.full((B,), N, dtype=torch.int32, device=DEV)
    want = qa.mla_index_select(logits, TOPK, seqused_k=used, num_splits=1)
    auto = _native.mla_index_select_auto_splits(B, N, TOPK, cus)
    cands = {}
    for s in SPLITS:
        assert torch.equal(qa.mla_index_select(logits, TOPK, seqused_k=used, num_splits=s), want), (B, N, kind, s)
        cands[str(s)] = captured(lambda s=s: qa.mla_index_select(logits, TOPK, seqused_k=used, num_splits=s))
    cands["auto"] = captured(lambda: qa.mla_index_select(logits, TOPK, seqused_k=used, num_splits=0))
    t = measure(cands, rounds, reps)
    return {"B": B, "N": N, "logits": kind, "topk": TOPK, "auto_splits": auto, "us_median_min_max": t,
            "beats_s1": [k for k, v in t.items() if k not in ("1", "auto") and v[2] < t["1"][1]]}


def step_shape(B, L, rounds, reps, cus):
    M = L // PAGE + 1
    ic = qa.alloc_paged_mla_index_cache_fp8(B * M, PAGE, batch_size=B, max_pages_per_seq=M, scale=0.05, dtype=torch.bfloat16, device=DEV)
    ic.block_table.copy_(torch.randperm(B * M, device=DEV).reshape(B, M).int())
    ic.pool.copy_((torch.randn(ic.pool.shape, device=DEV) * 20.0).to(ic.pool.dtype))      # N(0, 1) keys at scale 0.05
    q = torch.randn((B, HI, 1, D), device=DEV).bfloat16()
    w = torch.randn((B, 1, HI), device=DEV) * HI ** -0.5
    new = torch.randn((B, 1, D), device=DEV).bfloat16()
    lens = torch.full((B,), L - 1, dtype=torch.int32, device=DEV)

    def step(s):
        ic.seqlens.copy_(lens)     # (a device copy inside the graph: every replay appends at the same position)
        qa.paged_mla_index_cache_append_fp8(ic, new)
        return qa.fp8_mla_index_topk_func(q, w, ic, TOPK, max_seqlen_k=L, select_splits=s)

    def baseline():
        ic.seqlens.copy_(lens)
        qa.paged_mla_index_cache_append_fp8(ic, new)
        k = ic.pool[ic.block_table.long()].reshape(B, -1, D)[:, :L].to(torch.bfloat16)
        s = torch.relu(torch.einsum("bhic,bjc->bihj", q, k).float())
        logits = (s * w[..., None]).sum(dim=2) * ic.scale[:, None, None]
        return torch.topk(logits, TOPK, dim=-1).indices

    assert torch.equal(step(0), step(1))
    t = measure({"step_auto": captured(lambda: step(0)), "step_s1": captured(lambda: step(1)), "torch": captured(baseline)}, rounds, reps)
    return {"B": B, "L": L, "Hi": HI, "topk": TOPK, "auto_splits": _native.mla_index_select_auto_splits(B, L, TOPK, cus), "us_median_min_max": t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,4,32", help="the B of the sweep (Sq 1: the rows), comma-separated")
    ap.add_argument("--kinds", default="normal,relu")
    ap.add_argument("--no-steps", action="store_true", help="the sweep alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_mla_index_select.py measures on the GPU; none found")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sweep, steps = [], []
    for kind in a.kinds.split(","):
        for B in (int(b) for b in a.batches.split(",")):
            for N in (8192, 16384, 32768, 131072):
                sweep.append(sweep_shape(B, N, kind, a.rounds, a.reps, cus))
                print(sweep[-1], flush=True)
    for B, L in () if a.no_steps else ((1, 32768), (1, 131072), (32, 8192)):
        steps.append(step_shape(B, L, a.rounds, a.reps, cus))
        print(steps[-1], flush=True)
    line = json.dumps({"tool": "time_mla_index_select", "device": torch.cuda.get_device_name(0), "cus": cus, "rounds": a.rounds, "reps": a.reps,
                       "library": os.path.basename(_native.LIB_PATH), "sweep": sweep, "steps": steps})
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

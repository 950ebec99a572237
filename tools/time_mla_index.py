"""Times the lightning indexer's step "index append of 1 token + index top-k" (include/qattn_mla_index.h) at topk 2048, Hi 64 as a replayed
graph against the torch composition it replaces, in ONE run, the candidates alternated round by round (the method of
tools/time_mla_sparse.py):

  step     paged_mla_index_cache_append_fp8 + fp8_mla_index_topk_func (the scores launch and the selection launch)
  scores   the scores launch alone (qattn_fp8_mla_index_scores into the caller's logits)
  select   the selection launch alone (mla_index_select on the logits of the step's own data)
  torch    the baseline: de-quantise the gathered index keys, einsum with the de-quantised q, relu, weighted head sum, torch.topk -- eager
           torch ops on the same cache bytes, also captured and replayed (the gather through the table included: it is part of what a
           caller without the kernels has to do)

Shapes: Sq 1; B 1 over 32 768 and 131 072 keys, B 32 over 8 192 keys.  Every figure is the median of ROUNDS rounds of REPS replays with its
own spread (min .. max over the rounds).  The score sweep's QATTN_MLA_INDEX_WG_KEYS is a build-time constant: time a variant library with
QUANTUM_ATTN_LIBRARY=tools/ab_libs/libqattn_<variant>.so.  Needs the GPU; prints one line per shape and a JSON line at the end.

    python tools/time_mla_index.py [--rounds 7] [--reps 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantumattention_amd as qa  # noqa: E402
from quantumattention_amd import _native  # noqa: E402

TOPK, HI, D, PAGE = 2048, 64, 128, 64
DEV = "cuda"


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps     # us


def captured(step):
    step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    return g.replay


def one_shape(B, L, rounds, reps):
    M = L // PAGE + 1
    ic = qa.alloc_paged_mla_index_cache_fp8(B * M, PAGE, batch_size=B, max_pages_per_seq=M, scale=0.05, dtype=torch.bfloat16, device=DEV)
    ic.block_table.copy_(torch.randperm(B * M, device=DEV).reshape(B, M).int())
    ic.pool.copy_((torch.randn(ic.pool.shape, device=DEV) * 20.0).to(ic.pool.dtype))      # N(0, 1) keys at scale 0.05
    q = torch.randn((B, HI, 1, D), device=DEV).bfloat16()
    w = torch.randn((B, 1, HI), device=DEV) * HI ** -0.5
    new = torch.randn((B, 1, D), device=DEV).bfloat16()
    lens, full = torch.full((B,), L - 1, dtype=torch.int32, device=DEV), torch.full((B,), L, dtype=torch.int32, device=DEV)
    kw = dict(num_pages=ic.num_pages, page_size=PAGE, is_causal=True)

    def step():
        ic.seqlens.copy_(lens)     # (a 4 B-byte device copy inside the graph: every replay appends at the same position)
        qa.paged_mla_index_cache_append_fp8(ic, new)
        return qa.fp8_mla_index_topk_func(q, w, ic, TOPK, max_seqlen_k=L)

    def baseline():
        ic.seqlens.copy_(lens)
        qa.paged_mla_index_cache_append_fp8(ic, new)     # (the append has no torch form without a host read; the kernel's is used)
        k = ic.pool[ic.block_table.long()].reshape(B, -1, D)[:, :L].to(torch.bfloat16)
        s = torch.relu(torch.einsum("bhic,bjc->bihj", q, k).float())
        logits = (s * w[..., None]).sum(dim=2) * ic.scale[:, None, None]
        return torch.topk(logits, TOPK, dim=-1).indices

    ic.seqlens.copy_(full)
    logits = _native.fp8_mla_index_topk(q, w, ic.pool, ic.scale, ic.block_table, full, Skv=L, topk=TOPK, select=False, **kw)[1]
    cands = {"step": captured(step), "torch": captured(baseline),
             "scores": captured(lambda: _native.fp8_mla_index_topk(q, w, ic.pool, ic.scale, ic.block_table, full, Skv=L, topk=TOPK, select=False, **kw)),
             "select": captured(lambda: qa.mla_index_select(logits, TOPK, seqused_k=full))}
    times = {k: [] for k in cands}
    for _ in range(rounds):                    # alternated: one round times every candidate once
        for k, fn in cands.items():
            times[k].append(timed(fn, reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"B": B, "L": L, "Hi": HI, "topk": TOPK, "wg_keys_python": _native.MLA_INDEX_WG_KEYS, "library": os.path.basename(_native.LIB_PATH)}
    for k, v in times.items():
        res[k + "_us"] = round(med[k], 2)
        res[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    res["torch_over_step"] = round(med["torch"] / med["step"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_mla_index.py measures on the GPU; none found")
    rows = []
    for B, L in ((1, 32768), (1, 131072), (32, 8192)):
        rows.append(one_shape(B, L, a.rounds, a.reps))
        print(rows[-1], flush=True)
    line = json.dumps({"tool": "time_mla_index", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "rows": rows})
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

"""Times the lightning indexer on a PROMPT: the packed call (include/qattn_mla_index_prefill.h: 8 tokens share every key tile through LDS)
against the only form there was, the dense entry `fp8_mla_index_topk_func` on the same tokens (one workgroup per position pulls its keys
from global memory), at Hi 64, topk 2048, bottom-right causal, in ONE run, the candidates alternated round by round as replayed graphs (the
method of tools/time_mla_index.py):

  packed_scores / dense_scores   the score launch alone, logits with a filled tail into the caller's rows
  packed_call   / dense_call     the whole call: scores into the workspace and the exact top-k selection

Shapes (slots x tokens per slot over keys per slot): 1 x 4096 over 4096 (a whole prompt), 1 x 2048 over 32 768 (a chunk behind its cached
prefix), 4 x 1024 over 1024.  Before timing, the packed logits and indices are compared with the dense entry's bit for bit at the timed
size ("equal").  Every figure is the median of ROUNDS rounds of REPS replays with its own spread (min .. max over the rounds); a ratio is
dense / packed of the medians, and "wins" says whether the packed scores' max lies below the dense scores' min.  Needs the GPU; prints one
line per shape and a JSON line at the end.

    python tools/time_mla_index_prefill.py [--rounds 7] [--reps 10] [--out FILE]"""
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


def one_shape(B, n, L, rounds, reps):
    M = L // PAGE + 1
    ic = qa.alloc_paged_mla_index_cache_fp8(B * M, PAGE, batch_size=B, max_pages_per_seq=M, scale=0.05, dtype=torch.bfloat16, device=DEV)
    ic.block_table.copy_(torch.randperm(B * M, device=DEV).reshape(B, M).int())
    ic.pool.copy_((torch.randn(ic.pool.shape, device=DEV) * 20.0).to(ic.pool.dtype))      # N(0, 1) keys at scale 0.05
    ic.seqlens.fill_(L)
    q = torch.randn((B * n, HI, D), device=DEV).bfloat16()
    w = torch.randn((B * n, HI), device=DEV) * HI ** -0.5
    cu = torch.arange(B + 1, dtype=torch.int32, device=DEV) * n
    qd, wd = q.view(B, n, HI, D).transpose(1, 2), w.view(B, n, HI)                       # the same tokens as the dense entry reads them (views)
    kw = dict(Skv=L, topk=TOPK, num_pages=ic.num_pages, page_size=PAGE, is_causal=True)
    head = (ic.pool, ic.scale, ic.block_table)
    packed_scores = lambda: _native.fp8_mla_index_topk_varlen(q, w, *head, cu, ic.seqlens, select=False, **kw)[1]
    dense_scores = lambda: _native.fp8_mla_index_topk(qd, wd, *head, ic.seqlens, select=False, **kw)[1]
    packed_call = lambda: qa.fp8_mla_index_topk_varlen_func(q, w, ic, cu, TOPK, max_seqlen_k=L)
    dense_call = lambda: qa.fp8_mla_index_topk_func(qd, wd, ic, TOPK, max_seqlen_k=L)
    equal = bool(torch.equal(packed_scores().view(torch.int32), dense_scores().view(torch.int32).view(B * n, L))
                 and torch.equal(packed_call(), dense_call().view(B * n, TOPK)))
    cands = {"packed_scores": captured(packed_scores), "dense_scores": captured(dense_scores),
             "packed_call": captured(packed_call), "dense_call": captured(dense_call)}
    times = {k: [] for k in cands}
    for _ in range(rounds):                    # alternated: one round times every candidate once
        for k, fn in cands.items():
            times[k].append(timed(fn, reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"B": B, "tokens": n, "L": L, "Hi": HI, "topk": TOPK, "equal": equal, "library": os.path.basename(_native.LIB_PATH)}
    for k, v in times.items():
        res[k + "_us"] = round(med[k], 1)
        res[k + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
    res["scores_dense_over_packed"] = round(med["dense_scores"] / med["packed_scores"], 2)
    res["call_dense_over_packed"] = round(med["dense_call"] / med["packed_call"], 2)
    res["wins"] = max(times["packed_scores"]) < min(times["dense_scores"])
    # what the algorithm needs: Hi x 128 MACs per causal (token, key) pair
    pairs = B * sum(max(L - n + i + 1, 0) for i in range(n))
    res["packed_scores_tflops"] = round(2.0 * pairs * HI * D / med["packed_scores"] * 1e-6, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_mla_index_prefill.py measures on the GPU; none found")
    rows = []
    for B, n, L in ((1, 4096, 4096), (1, 2048, 32768), (4, 1024, 1024)):
        rows.append(one_shape(B, n, L, a.rounds, a.reps))
        print(rows[-1], flush=True)
    line = json.dumps({"tool": "time_mla_index_prefill", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "rows": rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

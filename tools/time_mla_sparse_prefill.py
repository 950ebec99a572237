"""Times sparse MLA on a PROMPT: the packed call (include/qattn_mla_sparse_prefill.h: one 8-wave workgroup per token and 128 heads) against
the only form there was, the 64-row kernel of `fp8_mla_paged_sparse_func` with num_splits=1 on the same tokens and lists -- at B = 1, Sq = n
for a one-prompt shape, as the per-slot loop for several prompts -- at topk 2048, bottom-right causal, in ONE run, the two alternated round
by round as replayed graphs (the method of tools/time_mla_index_prefill.py).  The lists come from the prefill indexer on random data.

Shapes (slots x tokens per slot over keys per slot, Hq): 1 x 4096 over 4096 at Hq 128 and at Hq 16 (a tensor-parallel shard: three quarters
of the 128-row tile idle), 1 x 2048 over 32 768 (a chunk behind its cached prefix), 4 x 1024 over 1024.  Before timing, out and lse of the
two are compared bit for bit at the timed size ("equal").  Every figure is the median of ROUNDS rounds of REPS replays with its own spread
(min .. max over the rounds); the ratio is baseline / packed of the medians, and "wins" says whether the packed call's max lies below the
baseline's min.  Needs the GPU; prints one line per shape and a JSON line at the end.

    python tools/time_mla_sparse_prefill.py [--rounds 7] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantumattention_amd as qa  # noqa: E402
from quantumattention_amd import _native  # noqa: E402
from quantumattention_amd.mla import PagedMLACacheFP8  # noqa: E402

TOPK, HI, PAGE, SCALE = 2048, 64, 64, 192.0 ** -0.5
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


def one_shape(B, n, L, Hq, rounds, reps):
    M = L // PAGE + 1
    table = torch.randperm(B * M, device=DEV).reshape(B, M).int()
    ic = qa.alloc_paged_mla_index_cache_fp8(B * M, PAGE, batch_size=B, max_pages_per_seq=M, scale=0.05, dtype=torch.bfloat16, device=DEV)
    rc = qa.alloc_paged_mla_row_cache_fp8(B * M, PAGE, batch_size=B, max_pages_per_seq=M, scale=0.05, dtype=torch.bfloat16, device=DEV)
    for c in (ic, rc):
        c.block_table.copy_(table)
        c.pool.copy_((torch.randn(c.pool.shape, device=DEV) * 20.0).to(c.pool.dtype))       # N(0, 1) keys at scale 0.05
        c.seqlens.fill_(L)
    cu = torch.arange(B + 1, dtype=torch.int32, device=DEV) * n
    idx = qa.fp8_mla_index_topk_varlen_func(torch.randn((B * n, HI, 128), device=DEV).bfloat16(), torch.randn((B * n, HI), device=DEV) * HI ** -0.5,
                                            ic, cu, TOPK, max_seqlen_k=L)
    q = torch.randn((B * n, Hq, 576), device=DEV).bfloat16()
    slots = [PagedMLACacheFP8(rc.pool, rc.scale[b:b + 1], rc.block_table[b:b + 1], rc.seqlens[b:b + 1], rc.num_pages, PAGE, rc.fp8_format,
                              rc.dtype, rc.layout) for b in range(B)]
    packed = lambda: qa.fp8_mla_paged_sparse_varlen_func(q, rc, idx, cu, scale=SCALE, return_lse=True)
    base = lambda: [qa.fp8_mla_paged_sparse_func(q[b * n:(b + 1) * n].transpose(0, 1)[None], slots[b], idx[None, b * n:(b + 1) * n], scale=SCALE,
                                                 num_splits=1, return_lse=True) for b in range(B)]
    (p_o, p_l), want = packed(), base()
    equal = all(torch.equal(p_o[b * n:(b + 1) * n].view(torch.int16), want[b][0][0].transpose(0, 1).view(torch.int16))
                and torch.equal(p_l[:, b * n:(b + 1) * n].view(torch.int32), want[b][1][0].view(torch.int32)) for b in range(B))
    del p_o, p_l, want
    cands = {"packed": captured(packed), "baseline": captured(base)}
    times = {k: [] for k in cands}
    for _ in range(rounds):                    # alternated: one round times every candidate once
        for k, fn in cands.items():
            times[k].append(timed(fn, reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"B": B, "tokens": n, "L": L, "Hq": Hq, "topk": TOPK, "equal": bool(equal), "library": os.path.basename(_native.LIB_PATH)}
    for k, v in times.items():
        res[k + "_us"] = round(med[k], 1)
        res[k + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
    res["baseline_over_packed"] = round(med["baseline"] / med["packed"], 2)
    res["wins"] = max(times["packed"]) < min(times["baseline"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_mla_sparse_prefill.py measures on the GPU; none found")
    rows = []
    for B, n, L, Hq in ((1, 4096, 4096, 128), (1, 2048, 32768, 128), (4, 1024, 1024, 128), (1, 4096, 4096, 16)):
        rows.append(one_shape(B, n, L, Hq, a.rounds, a.reps))
        print(rows[-1], flush=True)
    line = json.dumps({"tool": "time_mla_sparse_prefill", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "rows": rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

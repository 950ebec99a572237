"""Times the sparse MLA decode step "row append of 1 token + sparse attend" (include/qattn_mla_sparse.h) at topk 2048 as a replayed graph against
the two dense steps that bracket it, in ONE run, the candidates alternated round by round (the method of tools/time_mla.py):

  sparse_random / sparse_clustered
           paged_mla_row_cache_append_fp8 + fp8_mla_paged_sparse_func (num_splits 0: the auto rule) over L keys, the 2048 listed positions
           uniformly random / 32 runs of 64 consecutive positions at random starts
  dense    (a) what the library had before: paged_mla_cache_append_fp8 + fp8_mla_paged_func over ALL L keys of a chunk-image cache
  floor    (b) the same dense step on a chunk-image cache that holds only topk keys: the same bytes, contiguous, through the kernel the
           sparse one is derived from.  The sparse step is expected above it by the cost of the gather and the resolve pass
  ns=...   the sparse step (random lists) at every fixed split count of NS_SWEEP the shape admits: what the auto rule's E is chosen from

Shapes: Sq 1, Hq 16 and 128; B 1 over 32 768 and 131 072 keys, B 32 over 8 192 keys.  Every figure is the median of ROUNDS rounds of REPS
replays with its own spread (min .. max over the rounds).  Needs the GPU; prints one line per shape and a JSON line at the end.

    python tools/time_mla_sparse.py [--rounds 7] [--reps 20] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantumattention_amd as qa  # noqa: E402

SCALE = 1.0 / math.sqrt(192.0)
TOPK = 2048
NS_SWEEP = (1, 2, 4, 8, 16, 32)
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


def _filled(alloc, B, L, page):
    M = L // page + 1
    cache = alloc(B * M, page, batch_size=B, max_pages_per_seq=M, scale=0.05, dtype=torch.bfloat16, device=DEV)
    cache.block_table.copy_(torch.randperm(B * M, device=DEV).reshape(B, M).int())
    cache.pool.view(torch.uint8).copy_(torch.randint(0, 0x78, cache.pool.shape, dtype=torch.uint8, device=DEV))   # finite e4m3 bytes
    return cache


def one_shape(B, L, Hq, rounds, reps):
    q = torch.randn((B, Hq, 1, 576), device=DEV).bfloat16()
    new = torch.randn((B, 1, 576), device=DEV).bfloat16()
    row, whole, small = (_filled(qa.alloc_paged_mla_row_cache_fp8, B, L, 64), _filled(qa.alloc_paged_mla_cache_fp8, B, L, 64),
                         _filled(qa.alloc_paged_mla_cache_fp8, B, TOPK, 64))
    lists = {"random": torch.randint(0, L, (B, 1, TOPK), device=DEV, dtype=torch.int32),
             "clustered": (torch.randint(0, L - 64, (B, 1, TOPK // 64, 1), device=DEV, dtype=torch.int32)
                           + torch.arange(64, device=DEV, dtype=torch.int32)).reshape(B, 1, TOPK)}

    def step(cache, n, append, attend):
        lens = torch.full((B,), n - 1, dtype=torch.int32, device=DEV)
        def run():
            cache.seqlens.copy_(lens)     # (a 4 B-byte device copy inside the graph: every replay appends at the same position)
            append(cache, new[..., :512], new[..., 512:])
            return attend(cache)
        return captured(run)

    sparse = lambda idx, ns: step(row, L, qa.paged_mla_row_cache_append_fp8,
                                  lambda c: qa.fp8_mla_paged_sparse_func(q, c, idx, scale=SCALE, num_splits=ns))
    dense = lambda cache, n: step(cache, n, qa.paged_mla_cache_append_fp8, lambda c: qa.fp8_mla_paged_func(q, c, scale=SCALE, max_seqlen_k=n))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cands = {"sparse_random": sparse(lists["random"], 0), "sparse_clustered": sparse(lists["clustered"], 0), "dense": dense(whole, L),
             "floor": dense(small, TOPK)}
    for ns in NS_SWEEP:
        if B * -(-Hq // 64) * ns <= cus:
            cands[f"ns={ns}"] = sparse(lists["random"], ns)
    times = {k: [] for k in cands}
    for _ in range(rounds):                    # alternated: one round times every candidate once
        for k, fn in cands.items():
            times[k].append(timed(fn, reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"B": B, "L": L, "Hq": Hq, "topk": TOPK, "auto_splits": qa._native.mla_sparse_auto_splits(B, Hq, 1, TOPK, cus),
           "dense_splits": qa._native.mla_auto_splits(B, Hq, 1, L, cus), "floor_splits": qa._native.mla_auto_splits(B, Hq, 1, TOPK, cus)}
    for k, v in times.items():
        res[k + "_us"] = round(med[k], 2)
        res[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    res["dense_over_sparse_random"] = round(med["dense"] / med["sparse_random"], 2)
    res["sparse_random_over_floor"] = round(med["sparse_random"] / med["floor"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_mla_sparse.py measures on the GPU; none found")
    rows = []
    for B, L in ((1, 32768), (1, 131072), (32, 8192)):
        for Hq in (16, 128):
            rows.append(one_shape(B, L, Hq, a.rounds, a.reps))
            print(rows[-1], flush=True)
    line = json.dumps({"tool": "time_mla_sparse", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "rows": rows})
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

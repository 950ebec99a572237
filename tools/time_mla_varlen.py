"""Times dense MLA on PACKED variable-length queries (include/qattn_mla_varlen.h: one 8-wave workgroup per 128-row tile of a slot and key
split) against the forms `fp8_mla_paged_func` offers for the same step, in ONE run, the candidates alternated round by round as replayed
graphs (the method of tools/time_mla_sparse_prefill.py), every call with its own num_splits = 0 rule:

  decode   every slot n tokens: the dense call with Sq = n -- the shapes the dense entry was built for;
  mixed    one 512-token chunk beside 31 decodes over 8192 keys: the dense call on q right-aligned and padded to Sq = 512 ("padded"), and 32
           per-slot dense calls in one graph ("per_slot");
  chunk    one 2048-token chunk over 32 768 keys: the dense call with Sq = 2048.

Before timing, out and lse of the packed call are compared bit for bit with the per-slot dense calls at the packed call's split count
("equal").  Every figure is the median of ROUNDS rounds of REPS replays with its own spread (min .. max over the rounds); "wins" / "loses" say
whether the packed call's spread lies wholly below / above the baseline's.  Needs the GPU; prints one line per shape and a JSON line at the end.

    python tools/time_mla_varlen.py [--rounds 7] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantumattention_amd as qa  # noqa: E402
from quantumattention_amd import _native, mla_varlen  # noqa: E402
from quantumattention_amd.mla import PagedMLACacheFP8  # noqa: E402

PAGE, SCALE = 64, 192.0 ** -0.5
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


def one_shape(name, counts, L, Hq, rounds, reps):
    B, total, nmax = len(counts), sum(counts), max(counts)
    M = L // PAGE
    cache = qa.alloc_paged_mla_cache_fp8(B * M, PAGE, batch_size=B, max_pages_per_seq=M, scale=0.05, dtype=torch.bfloat16, device=DEV)
    cache.block_table.copy_(torch.randperm(B * M, device=DEV).reshape(B, M).int())
    cache.pool.copy_((torch.randn(cache.pool.shape, device=DEV) * 20.0).to(torch.float8_e4m3fn).view(torch.uint8))   # N(0, 1) keys at scale 0.05
    cache.seqlens.fill_(L)
    ends = [0]
    for n in counts:
        ends.append(ends[-1] + n)
    cu = torch.tensor(ends, dtype=torch.int32, device=DEV)
    q = torch.randn((total, Hq, 576), device=DEV).bfloat16()
    slots = [PagedMLACacheFP8(cache.pool, cache.scale[b:b + 1], cache.block_table[b:b + 1], cache.seqlens[b:b + 1], cache.num_pages, PAGE,
                              cache.fp8_format, cache.dtype, cache.layout) for b in range(B)]
    qs = [q[ends[b]:ends[b + 1]].transpose(0, 1)[None] for b in range(B)]
    per_slot = lambda ns=0: [qa.fp8_mla_paged_func(qs[b], slots[b], scale=SCALE, max_seqlen_k=L, num_splits=ns, return_lse=True) for b in range(B)]
    cands = {"packed": lambda: qa.fp8_mla_paged_varlen_func(q, cache, cu, nmax, scale=SCALE, max_seqlen_k=L, return_lse=True)}
    ns = mla_varlen._resolve_splits(0, B, total, Hq, L, q.device)
    (p_o, p_l), want = cands["packed"](), per_slot(ns)
    equal = all(torch.equal(p_o[ends[b]:ends[b + 1]].view(torch.int16), want[b][0][0].transpose(0, 1).view(torch.int16))
                and torch.equal(p_l[:, ends[b]:ends[b + 1]].view(torch.int32), want[b][1][0].view(torch.int32)) for b in range(B))
    del p_o, p_l, want
    if len(set(counts)) == 1:      # every slot the same count: the dense call as it is
        qd = q.view(B, nmax, Hq, 576).transpose(1, 2)
        cands["dense"] = lambda: qa.fp8_mla_paged_func(qd, cache, scale=SCALE, max_seqlen_k=L, return_lse=True)
    else:
        qp = torch.zeros((B, Hq, nmax, 576), dtype=q.dtype, device=DEV)
        for b in range(B):
            qp[b, :, nmax - counts[b]:] = qs[b][0]     # right-aligned: bottom-right causal gives the live rows their own keys
        cands["padded"] = lambda: qa.fp8_mla_paged_func(qp, cache, scale=SCALE, max_seqlen_k=L, return_lse=True)
        cands["per_slot"] = per_slot
    cands = {k: captured(fn) for k, fn in cands.items()}
    times = {k: [] for k in cands}
    for _ in range(rounds):                    # alternated: one round times every candidate once
        for k, fn in cands.items():
            times[k].append(timed(fn, reps))
    res = {"case": name, "B": B, "tokens": total, "max_tokens": nmax, "L": L, "Hq": Hq, "packed_splits": ns, "equal": bool(equal),
           "library": os.path.basename(_native.LIB_PATH)}
    for k, v in times.items():
        res[k + "_us"] = round(statistics.median(v), 1)
        res[k + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
        if k != "packed":
            res[k + "_over_packed"] = round(statistics.median(v) / statistics.median(times["packed"]), 2)
            res["vs_" + k] = "wins" if max(times["packed"]) < min(v) else "loses" if min(times["packed"]) > max(v) else "overlap"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_mla_varlen.py measures on the GPU; none found")
    mixed = (512,) + (1,) * 31
    rows = []
    for name, counts, L, Hq in (("decode", (4,) * 32, 8192, 128), ("decode", (1,) * 32, 8192, 16), ("decode", (1,), 32768, 16),
                                ("mixed", mixed, 8192, 128), ("mixed", mixed, 8192, 16), ("chunk", (2048,), 32768, 128)):
        rows.append(one_shape(name, counts, L, Hq, a.rounds, a.reps))
        print(rows[-1], flush=True)
    line = json.dumps({"tool": "time_mla_varlen", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "rows": rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

"""Times the MLA decode step "append 1 + attend" (include/qattn_mla.h) as a replayed graph against what a user has without it and against the
byte floor, in ONE run, the candidates alternated round by round:

  mla      paged_mla_cache_append_fp8 + fp8_mla_paged_func, captured once, replayed
  sdpa     torch SDPA in bf16 on the DE-QUANTISED latent [B, 1, L, 576] / values [..., :512], the Hq Sq rows of a slot as the
           queries of its one kv head, under the same bottom-right causal mask as the MLA step (a boolean attn_mask [Hq Sq, L] at Sq > 1;
           at Sq 1 the mask hides nothing and none is passed).  The de-quantisation itself is NOT timed: the baseline is handed a bf16
           cache it would have to keep or rebuild
  floor    the cache bytes the step must read (B L 576) over the rate a plain device copy of that many bytes holds in this run.  This is
           the yardstick the feature's issue defines, NOT a true lower bound: the copy also WRITES as many bytes as it reads, and at B 1
           its 18.9 MB source may be served from the on-chip cache between replays -- a kernel that only reads could beat it

Shapes: B 1 / 32 768 keys and B 32 / 8 192 keys, Hq 128 and 16, Sq 1 and 4.  Every figure is the median of ROUNDS rounds of REPS replays with
its own spread (min .. max over the rounds).  Needs the GPU; prints one line per shape and a JSON line at the end.

    python tools/time_mla.py [--rounds 7] [--reps 20] [--out FILE]"""
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


def one_shape(B, L, Hq, Sq, rounds, reps):
    dev, page = "cuda", 64
    M = L // page + 1
    cache = qa.alloc_paged_mla_cache_fp8(B * M, page, batch_size=B, max_pages_per_seq=M, scale=0.05, dtype=torch.bfloat16, device=dev)
    cache.block_table.copy_(torch.randperm(B * M, device=dev).reshape(B, M).int())
    cache.pool.copy_(torch.randint(0, 0x78, cache.pool.shape, dtype=torch.uint8, device=dev))
    q = torch.randn((B, Hq, Sq, 576), device=dev).bfloat16()
    new = torch.randn((B, 1, 576), device=dev).bfloat16()
    lens = torch.full((B,), L - 1, dtype=torch.int32, device=dev)

    def mla_step():
        cache.seqlens.copy_(lens)     # (a 4 B-byte device copy inside the graph: every replay appends at the same position)
        qa.paged_mla_cache_append_fp8(cache, new[..., :512], new[..., 512:])
        return qa.fp8_mla_paged_func(q, cache, scale=SCALE, max_seqlen_k=L)

    lat = torch.randn((B, 1, L, 576), device=dev).bfloat16()
    qm = q.reshape(B, 1, Hq * Sq, 576)         # all heads share the latent: one kv head, the (head, position) rows as its queries (unmasked)
    mask = None
    if Sq > 1:                                 # row (h, i) attends keys j <= L - Sq + i, as causal=True of the MLA step
        pos = torch.arange(Hq * Sq, device=dev) % Sq
        mask = torch.arange(L, device=dev)[None, :] <= (L - Sq + pos)[:, None]
    sdpa_step = lambda: torch.nn.functional.scaled_dot_product_attention(qm, lat, lat[..., :512], attn_mask=mask, scale=SCALE)
    src = torch.empty((B * L * 576,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    cands = {"mla": captured(mla_step), "sdpa": captured(sdpa_step), "copy": captured(lambda: dst.copy_(src))}
    times = {k: [] for k in cands}
    for _ in range(rounds):                    # alternated: one round times every candidate once
        for k, fn in cands.items():
            times[k].append(timed(fn, reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"B": B, "L": L, "Hq": Hq, "Sq": Sq, "splits": qa._native.mla_auto_splits(B, Hq, Sq, L, torch.cuda.get_device_properties(0).multi_processor_count)}
    for k, v in times.items():
        res[k + "_us"] = round(med[k], 2)
        res[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    res["floor_us"] = res["copy_us"]           # B L 576 bytes read at the copy's rate (the issue's yardstick, not a lower bound: docstring)
    res["mla_over_floor"] = round(med["mla"] / med["copy"], 2)
    res["sdpa_over_mla"] = round(med["sdpa"] / med["mla"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_mla.py measures on the GPU; none found")
    rows = []
    for B, L in ((1, 32768), (32, 8192)):
        for Hq in (128, 16):
            for Sq in (1, 4):
                rows.append(one_shape(B, L, Hq, Sq, a.rounds, a.reps))
                print(rows[-1], flush=True)
    line = json.dumps({"tool": "time_mla", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "rows": rows})
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

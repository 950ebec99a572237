"""What tests/test_cpu_mla_varlen.py and tests/test_gpu_mla_varlen.py share (include/qattn_mla_varlen.h): packed problems on tests/mla_cases.py's
exact value grid -- the smallest at which the tile map, the 32-row blocks and the split plan can go wrong -- and the fp64 oracle per slot."""
import numpy as np
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, mla
from tests import mla_cases as C

PAD = 3   # bucket rows behind cu[B]; their q is NaN
# (Hq, tokens per slot, keys per slot): 9 x 16 = 144 rows cross a 128-row tile, an empty slot / 140 and 60 rows, no multiples of 32 / one tile
# per token.  The lengths cover {0, 1, 63, 64, 65, 130, 200} and L_b < n_b (rows without a key).
CASES = [(16, (1, 0, 5, 9), (200, 64, 1, 130)), (16, (1, 0, 5, 9), (63, 0, 65, 64)), (20, (7, 3), (65, 0)), (20, (7, 3), (130, 1)),
         (128, (1, 0, 2), (200, 63, 1)), (128, (1, 0, 2), (64, 130, 65))]


def cu_of(counts, device="cpu"):
    return torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=device)


def make_q(Hq, counts, dtype=torch.bfloat16, seed=0):
    """[sum(counts) + PAD, Hq, 576]: the grid with channel 0 = +-3.5 (scale_q = 2^-7 exactly); the bucket rows are NaN"""
    total = sum(counts)
    q = C.draw((total + PAD, Hq, C.D), seed)
    q[..., 0] = 3.5 * torch.where(C.draw((total + PAD, Hq), seed + 1) < 0, -1.0, 1.0)
    q[total:] = float("nan")
    return q.to(dtype)


def make_cache(device, B, page, lens, dtype=torch.bfloat16, fmt="e4m3", table_seed=7, prefill=0):
    """a cache of B slots of C.CAP keys behind a shuffled table; slot b holds the first lens[b] rows of the latent (returned, [B, CAP, 576])"""
    M = C.CAP // page
    g = torch.Generator().manual_seed(table_seed)
    cache = qa.alloc_paged_mla_cache_fp8(B * M + 3, page, batch_size=B, max_pages_per_seq=M, scale=C.SCALE_KV, dtype=dtype, device=device,
                                         fp8_format=fmt)
    cache.pool.view(torch.uint8).fill_(prefill)
    cache.block_table.copy_(torch.randperm(B * M + 3, generator=g)[: B * M].reshape(B, M).to(torch.int32))
    lat = (C.draw((B, C.CAP, C.D), 100) * C.SCALE_KV).to(dtype)
    dl = lat.to(device)
    qa.paged_mla_cache_append_fp8(cache, dl[..., :C.DV], dl[..., C.DV:], new_lens=torch.tensor(lens, dtype=torch.int32, device=device))
    return cache, lat


def slot_view(cache, b):
    return mla.PagedMLACacheFP8(cache.pool, cache.scale[b:b + 1], cache.block_table[b:b + 1], cache.seqlens[b:b + 1], cache.num_pages,
                                cache.page_size, cache.fp8_format, cache.dtype, cache.layout)


def dequant(cache):
    """fp64 [B, CAP, 576]: the cache's bytes gathered through the table"""
    rows = cache.pool if cache.layout == "rowmajor" else mla.pool_rowmajor(cache.pool, cache.num_pages, cache.page_size).view(_native.fp8_dtype_of(cache.fp8_format))
    return (rows[cache.block_table.long()].reshape(cache.batch_size, -1, C.D).double() * cache.scale.double()[:, None, None]).cpu().numpy()


def reference(qd, lat, counts, lens, causal):
    """fp64 softmax attention per slot (C.reference with Sq = n_b): qd [total + PAD, Hq, 576] -> (out [total + PAD, Hq, 512], lse [Hq, total + PAD]);
    the bucket rows are zero rows with lse -inf"""
    qd = np.asarray(qd, np.float64)
    out, lse, lo = np.zeros(qd.shape[:2] + (C.DV,)), np.full((qd.shape[1], qd.shape[0]), -np.inf), 0
    for b, n in enumerate(counts):
        if n:
            o, l = C.reference(qd[lo:lo + n].transpose(1, 0, 2)[None], lat[b:b + 1], lens[b:b + 1], C.SM_SCALE, causal)
            out[lo:lo + n], lse[:, lo:lo + n] = o[0].transpose(1, 0, 2), l[0]
        lo += n
    return out, lse


def check_against_reference(got_o, got_l, ref, what):
    from tests.gpu_utils import assert_within_bound
    got_o, got_l, fin = got_o.float().cpu().numpy(), got_l.cpu().numpy(), np.isfinite(ref[1])
    print(what, "max |err| out", np.abs(got_o - ref[0]).max(), "lse", np.abs(got_l[fin] - ref[1][fin]).max() if fin.any() else 0.0)
    assert_within_bound(got_o, ref[0], what=what)
    assert np.array_equal(np.isneginf(got_l), ~fin), what              # a row without a key and a bucket row: LSE -inf exactly ...
    assert (got_o[(~fin).T] == 0).all(), what                           # ... and a zero row
    assert not fin.any() or np.abs(got_l[fin] - ref[1][fin]).max() <= C.LSE_TOL, what

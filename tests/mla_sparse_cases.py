"""What tests/test_cpu_mla_sparse.py and tests/test_gpu_mla_sparse.py share (include/qattn_mla_sparse.h), on top of tests/mla_cases.py: the cases
of the oracle sweep, seeded index lists, a row-major cache filled through the append, and the fp64 oracle -- plain softmax attention over the
listed VALID keys, in list order, duplicates counted as often as they are listed."""
import numpy as np
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import mla_cases as C

TOPKS = (1, 63, 64, 65, 200)     # one entry / a group less one / one group / a group and a tail / three groups and a tail
PAGES = (1, 16, 64)
CASES = [(Hq, Sq, topk, causal, "e4m3", torch.bfloat16) for Hq, Sq in C.SHAPES for topk in TOPKS for causal in (True, False)]
CASES.append((16, 4, 65, True, "e5m2", torch.float16))


def draw_indices(Sq, topk, seed):
    """int32 [B, Sq, topk] from [-1, CAP); from four entries on every row holds a -1, a duplicate of entry 0 and a position at or behind
    every limit (CAP - 1 >= max(LENS))"""
    idx = torch.randint(-1, C.CAP, (C.B, Sq, topk), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    if topk >= 4:
        idx[..., 1], idx[..., 2], idx[..., 3] = -1, idx[..., 0], C.CAP - 1
    return idx


def make_cache(page, lens, dtype=torch.bfloat16, fmt="e4m3", device="cpu", table_seed=7, prefill=0x7f, lat=None):
    """a row-major cache whose slot b holds the first lens[b] rows of the latent behind a shuffled table; never-written bytes = prefill (NaN)"""
    table, num_pages = C.make_table(page, table_seed)
    cache = qa.alloc_paged_mla_row_cache_fp8(num_pages, page, batch_size=C.B, max_pages_per_seq=table.shape[1], scale=C.SCALE_KV, dtype=dtype,
                                             device=device, fp8_format=fmt)
    cache.pool.view(torch.uint8).fill_(prefill)
    cache.block_table.copy_(table)
    lat = C.make_latent(dtype).to(device) if lat is None else lat
    qa.paged_mla_row_cache_append_fp8(cache, lat[..., :C.DV], lat[..., C.DV:], new_lens=torch.tensor(lens, dtype=torch.int32, device=device))
    return cache


def dequant(cache):
    """fp64 [B, CAP, 576]: the cache's bytes gathered through the table (NaN where nothing was written)"""
    rows = cache.pool.view(_native.fp8_dtype_of(cache.fp8_format))[cache.block_table.long()]
    return (rows.reshape(C.B, -1, C.D).double() * cache.scale.double()[:, None, None]).cpu().numpy()


def reference(qd, lat, idx, lens, scale, causal):
    """fp64: qd [B, Hq, Sq, 576], lat [B, CAP, 576] de-quantised, idx [B, Sq, topk] -> (out [B, Hq, Sq, 512], lse [B, Hq, Sq])"""
    qd, idx = np.asarray(qd, np.float64), np.asarray(idx)
    Bn, Hq, Sq, _ = qd.shape
    out, lse = np.zeros((Bn, Hq, Sq, C.DV)), np.full((Bn, Hq, Sq), -np.inf)
    for b, L in enumerate(lens):
        for i in range(Sq):
            kend = L - Sq + i + 1 if causal else L
            j = idx[b, i][(idx[b, i] >= 0) & (idx[b, i] < kend)]
            if j.size == 0:
                continue
            s = qd[b, :, i] @ lat[b, j].T * scale
            m = s.max(axis=-1, keepdims=True)
            p = np.exp(s - m)
            den = p.sum(axis=-1, keepdims=True)
            out[b, :, i] = (p / den) @ lat[b, j, :C.DV]
            lse[b, :, i] = (m + np.log(den))[:, 0]
    return out, lse


def check_sweep(Hq, Sq, topk, causal, fmt, dtype, device, assert_within_bound):
    """the oracle sweep of one case over LENS x PAGES x SPLITS; the oracle is computed once per LENS (it does not depend on the paging)"""
    q = C.make_q(Hq, Sq, dtype).to(device)
    idx = draw_indices(Sq, topk, seed=1000 * topk + Sq).to(device)
    for lens in C.LENS:
        ref = None
        for page in PAGES:
            cache = make_cache(page, lens, dtype, fmt, device)
            assert cache.seqlens.tolist() == list(lens)
            for ns in C.SPLITS:
                out, lse, q8, sq = qa.fp8_mla_paged_sparse_func(q, cache, idx, scale=C.SM_SCALE, causal=causal, num_splits=ns, return_lse=True,
                                                                return_q8=True)
                if ref is None:
                    assert torch.equal(q8.float() * sq[..., None], q.float())      # exact inputs: the kernel's q8 is q itself
                    ref = reference((q8.double() * sq.double()[..., None]).cpu().numpy(), dequant(cache), idx.cpu().numpy(), lens, C.SM_SCALE, causal)
                what = (Hq, Sq, topk, causal, fmt, lens, page, ns)
                got_o, got_l, fin = out.float().cpu().numpy(), lse.cpu().numpy(), np.isfinite(ref[1])
                print(what, "max |err| out", np.abs(got_o - ref[0]).max(), "lse", np.abs(got_l[fin] - ref[1][fin]).max() if fin.any() else 0.0)
                assert_within_bound(got_o, ref[0], what=what)
                assert np.array_equal(np.isneginf(got_l), ~fin), what                # a row without a valid entry: LSE -inf exactly ...
                assert (got_o[~fin] == 0).all(), what                                # ... and a zero row
                assert not fin.any() or np.abs(got_l[fin] - ref[1][fin]).max() <= C.LSE_TOL, what

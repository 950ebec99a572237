"""GPU tests of sparse MLA on packed variable-length queries (include/qattn_mla_sparse_prefill.h): the packed call against the fp64 oracle of
tests/mla_sparse_cases.py (softmax over the listed valid keys of the de-quantised cache bytes and the q8 the kernel returns), bit identity with
`fp8_mla_paged_sparse_func(num_splits=1)` on every slot's tokens, the closed-form gather probe, and a replayed graph behind the indexer.

Bounds: the MLA tests' own -- out per element 2^-6 max(1, |ref| / 2) (tests/gpu_utils.py), lse 2e-3."""
import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd.mla import PagedMLACacheFP8
from tests import mla_cases as C
from tests import mla_index_cases as X
from tests import mla_sparse_cases as S
from tests.gpu_utils import assert_within_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
COUNTS = (0, 1, 5, 3)            # tokens per slot: an idle slot, one token, two counts that are no power of two
TOTAL = sum(COUNTS) + 4          # a bucket with four padded rows behind cu[B]
LENS = (64, 1, 3, 200)           # slot 2: L_b < n_b, its first causal rows have no key
# Hq: one live row block / a partial third block / the full tile / two tiles, the second partial.  topk: a ragged group / three groups /
# above the 2048 entries the 64-row kernel resolves per split.  A thinned product.
ORACLE_CASES = [(16, 70, "e4m3", torch.bfloat16, 1, True), (16, 2112, "e5m2", torch.float16, 64, False),
                (16, 130, "e4m3", torch.bfloat16, 64, True), (72, 130, "e4m3", torch.bfloat16, 64, True),
                (72, 70, "e5m2", torch.float16, 1, False), (72, 2112, "e4m3", torch.bfloat16, 1, True),
                (128, 2112, "e4m3", torch.bfloat16, 1, True), (128, 130, "e5m2", torch.float16, 64, True),
                (128, 70, "e4m3", torch.bfloat16, 64, False), (160, 130, "e4m3", torch.bfloat16, 1, False),
                (160, 2112, "e5m2", torch.float16, 64, True), (160, 70, "e4m3", torch.bfloat16, 64, True)]


def packed(Hq, topk, dtype, counts=COUNTS, seed=0):
    """(q [TOTAL, Hq, 576], indices [TOTAL, topk] with -1, duplicates and positions behind every limit, cu_seqlens_q) on the device"""
    q = C.make_q(Hq, 4, dtype, seed=seed).permute(0, 2, 1, 3).reshape(16, Hq, C.D)[:TOTAL]
    idx = S.draw_indices(4, topk, seed=1000 * topk + seed).reshape(16, topk)[:TOTAL]
    cu = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    return q.contiguous().to(DEV), idx.contiguous().to(DEV), cu.to(DEV)


def one_slot(cache, b):
    return PagedMLACacheFP8(cache.pool, cache.scale[b:b + 1], cache.block_table[b:b + 1], cache.seqlens[b:b + 1], cache.num_pages,
                            cache.page_size, cache.fp8_format, cache.dtype, cache.layout)


def assert_padding(out, lse, lo):
    assert (out[lo:].float() == 0).all() and torch.isneginf(lse[:, lo:]).all()


@pytest.mark.parametrize("Hq,topk,fmt,dtype,page,causal", ORACLE_CASES)
def test_against_the_fp64_oracle(Hq, topk, fmt, dtype, page, causal):
    q, idx, cu = packed(Hq, topk, dtype)
    cache = S.make_cache(page, LENS, dtype, fmt, DEV)      # NaN bytes wherever nothing was appended
    out, lse, q8, sq = qa.fp8_mla_paged_sparse_varlen_func(q, cache, idx, cu, scale=C.SM_SCALE, causal=causal, return_lse=True, return_q8=True)
    assert tuple(out.shape) == (TOTAL, Hq, C.DV) and tuple(lse.shape) == (Hq, TOTAL)
    lat, lo = S.dequant(cache), 0
    for b, n in enumerate(COUNTS):
        rows = slice(lo, lo + n)
        lo += n
        if n == 0:
            continue
        assert torch.equal(q8[rows].float() * sq[rows][..., None], q[rows].float())      # exact inputs: the kernel's q8 is q itself
        qd = (q8[rows].double() * sq[rows].double()[..., None]).transpose(0, 1)[None].cpu().numpy()
        ref_o, ref_l = S.reference(qd, lat[b:b + 1], idx[rows][None].cpu().numpy(), (LENS[b],), C.SM_SCALE, causal)
        got_o, got_l = out[rows].float().transpose(0, 1)[None].cpu().numpy(), lse[:, rows][None].cpu().numpy()
        what, fin = (Hq, topk, fmt, page, causal, b), np.isfinite(ref_l)
        print(what, "max |err| out", np.abs(got_o - ref_o).max(), "lse", np.abs(got_l[fin] - ref_l[fin]).max() if fin.any() else 0.0)
        assert_within_bound(got_o, ref_o, what=what)
        assert np.array_equal(np.isneginf(got_l), ~fin) and (got_o[~fin] == 0).all(), what
        assert not fin.any() or np.abs(got_l[fin] - ref_l[fin]).max() <= C.LSE_TOL, what
    assert_padding(out, lse, lo)


@pytest.mark.parametrize("Hq", [16, 128, 160])
def test_bit_identity_with_the_decode_entry(Hq):
    q, idx, cu = packed(Hq, 130, torch.bfloat16)
    cache = S.make_cache(16, LENS, device=DEV)
    for causal in (True, False):
        out, lse, q8, sq = qa.fp8_mla_paged_sparse_varlen_func(q, cache, idx, cu, scale=C.SM_SCALE, causal=causal, return_lse=True, return_q8=True)
        lo = 0
        for b, n in enumerate(COUNTS):
            rows = slice(lo, lo + n)
            lo += n
            if n == 0:
                continue
            w_o, w_l, w_q8, w_sq = qa.fp8_mla_paged_sparse_func(q[rows].transpose(0, 1)[None], one_slot(cache, b), idx[rows][None], scale=C.SM_SCALE,
                                                                causal=causal, num_splits=1, return_lse=True, return_q8=True)
            assert torch.equal(out[rows].view(torch.int16), w_o[0].transpose(0, 1).view(torch.int16)), (Hq, causal, b)
            assert torch.equal(lse[:, rows].view(torch.int32), w_l[0].view(torch.int32)), (Hq, causal, b)
            assert torch.equal(q8[rows].view(torch.uint8), w_q8[0].transpose(0, 1).view(torch.uint8)) and torch.equal(sq[rows], w_sq[0].transpose(0, 1))
        assert_padding(out, lse, lo)


@pytest.mark.parametrize("n", [40, 130])
def test_gather_probe(n):
    """tests/test_gpu_mla_sparse.py's probe through the packed entry at Hq 128: key j carries j % 7 + 1 in channel 37 j mod 512, q = 0, so
    out[c] = the values of the LISTED keys with 37 j mod 512 = c over their count.  A wrongly gathered, dropped or doubled key moves an
    element by >= 1 / n."""
    lat = torch.zeros((C.B, C.CAP, C.D))
    j = torch.arange(C.CAP)
    lat[:, j, (37 * j) % 512] = (j % 7 + 1).float()
    cache = S.make_cache(16, (C.CAP,) * C.B, device=DEV, lat=(lat * C.SCALE_KV).bfloat16().to(DEV))
    g = torch.Generator().manual_seed(n)
    idx = torch.full((C.B, n + 7), -1, dtype=torch.int32)                             # padded with -1; topk is no multiple of 64
    ref = np.zeros((C.B, 1, C.DV))
    for b in range(C.B):
        keys = torch.randperm(C.CAP, generator=g)[:n]                                 # a subset, in shuffled order
        idx[b, :n] = keys.to(torch.int32)
        for k in keys.tolist():
            ref[b, 0, (37 * k) % 512] += (k % 7 + 1) * C.SCALE_KV / n
    q = torch.zeros((C.B, 128, C.D), dtype=torch.bfloat16, device=DEV)
    cu = torch.arange(C.B + 1, dtype=torch.int32, device=DEV)
    out = qa.fp8_mla_paged_sparse_varlen_func(q, cache, idx.to(DEV), cu, scale=C.SM_SCALE).float().cpu().numpy()
    assert_within_bound(out, np.broadcast_to(ref, out.shape), what=n)
    assert np.abs(out - ref).max() < 0.25 / 130, n            # (bf16 rounding of values <= 7/64 is far below one misplaced key)


def test_captured_indexer_and_attend_follow_cu_lengths_table_and_tokens():
    page, Hq, Hi, topk = 16, 72, 4, 70
    cache = S.make_cache(page, LENS, device=DEV)
    cache.pool.view(torch.uint8).copy_(torch.randint(0, 0x78, cache.pool.shape, dtype=torch.uint8))   # every page holds finite e4m3 bytes
    icache = X.make_icache(page, (C.CAP,) * C.B, device=DEV, cap=C.CAP)
    q, _, cu = packed(Hq, topk, torch.bfloat16)
    q_idx = X.make_q(Hi, TOTAL, torch.bfloat16)[0].transpose(0, 1).contiguous().to(DEV)
    w = C.draw((TOTAL, Hi), 50).to(DEV)
    def step():
        idx = qa.fp8_mla_index_topk_varlen_func(q_idx, w, icache, cu, topk, max_seqlen_k=C.CAP)
        return qa.fp8_mla_paged_sparse_varlen_func(q, cache, idx, cu, scale=C.SM_SCALE, return_lse=True)
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_lse = step()
    for seed, counts, lens in ((11, (3, 0, 2, 4), (199, 7, 1, 64)), (12, (1, 6, 0, 1), (5, 128, 9, 200))):
        q.copy_(packed(Hq, topk, torch.bfloat16, seed=seed)[0])
        cu.copy_(packed(Hq, topk, torch.bfloat16, counts=counts)[2])
        for c in (cache, icache):
            c.seqlens.copy_(torch.tensor(lens, dtype=torch.int32))
        cache.block_table.copy_(C.make_table(page, seed)[0])
        graph.replay()
        got = (g_out.clone(), g_lse.clone())
        e_out, e_lse = step()
        assert torch.equal(got[0].view(torch.int16), e_out.view(torch.int16)) and torch.equal(got[1].view(torch.int32), e_lse.view(torch.int32))
        assert_padding(e_out, e_lse, sum(counts))

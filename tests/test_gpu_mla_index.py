"""GPU tests of the lightning indexer (include/qattn_mla_index.h): the score sweep bit for bit against fp64 on exact inputs and within the fp32
rounding bound on random data, the selection against a stable sort on crafted rows, the whole entry, the append against the CPU quantiser,
and the composition with sparse attention: bit identity with the dense kernel and a replayed graph of the whole decode step.

Bound of the random-data scores, per element: 256 x 2^-24 x scale_k sum_h |w_h| scale_q sum_c |q8 k8| -- at most 128 + 65 fp32 roundings,
(1 + 2^-24)^200 - 1 < 2^-16."""
import pytest
import torch

import quantumattention_amd as qa
from tests import mla_cases as C
from tests import mla_index_cases as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("Hi,Sq,causal,page,fmt,dtype", X.SCORE_CASES)
def test_scores_and_entry_are_exact_on_exact_inputs(Hi, Sq, causal, page, fmt, dtype):
    X.check_scores(Hi, Sq, causal, page, fmt, dtype, DEV)


@pytest.mark.parametrize("Hi,Sq,page", [(64, 3, 16), (20, 1, 64), (33, 2, 1)])
def test_scores_on_random_data_within_the_rounding_bound(Hi, Sq, page):
    worst = X.check_scores(Hi, Sq, True, page, "e4m3", torch.bfloat16, DEV, exact=False, topk=65)
    print("worst |err| / bound", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("kind,N", X.SELECT_CASES)
def test_selection_against_a_stable_sort(kind, N):
    X.check_select(kind, N, DEV)


@pytest.mark.parametrize("page", [1, 64])
@pytest.mark.parametrize("T,start", [(1, 0), (5, 60), (70, 64)])
def test_append_bytes_against_the_cpu_quantiser(T, start, page):
    X.check_append(T, start, page, DEV)


def _caches(page, lens):
    """a row-major latent cache and an index cache on ONE table and ONE length vector, both filled to lens"""
    table, num_pages = C.make_table(page)
    kw = dict(batch_size=C.B, max_pages_per_seq=table.shape[1], dtype=torch.bfloat16, device=DEV)
    row = qa.alloc_paged_mla_row_cache_fp8(num_pages, page, scale=C.SCALE_KV, **kw)
    icache = qa.alloc_paged_mla_index_cache_fp8(num_pages, page, scale=X.SCALE_K, block_table=row.block_table, seqlens=row.seqlens, **kw)
    row.block_table.copy_(table)
    n = torch.tensor(lens, dtype=torch.int32, device=DEV)
    lat, keys = C.make_latent(torch.bfloat16).to(DEV), (C.draw((C.B, C.CAP, X.D), 3) * X.SCALE_K).bfloat16().to(DEV)
    qa.paged_mla_index_cache_append_fp8(icache, keys, new_lens=n, advance=False)
    qa.paged_mla_row_cache_append_fp8(row, lat[..., :C.DV], lat[..., C.DV:], new_lens=n)
    return row, icache, lat


def test_indexed_sparse_attention_equals_the_dense_kernel_bit_for_bit():
    """topk = the capacity >= kend: the indexer's list is 0 .. L_b - 1 then -1, whose 64-entry groups are the dense kernel's chunks"""
    lens, q = C.LENS[1], C.make_q(16, 1, torch.bfloat16).to(DEV)
    row, icache, lat = _caches(64, lens)
    dense = qa.alloc_paged_mla_cache_fp8(row.num_pages, 64, batch_size=C.B, max_pages_per_seq=row.block_table.shape[1], scale=C.SCALE_KV,
                                         dtype=torch.bfloat16, device=DEV)
    dense.block_table.copy_(row.block_table)
    qa.paged_mla_cache_append_fp8(dense, lat[..., :C.DV], lat[..., C.DV:], new_lens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    want_o, want_l = qa.fp8_mla_paged_func(q, dense, scale=C.SM_SCALE, num_splits=1, max_seqlen_k=C.CAP, return_lse=True)
    idx = qa.fp8_mla_index_topk_func(X.make_q(20, 1, torch.bfloat16).to(DEV), C.draw((C.B, 1, 20), 9).to(DEV), icache, C.CAP)
    assert all(idx[b, 0].tolist() == list(range(L)) + [-1] * (C.CAP - L) for b, L in enumerate(lens))
    out, lse = qa.fp8_mla_paged_sparse_func(q, row, idx, scale=C.SM_SCALE, num_splits=1, return_lse=True)
    assert torch.equal(out.view(torch.int16), want_o.view(torch.int16)) and torch.equal(lse.view(torch.int32), want_l.view(torch.int32))


def test_captured_decode_step_follows_table_lengths_q_and_weights():
    page, lens0, topk, Sq = 16, (10, 64, 127, 199), 40, 3
    row, icache, lat = _caches(page, lens0)
    for cache in (row, icache):
        cache.pool.view(torch.uint8).copy_(torch.randint(0, 0x78, cache.pool.shape, dtype=torch.uint8))   # every page holds finite e4m3 bytes
    pools0 = (row.pool.clone(), icache.pool.clone())
    q = C.make_q(20, Sq, torch.bfloat16).to(DEV)
    qi, w = X.make_q(20, Sq, torch.bfloat16).to(DEV), C.draw((C.B, Sq, 20), 9).to(DEV)
    new, knew = lat[:, :1], (C.draw((C.B, 1, X.D), 4) * X.SCALE_K).bfloat16().to(DEV)
    def step():
        qa.paged_mla_index_cache_append_fp8(icache, knew, advance=False)
        qa.paged_mla_row_cache_append_fp8(row, new[..., :C.DV], new[..., C.DV:])
        idx = qa.fp8_mla_index_topk_func(qi, w, icache, topk)
        return (idx,) + qa.fp8_mla_paged_sparse_func(q, row, idx, scale=C.SM_SCALE, num_splits=2, return_lse=True)
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_res = step()
    for seed, lens in ((11, (199, 0, 63, 64)), (12, (65, 128, 1, 200)), (13, lens0)):
        def state():
            row.pool.view(torch.uint8).copy_(pools0[0].view(torch.uint8))
            icache.pool.view(torch.uint8).copy_(pools0[1].view(torch.uint8))
            row.block_table.copy_(C.make_table(page, seed)[0])
            row.seqlens.copy_(torch.tensor(lens, dtype=torch.int32))
            qi.copy_(X.make_q(20, Sq, torch.bfloat16, seed=seed))
            w.copy_(C.draw((C.B, Sq, 20), seed))
        state()
        graph.replay()
        got = [t.clone() for t in g_res + (row.seqlens, row.pool, icache.pool)]
        state()
        want = step() + (row.seqlens, row.pool, icache.pool)
        assert row.seqlens.tolist() == [x + 1 for x in lens]
        assert (want[0] >= 0).sum() > 0 and all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, want))

"""GPU tests of the packed (prefill) lightning indexer (include/qattn_mla_index_prefill.h): logits, indices, q8 and scale_q of every slot
against the dense entry on the slot's tokens BIT FOR BIT -- the arithmetic is specified to be the same -- and against fp64 (bit for bit on
exact inputs, within tests/test_gpu_mla_index.py's bound 256 x 2^-24 x scale_k sum_h |w_h| scale_q sum_c |q8 k8| on random data); a replayed
graph against the eager call.  Shapes: tests/mla_index_prefill_cases.py."""
import pytest
import torch

import quantumattention_amd as qa
from tests import mla_index_cases as X
from tests import mla_index_prefill_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("shape,Hi,page,causal,fmt,dtype", P.CASES)
def test_packed_call_equals_the_dense_entry_and_fp64_on_exact_inputs(shape, Hi, page, causal, fmt, dtype):
    assert P.check(shape, Hi, page, causal, fmt, dtype, DEV) == 0.0


@pytest.mark.parametrize("shape,Hi,page", [("a", 64, 16), ("b", 33, 1)])
def test_packed_call_on_random_data_within_the_rounding_bound(shape, Hi, page):
    worst = P.check(shape, Hi, page, True, "e4m3", torch.bfloat16, DEV, exact=False)
    print("worst |err| / bound", worst)
    assert 0.0 < worst <= 1.0


def test_captured_call_follows_cu_seqlens_lengths_table_q_and_weights():
    Hi, page, topk = 20, 16, 24
    icache = X.make_icache(page, P.SHAPES["a"][1], device=DEV, cap=P.CAP)
    icache.pool.view(torch.uint8).copy_(torch.randint(0, 0x78, icache.pool.shape, dtype=torch.uint8))   # every page holds finite e4m3 bytes
    q, w, cu = (t.clone() for t in P.make_packed("a", Hi, torch.bfloat16, DEV))
    call = lambda: qa.fp8_mla_index_topk_varlen_func(q, w, icache, cu, topk, max_seqlen_k=P.CAP, return_logits=True, return_q8=True)
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_res = call()
    for seed, shape in ((11, "b"), (12, "a"), (13, "b")):
        qn, wn, cun = P.make_packed(shape, Hi, torch.bfloat16, DEV, seed=seed)   # (both shapes hold the same number of rows)
        q.copy_(qn), w.copy_(wn), cu.copy_(cun)
        icache.seqlens.copy_(torch.tensor(P.SHAPES[shape][1], dtype=torch.int32))
        icache.block_table.copy_(torch.randperm(icache.num_pages, generator=torch.Generator().manual_seed(seed))[: icache.block_table.numel()]
                                 .reshape(icache.block_table.shape).to(torch.int32))
        graph.replay()
        got = [t.clone() for t in g_res]
        want = call()
        assert (want[0] >= 0).sum() > 0 and all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, want))

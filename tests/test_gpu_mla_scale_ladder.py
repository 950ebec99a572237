"""The scale ladder through the MLA kernels (the inputs, the references and the checks are tests/mla_scale_ladder.py's,
the teeth of every named mis-indexing are shown on the same case tables by tests/test_cpu_mla_scale_ladder.py).  Per entry:

1. oracle grading: the ladder (slot + q; index: plain weights; prefill: with GH) against fp64 on the inputs themselves, with the project's
   bounds (out 2^-6 max(1, |ref| / 2), lse 2e-3; the indexer: bit for bit) on out / 2^e, and the -inf / zero-row rules of the sweeps;
2. the quantiser echo: the pool bytes and q8 are the plain call's, every returned scale is exactly 2^e times the plain call's;
3. exact equivariance without an oracle: the slot ladder alone gives the plain call's lse bit for bit and 2^E_SLOT[b] times its out (the
   indexer: logits and equal indices; prefill without GH: lse and 2^EV out) -- on the elements whose 2^e-fold stays a normal fp16 number;
4. the chain on the ladder: packed sparse = sparse decode per slot, sparse with the indices 0 .. = dense, packed indexer = dense indexer.
Every test prints its worst |err| / bound."""
import pytest
import torch

import quantumattention_amd as qa
from tests import mla_cases as C
from tests import mla_scale_ladder as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
DECODE_IDS = [L.decode_id(c) for c in L.DECODE_CASES]


@pytest.mark.parametrize("case", L.DECODE_CASES, ids=DECODE_IDS)
def test_dense_decode(case):
    Hq, Sq, fmt, dtype = case
    print("dense", L.decode_id(case), "worst |err| / bound", L.check_decode("dense", Hq, Sq, fmt, dtype, DEV, L.DENSE_PAGES, L.DENSE_SPLITS))


@pytest.mark.parametrize("topk", L.SPARSE_TOPKS)
@pytest.mark.parametrize("case", L.DECODE_CASES, ids=DECODE_IDS)
def test_sparse_decode(case, topk):
    Hq, Sq, fmt, dtype = case
    print("sparse", L.decode_id(case), topk, "worst |err| / bound", L.check_decode("row", Hq, Sq, fmt, dtype, DEV, L.SPARSE_PAGES, L.SPARSE_SPLITS, topk=topk))


@pytest.mark.parametrize("fmt,dtype,page", [("e4m3", torch.bfloat16, 16), ("e5m2", torch.float16, 1)])
@pytest.mark.parametrize("Hq", L.VARLEN_HEADS)
def test_packed_sparse_and_its_chain_to_the_decode_entry(Hq, fmt, dtype, page):
    print("packed sparse", Hq, fmt, "worst |err| / bound", L.check_varlen(Hq, fmt, dtype, page, DEV))


@pytest.mark.parametrize("Hq", [16, 128])
def test_sparse_with_the_first_indices_equals_dense_on_the_ladder(Hq):
    """tests/test_gpu_mla_sparse.py's identity (indices 0 .. ceil(L_b / 64) 64 - 1, one split) with per-slot scales and the q ladder"""
    lens, inp = C.LENS[1], L.decode_inputs(Hq, 1, torch.bfloat16)
    q = inp.q.to(DEV)
    want_o, want_l = qa.fp8_mla_paged_func(q, L.make_cache("dense", 64, lens, inp, "e4m3", DEV), scale=C.SM_SCALE, num_splits=1, max_seqlen_k=C.CAP, return_lse=True)
    idx = torch.full((C.B, 1, C.CAP), -1, dtype=torch.int32)
    for b, n in enumerate(lens):
        idx[b, 0, : -(-n // 64) * 64] = torch.arange(-(-n // 64) * 64, dtype=torch.int32)
    out, lse = qa.fp8_mla_paged_sparse_func(q, L.make_cache("row", 16, lens, inp, "e4m3", DEV, table_seed=8), idx.to(DEV), scale=C.SM_SCALE, num_splits=1, return_lse=True)
    assert torch.equal(out.view(torch.int16), want_o.view(torch.int16)) and torch.equal(lse.view(torch.int32), want_l.view(torch.int32))


@pytest.mark.parametrize("case", L.INDEX_CASES, ids=[f"Hi{c[0]}_Sq{c[1]}_{c[3]}" for c in L.INDEX_CASES])
def test_indexer(case):
    print("index", case[:4], "worst |err| / rounding bound (0: bit for bit)", L.check_index(*case, DEV))


@pytest.mark.parametrize("case", L.INDEX_VARLEN_CASES, ids=[f"{c[0]}_Hi{c[1]}_{c[3]}" for c in L.INDEX_VARLEN_CASES])
def test_packed_indexer_and_its_chain_to_the_dense_indexer(case):
    print("packed index", case[:4], "worst |err| / rounding bound (0: bit for bit)", L.check_index_varlen(*case, DEV))


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("fmt,dtype", L.PREFILL_CASES)
def test_prefill(fmt, dtype, causal):
    print("prefill", fmt, causal, "worst |err| / bound", L.check_prefill(fmt, dtype, causal, DEV))

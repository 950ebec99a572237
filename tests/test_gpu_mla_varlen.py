"""GPU tests of dense MLA on packed variable-length queries (include/qattn_mla_varlen.h): every slot of the packed call against
`fp8_mla_paged_func` on that slot alone, bit for bit; the packed call against the fp64 oracle on the de-quantised cache bytes and the q8 the
kernel returns (tests/test_gpu_mla.py's bounds: 2^-6 max(1, |ref| / 2) per element of out, 2e-3 on the LSE); dead bytes, another table, and a
replayed graph of append + attend under rewritten cu_seqlens_q, lengths and table."""
import pytest
import torch

import quantumattention_amd as qa
from tests import mla_cases as C
from tests import mla_varlen_cases as V

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _packed(q, cache, counts, causal, ns, **kw):
    return qa.fp8_mla_paged_varlen_func(q, cache, V.cu_of(counts, DEV), max(counts), scale=C.SM_SCALE, causal=causal, num_splits=ns,
                                        max_seqlen_k=C.CAP, return_lse=True, **kw)


@pytest.mark.parametrize("case", V.CASES)
@pytest.mark.parametrize("page", C.PAGES)
@pytest.mark.parametrize("ns", [1, 2, 3])
@pytest.mark.parametrize("causal", [True, False])
def test_every_slot_equals_the_dense_call_bit_for_bit(case, page, ns, causal):
    Hq, counts, lens = case
    q, total = V.make_q(Hq, counts).to(DEV), sum(counts)
    cache, _ = V.make_cache(DEV, len(counts), page, lens)
    out, lse, po, pl, q8, sq = _packed(q, cache, counts, causal, ns, return_partials=True, return_q8=True)
    lo = 0
    for b, n in enumerate(counts):
        rows, what = slice(lo, lo + n), (case, page, ns, causal, b)
        lo += n
        if n == 0:
            continue
        d_out, d_lse, d_po, d_pl, d_q8, d_sq = qa.fp8_mla_paged_func(
            q[rows].transpose(0, 1)[None], V.slot_view(cache, b), scale=C.SM_SCALE, causal=causal, num_splits=ns, max_seqlen_k=C.CAP,
            return_lse=True, return_partials=True, return_q8=True)
        assert torch.equal(out[rows], d_out[0].transpose(0, 1)) and torch.equal(lse[:, rows], d_lse[0]), what
        assert torch.equal(q8[rows].view(torch.uint8), d_q8[0].transpose(0, 1).view(torch.uint8)) and torch.equal(sq[rows], d_sq[0].transpose(0, 1)), what
        if ns > 1:
            assert torch.equal(po[:, rows], d_po[:, 0].transpose(1, 2)) and torch.equal(pl[:, rows], d_pl[:, 0].transpose(1, 2)), what
        if causal and lens[b] < n:                                                   # the slot's first token has no key
            assert torch.isneginf(lse[:, lo - n]).all() and (out[lo - n] == 0).all(), what
    assert (out[total:] == 0).all() and torch.isneginf(lse[:, total:]).all() and (sq[total:] == 0).all() and (q8[total:].float() == 0).all()


@pytest.mark.parametrize("case", V.CASES)
@pytest.mark.parametrize("page", C.PAGES)
@pytest.mark.parametrize("ns", [1, 0])
@pytest.mark.parametrize("causal", [True, False])
def test_against_the_fp64_reference(case, page, ns, causal):
    Hq, counts, lens = case
    q, total = V.make_q(Hq, counts).to(DEV), sum(counts)
    cache, _ = V.make_cache(DEV, len(counts), page, lens)
    out, lse, q8, sq = _packed(q, cache, counts, causal, ns, return_q8=True)
    assert torch.equal((q8.float() * sq[..., None])[:total], q.float()[:total])          # exact inputs: the kernel's q8 is q itself
    ref = V.reference((q8.double() * sq.double()[..., None]).cpu().numpy(), V.dequant(cache), counts, lens, causal)
    V.check_against_reference(out, lse, ref, (case, page, ns, causal))


@pytest.mark.parametrize("case", [V.CASES[0], V.CASES[4]])
def test_dead_bytes_and_another_table_change_no_bit(case):
    Hq, counts, lens = case
    q = V.make_q(Hq, counts).to(DEV)
    call = lambda **kw: _packed(q, V.make_cache(DEV, len(counts), 128, lens, **kw)[0], counts, True, 3)
    out, lse = call()
    for other in (call(prefill=0x7f), call(table_seed=8)):      # NaN bytes behind every L_b and in never-written pages; the pages moved
        assert torch.equal(other[0].view(torch.int16), out.view(torch.int16)) and torch.equal(other[1].view(torch.int32), lse.view(torch.int32))


def test_captured_append_and_attend_follows_cu_seqlens_table_and_lengths():
    Hq, page, B, bucket = 16, 64, 4, 18
    cache, _ = V.make_cache(DEV, B, page, (10, 64, 127, 199))
    cache.pool.copy_(torch.randint(0, 0x78, cache.pool.shape, dtype=torch.uint8))          # every page holds finite e4m3 bytes
    pool0 = cache.pool.clone()
    q = V.make_q(Hq, (bucket - V.PAD,)).to(DEV).nan_to_num_(1.0)                           # the rows of the bucket are live in some replays
    new = (C.draw((B, 1, C.D), 5) * C.SCALE_KV).bfloat16().to(DEV)
    cu = V.cu_of((1, 0, 5, 9), DEV)
    def step():
        qa.paged_mla_cache_append_fp8(cache, new[..., :C.DV], new[..., C.DV:])
        return qa.fp8_mla_paged_varlen_func(q, cache, cu, bucket, scale=C.SM_SCALE, num_splits=2, max_seqlen_k=C.CAP, return_lse=True)
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_lse = step()
    for seed, lens, counts in ((11, (199, 0, 63, 64), (4, 4, 4, 6)), (12, (65, 128, 1, 200), (0, 17, 0, 1)), (13, (10, 64, 127, 199), (1, 0, 5, 9))):
        def state():
            cache.pool.copy_(pool0)
            g = torch.Generator().manual_seed(seed)
            cache.block_table.copy_(torch.randperm(cache.num_pages, generator=g)[: cache.block_table.numel()].reshape(B, -1).to(torch.int32))
            cache.seqlens.copy_(torch.tensor(lens, dtype=torch.int32))
            cu.copy_(V.cu_of(counts))
        state()
        graph.replay()
        got = (g_out.clone(), g_lse.clone(), cache.seqlens.clone())
        state()
        e_out, e_lse = step()
        assert cache.seqlens.tolist() == [x + 1 for x in lens] and torch.equal(got[2], cache.seqlens)
        assert torch.equal(got[0].view(torch.int16), e_out.view(torch.int16)) and torch.equal(got[1].view(torch.int32), e_lse.view(torch.int32))
        assert torch.isneginf(e_lse[:, sum(counts):]).all() and (e_out[sum(counts):] == 0).all()

"""GPU tests of sparse multi-head latent attention on the row-major paged FP8 latent cache (include/qattn_mla_sparse.h): the sweep against an
fp64 oracle over the listed valid keys of the de-quantised cache bytes and the q8 the kernel returns, a closed-form probe of the gather, bit
identity with the dense kernel (include/qattn_mla.h) on the same bytes, the row append against the CPU quantiser, and a replayed graph.

Bounds: the MLA tests' own -- out per element 2^-6 max(1, |ref| / 2) (tests/gpu_utils.py), lse 2e-3."""
import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import mla_cases as C
from tests import mla_sparse_cases as S
from tests.gpu_utils import assert_within_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("Hq,Sq,topk,causal,fmt,dtype", S.CASES)
def test_sweep_against_the_fp64_oracle(Hq, Sq, topk, causal, fmt, dtype):
    S.check_sweep(Hq, Sq, topk, causal, fmt, dtype, DEV, assert_within_bound)


@pytest.mark.parametrize("n", [40, 130])
def test_gather_probe(n):
    """key j carries j % 7 + 1 in channel 37 j mod 512 and zeros elsewhere, q = 0: uniform softmax, so out[c] = the values of the LISTED keys
    with 37 j mod 512 = c, over their count.  One wrongly gathered, dropped or misplaced key moves an element by >= 1 / 130."""
    lat = torch.zeros((C.B, C.CAP, C.D))
    j = torch.arange(C.CAP)
    lat[:, j, (37 * j) % 512] = (j % 7 + 1).float()
    cache = S.make_cache(16, (C.CAP,) * C.B, device=DEV, lat=(lat * C.SCALE_KV).bfloat16().to(DEV))
    g = torch.Generator().manual_seed(n)
    idx = torch.full((C.B, 1, n + 7), -1, dtype=torch.int32)                          # padded with -1; topk is no multiple of 64
    ref = np.zeros((C.B, 1, 1, C.DV))
    for b in range(C.B):
        keys = torch.randperm(C.CAP, generator=g)[:n]                                 # a subset, in shuffled order
        idx[b, 0, :n] = keys.to(torch.int32)
        for k in keys.tolist():
            ref[b, 0, 0, (37 * k) % 512] += (k % 7 + 1) * C.SCALE_KV / n
    q = torch.zeros((C.B, 16, 1, C.D), dtype=torch.bfloat16, device=DEV)
    for ns in (1, 2):
        out = qa.fp8_mla_paged_sparse_func(q, cache, idx.to(DEV), scale=C.SM_SCALE, num_splits=ns).float().cpu().numpy()
        assert_within_bound(out, np.broadcast_to(ref, out.shape), what=(n, ns))
        assert np.abs(out - ref).max() < 0.25 / 130, (n, ns)      # (bf16 rounding of values <= 7/64 is far below one misplaced key)


@pytest.mark.parametrize("Hq", [16, 128])
def test_bit_identity_with_the_dense_kernel(Hq):
    """indices = 0 .. ceil(L_b / 64) 64 - 1 over a row cache that holds a chunk-image cache's bytes: the gathered groups are the dense kernel's
    chunks, the entries >= L_b invalid by the rule, so out and lse equal fp8_mla_paged_func's bit for bit."""
    lens, q = C.LENS[1], C.make_q(Hq, 1, torch.bfloat16).to(DEV)
    lat = C.make_latent(torch.bfloat16).to(DEV)
    table, num_pages = C.make_table(64)
    dense = qa.alloc_paged_mla_cache_fp8(num_pages, 64, batch_size=C.B, max_pages_per_seq=table.shape[1], scale=C.SCALE_KV, dtype=torch.bfloat16,
                                         device=DEV)
    dense.block_table.copy_(table)
    qa.paged_mla_cache_append_fp8(dense, lat[..., :C.DV], lat[..., C.DV:], new_lens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    want_o, want_l = qa.fp8_mla_paged_func(q, dense, scale=C.SM_SCALE, num_splits=1, max_seqlen_k=C.CAP, return_lse=True)
    idx = torch.full((C.B, 1, C.CAP), -1, dtype=torch.int32)
    for b, L in enumerate(lens):
        idx[b, 0, : -(-L // 64) * 64] = torch.arange(-(-L // 64) * 64, dtype=torch.int32)
    # a zero-filled pool; NaN bytes at every invalid position with another shuffle of the table, the pages moved along
    for prefill, seed in ((0, 7), (0x7f, 8)):
        row = S.make_cache(16, lens, device=DEV, table_seed=seed, prefill=prefill)
        out, lse = qa.fp8_mla_paged_sparse_func(q, row, idx.to(DEV), scale=C.SM_SCALE, num_splits=1, return_lse=True)
        assert torch.equal(out.view(torch.int16), want_o.view(torch.int16)) and torch.equal(lse.view(torch.int32), want_l.view(torch.int32))


@pytest.mark.parametrize("page", [1, 64])
@pytest.mark.parametrize("T", [1, 5, 70])
@pytest.mark.parametrize("start", [0, 60, 64])
def test_row_append_bytes_against_the_cpu_quantiser(T, start, page):
    M, Bn, marker = 128 // page, 2, 0xA5                                              # capacity 128: start 64 + T 70 drops 6 tokens
    num_pages = Bn * M + 3
    for fmt, dtype in (("e4m3", torch.bfloat16), ("e5m2", torch.float16)):
        fp8, qmax = _native.fp8_dtype_of(fmt), torch.finfo(_native.fp8_dtype_of(fmt)).max
        cache = qa.alloc_paged_mla_row_cache_fp8(num_pages, page, batch_size=Bn, max_pages_per_seq=M, scale=torch.tensor([0.5, 0.03125]),
                                                 dtype=dtype, device=DEV, fp8_format=fmt)
        cache.pool.view(torch.uint8).fill_(marker)
        table = torch.randperm(num_pages, generator=torch.Generator().manual_seed(page))[: Bn * M].reshape(Bn, M).to(torch.int32)
        cache.block_table.copy_(table)
        cache.seqlens.fill_(start)
        g = torch.Generator().manual_seed(T * 100 + start)
        proj = (torch.randn((Bn, T, 640), generator=g) * 8.0).to(dtype)              # one projection tensor; |x| / 0.03125 passes qmax: saturation
        proj[0, 0, 3], proj[1, T - 1, 520] = float("inf"), float("-inf")
        n = (T, max(T - 3, 0))
        dproj = proj.to(DEV)
        qa.paged_mla_row_cache_append_fp8(cache, dproj[..., :512], dproj[..., 512:576], new_lens=torch.tensor(n, dtype=torch.int32, device=DEV))
        want = torch.full((num_pages, page, C.D), marker, dtype=torch.uint8)
        for b in range(Bn):
            kept = min(n[b], M * page - start)
            x8 = (proj[b, :kept, :576].float() / cache.scale[b].cpu()).to(dtype).clamp(-qmax, qmax).to(fp8).view(torch.uint8)
            for t in range(kept):
                want[table[b, (start + t) // page], (start + t) % page] = x8[t]
            assert int(cache.seqlens[b]) == start + kept
        assert torch.equal(cache.pool.view(torch.uint8).cpu(), want), (T, start, page, fmt)


def test_captured_append_and_attend_follows_indices_table_and_lengths():
    page, lens0, topk = 16, (10, 64, 127, 199), 130
    cache = S.make_cache(page, lens0, device=DEV)
    cache.pool.view(torch.uint8).copy_(torch.randint(0, 0x78, cache.pool.shape, dtype=torch.uint8))   # every page holds finite e4m3 bytes
    pool0 = cache.pool.clone()
    q = C.make_q(20, 3, torch.bfloat16).to(DEV)
    new = C.make_latent(torch.bfloat16, seed=5)[:, :1].to(DEV)
    idx = S.draw_indices(3, topk, 0).to(DEV)
    def step():
        qa.paged_mla_row_cache_append_fp8(cache, new[..., :C.DV], new[..., C.DV:])
        return qa.fp8_mla_paged_sparse_func(q, cache, idx, scale=C.SM_SCALE, num_splits=2, return_lse=True)
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_lse = step()
    for seed, lens in ((11, (199, 0, 63, 64)), (12, (65, 128, 1, 200)), (13, lens0)):
        def state():
            cache.pool.view(torch.uint8).copy_(pool0.view(torch.uint8))
            cache.block_table.copy_(C.make_table(page, seed)[0])
            cache.seqlens.copy_(torch.tensor(lens, dtype=torch.int32))
            idx.copy_(S.draw_indices(3, topk, seed))
        state()
        graph.replay()
        got = (g_out.clone(), g_lse.clone(), cache.seqlens.clone(), cache.pool.clone())
        state()
        e_out, e_lse = step()
        assert cache.seqlens.tolist() == [x + 1 for x in lens] and torch.equal(got[2], cache.seqlens)
        assert torch.equal(got[3].view(torch.uint8), cache.pool.view(torch.uint8))
        assert torch.equal(got[0].view(torch.int16), e_out.view(torch.int16)) and torch.equal(got[1].view(torch.int32), e_lse.view(torch.int32))

"""GPU tests of multi-head latent attention over the one-image paged FP8 latent cache (include/qattn_mla.h): the sweep against an fp64 oracle
on the de-quantised cache bytes and the q8 the kernel returns, a closed-form probe of the transposed value operand, the bit identities of the
contract, the append against the CPU quantiser laid out by the header's byte map, and a replayed graph.

Bounds: out per element 2^-6 max(1, |ref| / 2) (tests/gpu_utils.py: the bound of every FP8-P.V entry with two-term P; the reference shares the
quantised inputs, so it does not depend on the head dimension), lse 2e-3 (the FP8-P.V siblings' LSE_TOL)."""
import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, mla
from tests import mla_cases as C
from tests.gpu_utils import assert_within_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cache(page, lens, dtype=torch.bfloat16, fmt="e4m3", table_seed=7, prefill=0, lat=None):
    """a device cache whose slot b holds the first lens[b] rows of the latent, behind a shuffled table; never-written bytes = prefill"""
    table, num_pages = C.make_table(page, table_seed)
    cache = qa.alloc_paged_mla_cache_fp8(num_pages, page, batch_size=C.B, max_pages_per_seq=table.shape[1], scale=C.SCALE_KV, dtype=dtype,
                                         device=DEV, fp8_format=fmt)
    cache.pool.fill_(prefill)
    cache.block_table.copy_(table)
    lat = C.make_latent(dtype).to(DEV) if lat is None else lat
    qa.paged_mla_cache_append_fp8(cache, lat[..., :C.DV], lat[..., C.DV:], new_lens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    return cache


def _dequant(cache):
    """fp64 [B, CAP, 576]: the cache's bytes gathered through the table"""
    rows = mla.pool_rowmajor(cache.pool, cache.num_pages, cache.page_size).view(_native.fp8_dtype_of(cache.fp8_format))
    return (rows[cache.block_table.long()].reshape(C.B, -1, C.D).double() * cache.scale.double()[:, None, None]).cpu().numpy()


CASES = [(Hq, Sq, page, causal, "e4m3", torch.bfloat16) for Hq, Sq in C.SHAPES for page in C.PAGES for causal in (True, False)]
CASES.append((16, 4, 64, True, "e5m2", torch.float16))


@pytest.mark.parametrize("Hq,Sq,page,causal,fmt,dtype", CASES)
def test_sweep_against_the_fp64_oracle(Hq, Sq, page, causal, fmt, dtype):
    q = C.make_q(Hq, Sq, dtype).to(DEV)
    for lens in C.LENS:
        cache = _cache(page, lens, dtype, fmt)
        assert cache.seqlens.tolist() == list(lens)
        lat, ref = _dequant(cache), None
        for ns in C.SPLITS:
            out, lse, q8, sq = qa.fp8_mla_paged_func(q, cache, scale=C.SM_SCALE, causal=causal, num_splits=ns, max_seqlen_k=C.CAP,
                                                     return_lse=True, return_q8=True)
            if ref is None:
                assert torch.equal(q8.float() * sq[..., None], q.float())      # exact inputs: the kernel's q8 is q itself
                ref = C.reference((q8.double() * sq.double()[..., None]).cpu().numpy(), lat, lens, C.SM_SCALE, causal)
            what = (Hq, Sq, page, causal, fmt, lens, ns)
            got_o, got_l, fin = out.float().cpu().numpy(), lse.cpu().numpy(), np.isfinite(ref[1])
            print(what, "max |err| out", np.abs(got_o - ref[0]).max(), "lse", np.abs(got_l[fin] - ref[1][fin]).max() if fin.any() else 0.0)
            assert_within_bound(got_o, ref[0], what=what)
            assert np.array_equal(np.isneginf(got_l), ~fin), what                # a row without a key: LSE -inf exactly ...
            assert (got_o[~fin] == 0).all(), what                                # ... and a zero row
            assert np.abs(got_l[fin] - ref[1][fin]).max() <= C.LSE_TOL, what


@pytest.mark.parametrize("L", [64, 130])
def test_value_operand_orientation_probe(L):
    """key j carries j % 7 + 1 in channel 37 j mod 512 and zeros elsewhere, q = 0: uniform softmax, so out[c] = sum of the values of the keys
    j < L with 37 j mod 512 = c, over L.  A swapped key or channel in the transposed read moves an element by >= 1 / 130."""
    lat = torch.zeros((C.B, C.CAP, C.D))
    j = torch.arange(C.CAP)
    lat[:, j, (37 * j) % 512] = (j % 7 + 1).float()
    cache = _cache(64, (L,) * C.B, lat=(lat * C.SCALE_KV).bfloat16().to(DEV))
    ref = np.zeros(C.DV)
    for k in range(L):
        ref[(37 * k) % 512] += (k % 7 + 1) * C.SCALE_KV / L
    q = torch.zeros((C.B, 16, 1, C.D), dtype=torch.bfloat16, device=DEV)
    for ns in (1, 2):
        out = qa.fp8_mla_paged_func(q, cache, scale=C.SM_SCALE, num_splits=ns, max_seqlen_k=C.CAP).float().cpu().numpy()
        assert_within_bound(out, np.broadcast_to(ref, out.shape), what=(L, ns))
        assert np.abs(out - ref).max() < 0.25 / 130, (L, ns)      # (bf16 rounding of values <= 7/64 is far below one misplaced key)


def test_bit_identities():
    lens, q = C.LENS[1], C.make_q(20, 3, torch.bfloat16).to(DEV)
    call = lambda cache, **kw: qa.fp8_mla_paged_func(q, cache, scale=C.SM_SCALE, num_splits=3, max_seqlen_k=C.CAP, return_lse=True, **kw)
    out, lse, po, plse = call(_cache(128, lens), return_partials=True)
    # the partials merged by the eager combine definition: the fp32 order of the sum is the kernel's, exp / log are not -> the out bound
    m_out, m_lse = mla.combine_eager(po, plse, torch.bfloat16)
    assert_within_bound(m_out.float().cpu().numpy(), out.float().cpu().numpy(), what="combine")
    assert torch.equal(torch.isneginf(m_lse), torch.isneginf(lse)) and float((m_lse - lse)[torch.isfinite(lse)].abs().max()) <= 1e-5
    # NaN bytes behind L_b (and in never-written pages) change no bit; neither does another shuffle of the table with the pages moved along
    for other in (_cache(128, lens, prefill=0x7f), _cache(128, lens, table_seed=8)):
        o2, l2 = call(other)
        assert torch.equal(o2.view(torch.int16), out.view(torch.int16)) and torch.equal(l2.view(torch.int32), lse.view(torch.int32))


@pytest.mark.parametrize("T", [1, 5, 64, 70])
@pytest.mark.parametrize("start", [0, 60, 64])
def test_append_bytes_against_the_cpu_quantiser(T, start):
    page, M, Bn, marker = 64, 2, 2, 0xA5                                             # capacity 128: start 64 + T 70 drops 6 tokens
    for fmt, dtype in (("e4m3", torch.bfloat16), ("e5m2", torch.float16)):
        fp8, qmax = _native.fp8_dtype_of(fmt), torch.finfo(_native.fp8_dtype_of(fmt)).max
        cache = qa.alloc_paged_mla_cache_fp8(7, page, batch_size=Bn, max_pages_per_seq=M, scale=torch.tensor([0.5, 0.03125]), dtype=dtype,
                                             device=DEV, fp8_format=fmt)
        cache.pool.fill_(marker)
        table = torch.tensor([[5, 2], [0, 6]], dtype=torch.int32)
        cache.block_table.copy_(table)
        cache.seqlens.fill_(start)
        g = torch.Generator().manual_seed(T * 100 + start)
        proj = (torch.randn((Bn, T, 640), generator=g) * 8.0).to(dtype)             # one projection tensor; |x| / 0.03125 passes qmax: saturation
        proj[0, 0, 3], proj[1, T - 1, 520] = float("inf"), float("-inf")
        n = (T, max(T - 3, 0))
        dproj = proj.to(DEV)
        qa.paged_mla_cache_append_fp8(cache, dproj[..., :512], dproj[..., 512:576], new_lens=torch.tensor(n, dtype=torch.int32, device=DEV))
        want = torch.full((7, page, C.D), marker, dtype=torch.uint8)
        for b in range(Bn):
            kept = min(n[b], M * page - start)
            x8 = (proj[b, :kept, :576].float() / cache.scale[b].cpu()).to(dtype).clamp(-qmax, qmax).to(fp8).view(torch.uint8)
            for t in range(kept):
                want[table[b, (start + t) // page], (start + t) % page] = x8[t]
            assert int(cache.seqlens[b]) == start + kept
        assert torch.equal(mla.pool_rowmajor(cache.pool, 7, page).cpu(), want), (T, start, fmt)


def test_captured_append_and_attend_follows_table_and_lengths():
    page, lens0 = 64, (10, 64, 127, 199)
    cache = _cache(page, lens0)
    cache.pool.copy_(torch.randint(0, 0x78, cache.pool.shape, dtype=torch.uint8))          # every page holds finite e4m3 bytes
    pool0 = cache.pool.clone()
    q = C.make_q(16, 4, torch.bfloat16).to(DEV)
    new = C.make_latent(torch.bfloat16, seed=5)[:, :1].to(DEV)
    def step():
        qa.paged_mla_cache_append_fp8(cache, new[..., :C.DV], new[..., C.DV:])
        return qa.fp8_mla_paged_func(q, cache, scale=C.SM_SCALE, num_splits=2, max_seqlen_k=C.CAP, return_lse=True)
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_lse = step()
    for seed, lens in ((11, (199, 0, 63, 64)), (12, (65, 128, 1, 200)), (13, lens0)):
        def state():
            cache.pool.copy_(pool0)
            cache.block_table.copy_(C.make_table(page, seed)[0])
            cache.seqlens.copy_(torch.tensor(lens, dtype=torch.int32))
        state()
        graph.replay()
        got = (g_out.clone(), g_lse.clone(), cache.seqlens.clone(), cache.pool.clone())
        state()
        e_out, e_lse = step()
        assert cache.seqlens.tolist() == [x + 1 for x in lens] and torch.equal(got[2], cache.seqlens) and torch.equal(got[3], cache.pool)
        assert torch.equal(got[0].view(torch.int16), e_out.view(torch.int16)) and torch.equal(got[1].view(torch.int32), e_lse.view(torch.int32))

"""-m gpu: the serving entries at byte offsets above 2^31 and 2^32 -- a paged pool of more than 2^32 bytes, a contiguous cache whose image
exceeds 2^32 bytes, partial buffers of more than 2^31 floats.  The dense and packed entries have such tests
(tests/test_gpu_long_sequences.py, test_gpu_varlen.py, test_gpu_attention.py); a pool, a cache image and a partial buffer had none.

Every test ALLOCATES the large buffer and does not fill it (torch.empty; the few pages / keys a test uses are zeroed), runs the same calls
on the large geometry and on a small one that holds the same tokens at low addresses, and asks for the same BITS: an address computed in
32 bits lands somewhere else and the bits differ.  A test first asks torch.cuda.mem_get_info and skips, naming the bytes, on a card that
cannot hold its buffers (an MI355X holds them).  Every table entry and every length is in range."""
import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import kvcache_cases as KC

pytestmark = pytest.mark.gpu

DEV = "cuda"
GIB = 1 << 30


def _rand(shape, dtype, seed, mul=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * mul).to(dtype)


def _su(x):
    return torch.tensor(np.asarray(x), dtype=torch.int32, device=DEV)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _need(nbytes, what):
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes:
        pytest.skip(f"{what} needs {nbytes} bytes of device memory ({nbytes / GIB:.1f} GiB); {free} are free")
    print(f"{what}: {nbytes / GIB:.2f} GiB of device memory asked for, {free / GIB:.1f} GiB free")


def _all_same(got, want, what):
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert _same_bits(x, y), (what, i)
    assert torch.isfinite(got[0].float()).all(), what


# ---- 1. a paged pool of more than 2^32 bytes ---------------------------------------------------------------------------------------------------
def test_a_paged_pool_of_more_than_4_gib_gives_the_bits_of_a_small_pool():
    """D 128, Hkv 2, page 64: a page is 16 KiB, so page 131072 starts at byte 2^31 and page 262144 at byte 2^32 of either pool.  Slot 0 owns
    the LAST pages of the pool, slot 1's pages straddle both marks, slot 2 mixes low and high pages.  Two appends (the second starts
    mid-chunk), then the dense, packed and windowed paged entries; the small pool holds the same pages at low indices and the table is
    remapped.  Every output and every written page: the same bits."""
    D, Hkv, G, ps, P, Bq, M = 128, 2, 4, 64, 262208, 3, 8
    dtype, fmt = torch.bfloat16, "e4m3"
    page_bytes = Hkv * ps * D
    assert P >= 262200 and P * page_bytes > 1 << 32 and 131072 * page_bytes == 1 << 31 and 262144 * page_bytes == 1 << 32
    _need(2 * P * page_bytes + GIB, "the paged pool test")
    spare = 9                                                      # what every unused table entry points at (in range, zeroed)
    big_table = np.full((Bq, M), spare, np.int64)
    big_table[0, :5] = [P - 1, P - 2, P - 3, P - 4, P - 5]
    big_table[1, :5] = [131071, 131072, 262143, 262144, 131073]
    big_table[2, :5] = [1, 0, 262145, 5, 131070]
    pages = sorted(set(big_table.flatten().tolist()))
    order = np.random.RandomState(0).permutation(len(pages))
    small_of = {p: int(order[i]) for i, p in enumerate(pages)}
    small_table = np.vectorize(small_of.get)(big_table)
    sk, sv = torch.tensor([[0.010, 0.020], [0.015, 0.012], [0.030, 0.008]]), torch.tensor([[0.02, 0.04], [0.03, 0.024], [0.06, 0.016]])
    small = qa.alloc_paged_kv_cache_fp8(len(pages), Hkv, ps, D, batch_size=Bq, max_pages_per_seq=M, scale_k=sk.to(DEV), scale_v=sv.to(DEV), dtype=dtype,
                                        device=DEV, fp8_format=fmt)
    L = _native.lib()
    pools = [torch.empty((L.qattn_fp8_tensor_bytes(layout, P, Hkv, ps, D),), dtype=torch.uint8, device=DEV)
             for layout in (_native.LAYOUT_KFRAG, _native.LAYOUT_VFRAG)]
    assert all(p.numel() == P * page_bytes for p in pools)
    big = qa.PagedKVCacheFP8(pools[0], pools[1], small.scale_k, small.scale_v, torch.zeros_like(small.block_table), torch.zeros_like(small.seqlens),
                             (P, Hkv, ps, D), fmt, dtype, small.numerics, "frag")
    idx_big, idx_small = torch.tensor(pages, device=DEV), torch.tensor([small_of[p] for p in pages], device=DEV)
    for pool in pools:
        pool.view(P, page_bytes)[idx_big] = 0
    big.block_table.copy_(_su(big_table))
    small.block_table.copy_(_su(small_table))
    lens = [0, 0, 0]
    for step, counts in enumerate(([130, 70, 129], [130, 130, 65])):
        kn, vn = _rand((Bq, Hkv, 130, D), dtype, 10 + step, 1.5), _rand((Bq, Hkv, 130, D), dtype, 20 + step, 3.0)
        for c in (big, small):
            qa.paged_kv_cache_append_fp8(c, kn, vn, new_lens=_su(counts))
        lens = [a + n for a, n in zip(lens, counts)]
        assert big.seqlens.tolist() == small.seqlens.tolist() == lens
        for pb, psm in zip(pools, (small.k, small.v)):
            assert torch.equal(pb.view(P, page_bytes)[idx_big], psm.view(len(pages), page_bytes)[idx_small]), ("the written pages", step)
    assert small.k.view(len(pages), page_bytes)[small_of[P - 1]].any() and small.k.view(len(pages), page_bytes)[small_of[262144]].any()
    Hq = Hkv * G
    qd = _rand((Bq, Hq, 5, D), dtype, 30, 1.5)
    counts = (5, 1, 130)
    qp, cu = _rand((sum(counts), Hq, D), dtype, 31, 1.5), _su([0] + np.cumsum(counts).tolist())
    kw = dict(max_seqlen_k=320, return_lse=True, return_partials=True)
    calls = {
        "paged": lambda c: qa.fp8_attn_paged_func(qd, c, causal=True, num_splits=2, **kw),
        "packed": lambda c: qa.fp8_attn_paged_varlen_func(qp, c, cu, 130, causal=True, num_splits=3, **kw),
        "paged window": lambda c: qa.fp8_attn_paged_window_func(qd, c, (100, 0), num_splits=2, **kw),
        "packed window": lambda c: qa.fp8_attn_paged_varlen_window_func(qp, c, cu, 130, (100, 0), num_splits=3, **kw),
        "packed fast": lambda c: qa.fp8_attn_paged_varlen_func(qp, c, cu, 130, causal=True, num_splits=1, precision="fast", **kw),
    }
    for what, f in calls.items():
        _all_same(f(big), f(small), what)


# ---- 2. a contiguous cache whose image exceeds 2^32 bytes --------------------------------------------------------------------------------------
def test_a_contiguous_cache_image_of_more_than_4_gib_gives_the_bits_of_a_small_cache():
    """B 2, Hkv 4, D 128, capacity 4 800 000 keys: the image of the last (batch element, kv head) starts at byte 7 x 4.8 M x 128 > 2^32 and
    that of (1, 0) above 2^31.  Short used lengths; every head is appended to and attended, and holds the bits of a 256-key cache."""
    B, Hkv, G, D, cap, small_cap = 2, 4, 2, 128, 4_800_000, 256
    dtype, fmt = torch.bfloat16, "e4m3"
    assert cap % 64 == 0 and (B * Hkv - 1) * cap * D > 1 << 32 and Hkv * cap * D > 1 << 31
    _need(2 * B * Hkv * cap * D + GIB, "the contiguous cache test")
    sk, sv = torch.full((B, Hkv), 0.012), torch.full((B, Hkv), 0.025)
    small = qa.alloc_kv_cache_fp8(B, Hkv, small_cap, D, scale_k=sk.to(DEV), scale_v=sv.to(DEV), dtype=dtype, device=DEV, fp8_format=fmt)
    L = _native.lib()
    imgs = [torch.empty((L.qattn_fp8_tensor_bytes(layout, B, Hkv, cap, D),), dtype=torch.uint8, device=DEV)
            for layout in (_native.LAYOUT_KFRAG, _native.LAYOUT_VFRAG)]
    assert all(i.numel() == B * Hkv * cap * D for i in imgs)
    for img in imgs:
        img.view(B * Hkv, cap * D)[:, :small_cap * D] = 0
    big = qa.KVCacheFP8(imgs[0], imgs[1], small.scale_k, small.scale_v, (B, Hkv, cap, D), fmt, dtype, small.numerics, "frag", torch.zeros_like(small.seqlens))
    lens = [0, 0]
    for step, counts in enumerate(([130, 100], [70, 70])):
        kn, vn = _rand((B, Hkv, 130, D), dtype, 40 + step, 1.5), _rand((B, Hkv, 130, D), dtype, 50 + step, 3.0)
        for c in (big, small):
            qa.kv_cache_append_fp8(c, kn, vn, new_lens=_su(counts))
        lens = [a + n for a, n in zip(lens, counts)]
        assert big.seqlens.tolist() == small.seqlens.tolist() == lens
        for ib, ism in zip(imgs, (small.k, small.v)):
            assert torch.equal(ib.view(B * Hkv, cap * D)[:, :small_cap * D], ism.view(B * Hkv, small_cap * D)), ("the written keys", step)
    assert small.k.view(B * Hkv, -1)[-1].any()
    q = _rand((B, Hkv * G, 5, D), dtype, 60, 1.5)
    kw = dict(num_splits=2, return_lse=True, return_partials=True)
    calls = {
        "causal": lambda c: qa.fp8_attn_splitkv_func(q, c, causal=True, seqused_k=c.seqlens, **kw),
        "window": lambda c: qa.fp8_attn_splitkv_window_func(q, c, (100, 0), seqused_k=c.seqlens, **kw),
        "one split": lambda c: qa.fp8_attn_splitkv_func(q, c, causal=True, seqused_k=c.seqlens, num_splits=1, return_lse=True),
    }
    for what, f in calls.items():
        _all_same(f(big), f(small), what)


# ---- 3. partial buffers of more than 2^31 floats -----------------------------------------------------------------------------------------------
def test_partial_buffers_of_more_than_2_31_floats_keep_the_batched_equals_per_element_rule():
    """B 32, Hq 32, Sq 130, D 256, 64 splits over 8192 keys: partial_o holds 64 B Hq Sq D > 2^31 floats (and the workspace a second buffer
    of that size).  The last batch element's out, lse and partials are the bits of the call on that element alone with the same split
    count (contract (e) of include/qattn_splitkv.h); so are the first's."""
    B, Hq, Hkv, Sq, Skv, D, ns = 32, 32, 4, 130, 8192, 256, 64
    dtype = torch.bfloat16
    floats = ns * B * Hq * Sq * D
    assert floats > 1 << 31
    _need(2 * 4 * floats + 3 * GIB, "the partial buffer test")
    kv = qa.prepare_kv_fp8(_rand((B, Hkv, Skv, D), dtype, 70), _rand((B, Hkv, Skv, D), dtype, 71))
    q = _rand((B, Hq, Sq, D), dtype, 72, 1.5)
    kw = dict(causal=True, num_splits=ns, return_lse=True, return_partials=True)
    out, lse, po, plse, ppath = qa.fp8_attn_splitkv_func(q, kv, **kw)
    assert po.shape == (ns, B, Hq, Sq, D) and po.numel() == floats
    for b in (B - 1, 0):
        one = qa.PreparedKV(kv.k.view(B, -1)[b].contiguous(), kv.v.view(B, -1)[b].contiguous(), kv.scale_k[b:b + 1].contiguous(),
                            kv.scale_v[b:b + 1].contiguous(), (1, Hkv, Skv, D), kv.fp8_format, kv.dtype, kv.numerics, "frag")
        wo, wl, wpo, wpl, wpp = qa.fp8_attn_splitkv_func(q[b:b + 1], one, **kw)
        _all_same((out[b:b + 1], lse[b:b + 1], po[:, b:b + 1], plse[:, b:b + 1], ppath[:, b:b + 1]), (wo, wl, wpo, wpl, wpp), f"batch element {b}")
    # every partial of the last element was written: the causal rows of the last split own keys, so its LSEs are finite
    assert torch.isfinite(plse[ns - 1, B - 1, :, Sq - 1]).all() and torch.isfinite(out[B - 1].float()).all()

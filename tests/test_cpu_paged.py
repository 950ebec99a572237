"""The paged FP8 K/V cache (quantumattention_amd/paged.py, include/qattn_paged.h) without a GPU: exports and signatures, every validation
reason, the C entries' argument checks (returned before any device call), the pool's address map against qattn_fp8_tensor_bytes, the eager
definitions -- paged "append + attend" = contiguous "append + attend" on the gathered cache, bit for bit -- and the teeth of the shared
tables (tests/paged_cases.py): each table mutant changes the gathered bytes and the eager output by more than the GPU tests' bound."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, paged, splitkv
from tests import paged_cases as P

B, HKV = P.B, P.HKV


def _cache(num_pages=8, page_size=64, D=64, M=4, dtype=torch.bfloat16, sk=0.01, sv=0.02, batch=B, **kw):
    return qa.alloc_paged_kv_cache_fp8(num_pages, HKV, page_size, D, batch_size=batch, max_pages_per_seq=M, scale_k=sk, scale_v=sv, dtype=dtype,
                                       device="cpu", **kw)


def _new(T, D=64, dtype=torch.bfloat16, seed=0, batch=B):
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.randn(batch, HKV, T, D, generator=g) * 1.5).to(dtype) for _ in range(2))


# ---- surface ------------------------------------------------------------------------------------------------------------------------------
def test_exports_and_signatures():
    for name in ("PagedKVCacheFP8", "alloc_paged_kv_cache_fp8", "paged_kv_cache_append_fp8", "fp8_attn_paged_func"):
        assert getattr(qa, name) is getattr(paged, name) and name not in qa.__all__
    assert hasattr(qa.ops, "fp8_paged_kv_cache_append_") and hasattr(qa.ops, "fp8_paged_splitkv_attention_forward")
    sig = lambda f: str(inspect.signature(f)).replace("typing.", "").replace("torch.Tensor", "Tensor")
    assert sig(qa.alloc_paged_kv_cache_fp8) == (
        "(num_pages: int, Hkv: int, page_size: int, D: int, *, batch_size: int, max_pages_per_seq: int, scale_k, scale_v, dtype, device, "
        "fp8_format: Optional[str] = None, numerics: Optional[str] = None) -> quantumattention_amd.paged.PagedKVCacheFP8")
    assert sig(qa.paged_kv_cache_append_fp8) == (
        "(cache: quantumattention_amd.paged.PagedKVCacheFP8, k_new: Tensor, v_new: Tensor, *, new_lens: Optional[Tensor] = None, "
        "advance: bool = True) -> quantumattention_amd.paged.PagedKVCacheFP8")
    assert sig(qa.fp8_attn_paged_func) == (
        "(q, cache: quantumattention_amd.paged.PagedKVCacheFP8, *, causal: bool = False, scale: Optional[float] = None, "
        "seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, num_splits: int = 0, precision: str = 'accurate', "
        "return_lse: bool = False, return_partials: bool = False)")
    for name in ("qattn_paged_kv_cache_append_fp8", "qattn_fp8_attention_paged_splitkv_workspace_bytes", "qattn_fp8_attention_paged_splitkv_forward"):
        assert name in _native.EXPORTS
    # the contiguous functions keep their signatures: the paged ones are siblings
    assert "block_table" not in sig(qa.fp8_attn_splitkv_func) and "block_table" not in sig(qa.kv_cache_append_fp8)


def test_alloc_gives_zero_pools_a_zero_table_zero_lengths_and_fp32_scales_per_slot():
    c = _cache(num_pages=5, page_size=128, D=128, M=3, sk=torch.tensor([0.5, 0.25]), sv=3, fp8_format="e5m2", numerics="eager")
    assert isinstance(c, qa.PagedKVCacheFP8) and c.shape == (5, HKV, 128, 128) and c.layout == "rowmajor"
    assert (c.num_pages, c.page_size, c.batch_size, c.max_pages_per_seq, c.capacity) == (5, 128, B, 3, 384)
    assert c.fp8_format == "e5m2" and c.numerics == "eager" and c.dtype == torch.bfloat16
    assert c.k.dtype == torch.float8_e5m2 and c.k.shape == c.shape and not c.k.view(torch.uint8).any() and not c.v.view(torch.uint8).any()
    assert c.block_table.dtype == torch.int32 and c.block_table.shape == (B, 3) and not c.block_table.any()
    assert c.seqlens.dtype == torch.int32 and c.seqlens.tolist() == [0] * B
    assert c.scale_k.dtype == torch.float32 and torch.equal(c.scale_k, torch.tensor([[0.5, 0.25]] * B)) and torch.equal(c.scale_v, torch.full((B, HKV), 3.0))


@pytest.mark.parametrize("bad", ["num_pages", "Hkv", "batch", "M", "ps_0", "ps_96", "ps_32", "ps_bool", "D", "dtype", "chunks_2^31", "capacity_2^31",
                                 "scale_zero", "scale_shape", "fmt", "numerics"])
def test_alloc_refuses(bad):
    a = dict(num_pages=8, Hkv=2, page_size=64, D=64)
    kw = dict(batch_size=3, max_pages_per_seq=4, scale_k=0.01, scale_v=0.01, dtype=torch.bfloat16, device="cpu")
    edits = {"num_pages": (a, "num_pages", 0), "Hkv": (a, "Hkv", -1), "batch": (kw, "batch_size", 0), "M": (kw, "max_pages_per_seq", 0),
             "ps_0": (a, "page_size", 0), "ps_96": (a, "page_size", 96), "ps_32": (a, "page_size", 32), "ps_bool": (a, "page_size", True),
             "D": (a, "D", 48), "dtype": (kw, "dtype", torch.float32), "chunks_2^31": (a, "num_pages", 2 ** 30),
             "capacity_2^31": (kw, "max_pages_per_seq", 2 ** 25), "scale_zero": (kw, "scale_k", 0.0), "scale_shape": (kw, "scale_v", torch.ones(5)),
             "fmt": (kw, "fp8_format", "e3m4"), "numerics": (kw, "numerics", "exact")}
    d, key, val = edits[bad]
    d[key] = val
    with pytest.raises(ValueError):
        qa.alloc_paged_kv_cache_fp8(a["num_pages"], a["Hkv"], a["page_size"], a["D"], **kw)
    if bad not in ("fmt", "numerics"):
        assert paged.paged_alloc_input_reason(a["num_pages"], a["Hkv"], a["page_size"], a["D"], kw["batch_size"], kw["max_pages_per_seq"],
                                              kw["scale_k"], kw["scale_v"], kw["dtype"])


@pytest.mark.parametrize("bad", ["cache", "k_3d", "grad", "dtype", "shape_kv", "batch", "heads", "D", "T0", "strides", "table_dtype", "table_1d",
                                 "table_strided", "seqlens_dtype", "seqlens_shape", "new_lens_dtype", "new_lens_shape", "scale_shape", "pool_dtype"])
def test_append_refuses(bad):
    c = _cache()
    k, v = _new(3)
    nl = None
    if bad == "cache":
        c = qa.alloc_kv_cache_fp8(B, HKV, 256, 64, scale_k=1.0, scale_v=1.0, dtype=torch.bfloat16, device="cpu")
    elif bad == "k_3d":
        k = k[0]
    elif bad == "grad":
        k = k.float().requires_grad_().to(torch.bfloat16)
    elif bad == "dtype":
        k, v = k.half(), v.half()
    elif bad == "shape_kv":
        v = v[:, :, :2]
    elif bad == "batch":
        k, v = _new(3, batch=B + 1)
    elif bad == "heads":
        k, v = k[:, :1], v[:, :1]
    elif bad == "D":
        k, v = _new(3, D=128)
    elif bad == "T0":
        k, v = k[:, :, :0], v[:, :, :0]
    elif bad == "strides":
        k = torch.randn(B, HKV, 3, 68).to(torch.bfloat16)[..., 2:66]
    elif bad == "table_dtype":
        c.block_table = c.block_table.long()
    elif bad == "table_1d":
        c.block_table = c.block_table[0]
    elif bad == "table_strided":
        c.block_table = torch.zeros(B, 8, dtype=torch.int32)[:, ::2]
    elif bad == "seqlens_dtype":
        c.seqlens = c.seqlens.long()
    elif bad == "seqlens_shape":
        c.seqlens = c.seqlens[:2]
    elif bad == "new_lens_dtype":
        nl = torch.zeros(B)
    elif bad == "new_lens_shape":
        nl = torch.zeros(B + 1, dtype=torch.int32)
    elif bad == "scale_shape":
        c.scale_k = c.scale_k[:, :1]
    else:
        c.k = c.k.view(torch.uint8)
    assert paged.paged_append_input_reason(c, k, v, nl)
    with pytest.raises(ValueError):
        qa.paged_kv_cache_append_fp8(c, k, v, new_lens=nl)


@pytest.mark.parametrize("bad", ["q_3d", "grad", "q_f32", "cache", "dtype", "D", "batch", "heads", "Hq0", "seqused_dtype", "seqused_shape", "max_0", "max_big",
                                 "max_float", "max_bool", "splits", "splits_bool", "scale_0", "scale_nan", "table_dtype", "auto"])
def test_attention_refuses(bad):
    c = _cache()
    q = torch.randn(B, 4, 2, 64).to(torch.bfloat16)
    kw = {}
    if bad == "q_3d":
        q = q[0]
    elif bad == "grad":
        q = q.float().requires_grad_().to(torch.bfloat16)
    elif bad == "q_f32":
        q = q.float()
    elif bad == "cache":
        c = qa.alloc_kv_cache_fp8(B, HKV, 256, 64, scale_k=1.0, scale_v=1.0, dtype=torch.bfloat16, device="cpu")
    elif bad == "dtype":
        q = q.half()
    elif bad == "D":
        q = torch.randn(B, 4, 2, 128).to(torch.bfloat16)
    elif bad == "batch":
        q = q[:2]
    elif bad == "heads":
        q = q[:, :3]
    elif bad == "Hq0":
        q = q[:, :0]
    elif bad == "seqused_dtype":
        kw["seqused_k"] = torch.zeros(B)
    elif bad == "seqused_shape":
        kw["seqused_k"] = torch.zeros(B - 1, dtype=torch.int32)
    elif bad == "max_0":
        kw["max_seqlen_k"] = 0
    elif bad == "max_big":
        kw["max_seqlen_k"] = c.capacity + 1
    elif bad == "max_float":
        kw["max_seqlen_k"] = 64.0
    elif bad == "max_bool":
        kw["max_seqlen_k"] = True
    elif bad == "splits":
        kw["num_splits"] = 65
    elif bad == "splits_bool":
        kw["num_splits"] = True
    elif bad == "scale_0":
        kw["scale"] = 0.0
    elif bad == "scale_nan":
        kw["scale"] = float("nan")
    elif bad == "table_dtype":
        c.block_table = c.block_table.long()
    else:
        kw["precision"] = "auto"
    if bad != "auto":
        assert paged.paged_attn_input_reason(q, c, kw.get("seqused_k"), kw.get("scale"), kw.get("num_splits", 0), kw.get("max_seqlen_k"))
    with pytest.raises(ValueError):
        qa.fp8_attn_paged_func(q, c, **kw)


def test_the_c_entries_refuse_before_any_device_call():
    """the argument checks of include/qattn_paged.h; the pointers are never dereferenced on these paths"""
    L = _native.lib()
    INVALID, DIM, FMT, WORKSPACE = -1, -2, -3, L.qattn_fp8_attention_splitkv_forward(4096, _native.FMT_BF16, 1 << 20, 2 << 20, 256, 512, 8192, None,
                                                                                     None, 1, 4, 2, 1, 256, 64, _native.FMT_E4M3, 0, 0, 0.0, 1, 1,
                                                                                     None, None, None, None, None, None, None, 0, None)
    assert WORKSPACE < 0 and WORKSPACE not in (INVALID, DIM, FMT)     # (the contiguous entry's own code for a missing workspace)
    s3 = (ctypes.c_longlong * 3)(2 * 3 * 64, 3 * 64, 64)
    ok = dict(k16=4096, v16=8192, in_fmt=_native.FMT_BF16, ks=s3, vs=s3, kp=1 << 20, vp=2 << 20, sk=256, sv=512, table=2048, tstride=4, seqlens=1024,
              new_lens=None, advance=1, B=2, Hkv=2, T=3, num_pages=8, page_size=64, max_pages=4, D=64, fp8_fmt=_native.FMT_E4M3, stream=None)
    order = ("k16", "v16", "in_fmt", "ks", "vs", "kp", "vp", "sk", "sv", "table", "tstride", "seqlens", "new_lens", "advance", "B", "Hkv", "T",
             "num_pages", "page_size", "max_pages", "D", "fp8_fmt", "stream")
    call = lambda **over: L.qattn_paged_kv_cache_append_fp8(*[dict(ok, **over)[n] for n in order])
    for name in ("k16", "v16", "ks", "vs", "kp", "vp", "sk", "sv", "table", "seqlens"):
        assert call(**{name: None}) == INVALID, name
    for name in ("kp", "vp", "k16"):
        assert call(**{name: ok[name] + 8}) == INVALID, name
    assert call(table=2050) == INVALID
    for ps in (0, 32, 96, -64, 65):
        assert call(page_size=ps) == INVALID, ps
    assert call(tstride=3) == INVALID and call(num_pages=0) == INVALID and call(max_pages=0) == INVALID
    assert call(num_pages=1 << 30, page_size=256) == INVALID                   # num_pages Hkv pc beyond 2^31 - 1
    assert call(max_pages=1 << 25, tstride=1 << 25, page_size=64) == INVALID   # a capacity beyond 2^31 - 65
    assert call(D=96) == DIM and call(in_fmt=_native.FMT_E4M3) == FMT and call(fp8_fmt=_native.FMT_BF16) == FMT
    for name in ("B", "Hkv", "T"):
        assert call(**{name: 0}) == INVALID, name

    fok = dict(q16=4096, in_fmt=_native.FMT_BF16, kp=1 << 20, vp=2 << 20, table=2048, tstride=4, num_pages=8, page_size=64, max_pages=4, sk=256, sv=512,
               out=8192, lse=None, used=1024, B=2, Hq=4, Hkv=2, Sq=1, Skv=256, D=64, fp8_fmt=_native.FMT_E4M3, numerics=0, causal=0, sm=0.0,
               precision=1, ns=1, q8=None, sq=None, path=None, po=None, plse=None, ppath=None, ws=None, ws_bytes=0, stream=None)
    fcall = lambda **over: L.qattn_fp8_attention_paged_splitkv_forward(*dict(fok, **over).values())
    assert fcall() == WORKSPACE                                                # every argument check passed: the next one is the workspace's
    for name in ("q16", "kp", "vp", "table", "sk", "sv", "out", "used"):        # seqused_k is REQUIRED here
        assert fcall(**{name: None}) == INVALID, name
    for name in ("kp", "vp", "q16", "out"):
        assert fcall(**{name: fok[name] + 8}) == INVALID, name
    for ps in (0, 32, 96, -64):
        assert fcall(page_size=ps) == INVALID, ps
    assert fcall(tstride=3) == INVALID and fcall(num_pages=0) == INVALID and fcall(max_pages=0) == INVALID
    assert fcall(Skv=257) == INVALID and fcall(Skv=0) == INVALID               # Skv <= max_pages page_size
    assert fcall(num_pages=1 << 30, page_size=256, Skv=256) == INVALID
    assert fcall(D=96) == DIM and fcall(Hq=3) == DIM and fcall(fp8_fmt=_native.FMT_BF16) == FMT
    assert fcall(ns=65) == INVALID and fcall(ns=0, po=4096) == INVALID
    assert (L.qattn_fp8_attention_paged_splitkv_workspace_bytes(2, 4, 2, 1, 256, 64, 3)
            == L.qattn_fp8_attention_splitkv_workspace_bytes(2, 4, 2, 1, 256, 64, 3) > 0)


# ---- the address map ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_the_address_map_tiles_the_pool_and_a_pool_is_a_contiguous_cache_of_pages(D, page_size):
    L = _native.lib()
    num_pages, Hkv, pc = 7, 3, page_size // 64
    for layout in (_native.LAYOUT_KFRAG, _native.LAYOUT_VFRAG):
        total = L.qattn_fp8_tensor_bytes(layout, num_pages, Hkv, page_size, D)
        assert total == P.pool_bytes(num_pages, Hkv, page_size, D)
        # a pool is the image of a [num_pages, Hkv, page_size, D] cache: page p's head h starts where (b = p, h) of that cache starts
        assert P.chunk_start(1, 0, 0, Hkv, page_size, D) == L.qattn_fp8_tensor_bytes(layout, 1, Hkv, page_size, D)
        assert P.chunk_start(0, 1, 0, Hkv, page_size, D) == L.qattn_fp8_tensor_bytes(layout, 1, 1, page_size, D)
    starts = [P.chunk_start(p, h, c, Hkv, page_size, D) for p in range(num_pages) for h in range(Hkv) for c in range(pc)]
    assert starts == list(range(0, total, 64 * D))                              # the chunks tile the pool in (p, h, c) order, none straddles a page
    # the index copy of `gather` is the address map's
    pool = torch.randint(0, 256, (total,), dtype=torch.uint8)
    table = [[3, 0, 6], [6, 6, 1]]
    assert np.array_equal(P.gather(pool, table, Hkv, page_size, D).numpy(), P.gather_by_address(pool.numpy(), table, Hkv, page_size, D))


@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
def test_the_shared_tables_have_the_properties_the_gpu_tests_rely_on(page_size):
    seen = set()
    for t in P.shared_tables(page_size):
        t.check()
        assert t.num_pages == B * t.M + 2 and t.M * page_size == P.CAP
        seen |= set(t.lens)
        assert max(t.lens) >= 1100
    assert seen == {0, 1, 63, 64, 65, page_size - 1, page_size, page_size + 1, 1100, 1280}
    assert any(t.shared for t in P.shared_tables(page_size))


# ---- the eager definitions ------------------------------------------------------------------------------------------------------------------
def _paged_and_contiguous(page_size, D, dtype, fmt, M=4, seed=0):
    """a paged CPU cache with a shuffled private table and a contiguous CPU cache with the same scales"""
    num_pages = B * M + 1
    sk = torch.tensor([[0.010, 0.020], [0.015, 0.012], [0.030, 0.008]])
    pc = qa.alloc_paged_kv_cache_fp8(num_pages, HKV, page_size, D, batch_size=B, max_pages_per_seq=M, scale_k=sk, scale_v=sk * 2, dtype=dtype,
                                     device="cpu", fp8_format=fmt)
    perm = np.random.RandomState(seed).permutation(num_pages)[:B * M].reshape(B, M)
    pc.block_table.copy_(torch.from_numpy(perm.astype(np.int32)))
    cc = qa.alloc_kv_cache_fp8(B, HKV, M * page_size, D, scale_k=sk, scale_v=sk * 2, dtype=dtype, device="cpu", fp8_format=fmt)
    return pc, cc


@pytest.mark.parametrize("page_size,D,dtype,fmt", [(64, 64, torch.bfloat16, "e4m3"), (128, 128, torch.float16, "e5m2"), (256, 64, torch.bfloat16, "e5m2")])
def test_eager_paged_append_and_attend_equal_the_contiguous_ones_on_the_gathered_cache(page_size, D, dtype, fmt):
    pc, cc = _paged_and_contiguous(page_size, D, dtype, fmt)
    cap = pc.capacity
    steps = [(1, None, True), (7, None, True), (page_size - 3, None, True), (130, None, True), (4, [0, 3, 4], True), (5, None, False),
             (cap, [cap, 9, 0], True)]                                        # the last one overflows sequence 0: dropped tokens, seqlens saturates
    before = pc.k.view(torch.uint8).clone()
    for i, (T, nl, adv) in enumerate(steps):
        k, v = _new(T, D, dtype, seed=10 + i)
        nlt = None if nl is None else torch.tensor(nl, dtype=torch.int32)
        assert qa.paged_kv_cache_append_fp8(pc, k, v, new_lens=nlt, advance=adv) is pc
        qa.kv_cache_append_fp8(cc, k, v, new_lens=nlt, advance=adv)
        assert pc.seqlens.tolist() == cc.seqlens.tolist()
        g = paged.gather_paged_eager(pc)
        assert torch.equal(g.k.view(torch.uint8), cc.k.view(torch.uint8)) and torch.equal(g.v.view(torch.uint8), cc.v.view(torch.uint8)), i
    assert pc.seqlens[0] == cap
    unused = sorted(set(range(pc.num_pages)) - set(pc.block_table.flatten().tolist()))
    assert unused and torch.equal(pc.k.view(torch.uint8)[unused], before[unused])         # a page no table row names is never written
    q = (torch.randn(B, 4, 3, D) * 1.5).to(dtype)
    for ns, causal, prec, mx in ((1, False, "accurate", None), (3, True, "accurate", None), (2, True, "fast", cap - 70), (0, False, "accurate", 200)):
        got = qa.fp8_attn_paged_func(q, pc, causal=causal, num_splits=ns, precision=prec, max_seqlen_k=mx, return_lse=True, return_partials=True)
        kv = cc if mx is None else qa.PreparedKV(cc.k[:, :, :mx].contiguous(), cc.v[:, :, :mx].contiguous(), cc.scale_k, cc.scale_v,
                                                 (B, HKV, mx, D), cc.fp8_format, cc.dtype, cc.numerics, "rowmajor")
        want = qa.fp8_attn_splitkv_func(q, kv, causal=causal, seqused_k=cc.seqlens, num_splits=ns, precision=prec, return_lse=True, return_partials=True)
        assert len(got) == len(want) == 5
        for x, y in zip(got, want):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (ns, causal, prec, mx)
    # seqused_k overrides cache.seqlens
    su = torch.tensor([5, 0, 70], dtype=torch.int32)
    a = qa.fp8_attn_paged_func(q, pc, seqused_k=su, num_splits=1)
    b = qa.fp8_attn_splitkv_func(q, cc, seqused_k=su, num_splits=1)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and not a[1].any()


def test_eager_table_entries_are_clamped_and_unread_ones_are_ignored():
    pc, cc = _paged_and_contiguous(64, 64, torch.bfloat16, "e4m3", M=3)
    k, v = _new(70, seed=3)
    qa.paged_kv_cache_append_fp8(pc, k, v)
    q = torch.randn(B, 2, 1, 64).to(torch.bfloat16)
    want = qa.fp8_attn_paged_func(q, pc, num_splits=1)
    t = pc.block_table.clone()
    pc.block_table[:, 2] = 10 ** 6                                # behind ceil(70 / 64) = 2 pages: never read
    assert torch.equal(qa.fp8_attn_paged_func(q, pc, num_splits=1).view(torch.int16), want.view(torch.int16))
    pc.block_table.copy_(t)
    pc.block_table[0, 1] = -7                                     # read: clamped to page 0, never an index error
    pc.block_table[1, 1] = 10 ** 6                                # clamped to the last page
    out = qa.fp8_attn_paged_func(q, pc, num_splits=1)
    assert out.shape == want.shape and torch.equal(out[2].view(torch.int16), want[2].view(torch.int16))
    qa.paged_kv_cache_append_fp8(pc, k[:, :, :1], v[:, :, :1])    # the append clamps too
    assert pc.seqlens.tolist() == [71] * B


def test_max_seqlen_k_tightens_what_the_auto_rule_sees():
    """a serving table is far wider than any live sequence: the num_splits = 0 rule (a pure function of the shape) over-splits on it"""
    live, wide = 8192, 4 * 8192
    rule = lambda Skv: _native.splitkv_auto_splits(1, 32, 8, 1, Skv, 128, 256)
    assert rule(wide) > rule(live) >= 1
    assert splitkv._resolve_splits(0, 1, 32, 8, 1, live, 128, "cpu") == rule(live)


# ---- teeth: what a wrong use of the table does on the shared tables --------------------------------------------------------------------------
@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
def test_every_table_mutant_changes_the_gathered_bytes_and_the_eager_output_beyond_the_gpu_bound(page_size):
    D, fmt, dtype = 64, "e4m3", torch.bfloat16
    fp8 = P.FP8[fmt]
    q = (torch.randn(B, 2, 1, D, generator=torch.Generator().manual_seed(5)) * 2).to(dtype)
    sk, sv = torch.full((B, HKV), 0.05), torch.full((B, HKV), 0.5)
    for t in P.shared_tables(page_size):
        rk, rv = P.random_rows(t.num_pages, page_size, D, fmt, seed=page_size + t.lens[0])
        # V: every page carries its own level (+ noise), so that an output is a weighted mean of the levels of the pages it read -- random
        # zero-mean V would average any mix of pages to ~0, inside the bound.  (The poison page stays finite here: the eager definition
        # multiplies the masked keys' V by P = 0, and 0 x NaN is NaN.)
        level = ((torch.arange(t.num_pages) * 7) % t.num_pages - t.num_pages // 2).float()
        rv = (level[:, None, None, None] + rv.view(fp8).float()).to(fp8).view(torch.uint8)
        su = torch.tensor(t.lens, dtype=torch.int32)

        def attend(mutant):
            gk, gv = (torch.from_numpy(P.gather_rows(r.numpy(), t.table, page_size, mutant)) for r in (rk, rv))
            kv = qa.PreparedKV(gk.view(fp8), gv.view(fp8), sk, sv, (B, HKV, P.CAP, D), fmt, dtype, "compiled", "rowmajor")
            return gk, qa.fp8_attn_splitkv_func(q, kv, seqused_k=su, num_splits=1).float()

        gk0, ref = attend(None)
        assert torch.isfinite(ref).all()
        # the product's eager definition is the unmutated lookup
        c = qa.alloc_paged_kv_cache_fp8(t.num_pages, HKV, page_size, D, batch_size=B, max_pages_per_seq=t.M, scale_k=sk, scale_v=sv, dtype=dtype,
                                        device="cpu", fp8_format=fmt)
        c.k.view(torch.uint8).copy_(rk)
        c.v.view(torch.uint8).copy_(rv)
        c.block_table.copy_(torch.from_numpy(t.table))
        c.seqlens.copy_(su)
        assert torch.equal(qa.fp8_attn_paged_func(q, c, num_splits=1).float(), ref)
        bound = 2.0 ** -6 * torch.clamp(ref.abs() / 2, min=1.0)
        for mutant in ("identity", "row0", "round-up"):
            gk, out = attend(mutant)
            used = torch.arange(P.CAP)[None, :] < su[:, None]
            assert (gk != gk0).any(-1).any(1)[used].any(), (t.lens, mutant, "the used keys' bytes did not change")
            err = (out - ref).abs()
            assert bool((~torch.isfinite(out)).any()) or bool((err > bound).any()), (t.lens, mutant, float((err / bound).max()))

"""Sliding windows for the split-KV, paged and packed-paged entries without a GPU (quantumattention_amd/splitkv_window.py,
include/qattn_splitkv_window.h): the surface, every ValueError, the split plan and the num_splits = 0 rules, the page count a window lets
a paged cache forget, the C entries' window checks, the fake registrations, the eager definitions against the fp64 reference of
tests/splitkv_window_cases.py that walks (kv head, tile, split) -- path bytes included -- and the TEETH of the membership probes the GPU
tests run: every named way of getting the window wrong moves a row of those very inputs by >= 4x the bound."""
import inspect
import math

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, splitkv, splitkv_window
from tests import paged_cases as P
from tests import paged_varlen_cases as V
from tests import probes as PR
from tests import splitkv_window_cases as W

B, HKV, CAP = P.B, P.HKV, P.CAP


def _sig(f):
    return str(inspect.signature(f)).replace("typing.", "").replace("torch.Tensor", "Tensor")


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _rand(shape, dtype, seed, mul=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * mul).to(dtype)


# ---- surface --------------------------------------------------------------------------------------------------------------------------------
def test_exports_and_literal_signatures():
    for name in ("fp8_attn_splitkv_window_func", "fp8_attn_paged_window_func", "fp8_attn_paged_varlen_window_func", "paged_window_dead_pages"):
        assert getattr(qa, name) is getattr(splitkv_window, name) and name not in qa.__all__
    assert _sig(qa.fp8_attn_splitkv_window_func) == (
        "(q, kv, window_size, *, scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, num_splits: int = 0, "
        "precision: str = 'accurate', return_lse: bool = False, return_partials: bool = False)")
    assert _sig(qa.fp8_attn_paged_window_func) == (
        "(q, cache: quantumattention_amd.paged.PagedKVCacheFP8, window_size, *, scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, "
        "max_seqlen_k: Optional[int] = None, num_splits: int = 0, precision: str = 'accurate', return_lse: bool = False, "
        "return_partials: bool = False)")
    assert _sig(qa.fp8_attn_paged_varlen_window_func) == (
        "(q, cache: quantumattention_amd.paged.PagedKVCacheFP8, cu_seqlens_q: Tensor, max_seqlen_q: int, window_size, *, "
        "scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, num_splits: int = 0, "
        "precision: str = 'accurate', return_lse: bool = False, return_partials: bool = False)")
    assert _sig(qa.paged_window_dead_pages) == "(seqlens: Tensor, window_left: int, page_size: int, *, num_queries: int = 1) -> Tensor"
    assert _sig(splitkv.split_plan_window) == "(L: int, Sq: int, window_left: int, num_splits: int)"
    for op in ("fp8_splitkv_window_attention_forward", "fp8_paged_splitkv_window_attention_forward",
               "fp8_paged_varlen_splitkv_window_attention_forward"):
        assert hasattr(qa.ops, op) and hasattr(torch.ops.quantumattention_amd, op)
    for name in ("qattn_splitkv_window_auto_splits", "qattn_paged_varlen_window_auto_splits", "qattn_fp8_attention_splitkv_window_forward",
                 "qattn_fp8_attention_paged_splitkv_window_forward", "qattn_fp8_attention_paged_varlen_window_forward"):
        assert name in _native.EXPORTS and hasattr(_native.lib(), name)
    assert _native.ABI_VERSION == 8 == _native.lib().qattn_abi_version()


def test_the_released_signatures_are_unchanged():
    assert _sig(qa.fp8_attn_splitkv_func) == (
        "(q, kv, *, causal: bool = False, scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, num_splits: int = 0, "
        "precision: str = 'accurate', return_lse: bool = False, return_partials: bool = False)")
    assert _sig(qa.fp8_attn_paged_func) == (
        "(q, cache: quantumattention_amd.paged.PagedKVCacheFP8, *, causal: bool = False, scale: Optional[float] = None, "
        "seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, num_splits: int = 0, precision: str = 'accurate', "
        "return_lse: bool = False, return_partials: bool = False)")
    assert _sig(qa.fp8_attn_paged_varlen_func) == (
        "(q, cache: quantumattention_amd.paged.PagedKVCacheFP8, cu_seqlens_q: Tensor, max_seqlen_q: int, *, causal: bool = False, "
        "scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, num_splits: int = 0, "
        "precision: str = 'accurate', return_lse: bool = False, return_partials: bool = False)")
    assert _sig(splitkv.split_plan) == "(L: int, num_splits: int)"
    # the eager definition's new argument is optional and last
    assert list(inspect.signature(splitkv._splitkv_eager).parameters)[-1] == "window"
    assert inspect.signature(splitkv._splitkv_eager).parameters["window"].default is None


# ---- a small CPU problem for the three functions --------------------------------------------------------------------------------------------------
def _cpu_cache(t, D, dtype, fmt, seed, scale_k=0.02, scale_v=0.04):
    c = qa.alloc_paged_kv_cache_fp8(t.num_pages, HKV, t.page_size, D, batch_size=B, max_pages_per_seq=t.M, scale_k=scale_k, scale_v=scale_v,
                                    dtype=dtype, device="cpu", fp8_format=fmt)
    rk, rv = P.random_rows(t.num_pages, t.page_size, D, fmt, seed)
    c.k.view(torch.uint8).copy_(rk)
    c.v.view(torch.uint8).copy_(rv)
    c.block_table.copy_(torch.from_numpy(t.table))
    c.seqlens.copy_(torch.tensor(t.lens, dtype=torch.int32))
    return c


def _small():
    t = P.shared_tables(64)[1]
    c = _cpu_cache(t, 64, torch.bfloat16, "e4m3", 3)
    return t, c, _rand((B, 4, 3, 64), torch.bfloat16, 4), _rand((9, 4, 64), torch.bfloat16, 5), torch.tensor([0, 3, 6, 9], dtype=torch.int32)


BAD_WINDOWS = [None, 5, (1,), (1, 2, 3), (1.0, 0), (True, 0), (0, False), (-2, 0), (0, -2), ("1", 0), (torch.tensor(1), 0)]


@pytest.mark.parametrize("bad", BAD_WINDOWS, ids=[repr(b) for b in BAD_WINDOWS])
def test_a_window_that_is_no_pair_of_ints_from_minus_one_up_is_refused_by_all_three(bad):
    t, c, q, qp, cu = _small()
    kv = qa.prepare_kv_fp8(_rand((B, HKV, 70, 64), torch.bfloat16, 6), _rand((B, HKV, 70, 64), torch.bfloat16, 7))
    with pytest.raises(ValueError, match="window_size"):
        qa.fp8_attn_splitkv_window_func(q, kv, bad)
    with pytest.raises(ValueError, match="window_size"):
        qa.fp8_attn_paged_window_func(q, c, bad)
    with pytest.raises(ValueError, match="window_size"):
        qa.fp8_attn_paged_varlen_window_func(qp, c, cu, 3, bad)


def test_every_other_value_error():
    t, c, q, qp, cu = _small()
    k16, v16 = _rand((B, HKV, 70, 64), torch.bfloat16, 6), _rand((B, HKV, 70, 64), torch.bfloat16, 7)
    kv = qa.prepare_kv_fp8(k16, v16)
    calls = {
        "contig": lambda **kw: qa.fp8_attn_splitkv_window_func(kw.pop("q", q), kw.pop("kv", kv), (8, 0), **kw),
        "paged": lambda **kw: qa.fp8_attn_paged_window_func(kw.pop("q", q), kw.pop("kv", c), (8, 0), **kw),
        "packed": lambda **kw: qa.fp8_attn_paged_varlen_window_func(kw.pop("q", qp), kw.pop("kv", c), kw.pop("cu", cu), kw.pop("mq", 3), (8, 0), **kw),
    }
    for name, call in calls.items():
        call()                                                     # (the arguments are fine as they stand)
        for prec in ("auto", "exact", None):
            with pytest.raises(ValueError, match="precision"):
                call(precision=prec)
        for ns in (-1, 65, True, 2.0):
            with pytest.raises(ValueError, match="num_splits"):
                call(num_splits=ns)
        for sc in (0, -1.0, math.nan, math.inf, True):
            with pytest.raises(ValueError, match="scale"):
                call(scale=sc)
        with pytest.raises(ValueError, match="seqused_k"):
            call(seqused_k=torch.zeros(B, dtype=torch.int64))
        with pytest.raises(ValueError, match="seqused_k"):
            call(seqused_k=torch.zeros(B + 1, dtype=torch.int32))
        with pytest.raises(ValueError, match="dtype"):
            call(q=(q if name != "packed" else qp).to(torch.float16))
        with pytest.raises(ValueError, match="dtype"):
            call(q=(q if name != "packed" else qp).float())
        with pytest.raises(ValueError):
            call(q=(q if name != "packed" else qp)[..., :32])
    with pytest.raises(ValueError, match="PreparedKV"):
        calls["contig"](kv=(k16,))
    with pytest.raises(ValueError, match="PreparedKV"):
        calls["contig"](kv=c)
    with pytest.raises(ValueError, match="4-D"):
        calls["contig"](q=qp)
    with pytest.raises(ValueError, match="batch"):
        calls["contig"](q=q[:2])
    with pytest.raises(ValueError, match="4-D"):
        calls["paged"](q=qp)
    with pytest.raises(ValueError, match="max_seqlen_k"):
        calls["paged"](max_seqlen_k=CAP + 1)
    with pytest.raises(ValueError, match="3-D"):
        calls["packed"](q=q)
    with pytest.raises(ValueError, match="cu_seqlens_q"):
        calls["packed"](cu=cu.long())
    with pytest.raises(ValueError, match="cu_seqlens_q"):
        calls["packed"](cu=cu[:3])
    with pytest.raises(ValueError, match="max_seqlen_q"):
        calls["packed"](mq=0)
    with pytest.raises(ValueError, match="max_seqlen_k"):
        calls["packed"](max_seqlen_k=0)
    # a (k, v) pair is prepared inside the call: the bits of the PreparedKV call
    assert _same_bits(calls["contig"](kv=(k16, v16)), calls["contig"]())
    # the dead-page function's own arguments
    sl = torch.tensor([5, 700], dtype=torch.int32)
    for bad in (dict(seqlens=sl.long()), dict(seqlens=sl[None]), dict(seqlens=[5, 700]), dict(window_left=-1), dict(window_left=1.0),
                dict(window_left=True), dict(page_size=0), dict(page_size=64.0), dict(num_queries=0), dict(num_queries=True)):
        args = dict(seqlens=sl, window_left=63, page_size=64, num_queries=1)
        args.update(bad)
        with pytest.raises(ValueError):
            qa.paged_window_dead_pages(args["seqlens"], args["window_left"], args["page_size"], num_queries=args["num_queries"])


# ---- the plan and the rules --------------------------------------------------------------------------------------------------------------------------
def test_split_plan_window_is_the_literal_rule_and_the_old_plan_without_a_left_edge():
    for L in (0, 1, 63, 64, 127, 128, 129, 300, 1100, 1280, 32768):
        for Sq in (1, 5, 40, 130, 2000):
            for ns in (1, 2, 3, 9, 64):
                assert splitkv.split_plan_window(L, Sq, -1, ns) == splitkv.split_plan(L, ns) == W.plan_without_window(L, ns) == W.plan(L, Sq, -1, ns)
                for left in (0, 1, 63, 64, 127, 128, 200, 1050, 4095, 1 << 30):
                    got = splitkv.split_plan_window(L, Sq, left, ns)
                    assert got == W.plan(L, Sq, left, ns), (L, Sq, left, ns)
                    lo = W.interval_lo(L, Sq, left)
                    # the splits tile [128 (lo // 128), L) in order, each a whole number of blocks but the last
                    assert got[0][0] == min(128 * (lo // 128), L) and got[-1][1] == L
                    assert all(a[1] == b[0] for a, b in zip(got, got[1:])) and all((hi - lo_) % 128 == 0 or hi == L for lo_, hi in got)
    # the point of it: a 4096-key window over 32768 keys leaves no split empty (over [0, L) 7 of 8 would be)
    plan = splitkv.split_plan_window(32768, 1, 4095, 8)
    assert all(hi > lo for lo, hi in plan) and plan[0][0] == 28672 and len({hi - lo for lo, hi in plan}) == 1
    old = splitkv.split_plan(32768, 8)
    assert sum(hi <= 32768 - 4096 for lo, hi in old) == 7


def test_auto_split_rules_are_the_old_rules_without_a_left_edge_and_monotone_in_it():
    dense, packed = _native.splitkv_auto_splits, _native.paged_varlen_auto_splits
    wd, wp = _native.splitkv_window_auto_splits, _native.paged_varlen_window_auto_splits
    lefts = (0, 1, 63, 127, 128, 1023, 4095, 8191, 100000, (1 << 31) - 1)
    for D in (64, 128, 256):
        for cus in (1, 104, 256, 304):
            for Bn in (1, 4, 32):
                for Hq, Hkv in ((8, 8), (32, 8)):
                    for Sq in (1, 5, 128):
                        for Skv in (1, 1100, 8192, 32768, 131072):
                            what = (D, cus, Bn, Hq, Hkv, Sq, Skv)
                            assert wd(Bn, Hq, Hkv, Sq, Skv, D, -1, cus) == dense(Bn, Hq, Hkv, Sq, Skv, D, cus), what
                            assert wp(Bn, Hq, Hkv, Bn * Sq, Sq, Skv, D, -1, cus) == packed(Bn, Hq, Hkv, Bn * Sq, Sq, Skv, D, cus), what
                            prev_d = prev_p = 1
                            for left in lefts:
                                d, p = wd(Bn, Hq, Hkv, Sq, Skv, D, left, cus), wp(Bn, Hq, Hkv, Bn * Sq, Sq, Skv, D, left, cus)
                                assert d == dense(Bn, Hq, Hkv, Sq, W.window_keys(Skv, Sq, left), D, cus), what + (left,)
                                assert p == packed(Bn, Hq, Hkv, Bn * Sq, Sq, W.window_keys(Skv, Sq, left), D, cus), what + (left,)
                                assert d >= prev_d and p >= prev_p, what + (left,)
                                prev_d, prev_p = d, p
                            assert prev_d == dense(Bn, Hq, Hkv, Sq, Skv, D, cus)      # a window wider than the keys: the old rule
    assert wd(1, 32, 8, 1, 32768, 128, 4095, 256) < dense(1, 32, 8, 1, 32768, 128, 256)
    # invalid arguments: 1
    assert wd(0, 8, 8, 1, 1024, 128, 5, 256) == 1 and wd(1, 8, 8, 1, 1024, 128, -2, 256) == 1 and wd(1, 8, 8, 1, 8192, 96, 5, 256) == 1
    assert wp(1, 8, 8, 1, 0, 8192, 128, 5, 256) == 1 and wp(1, 8, 8, 1, 1, 8192, 128, -2, 256) == 1 and wp(1, 8, 8, 1, 1, 8192, 128, 5, 0) == 1


def test_dead_pages_is_the_formula_and_no_later_call_reads_a_dead_page():
    lens = [0, 1, 63, 64, 65, 127, 128, 129, 300, 1100, 1280, 32768]
    sl = torch.tensor(lens, dtype=torch.int32)
    for left in (0, 1, 63, 64, 200, 1050, 4095):
        for ps in (64, 128, 256):
            for nq in (1, 5, 40):
                got = qa.paged_window_dead_pages(sl, left, ps, num_queries=nq)
                assert got.dtype == torch.int32 and got.shape == sl.shape
                assert got.tolist() == [W.dead_pages(L, left, ps, nq) for L in lens] == [max(L - nq - left, 0) // ps for L in lens]
                # a call with Sq <= nq queries at this length or any later one starts at a page >= the dead count
                for L, dead in zip(lens, got.tolist()):
                    for later in (0, 1, nq, 500):
                        for Sq in {1, nq}:
                            assert W.interval_lo(L + later, Sq, left) // ps >= dead, (L, later, Sq, left, ps, nq)
    assert qa.paged_window_dead_pages(torch.tensor([2 ** 31 - 1], dtype=torch.int32), 0, 64).tolist() == [(2 ** 31 - 2) // 64]


def test_the_c_entries_refuse_a_window_below_minus_one_before_anything_else():
    L = _native.lib()
    INVALID = -1
    contig = lambda wl, wr: L.qattn_fp8_attention_splitkv_window_forward(4096, _native.FMT_BF16, 1 << 20, 2 << 20, 256, 512, 8192, None, None, 2, 4, 2, 1,
                                                                         256, 64, _native.FMT_E4M3, 0, wl, wr, 0.0, 1, 1, None, None, None, None, None,
                                                                         None, None, 0, None)
    paged = lambda wl, wr: L.qattn_fp8_attention_paged_splitkv_window_forward(4096, _native.FMT_BF16, 1 << 20, 2 << 20, 2048, 4, 8, 64, 4, 256, 512, 8192,
                                                                              None, 1024, 2, 4, 2, 1, 256, 64, _native.FMT_E4M3, 0, wl, wr, 0.0, 1, 1, None,
                                                                              None, None, None, None, None, None, 0, None)
    packed = lambda wl, wr: L.qattn_fp8_attention_paged_varlen_window_forward(4096, None, _native.FMT_BF16, 1 << 20, 2 << 20, 2048, 4, 8, 64, 4, 256, 512,
                                                                              8192, None, 3072, 1024, 2, 4, 2, 5, 4, 256, 64, _native.FMT_E4M3, 0, wl, wr,
                                                                              0.0, 1, 1, None, None, None, None, None, None, None, 0, None)
    workspace = L.qattn_fp8_attention_paged_splitkv_forward(4096, _native.FMT_BF16, 1 << 20, 2 << 20, 2048, 4, 8, 64, 4, 256, 512, 8192, None, 1024, 2, 4, 2,
                                                            1, 256, 64, _native.FMT_E4M3, 0, 0, 0.0, 1, 1, None, None, None, None, None, None, None, 0, None)
    assert workspace < 0 and workspace != INVALID
    for f in (contig, paged, packed):
        for ok in ((-1, -1), (-1, 0), (0, 0), (4095, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert f(*ok) == workspace, ok           # every argument check passed: the next one is the workspace's (the siblings' order)
        for bad in ((-2, 0), (0, -2), (-2 ** 31, 0)):
            assert f(*bad) == INVALID, bad


def test_the_fake_registrations_give_the_shapes_and_dtypes_of_the_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        u8, f32, i32 = torch.empty(16, dtype=torch.uint8), torch.empty(3, 2), torch.empty(4, dtype=torch.int32)
        ops = torch.ops.quantumattention_amd
        for ns, lse, parts in ((1, False, False), (1, True, True), (3, True, True), (9, False, True)):
            qd = torch.empty(3, 8, 5, 128, dtype=torch.float16)
            for res in (ops.fp8_splitkv_window_attention_forward(qd, u8, u8, f32, f32, i32[:3], 1280, ns, 200, 0, "e4m3", "compiled", "accurate", lse, parts),
                        ops.fp8_paged_splitkv_window_attention_forward(qd, u8, u8, f32, f32, i32.view(1, 4).expand(3, 4), i32[:3], 1280, 20, 64, ns, 200, 0,
                                                                       "e4m3", "compiled", "fast", lse, parts)):
                out, l, po, pl, pp = res
                assert out.shape == (3, 8, 5, 128) and out.dtype == torch.float16 and l.shape == ((3, 8, 5) if lse else (0,))
                assert l.dtype == pl.dtype == po.dtype == torch.float32 and pp.dtype == torch.uint8
                if parts and ns > 1:
                    assert po.shape == (ns, 3, 8, 5, 128) and pl.shape == pp.shape == (ns, 3, 8, 5)
                else:
                    assert po.numel() == pl.numel() == pp.numel() == 0
            qp = torch.empty(39, 8, 128, dtype=torch.bfloat16)
            out, l, po, pl, pp = ops.fp8_paged_varlen_splitkv_window_attention_forward(qp, u8, u8, f32, f32, i32.view(1, 4).expand(3, 4), i32[:3], i32, 33, 1280,
                                                                                       20, 64, ns, 200, 0, "e4m3", "compiled", "accurate", lse, parts)
            assert out.shape == (39, 8, 128) and out.dtype == torch.bfloat16 and l.shape == ((8, 39) if lse else (0,))
            if parts and ns > 1:
                assert po.shape == (ns, 39, 8, 128) and pl.shape == pp.shape == (ns, 8, 39) and pp.dtype == torch.uint8
            else:
                assert po.numel() == pl.numel() == pp.numel() == 0


# ---- the eager definitions ---------------------------------------------------------------------------------------------------------------------------
def _deq(x8, scale):
    return x8.float().double().numpy() * scale.double().numpy()[..., None, None]


EAGER_WINDOWS = [(0, 0), (63, 0), (64, 0), (200, 0), (1050, 0), (1024, 37), (-1, 0), (300, -1), (-1, -1), (5, 1100)]


@pytest.mark.parametrize("G,Sq", [(4, 5), (4, 40), (1, 130), (2, 1)])
def test_the_eager_definition_is_the_fp64_reference_that_walks_kv_head_tile_and_split(G, Sq):
    """out, lse, the partials and the PATH BYTES of `_splitkv_eager(window=)` against tests/splitkv_window_cases.reference on the same
    de-quantised operands: fp32 softmax against fp64 (1e-5 on the fp32 partials and LSEs, one output ulp on out)"""
    D, dtype, Skv = 64, torch.bfloat16, 1280
    k16, v16 = _rand((2, HKV, Skv, D), dtype, 11, mul=1.5), _rand((2, HKV, Skv, D), dtype, 12)
    kv = qa.prepare_kv_fp8(k16, v16)
    q = _rand((2, HKV * G, Sq, D), dtype, 13 + Sq, mul=1.5)
    fp8 = _native.fp8_dtype_of(kv.fp8_format)
    q8, sq = qa.nn._dynamically_quantize_fp8(q, reduction_dim=[2, 3], fp8_dtype=fp8)
    dq, dk, dv = _deq(q8, sq), _deq(kv.k, kv.scale_k), _deq(kv.v, kv.scale_v)
    used = [1100, 300]
    su = torch.tensor(used, dtype=torch.int32)
    sm = 1.0 / math.sqrt(D)
    for window in EAGER_WINDOWS:
        for ns in (1, 3):
            for precision in ("accurate", "fast"):
                out, lse, po, plse, ppath = qa.fp8_attn_splitkv_window_func(q, kv, window, seqused_k=su, num_splits=ns, precision=precision,
                                                                            return_lse=True, return_partials=True)
                for b, L in enumerate(used):
                    ro, rl, rpo, rpl, rpp, _ = W.reference(dq[b], dk[b], dv[b], L, window, ns, sm, precision)
                    what = (G, Sq, L, window, ns, precision)
                    o = out[b].float().numpy()
                    assert np.all(np.abs(o - ro) <= 2.0 ** -8 * np.abs(ro) + 1e-5), what
                    assert np.array_equal(np.isneginf(lse[b].numpy()), np.isneginf(rl)), what
                    live = ~np.isneginf(rl)
                    assert np.all(np.abs(lse[b].numpy()[live] - rl[live]) <= 1e-4), what
                    assert (o[~live] == 0).all(), what
                    if ns > 1:
                        assert np.all(np.abs(po[:, b].numpy() - rpo) <= 1e-4), what
                        assert np.array_equal(np.isneginf(plse[:, b].numpy()), np.isneginf(rpl)), what
                        plive = ~np.isneginf(rpl)
                        assert np.all(np.abs(plse[:, b].numpy()[plive] - rpl[plive]) <= 1e-4), what
                        assert np.array_equal(ppath[:, b].numpy(), rpp), what
                    else:
                        assert po.numel() == plse.numel() == ppath.numel() == 0
    # (-1, 0) and (-1, -1) are the siblings, bit for bit; the released default path is untouched by the new argument
    for ns in (1, 3):
        for causal, window in ((True, (-1, 0)), (False, (-1, -1))):
            a = qa.fp8_attn_splitkv_window_func(q, kv, window, seqused_k=su, num_splits=ns, precision="fast", return_lse=True, return_partials=True)
            b = qa.fp8_attn_splitkv_func(q, kv, causal=causal, seqused_k=su, num_splits=ns, precision="fast", return_lse=True, return_partials=True)
            assert all(_same_bits(x, y) for x, y in zip(a, b)), (ns, window)


def test_fast_reaches_the_one_term_path_byte_only_where_a_workgroup_sweeps_1024_keys():
    D, dtype = 64, torch.bfloat16
    kv = qa.prepare_kv_fp8(_rand((1, HKV, 1280, D), dtype, 21), _rand((1, HKV, 1280, D), dtype, 22))
    q = _rand((1, HKV * 4, 8, D), dtype, 23)
    paths = lambda window, ns: qa.fp8_attn_splitkv_window_func(q, kv, window, num_splits=ns, precision="fast", return_partials=True)[3]
    assert (paths((1100, 0), 2)[0] == W.PATH_TWO_TERM).all()                 # 1108 keys in two splits of 640
    # one split: the partials are empty; the rule shows in the reference's row_path
    ref = W.reference(np.zeros((8, 8, D)), np.zeros((HKV, 1280, D)), np.zeros((HKV, 1280, D)), 1280, (1100, 0), 1, 1.0, "fast")
    assert (ref[5] == W.PATH_ONE_TERM).all()
    ref = W.reference(np.zeros((8, 8, D)), np.zeros((HKV, 1280, D)), np.zeros((HKV, 1280, D)), 1280, (1000, 0), 1, 1.0, "fast")
    assert (ref[5] == W.PATH_TWO_TERM).all()                                  # 1008 keys


@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
def test_eager_paged_is_the_contiguous_entry_on_the_gathered_cache_and_packed_is_paged_on_each_slot_alone(page_size):
    D, dtype, fmt = 64, torch.bfloat16, "e4m3"
    for i, t in enumerate(P.shared_tables(page_size)):
        G, sq = V.qcase(page_size, i)
        c = _cpu_cache(t, D, dtype, fmt, 3 * page_size + i)
        cu, total = V.cu_of(sq), sum(sq)
        qp = _rand((total, HKV * G, D), dtype, 5 + i, mul=1.5)
        cud = torch.tensor(cu, dtype=torch.int32)
        window = W.PROBE_WINDOWS[(i + page_size // 64) % len(W.PROBE_WINDOWS)]
        for ns in (1, 3):
            kw = dict(num_splits=ns, precision="fast", return_lse=True, return_partials=True)
            out, lse, po, plse, ppath = qa.fp8_attn_paged_varlen_window_func(qp, c, cud, max(sq), window, **kw)
            assert out.shape == (total, HKV * G, D) and lse.shape == (HKV * G, total)
            for b in range(B):
                if sq[b] == 0:
                    continue
                want = qa.fp8_attn_paged_window_func(V.alone(qp, cu, b), V.one_slot(c, b), window, **kw)
                assert _same_bits(V.rows_of(out, "o", cu, b), want[0]) and _same_bits(V.rows_of(lse, "l", cu, b), want[1]), (t.lens, sq, b, ns, window)
                if ns > 1:
                    assert _same_bits(V.rows_of(po, "po", cu, b), want[2]) and _same_bits(V.rows_of(plse, "pl", cu, b), want[3])
                    assert _same_bits(V.rows_of(ppath, "pl", cu, b), want[4])
            qd = _rand((B, HKV * G, 3, D), dtype, 9 + i)
            got = qa.fp8_attn_paged_window_func(qd, c, window, **kw)
            ref = qa.fp8_attn_splitkv_window_func(qd, qa.paged.gather_paged_eager(c), window, seqused_k=c.seqlens, **kw)
            assert all(_same_bits(x, y) for x, y in zip(got, ref)), (t.lens, ns, window)


# ---- teeth: the membership probes of the GPU tests ------------------------------------------------------------------------------------------------------------
def test_the_probe_shapes_are_the_ones_the_issue_names():
    assert W.PROBE_LQ == [1, 5, 40, 130] and W.PROBE_LK == [1100, 1280, 65, 300] and (W.PROBE_HQ, W.PROBE_HKV) == (4, 2)
    assert W.PROBE_WINDOWS == [(0, 0), (63, 0), (64, 0), (200, 0), (1050, 0), (1024, 37), (-1, 0), (300, -1)]
    assert W.LSE_TOL == PR.LSE_TOL == 2e-3 and PR.TEETH == 4.0
    # the literal mask of this file's rules is the probes' own band mask
    for window in W.PROBE_WINDOWS:
        for n, m in zip(W.PROBE_LQ, W.PROBE_LK):
            lo, hi = PR.band_edges(n, m, "window", window)
            assert np.array_equal(W.alive(n, m, window, PR.pad64(m) + 2), PR.band_mask(lo, hi, m, PR.pad64(m) + 2)), (window, n, m)


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("window", W.PROBE_WINDOWS, ids=[f"w{a}_{b}" for a, b in W.PROBE_WINDOWS])
def test_every_mutant_of_the_probes_has_teeth_on_the_inputs_the_gpu_tests_use(D, window):
    """band (both edges off by one either way, the padding admitted), a dropped chunk, an extra column, the decoy admitted, the pointed key
    or its chunk dropped, another kv head read: each moves some element of every row it touches by >= TEETH x that element's bound"""
    res = {}
    case = W.probe_case("count", D, window)
    for i, (seq, mut) in enumerate(zip(case.seqs, case.mutants)):
        for name, t in PR.count_teeth(seq, mut, PR_DTYPE[D], lse_tol=W.LSE_TOL).items():
            res[f"count seq {i} {name}"] = t
    case = W.probe_case("decoy", D, window)
    for i, (seq, aux) in enumerate(zip(case.seqs, case.aux)):
        if (aux >= 0).any():
            res[f"decoy seq {i}"] = PR.decoy_teeth(seq, aux, v16=False)["decoy admitted"]
    case = W.probe_case("pointer", D, window)
    for i, (seq, aux) in enumerate(zip(case.seqs, case.aux)):
        if (aux >= 0).any():
            other = {"the other kv head": (seq.k[::-1].copy(), seq.v[::-1].copy())}
            for name, t in PR.pointer_teeth(seq, aux, v16=False, other_kv=other).items():
                res[f"pointer seq {i} {name}"] = t
    assert res and all(t >= PR.TEETH for t in res.values()), {k: v for k, v in res.items() if v < PR.TEETH}


PR_DTYPE = PR.WINDOW_COUNT_DTYPE


@pytest.mark.parametrize("D", [64, 128, 256])
def test_the_window_specific_mutants_move_a_row_of_the_probes_by_four_times_the_fp8_v_bound(D):
    """delta taken top-left, the plan cut from key 0 with the interval's block count, the tile's klo as every row's lower edge, the first
    chunk dropped when lo is no multiple of 64 (tests/splitkv_window_cases.wrong_masks; the lower edge off by one either way is the band
    mutant lo-1 / lo+1 of the test above): on the decoy and pointer probes of the GPU tests each moves some row by >= 4x the fp8-V bound
    2^-6 max(1, |ref| / 2) of tests/gpu_utils.py -- over the windows and sequences, every mutant at least once, with three splits"""
    G = W.PROBE_HQ // W.PROBE_HKV
    worst = {}
    for window in W.PROBE_WINDOWS:
        for probe in ("decoy", "pointer"):
            case = W.probe_case(probe, D, window)
            for seq, n, m in zip(case.seqs, W.PROBE_LQ, W.PROBE_LK):
                M = seq.k.shape[1]
                ref, _ = seq.softmax()
                bound = PR.project_bound(ref, False)
                for name, mm in W.wrong_masks(n, m, G, window, 3, M).items():
                    full = np.concatenate([mm] * W.PROBE_HKV, 0)              # [Hq, n, M]: the same rule for every kv head's G heads
                    mut, _ = seq.softmax(full)
                    worst[name] = max(worst.get(name, 0.0), float((np.abs(mut - ref) / bound).max()))
    assert set(worst) == {"delta top-left", "plan from key 0 with the interval's block count", "the tile's klo as every row's lower edge",
                          "first chunk dropped"}, worst
    assert all(v >= PR.TEETH for v in worst.values()), worst

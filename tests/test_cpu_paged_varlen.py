"""Packed variable-length queries over the paged FP8 K/V cache without a GPU (quantumattention_amd/paged_varlen.py,
include/qattn_paged_varlen.h): the surface, the eager definition against fp8_attn_paged_func on each sequence alone, the num_splits = 0
rule, the C entry's argument checks, the reason function, the fake registration -- and the teeth of the shared cases
(tests/paged_varlen_cases.py): what a wrong use of the packed addressing does to the outputs."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, paged_varlen
from tests import paged_cases as P
from tests import paged_varlen_cases as V

B, HKV, CAP = P.B, P.HKV, P.CAP


def _cache(t, D, dtype, fmt, seed, scale_k=0.02, scale_v=0.04, level=False):
    """a CPU (row-major) paged cache on one of the shared tables, finite random bytes everywhere (the eager definition multiplies masked
    keys' V by P = 0, and 0 x NaN is NaN).  level: every page's V carries its own level, as tests/test_cpu_paged.py's teeth test."""
    c = qa.alloc_paged_kv_cache_fp8(t.num_pages, HKV, t.page_size, D, batch_size=B, max_pages_per_seq=t.M, scale_k=scale_k, scale_v=scale_v,
                                    dtype=dtype, device="cpu", fp8_format=fmt)
    rk, rv = P.random_rows(t.num_pages, t.page_size, D, fmt, seed)
    if level:
        fp8 = P.FP8[fmt]
        lv = ((torch.arange(t.num_pages) * 7) % t.num_pages - t.num_pages // 2).float()
        rv = (lv[:, None, None, None] + rv.view(fp8).float()).to(fp8).view(torch.uint8)
    c.k.view(torch.uint8).copy_(rk)
    c.v.view(torch.uint8).copy_(rv)
    c.block_table.copy_(torch.from_numpy(t.table))
    c.seqlens.copy_(torch.tensor(t.lens, dtype=torch.int32))
    return c


def _q(total, Hq, D, dtype, seed, mul=1.5):
    return (torch.randn(total, Hq, D, generator=torch.Generator().manual_seed(seed)) * mul).to(dtype)


def _cu(sq):
    return torch.tensor(V.cu_of(sq), dtype=torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- surface ------------------------------------------------------------------------------------------------------------------------------
def test_exports_and_signature():
    assert qa.fp8_attn_paged_varlen_func is paged_varlen.fp8_attn_paged_varlen_func and "fp8_attn_paged_varlen_func" not in qa.__all__
    assert hasattr(qa.ops, "fp8_paged_varlen_splitkv_attention_forward")
    sig = str(inspect.signature(qa.fp8_attn_paged_varlen_func)).replace("typing.", "").replace("torch.Tensor", "Tensor")
    assert sig == ("(q, cache: quantumattention_amd.paged.PagedKVCacheFP8, cu_seqlens_q: Tensor, max_seqlen_q: int, *, causal: bool = False, "
                   "scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, num_splits: int = 0, "
                   "precision: str = 'accurate', return_lse: bool = False, return_partials: bool = False)")
    for name in ("qattn_fp8_attention_paged_varlen_workspace_bytes", "qattn_paged_varlen_auto_splits", "qattn_fp8_attention_paged_varlen_forward"):
        assert name in _native.EXPORTS and hasattr(_native.lib(), name)
    assert _native.ABI_VERSION == 8 == _native.lib().qattn_abi_version()
    # the dense function keeps its signature: the packed one is a sibling
    assert "cu_seqlens_q" not in str(inspect.signature(qa.fp8_attn_paged_func))


def test_the_shared_cases_have_the_properties_the_gpu_tests_rely_on():
    V.check_rotation()
    assert [g * sum(s) for g, s in V.QCASES] == [164, 131, 156, 9]
    # pair 0: two tiles of sequence 1, the first crossing head boundaries (rows 0 .. 127 of 4 x 40); pair 2: sequence 2 has two tiles
    cu = V.cu_of(V.QCASES[0][1])
    hits = [V.slot_to_tile(j, cu, 4, 41) for j in range(V.num_slots(4, 41))]
    assert hits == [(0, 0), (1, 0), (1, 1), None, None]          # B + ceil(164 / 128) = 5 slots, two of them no tile
    cu = V.cu_of(V.QCASES[1][1])
    assert [V.slot_to_tile(j, cu, 1, 131) for j in range(V.num_slots(1, 131))] == [(0, 0), (0, 1), None, (2, 0), None]
    cu = V.cu_of(V.QCASES[2][1])
    assert [V.slot_to_tile(j, cu, 4, 39) for j in range(V.num_slots(4, 39))] == [(0, 0), (1, 0), (2, 0), (2, 1), None]
    # every tile of every sequence is reached exactly once
    for G, sq in V.QCASES:
        cu, total = V.cu_of(sq), sum(sq)
        hits = [h for h in (V.slot_to_tile(j, cu, G, total) for j in range(V.num_slots(G, total))) if h]
        assert sorted(hits) == sorted((b, t) for b in range(B) for t in range(-(-G * sq[b] // V.TILE)))


# ---- the eager definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
def test_eager_rows_of_a_sequence_are_the_bits_of_the_dense_paged_call_on_that_sequence_alone(page_size):
    D, dtype, fmt = 64, torch.bfloat16, "e4m3"
    for i, t in enumerate(P.shared_tables(page_size)):
        G, sq = V.qcase(page_size, i)
        c = _cache(t, D, dtype, fmt, 3 * page_size + i)
        cu, total = V.cu_of(sq), sum(sq)
        q = _q(total, HKV * G, D, dtype, 5 + i)
        for ns in (1, 3):
            for causal in (False, True):
                kw = dict(causal=causal, num_splits=ns, return_lse=True, return_partials=True)
                out, lse, po, plse, ppath = qa.fp8_attn_paged_varlen_func(q, c, _cu(sq), max(sq), **kw)
                assert out.shape == (total, HKV * G, D) and out.dtype == dtype and lse.shape == (HKV * G, total) and lse.dtype == torch.float32
                if ns == 1:
                    assert po.numel() == plse.numel() == ppath.numel() == 0
                else:
                    assert po.shape == (ns, total, HKV * G, D) and plse.shape == ppath.shape == (ns, HKV * G, total) and ppath.dtype == torch.uint8
                for b in range(B):
                    if sq[b] == 0:
                        continue
                    want = qa.fp8_attn_paged_func(V.alone(q, cu, b), V.one_slot(c, b), **kw)
                    what = (t.lens, G, sq, b, ns, causal)
                    assert _same_bits(V.rows_of(out, "o", cu, b), want[0]) and _same_bits(V.rows_of(lse, "l", cu, b), want[1]), what
                    if ns > 1:
                        assert _same_bits(V.rows_of(po, "po", cu, b), want[2]) and _same_bits(V.rows_of(plse, "pl", cu, b), want[3]), what
                        assert _same_bits(V.rows_of(ppath, "pl", cu, b), want[4]), what
        # seqused_k and max_seqlen_k go through as in the dense call
        su = torch.tensor([min(L, 70) for L in t.lens], dtype=torch.int32)
        got = qa.fp8_attn_paged_varlen_func(q, c, _cu(sq), max(sq), causal=True, seqused_k=su, max_seqlen_k=128, num_splits=2)
        for b in range(B):
            if sq[b]:
                one = V.one_slot(c, b)
                want = qa.fp8_attn_paged_func(V.alone(q, cu, b), one, causal=True, seqused_k=su[b:b + 1], max_seqlen_k=128, num_splits=2)
                assert _same_bits(V.rows_of(got, "o", cu, b), want)


def test_idle_sequences_have_no_rows_and_no_query_gives_empty_tensors():
    t = P.shared_tables(64)[0]
    c = _cache(t, 64, torch.bfloat16, "e4m3", 1)
    # only the middle sequence has queries: its rows are the whole output
    q = _q(4, 4, 64, torch.bfloat16, 2)
    out = qa.fp8_attn_paged_varlen_func(q, c, _cu((0, 4, 0)), 4, causal=True, num_splits=2)
    assert _same_bits(out.transpose(0, 1)[None], qa.fp8_attn_paged_func(V.alone(q, [0, 0, 4, 4], 1), V.one_slot(c, 1), causal=True, num_splits=2))
    # a strided view (the q slice of a packed projection) is read as it is
    qkv = torch.zeros(4, 3, 4, 64, dtype=torch.bfloat16)
    qkv[:, 0] = q
    assert _same_bits(qa.fp8_attn_paged_varlen_func(qkv[:, 0], c, _cu((0, 4, 0)), 4, causal=True, num_splits=2), out)
    for ns in (0, 1, 3):
        res = qa.fp8_attn_paged_varlen_func(q[:0], c, _cu((0, 0, 0)), 1, num_splits=ns, return_lse=True, return_partials=True)
        assert res[0].shape == (0, 4, 64) and res[0].dtype == torch.bfloat16 and res[1].shape == (4, 0) and res[1].dtype == torch.float32
        assert all(x.numel() == 0 for x in res[2:]) and res[4].dtype == torch.uint8
    # tokens behind cu[B] (a padded token bucket) belong to nobody; the sequences' rows do not move
    padded = torch.cat([q, _q(3, 4, 64, torch.bfloat16, 9)])
    assert _same_bits(qa.fp8_attn_paged_varlen_func(padded, c, _cu((0, 4, 0)), 4, causal=True, num_splits=2)[:4], out)


# ---- the num_splits = 0 rule and the workspace ----------------------------------------------------------------------------------------------
def test_auto_splits_is_the_dense_rule_when_all_counts_are_equal_and_never_splits_more_than_one_sequence_would():
    rule, dense = _native.paged_varlen_auto_splits, _native.splitkv_auto_splits
    L = _native.lib()
    for D in (64, 128, 256):
        for cus in (1, 8, 104, 256, 304):
            for Bn in (1, 2, 4, 32):
                for Hq, Hkv in ((8, 8), (32, 8), (16, 1)):
                    for Sq in (1, 5, 33, 128, 512):
                        for Skv in (1, 1100, 8192, 32768, 131072):
                            assert rule(Bn, Hq, Hkv, Bn * Sq, Sq, Skv, D, cus) == dense(Bn, Hq, Hkv, Sq, Skv, D, cus), (D, cus, Bn, Hq, Hkv, Sq, Skv)
                    # a mixed step: never more splits than the longest sequence alone would get; a wider batch never gets more
                    for mx, total in ((512, 543), (33, 39), (8, 8 + Bn), (1, 1)):
                        for Skv in (8192, 32768):
                            got = rule(Bn, Hq, Hkv, total, mx, Skv, D, cus)
                            assert 1 <= got <= dense(1, Hq, Hkv, mx, Skv, D, cus), (D, cus, Bn, Hq, Hkv, mx, total, Skv)
    # the mixed step of the issue: one 512-query chunk beside 31 decodes -- the padded form would see 32 x the tiles
    assert rule(32, 32, 8, 543, 512, 8192, 128, 256) >= dense(32, 32, 8, 512, 8192, 128, 256)
    for bad in ((0, 8, 8, 4, 1, 256, 64, 256), (2, 0, 8, 4, 1, 256, 64, 256), (2, 8, 0, 4, 1, 256, 64, 256), (2, 8, 3, 4, 1, 256, 64, 256),
                (2, 8, 8, -1, 1, 256, 64, 256), (2, 8, 8, 0, 1, 256, 64, 256), (2, 8, 8, 4, 0, 256, 64, 256), (2, 8, 8, 4, 1, 0, 64, 256),
                (2, 8, 8, 4, 1, 256, 96, 256), (2, 8, 8, 4, 1, 256, 64, 0), (2, 32, 1, 1 << 27, 1, 256, 64, 256)):
        assert rule(*bad) == 1, bad
    # the Python resolution is that function on the CPU's stand-in CU count
    assert paged_varlen._resolve_varlen_splits(0, 4, 32, 8, 4, 1, 8192, 128, "cpu") == rule(4, 32, 8, 4, 1, 8192, 128, 256)
    assert paged_varlen._resolve_varlen_splits(5, 4, 32, 8, 4, 1, 8192, 128, "cpu") == 5
    ws = L.qattn_fp8_attention_paged_varlen_workspace_bytes
    for bad in ((0, 8, 8, 4, 256, 64, 1), (2, 0, 8, 4, 256, 64, 1), (2, 8, 3, 4, 256, 64, 1), (2, 8, 8, -1, 256, 64, 1), (2, 8, 8, 4, 0, 64, 1),
                (2, 8, 8, 4, 256, 96, 1), (2, 8, 8, 4, 256, 64, -1), (2, 8, 8, 4, 256, 64, 65), (2, 32, 1, 1 << 27, 256, 64, 1)):
        assert ws(*bad) == 0, bad
    sizes = [ws(3, 8, 2, 39, 1280, 128, ns) for ns in range(1, 65)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] > sizes[0] and sizes[8] > sizes[7]
    assert ws(3, 8, 2, 39, 1280, 128, 0) == sizes[9]          # 0: the most the rule can pick, ceil(1280 / 128) = 10 splits
    assert ws(3, 8, 2, 0, 1280, 128, 1) > 0                    # no query: still a valid call


# ---- the C entry's argument checks ----------------------------------------------------------------------------------------------------------
def test_the_c_entry_refuses_before_any_device_call():
    """the argument checks of include/qattn_paged_varlen.h; the pointers are never dereferenced on these paths"""
    L = _native.lib()
    INVALID, DIM, FMT = -1, -2, -3
    WORKSPACE = L.qattn_fp8_attention_paged_splitkv_forward(4096, _native.FMT_BF16, 1 << 20, 2 << 20, 2048, 4, 8, 64, 4, 256, 512, 8192, None, 1024, 2, 4,
                                                            2, 1, 256, 64, _native.FMT_E4M3, 0, 0, 0.0, 1, 1, None, None, None, None, None, None, None, 0,
                                                            None)
    assert WORKSPACE < 0 and WORKSPACE not in (INVALID, DIM, FMT)
    s2 = (ctypes.c_longlong * 2)(3 * 4 * 64, 64)
    ok = dict(q16=4096, qs=None, in_fmt=_native.FMT_BF16, kp=1 << 20, vp=2 << 20, table=2048, tstride=4, num_pages=8, page_size=64, max_pages=4, sk=256,
              sv=512, out=8192, lse=None, cu=3072, used=1024, B=2, Hq=4, Hkv=2, total_q=5, max_q=4, Skv=256, D=64, fp8_fmt=_native.FMT_E4M3, numerics=0,
              causal=0, sm=0.0, precision=1, ns=1, q8=None, sq=None, path=None, po=None, plse=None, ppath=None, ws=None, ws_bytes=0, stream=None)
    call = lambda **over: L.qattn_fp8_attention_paged_varlen_forward(*dict(ok, **over).values())
    assert call() == WORKSPACE and call(qs=s2) == WORKSPACE     # every argument check passed: the next one is the workspace's
    assert call(total_q=0) == 0                                  # no query: QATTN_OK, nothing launched, no workspace looked at
    for name in ("q16", "kp", "vp", "table", "sk", "sv", "out", "used", "cu"):
        assert call(**{name: None}) == INVALID, name
    for name in ("kp", "vp", "q16", "out"):
        assert call(**{name: ok[name] + 8}) == INVALID, name
    assert call(cu=3074) == INVALID and call(table=2050) == INVALID
    assert call(total_q=-1) == INVALID and call(max_q=0) == INVALID and call(max_q=-3) == INVALID
    for bad in ((-8, 64), (3 * 4 * 64, 60), (100, 64), (768, -64)):
        assert call(qs=(ctypes.c_longlong * 2)(*bad)) == INVALID, bad
    assert call(Hq=32, Hkv=1, total_q=1 << 27) == INVALID        # G total_q beyond 2^31 - 1
    assert call(Hkv=4, Hq=4, total_q=(1 << 31) - 1, ns=64) == INVALID   # the grid Hkv NT ns beyond 2^31 - 1
    for ps in (0, 32, 96, -64):
        assert call(page_size=ps) == INVALID, ps
    assert call(tstride=3) == INVALID and call(num_pages=0) == INVALID and call(max_pages=0) == INVALID
    assert call(Skv=257) == INVALID and call(Skv=0) == INVALID
    assert call(num_pages=1 << 30, page_size=256, Skv=256) == INVALID
    assert call(D=96) == DIM and call(Hq=3) == DIM and call(fp8_fmt=_native.FMT_BF16) == FMT and call(in_fmt=_native.FMT_E4M3) == FMT
    assert call(ns=65) == INVALID and call(ns=-1) == INVALID and call(ns=0, po=4096) == INVALID
    assert call(B=0) == INVALID and call(Hq=0) == INVALID and call(Hkv=0) == INVALID and call(Hq=65536 * 2, Hkv=2) == INVALID
    assert call(B=65536) == WORKSPACE                            # B enters the x dimension of the grids only
    assert call(numerics=7) == INVALID and call(precision=0) == INVALID
    # a workspace of the documented size minus one byte is refused; total_q = 0: QATTN_OK whatever the workspace's size, after the other checks
    need = L.qattn_fp8_attention_paged_varlen_workspace_bytes(2, 4, 2, 5, 256, 64, 1)
    assert call(ws=1 << 22, ws_bytes=need - 1) == WORKSPACE and call(ws=(1 << 22) + 8, ws_bytes=need) == INVALID
    need0 = L.qattn_fp8_attention_paged_varlen_workspace_bytes(2, 4, 2, 0, 256, 64, 1)
    assert call(total_q=0, ws=1 << 22, ws_bytes=need0) == 0 and call(total_q=0, max_q=0) == INVALID and call(total_q=0, cu=None) == INVALID


# ---- the reason function --------------------------------------------------------------------------------------------------------------------
BAD = ["q_4d", "grad", "q_f32", "cache", "dtype", "D", "heads", "Hq0", "rows_big", "q_inner", "q_stride", "q_offset", "q_device", "cu_none", "cu_dtype",
       "cu_shape", "cu_device", "cu_strided", "maxq_0", "maxq_float", "maxq_bool", "seqused_dtype", "seqused_shape", "max_0", "max_big", "max_bool", "splits",
       "splits_bool", "scale_0", "scale_nan", "table_dtype", "auto"]


@pytest.mark.parametrize("bad", BAD)
def test_the_function_refuses(bad):
    c = qa.alloc_paged_kv_cache_fp8(8, HKV, 64, 64, batch_size=B, max_pages_per_seq=4, scale_k=0.01, scale_v=0.02, dtype=torch.bfloat16, device="cpu")
    q = torch.randn(6, 4, 64).to(torch.bfloat16)
    cu, mx, kw = _cu((1, 2, 3)), 3, {}
    if bad == "q_4d":
        q = q[None]
    elif bad == "grad":
        q = q.float().requires_grad_().to(torch.bfloat16)
    elif bad == "q_f32":
        q = q.float()
    elif bad == "cache":
        c = qa.alloc_kv_cache_fp8(B, HKV, 256, 64, scale_k=1.0, scale_v=1.0, dtype=torch.bfloat16, device="cpu")
    elif bad == "dtype":
        q = q.half()
    elif bad == "D":
        q = torch.randn(6, 4, 128).to(torch.bfloat16)
    elif bad == "heads":
        q = q[:, :3]
    elif bad == "Hq0":
        q = q[:, :0]
    elif bad == "rows_big":
        q = torch.zeros(4, 64, dtype=torch.bfloat16).expand((1 << 31) // 2, 4, 64)     # G total_q = 2^31 on one row of memory
    elif bad == "q_inner":
        q = torch.randn(6, 64, 4).to(torch.bfloat16).transpose(1, 2)
    elif bad == "q_stride":
        q = torch.randn(6, 4, 68).to(torch.bfloat16)[:, :, :64]
    elif bad == "q_offset":
        q = torch.randn(6 * 4 * 64 + 4).to(torch.bfloat16)[4:].view(6, 4, 64)
    elif bad == "q_device":
        q = q.to("meta")                       # (another device than the cache's, without a GPU)
    elif bad == "cu_device":
        cu = cu.to("meta")
    elif bad == "cu_none":
        cu = None
    elif bad == "cu_dtype":
        cu = cu.long()
    elif bad == "cu_shape":
        cu = cu[:B]
    elif bad == "cu_strided":
        cu = torch.zeros(2 * (B + 1), dtype=torch.int32)[::2]
    elif bad == "maxq_0":
        mx = 0
    elif bad == "maxq_float":
        mx = 3.0
    elif bad == "maxq_bool":
        mx = True
    elif bad == "seqused_dtype":
        kw["seqused_k"] = torch.zeros(B)
    elif bad == "seqused_shape":
        kw["seqused_k"] = torch.zeros(B - 1, dtype=torch.int32)
    elif bad == "max_0":
        kw["max_seqlen_k"] = 0
    elif bad == "max_big":
        kw["max_seqlen_k"] = c.capacity + 1
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
        assert paged_varlen.paged_varlen_attn_input_reason(q, c, cu, mx, kw.get("seqused_k"), kw.get("scale"), kw.get("num_splits", 0),
                                                           kw.get("max_seqlen_k"))
    with pytest.raises(ValueError):
        qa.fp8_attn_paged_varlen_func(q, c, cu, mx, **kw)


def test_valid_arguments_have_no_reason():
    c = qa.alloc_paged_kv_cache_fp8(8, HKV, 64, 64, batch_size=B, max_pages_per_seq=4, scale_k=0.01, scale_v=0.02, dtype=torch.bfloat16, device="cpu")
    q = torch.randn(6, 3, 4, 64).to(torch.bfloat16)[:, 1]                    # a slice of a packed projection
    assert not q.is_contiguous()
    assert paged_varlen.paged_varlen_attn_input_reason(q, c, _cu((1, 2, 3)), 3, None, 0.5, 3, 128) is None
    assert paged_varlen.paged_varlen_attn_input_reason(q[:0], c, _cu((0, 0, 0)), 1) is None


# ---- the fake registration ------------------------------------------------------------------------------------------------------------------
def test_the_fake_registration_gives_the_shapes_and_dtypes_of_the_op():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        q = torch.empty(39, 8, 128, dtype=torch.float16)
        u8 = torch.empty(16, dtype=torch.uint8)
        f32 = torch.empty(3, 2)
        i32 = torch.empty(4, dtype=torch.int32)
        op = torch.ops.quantumattention_amd.fp8_paged_varlen_splitkv_attention_forward
        for ns, lse, parts in ((1, False, False), (1, True, True), (3, True, True), (9, False, True)):
            out, l, po, pl, pp = op(q, u8, u8, f32, f32, i32.view(1, 4).expand(3, 4), i32[:3], i32, 33, 1280, 20, 64, ns, "e4m3", "compiled", True,
                                    "accurate", lse, parts)
            assert out.shape == (39, 8, 128) and out.dtype == torch.float16
            assert l.dtype == pl.dtype == po.dtype == torch.float32 and pp.dtype == torch.uint8
            assert l.shape == ((8, 39) if lse else (0,))
            if parts and ns > 1:
                assert po.shape == (ns, 39, 8, 128) and pl.shape == pp.shape == (ns, 8, 39)
            else:
                assert po.numel() == pl.numel() == pp.numel() == 0


# ---- teeth: what a wrong use of the packed addressing does on the shared cases ---------------------------------------------------------------
def _teeth_case(t, page_size, i, D, dtype, fmt):
    """a shared table with its (G, counts) pair, made to discriminate: keys of order 1 and queries of order 2 .. 6 (a head's softmax is
    peaked on a few keys of its own), and V with a level of its own per KEY (page and slot), so that two heads of a sequence, two causal
    cuts of a row and two sequences give outputs that differ by whole levels.  Returns the eager output and the reference's inputs."""
    fp8 = P.FP8[fmt]
    G, sq = V.qcase(page_size, i)
    total, Hq = sum(sq), HKV * G
    c = _cache(t, D, dtype, fmt, 7 * page_size + i, scale_k=1.0, scale_v=0.5)
    lv = ((torch.arange(t.num_pages)[:, None] * 7 + torch.arange(page_size)[None, :] * 5) % 23 - 11).float()      # [page, slot]
    c.v.copy_((lv[:, None, :, None] + c.v.float()).to(fp8))
    q = (_q(total, Hq, D, dtype, 11 + i, mul=2.0).float() * (1 + torch.arange(Hq)[None, :, None] % 3)).to(dtype)
    got = qa.fp8_attn_paged_varlen_func(q, c, _cu(sq), max(sq), causal=True, num_splits=1).double().numpy()
    # the reference attends what the eager definition attends: its quantised q, de-quantised, and the gathered de-quantised cache
    cu = V.cu_of(sq)
    dq = np.zeros((total, Hq, D))
    for b in range(B):
        if sq[b]:
            x8, s8 = qa.nn._dynamically_quantize_fp8(V.alone(q, cu, b), reduction_dim=[2, 3], fp8_dtype=fp8)
            dq[cu[b]:cu[b + 1]] = (x8.double() * s8.double()[..., None, None])[0].transpose(0, 1).numpy()
    k, v = (P.gather_rows(r.view(torch.uint8).numpy(), t.table, page_size) for r in (c.k, c.v))
    dk = torch.from_numpy(k).view(fp8).double().numpy() * c.scale_k.double().numpy()[..., None, None]
    dv = torch.from_numpy(v).view(fp8).double().numpy() * c.scale_v.double().numpy()[..., None, None]
    return G, sq, got, dq, dk, dv


@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
def test_every_packing_mutant_moves_an_output_beyond_four_times_the_gpu_bound(page_size):
    """the fp64 per-row reference of tests/paged_varlen_cases.py, which walks (kv head, tile slot, row) as the kernel does, agrees with the
    product's eager definition; with the causal offset taken from max_seqlen_q, with the head of a packed row taken as r / max_seqlen_q,
    or with a tile's rows handed to the neighbouring sequence, some element THE MUTANT WRITES lies at least 4 x 2^-6 max(1, |ref| / 2) from
    the reference -- the bound the GPU tests grade with (tests/gpu_utils.py), times the factor of the membership probes.  Rows a mutant
    never writes are counted beside that, not as movement.  Which cases can see a mutant follows from the case alone:
      delta-max  a sequence with keys whose count lies below max_seqlen_q (its causal edge moves);
      head-max   the same, with G > 1 (with G = 1 every row is head 0 under either rule);
      neighbour  every case."""
    D, fmt, dtype = 64, "e4m3", torch.bfloat16
    for i, t in enumerate(P.shared_tables(page_size)):
        G, sq, got, dq, dk, dv = _teeth_case(t, page_size, i, D, dtype, fmt)
        ref = V.reference(dq, dk, dv, t.lens, sq, G, max(sq), 1.0 / np.sqrt(D))
        assert np.isfinite(ref).all(), "the work-item map reaches every row of every sequence"
        bound = 2.0 ** -6 * np.maximum(1.0, np.abs(ref) / 2)
        assert (np.abs(got - ref) < bound).all(), (t.lens, G, sq, float((np.abs(got - ref) / bound).max()))
        shorter = any(0 < n < max(sq) and L > 0 for n, L in zip(sq, t.lens))
        visible = {"delta-max": shorter, "head-max": shorter and G > 1, "neighbour": True}
        for mutant, want in visible.items():
            out = V.reference(dq, dk, dv, t.lens, sq, G, max(sq), 1.0 / np.sqrt(D), mutant=mutant)
            written = np.isfinite(out)
            worst = float((np.abs(out - ref)[written] / bound[written]).max())
            print(f"page {page_size} lens {t.lens} G {G} counts {sq} {mutant}: worst |moved| / bound on written elements {worst:.1f}, "
                  f"{int((~written).all(-1).sum())} rows never written")
            assert (worst >= 4.0) == want, (t.lens, G, sq, mutant, worst)
            if not want:
                assert worst == 0.0 and written.all(), (t.lens, G, sq, mutant, "a blind case is blind exactly")
        # head-max stacks the heads of a short sequence onto head 0: the other heads' rows are never written
        if visible["head-max"]:
            out = V.reference(dq, dk, dv, t.lens, sq, G, max(sq), 1.0 / np.sqrt(D), mutant="head-max")
            assert (~np.isfinite(out)).any()

"""The rotary embedding at the paged cache's positions without a GPU (quantumattention_amd/paged_varlen.py,
include/qattn_paged_varlen_rope.h): the surface, the ops' schemas and fake registrations, the reason function, the C entries' argument
checks, the eager definitions against THE RULE (whole pools and seqlens, byte for byte), the kernel's unit map as arithmetic, and a check
in fp64 that does not use apply_rope_eager, with its teeth: positions shifted by one break it in every row."""
import ctypes
import inspect

import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, paged, paged_varlen
from quantumattention_amd.paged import gather_paged_eager
from tests import paged_varlen_rope_cases as RC

HKV, CAP, T, COUNTS, STARTS, B = RC.HKV, RC.CAP, RC.T, RC.COUNTS, RC.STARTS, RC.B
TOTAL = sum(COUNTS)


def _cache(D, dtype, fmt, page_size, seed=0, spare=3, scale_k=0.02):
    """a CPU (row-major) cache of B slots of 256 keys: a shuffled table with spare pages, pools filled with the sentinel byte 0x5a"""
    M = CAP // page_size
    num_pages = B * M + spare
    c = qa.alloc_paged_kv_cache_fp8(num_pages, HKV, page_size, D, batch_size=B, max_pages_per_seq=M, scale_k=scale_k, scale_v=0.04, dtype=dtype,
                                    device="cpu", fp8_format=fmt)
    g = torch.Generator().manual_seed(seed)
    c.block_table.copy_(torch.randperm(num_pages, generator=g)[:B * M].view(B, M).to(torch.int32))
    c.k.view(torch.uint8).fill_(RC.SENTINEL)
    c.v.view(torch.uint8).fill_(RC.SENTINEL)
    c.seqlens.copy_(torch.tensor(STARTS, dtype=torch.int32))
    return c


def _clone(c):
    return paged.PagedKVCacheFP8(c.k.clone(), c.v.clone(), c.scale_k, c.scale_v, c.block_table.clone(), c.seqlens.clone(), c.shape, c.fp8_format,
                                 c.dtype, c.numerics, c.layout)


def _tokens(total, D, dtype, seed, mul=2.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(total, HKV, D, generator=g) * mul).to(dtype), (torch.randn(total, HKV, D, generator=g) * mul).to(dtype)


def _cu(counts=COUNTS):
    return torch.tensor(RC.cu_list(counts), dtype=torch.int32)


def _same_state(a, b):
    return (torch.equal(a.k.view(torch.uint8), b.k.view(torch.uint8)) and torch.equal(a.v.view(torch.uint8), b.v.view(torch.uint8))
            and torch.equal(a.seqlens, b.seqlens))


# ---- surface ------------------------------------------------------------------------------------------------------------------------------
def test_exports_and_pinned_signatures():
    assert qa.paged_kv_cache_append_varlen_rope_fp8 is paged_varlen.paged_kv_cache_append_varlen_rope_fp8
    assert qa.apply_rope_paged_varlen is paged_varlen.apply_rope_paged_varlen
    assert "paged_kv_cache_append_varlen_rope_fp8" not in qa.__all__ and "apply_rope_paged_varlen" not in qa.__all__ and len(qa.__all__) == 7
    sig = lambda f: str(inspect.signature(f)).replace("typing.", "").replace("torch.Tensor", "Tensor")
    assert sig(qa.paged_kv_cache_append_varlen_rope_fp8) == (
        "(cache: quantumattention_amd.paged.PagedKVCacheFP8, k_new: Tensor, v_new: Tensor, cu_seqlens: Tensor, cos: Tensor, sin: Tensor, *, "
        "interleaved: bool = False, advance: bool = True) -> quantumattention_amd.paged.PagedKVCacheFP8")
    assert sig(qa.apply_rope_paged_varlen) == (
        "(x: Tensor, cache: quantumattention_amd.paged.PagedKVCacheFP8, cu_seqlens: Tensor, cos: Tensor, sin: Tensor, *, "
        "interleaved: bool = False, appended: bool = False, out: Optional[Tensor] = None) -> Tensor")
    # the plain packed append keeps its signature
    assert sig(qa.paged_kv_cache_append_varlen_fp8) == (
        "(cache: quantumattention_amd.paged.PagedKVCacheFP8, k_new: Tensor, v_new: Tensor, cu_seqlens: Tensor, *, "
        "advance: bool = True) -> quantumattention_amd.paged.PagedKVCacheFP8")
    for name in ("qattn_paged_kv_cache_append_varlen_rope_fp8", "qattn_rope_paged_varlen"):
        assert name in _native.EXPORTS and hasattr(_native.lib(), name)
    assert _native.ABI_VERSION == 8 == _native.lib().qattn_abi_version()
    assert callable(paged_varlen.paged_varlen_rope_append_input_reason)


def test_the_ops_schemas_and_fake_registrations():
    assert hasattr(qa.ops, "fp8_paged_varlen_rope_kv_cache_append_") and hasattr(qa.ops, "rope_paged_varlen")
    app = torch.ops.quantumattention_amd.fp8_paged_varlen_rope_kv_cache_append_.default
    schema = str(app._schema)
    assert "Tensor(a0!) k_pool" in schema and "Tensor(a1!) v_pool" in schema and "Tensor(a5!) seqlens" in schema, schema
    assert "Tensor cos, Tensor sin" in schema and "bool interleaved=False, bool advance=True" in schema and schema.endswith("-> ()"), schema
    rot = torch.ops.quantumattention_amd.rope_paged_varlen.default
    schema = str(rot._schema)
    assert "!" not in schema and "bool interleaved=False, bool appended=False" in schema and schema.endswith("-> Tensor"), schema
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        pool = torch.empty((4 * HKV * 64 * 64,), dtype=torch.uint8)
        sc = torch.empty((2, HKV), dtype=torch.float32)
        x = torch.empty((5, HKV, 64), dtype=torch.bfloat16)
        tab = torch.empty((128, 32), dtype=torch.float32)
        lens, cu = torch.empty((2,), dtype=torch.int32), torch.empty((3,), dtype=torch.int32)
        assert app(pool, pool.clone(), sc, sc, torch.empty((2, 2), dtype=torch.int32), lens, x, x, cu, tab, tab, 4, 64) is None
        wide = torch.empty((5, 8, 64), dtype=torch.bfloat16)
        y = rot(wide[:, :4], lens, cu, tab, tab, 128)
        assert tuple(y.shape) == (5, 4, 64) and y.dtype == torch.bfloat16 and y.is_contiguous()


# ---- the reason function ------------------------------------------------------------------------------------------------------------------
def test_every_validation_rule_returns_its_reason():
    D, dtype = 64, torch.bfloat16
    c = _cache(D, dtype, "e4m3", 64)
    k, v = _tokens(TOTAL, D, dtype, 1)
    cu = _cu()
    cos, sin = RC.tables(D)
    reason = paged_varlen.paged_varlen_rope_append_input_reason
    assert reason(c, k, v, cu, cos, sin) is None
    # the plain append's rules come first
    assert "3-D tensors" in reason(c, k[None], v[None], cu, None, None)
    assert "torch.int32" in reason(c, k, v, cu.long(), cos, sin)
    # the table rules
    assert "must be tensors" in reason(c, k, v, cu, None, sin)
    assert "same shape" in reason(c, k, v, cu, cos, sin[:-1])
    assert "share a dtype" in reason(c, k, v, cu, cos, sin.half())
    assert "share a dtype" in reason(c, k, v, cu, cos.double(), sin.double())
    assert "device" in reason(c, k, v, cu, cos.to("meta"), sin.to("meta"))
    assert "[B, T, D/2] form" in reason(c, k, v, cu, cos[None].expand(B, T, D // 2), sin[None].expand(B, T, D // 2))
    assert "partial rotary_dim" in reason(c, k, v, cu, cos[:, :16], sin[:, :16])                        # D/2 mismatched
    assert "partial rotary_dim" in reason(c, k, v, cu, torch.cat([cos, cos], 1), torch.cat([sin, sin], 1))
    assert f"fewer than the cache's capacity max_pages_per_seq * page_size = {CAP}" in reason(c, k, v, cu, cos[:CAP - 1], sin[:CAP - 1])
    wide_c, wide_s = torch.zeros(T, D // 2 + 6), torch.zeros(T, D // 2 + 6)
    assert "multiple of 4 floats" in reason(c, k, v, cu, wide_c[:, :D // 2], wide_s[:, :D // 2])     # a row stride that is no multiple of 4
    off = torch.zeros(T * (D // 2) + 2)[2:].view(T, D // 2)
    assert "16-byte-aligned base" in reason(c, k, v, cu, off, off)                                    # a misaligned table slice
    assert "16-byte-aligned base" in reason(c, k, v, cu, torch.zeros(T, D)[:, 2:D // 2 + 2], torch.zeros(T, D)[:, 2:D // 2 + 2])
    assert "dense rows" in reason(c, k, v, cu, torch.zeros(T, D)[:, ::2], torch.zeros(T, D)[:, ::2])
    assert "same row stride" in reason(c, k, v, cu, torch.zeros(T, D)[:, :D // 2], sin)
    # accepted: a slice of a wider table, more rows than the capacity, 16-bit tables (whatever their strides: they are up-cast)
    both = torch.zeros(T + 5, D)
    assert reason(c, k, v, cu, both[:, :D // 2], both[:, D // 2:]) is None
    assert reason(c, k, v, cu, cos.bfloat16(), sin.bfloat16()) is None
    assert reason(c, k, v, cu, cos.half()[:, :], sin.half()) is None
    assert reason(c, k[:0], v[:0], cu, cos, sin) is None
    with pytest.raises(ValueError, match="fewer than the cache's capacity"):
        qa.paged_kv_cache_append_varlen_rope_fp8(c, k, v, cu, cos[:100], sin[:100])
    with pytest.raises(ValueError, match="fewer than the cache's capacity"):
        qa.apply_rope_paged_varlen(k, c, cu, cos[:100], sin[:100])
    q_reason = paged_varlen.paged_varlen_rope_input_reason
    q = torch.zeros(TOTAL, 4 + 2 * HKV, D, dtype=dtype)[:, :4]
    assert q_reason(q, c, cu, cos, sin) is None
    assert "cache's dtype" in q_reason(q.half(), c, cu, cos, sin)
    assert "head dimension" in q_reason(q[..., :32], c, cu, cos, sin)
    assert "out" in q_reason(q, c, cu, cos, sin, out=torch.zeros(TOTAL, 4, D, dtype=torch.float16))
    assert "contiguous" in q_reason(q, c, cu, cos, sin, out=q)


# ---- the C entries' argument checks (before any device call: they run without a GPU) ---------------------------------------------------
def test_the_c_entries_reject_bad_arguments_before_any_device_call():
    L = _native.lib()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    s2 = (ctypes.c_longlong * 2)(2 * 64, 64)
    e4m3 = _native.fmt_of(torch.float8_e4m3fn)

    def append(**kw):
        a = dict(k16=base, v16=base, in_fmt=_native.FMT_BF16, ks=s2, vs=s2, k_pool=base, v_pool=base, scale_k=base, scale_v=base, table=base,
                 tstride=4, seqlens=base, cu=base, advance=1, B=2, Hkv=2, total=0, num_pages=8, page_size=64, max_pages=4, D=64, fp8=e4m3,
                 cos=base, sin=base, tr=32, T=1, il=0)
        a.update(kw)
        return L.qattn_paged_kv_cache_append_varlen_rope_fp8(
            a["k16"], a["v16"], a["in_fmt"], a["ks"], a["vs"], a["k_pool"], a["v_pool"], a["scale_k"], a["scale_v"], a["table"], a["tstride"],
            a["seqlens"], a["cu"], a["advance"], a["B"], a["Hkv"], a["total"], a["num_pages"], a["page_size"], a["max_pages"], a["D"], a["fp8"],
            a["cos"], a["sin"], a["tr"], a["T"], a["il"], None)

    assert append() == 0 and append(il=1) == 0 and append(tr=0) == 0                  # total = 0: QATTN_OK, nothing launched
    bad_arg = append(cu=None)
    assert bad_arg != 0
    for kw in (dict(cos=None), dict(sin=None), dict(cos=base + 4), dict(sin=base + 8), dict(tr=-4), dict(tr=30), dict(T=0), dict(T=-1), dict(il=2),
               dict(il=-1),
               # ... and the plain packed append's checks
               dict(cu=base + 2), dict(total=-1), dict(table=None), dict(page_size=96), dict(num_pages=0), dict(tstride=3), dict(k16=None),
               dict(v16=base + 8), dict(k_pool=base + 8), dict(seqlens=None), dict(B=0), dict(Hkv=0), dict(ks=None),
               dict(ks=(ctypes.c_longlong * 2)(-128, 64)), dict(vs=(ctypes.c_longlong * 2)(128, 12)), dict(B=2 ** 29, Hkv=4)):
        assert append(**kw) == bad_arg, kw
    assert append(D=96) not in (0, bad_arg)                                             # QATTN_ERR_UNSUPPORTED_DIM
    assert append(in_fmt=e4m3) not in (0, bad_arg) and append(fp8=_native.FMT_BF16) == append(in_fmt=e4m3)   # QATTN_ERR_UNSUPPORTED_FMT

    def rotate(**kw):
        a = dict(x=base, in_fmt=_native.FMT_BF16, xs=s2, out=base + 2048, cu=base, seqlens=base, appended=0, B=2, H=2, total=0, capacity=256, D=64,
                 cos=base, sin=base, tr=32, T=1, il=0)
        a.update(kw)
        return L.qattn_rope_paged_varlen(a["x"], a["in_fmt"], a["xs"], a["out"], a["cu"], a["seqlens"], a["appended"], a["B"], a["H"], a["total"],
                                         a["capacity"], a["D"], a["cos"], a["sin"], a["tr"], a["T"], a["il"], None)

    assert rotate() == 0 and rotate(appended=1, il=1) == 0
    for kw in (dict(x=None), dict(out=None), dict(cu=None), dict(seqlens=None), dict(xs=None), dict(x=base + 8), dict(out=base + 8), dict(cu=base + 2),
               dict(seqlens=base + 1), dict(xs=(ctypes.c_longlong * 2)(-128, 64)), dict(xs=(ctypes.c_longlong * 2)(128, 12)), dict(B=0), dict(H=0),
               dict(total=-1), dict(capacity=0), dict(capacity=2 ** 31), dict(appended=2), dict(cos=None), dict(sin=base + 4), dict(tr=-4),
               dict(tr=6), dict(T=0), dict(il=2), dict(total=2 ** 31 - 1, H=2 ** 20)):
        assert rotate(**kw) == bad_arg, kw
    assert rotate(D=96) == append(D=96) and rotate(in_fmt=e4m3) == append(in_fmt=e4m3)


# ---- the eager definitions are THE RULE -----------------------------------------------------------------------------------------------------
EAGER = [(64, torch.bfloat16, "e4m3", 64, False), (64, torch.float16, "e5m2", 256, True), (128, torch.float16, "e4m3", 128, False),
         (128, torch.bfloat16, "e5m2", 64, True), (256, torch.bfloat16, "e4m3", 256, True), (256, torch.float16, "e5m2", 128, False)]


@pytest.mark.parametrize("D,dtype,fmt,page_size,il", EAGER, ids=[f"d{d}-{str(t)[6:]}-{f}-ps{p}-il{int(i)}" for d, t, f, p, i in EAGER])
def test_the_eager_definition_is_the_rule_on_whole_pools_and_seqlens(D, dtype, fmt, page_size, il):
    c0 = _cache(D, dtype, fmt, page_size, seed=D)
    k, v = _tokens(TOTAL + 3, D, dtype, D + 1)
    k[5, 0, 3], k[70, 1, 0], k[200, 0, 1], v[9, 0, 0] = float("inf"), float("nan"), -float("inf"), -float("inf")
    if dtype == torch.float16:
        k[150, 1, :4] = 60000.0                                                           # an fp16 product that overflows in the rotation
    k[TOTAL:], v[TOTAL:] = float("nan"), float("nan")                                      # a padded token bucket: rows nobody owns
    cu = _cu()
    cos, sin = RC.tables(D)
    for advance in (True, False):
        a, b = _clone(c0), _clone(c0)
        assert qa.paged_kv_cache_append_varlen_rope_fp8(a, k, v, cu, cos, sin, interleaved=il, advance=advance) is a
        RC.rule(b, k, v, cu, COUNTS, STARTS, cos, sin, il, advance)
        assert _same_state(a, b) and not _same_state(a, c0)
        want = [min(p + n, CAP) for p, n in zip(STARTS, COUNTS)] if advance else STARTS
        assert a.seqlens.tolist() == want
        # V is not rotated: its pool is the plain append's
        p = _clone(c0)
        qa.paged_kv_cache_append_varlen_fp8(p, k, v, cu, advance=advance)
        assert torch.equal(a.v.view(torch.uint8), p.v.view(torch.uint8)) and not torch.equal(a.k.view(torch.uint8), p.k.view(torch.uint8))
        changed = (a.k.view(torch.uint8) != RC.SENTINEL).any(-1).any(1).sum().item()
        assert changed <= sum(min(n, CAP - s) for s, n in zip(STARTS, COUNTS))
    # 16-bit tables are up-cast; a slice of a wider table is read in place
    a, b = _clone(c0), _clone(c0)
    qa.paged_kv_cache_append_varlen_rope_fp8(a, k, v, cu, cos.bfloat16(), sin.bfloat16(), interleaved=il)
    RC.rule(b, k, v, cu, COUNTS, STARTS, cos.bfloat16().float(), sin.bfloat16().float(), il, True)
    assert _same_state(a, b)
    both = torch.cat([cos, sin], 1)
    a, b = _clone(c0), _clone(c0)
    qa.paged_kv_cache_append_varlen_rope_fp8(a, k, v, cu, both[:, :D // 2], both[:, D // 2:], interleaved=il)
    RC.rule(b, k, v, cu, COUNTS, STARTS, cos, sin, il, True)
    assert _same_state(a, b)


@pytest.mark.parametrize("il", [False, True])
def test_apply_rope_paged_varlen_eager_is_apply_rope_eager_at_host_positions(il):
    D, dtype, Hq = 64, torch.bfloat16, 4
    c = _cache(D, dtype, "e4m3", 64)
    cos, sin = RC.tables(D)
    qkv = (torch.randn(TOTAL + 3, Hq + 2 * HKV, D, generator=torch.Generator().manual_seed(3)) * 2).to(dtype)
    q = qkv[:, :Hq]
    cu = _cu()
    got = qa.apply_rope_paged_varlen(q, c, cu, cos, sin, interleaved=il)
    want = RC.rotate_at(q, RC.positions(COUNTS, STARTS, TOTAL + 3), cos, sin, il)
    assert got.is_contiguous() and got.dtype == dtype and torch.equal(got[:TOTAL].view(torch.int16), want[:TOTAL].view(torch.int16))
    # after an advancing append the same rows are had with appended=True
    after = _clone(c)
    qa.paged_kv_cache_append_varlen_rope_fp8(after, qkv[:, Hq:Hq + HKV], qkv[:, Hq + HKV:], cu, cos, sin, interleaved=il)
    live = [i for i in range(TOTAL) if not RC.cu_list(COUNTS)[5] <= i < RC.cu_list(COUNTS)[6]]       # (slot 5 dropped its tail: p - n is not its start)
    got2 = qa.apply_rope_paged_varlen(q, after, cu, cos, sin, interleaved=il, appended=True)
    assert torch.equal(got2[live].view(torch.int16), want[live].view(torch.int16))
    want2 = RC.rotate_at(q, RC.positions(COUNTS, after.seqlens.tolist(), TOTAL + 3, appended=True), cos, sin, il)
    assert torch.equal(got2[:TOTAL].view(torch.int16), want2[:TOTAL].view(torch.int16))
    # out=: rows behind cu[B] are not written
    out = torch.full((TOTAL + 3, Hq, D), 7.0, dtype=dtype)
    assert qa.apply_rope_paged_varlen(q, c, cu, cos, sin, interleaved=il, out=out) is out
    assert torch.equal(out[:TOTAL].view(torch.int16), want[:TOTAL].view(torch.int16)) and (out[TOTAL:] == 7.0).all()


# ---- the kernel's unit map (include/qattn_paged_varlen_rope.h), as arithmetic ---------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128, 256])
def test_every_piece_of_a_chunk_belongs_to_one_unit_and_the_units_float4_cover_its_pairs(D):
    HV, VPR = D // 16, D // 8
    iters = 64 * VPR // 256                                  # vectors a thread of the plain mapping holds
    units = 64 * HV
    assert units % 256 == 0 and units // 256 == iters // 2 and units // 256 in (1, 2, 4)
    seen = {}
    for unit in range(units):
        r, dvh = unit // HV, unit % HV
        for piece in (dvh, dvh + HV):
            assert (r, piece) not in seen
            seen[(r, piece)] = unit
        elems = lambda piece: range(8 * piece, 8 * piece + 8)
        # pairs (i, i + D/2): element j of piece dvh with element j of piece dvh + HV, table entry 8 dvh + j
        assert [e + D // 2 for e in elems(dvh)] == list(elems(dvh + HV))
        assert sorted({e // 4 for e in elems(dvh)}) == [2 * dvh, 2 * dvh + 1] and 2 * dvh + 1 < D // 8
        # pairs (2i, 2i + 1): inside a piece, table entries 4 piece .. 4 piece + 3 = float4 `piece`
        for piece, f4 in ((dvh, dvh), (dvh + HV, dvh + HV)):
            pairs = {e // 2 for e in elems(piece)}
            assert all(e ^ 1 in elems(piece) for e in elems(piece)) and {p // 4 for p in pairs} == {f4} and f4 < D // 8
    assert len(seen) == 64 * VPR and set(seen) == {(r, p) for r in range(64) for p in range(VPR)}


# ---- independent of apply_rope_eager: fp64 ------------------------------------------------------------------------------------------------
def _fp64_rotation(k, pos, cos, sin, il):
    """(y, |a| + |b|) in fp64: k [total, H, D] rotated at table rows pos with the fp32 tables' values"""
    x = k.double()
    h = x.shape[-1] // 2
    at = torch.tensor(pos, dtype=torch.long)
    c, s = cos.double()[at][:, None], sin.double()[at][:, None]
    y, mag = torch.empty_like(x), torch.empty_like(x)
    if il:
        a, b = x[..., 0::2], x[..., 1::2]
        y[..., 0::2], y[..., 1::2] = a * c - b * s, b * c + a * s
        mag[..., 0::2] = mag[..., 1::2] = a.abs() + b.abs()
    else:
        a, b = x[..., :h], x[..., h:]
        y[..., :h], y[..., h:] = a * c - b * s, b * c + a * s
        mag[..., :h] = mag[..., h:] = a.abs() + b.abs()
    return y, mag


def _appended_rows(c, kpool_rows):
    """[n_rows, Hkv, D] of a gathered [B, Hkv, CAP, D] tensor: the keys the step appended, in token order (slot 5 without its dropped tail),
    and the token index of each"""
    rows, toks = [], []
    cu = RC.cu_list(COUNTS)
    for i, (p, n) in enumerate(zip(STARTS, COUNTS)):
        n = min(n, CAP - p)
        rows.append(kpool_rows[i, :, p:p + n].transpose(0, 1))
        toks += range(cu[i], cu[i] + n)
    return torch.cat(rows), toks


FP64 = [(D, dt, il) for D in (64, 128, 256) for dt in (torch.bfloat16, torch.float16) for il in (False, True)]


@pytest.mark.parametrize("D,dtype,il", FP64, ids=[f"d{d}-{str(t)[6:]}-il{int(i)}" for d, t, i in FP64])
def test_the_cache_holds_the_fp64_rotation_within_the_formats_steps_and_shifted_positions_break_it_in_every_row(D, dtype, il):
    """|deq - y| <= (2^-4 + 2^-7) |y| + 2^-10 scale + 2^-18 (|a| + |b|) on unsaturated elements: e4m3's half step, the two 16-bit
    roundings (input dtype after the rotation; bf16's half step 2^-8 twice, which bounds fp16's), the subnormal half step, the fp32 operations."""
    scale = 0.02
    c = _cache(D, dtype, "e4m3", 64, seed=D, scale_k=scale)
    k, v = _tokens(TOTAL, D, dtype, 9 * D + int(il))
    cos, sin = RC.tables(D, rows=T + 1)
    cu = _cu()
    qa.paged_kv_cache_append_varlen_rope_fp8(c, k, v, cu, cos[:T], sin[:T], interleaved=il)
    deq, toks = _appended_rows(c, gather_paged_eager(c).k.double() * scale)
    stored, _ = _appended_rows(c, gather_paged_eager(c).k.view(torch.uint8))

    def misses(shift):
        y, mag = _fp64_rotation(k, RC.positions(COUNTS, STARTS, TOTAL, rows=T + 1, shift=shift), cos, sin, il)
        y, mag = y[toks], mag[toks]
        ok = y.abs() / scale <= 448.0                                                    # unsaturated
        bound = (2.0 ** -4 + 2.0 ** -7) * y.abs() + 2.0 ** -10 * scale + 2.0 ** -18 * mag
        ratio = ((deq - y).abs() / bound)[ok].max().item()
        return ((deq - y).abs() > bound) & ok, ok, ratio

    miss, ok, ratio = misses(0)
    print(f"worst |deq - y| / bound {ratio:.3f}, unsaturated {ok.float().mean().item():.5f}")
    assert ok.float().mean().item() > 0.999 and not miss.any(), ratio
    # teeth: the same bytes against the rotation one position further break the bound in every row ...
    miss1, _, _ = misses(1)
    print(f"shifted by one: rows {miss1.any(-1).float().mean().item():.3f}, elements {miss1.float().mean().item():.3f}")
    assert miss1.any(-1).all()
    # ... and the bytes of an append at the shifted positions differ from the true ones in every row: the tables are not degenerate
    s = _cache(D, dtype, "e4m3", 64, seed=D, scale_k=scale)
    qa.paged_kv_cache_append_varlen_rope_fp8(s, k, v, cu, cos[1:], sin[1:], interleaved=il)
    shifted, _ = _appended_rows(s, gather_paged_eager(s).k.view(torch.uint8))
    assert (shifted != stored).any(-1).all()

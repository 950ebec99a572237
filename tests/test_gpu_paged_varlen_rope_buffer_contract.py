"""Buffer contract of qattn_paged_kv_cache_append_varlen_rope_fp8 and qattn_rope_paged_varlen (include/qattn_paged_varlen_rope.h), held the
way tests/test_gpu_paged_varlen_append_buffer_contract.py holds the plain packed append: the C entries through ctypes, every
caller-provided buffer carved from a guarded arena (tests/arena.py) of EXACTLY the documented size at the documented alignment -- k16 / v16
/ x16 of exactly `total` rows (the last row of a strided view ends where the buffer ends), cos / sin of exactly T rows (the last row of a
sliced table ends where the buffer ends) at 16 bytes, cu_seqlens of exactly B + 1 ints.  After the call every guard is intact, the outputs
are bit-equal to the ordinary call's, every other pool byte holds its pre-fill, and no bit depends on what the guards, the pads of a
strided view or the pools held.  Every table entry is a valid page; T = capacity, so the last table row is the last key's."""
import ctypes

import pytest
import torch

from quantumattention_amd import _native
from tests import arena as A
from tests import kvcache_cases as KC
from tests import paged_cases as P
from tests import paged_varlen_rope_cases as RC
from tests.test_gpu_buffer_contract import _stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
HKV, CAP, B = 2, 512, 4
CASES = [   # D, dtype, fp8 format, page size, counts, seqlens, input view, table view, interleaved
    (64, torch.bfloat16, "e4m3", 64, [7, 0, 1, 64], [0, 61, 125, 64], "dense", "dense", 0),
    (128, torch.bfloat16, "e4m3", 64, [130, 1, 1, 0], [5, 66, 511, 3], "qkv", "wide", 1),        # slot 2's token is key 511: the last table row
    (128, torch.float16, "e5m2", 128, [1, 1, 1, 1], [63, 127, 512, 0], "padded", "dense", 0),    # slot 2 is full: its token is dropped
    (256, torch.bfloat16, "e4m3", 256, [0, 3, 65, 0], [255, 2, 500, 9], "qkv", "wide", 0),        # slot 2 overflows: 12 of 65 stored
    (128, torch.bfloat16, "e5m2", 256, [70, 2, 1, 5], [-5, 1300, 200, 64], "dense", "dense", 1),  # seqlens outside [0, capacity]: clamped
]
IDS = ["d64-ps64", "d128-ps64-chunk-and-decodes-qkv-il", "d128-fp16-e5m2-ps128-decode", "d256-ps256-overflow-qkv", "d128-e5m2-clamped-seqlens-il"]


def _view(kind, total, H, D):
    """(element strides {token, head, 1}, span in elements) of a [total, H, D] view whose last row ends the buffer"""
    if kind == "dense":
        ts, hs = H * D, D
    elif kind == "qkv":
        ts, hs = (4 + 2 * HKV) * D, D          # a slice of a [total, (Hq + 2 Hkv) D] projection, Hq 4
    else:
        hs = D + 8
        ts = H * hs + 16
    return (ts, hs, 1), (total - 1) * ts + (H - 1) * hs + D


def _table_view(kind, T, D):
    """(row stride in floats, span in floats) of a [T, D/2] table whose last row ends the buffer"""
    tr = D // 2 if kind == "dense" else D + 4      # wide: a slice [:, :D/2] of rows of D + 4 floats
    return tr, (T - 1) * tr + D // 2


def _carve_tables(ar, D, kind):
    tr, span = _table_view(kind, CAP, D)
    cos, sin = RC.tables(D, rows=CAP, device=DEV)
    rc_ = ar.carve("cos", 4 * span, align=16, row_bytes=2 * D, role="in", kind="fp32")
    rs_ = ar.carve("sin", 4 * span, align=16, row_bytes=2 * D, role="in", kind="fp32")
    return cos, sin, rc_, rs_, tr


@pytest.mark.parametrize("advance", [1, 0], ids=["advance", "no-advance"])
@pytest.mark.parametrize("D,dtype,fmt,ps,counts,lens,view,tview,il", CASES, ids=IDS)
def test_paged_kv_cache_append_varlen_rope_fp8(D, dtype, fmt, ps, counts, lens, view, tview, il, advance):
    L = _native.lib()
    fp8 = P.FP8[fmt]
    M = CAP // ps
    g = torch.Generator().manual_seed(1000 * sum(counts) + D)
    num_pages = B * M + 2
    table = torch.randperm(num_pages, generator=g)[:B * M].view(B, M).to(torch.int32)       # every sequence owns all its pages: private, shuffled
    total = sum(counts)
    cu = RC.cu_list(counts)
    k, v = ((torch.randn(total, HKV, D, generator=g) * 3).to(dtype).to(DEV) for _ in range(2))
    sk = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    sv = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    strides, span = _view(view, total, HKV, D)
    ar = A.Arena(DEV)
    rk = ar.carve("k16", span * 2, align=16, row_bytes=2 * D, role="in", kind=A.KIND_OF_DTYPE[dtype])
    rv = ar.carve("v16", span * 2, align=16, row_bytes=2 * D, role="in", kind=A.KIND_OF_DTYPE[dtype])
    rsk = ar.carve("scale_k", 4 * B * HKV, align=4, role="in", kind="fp32")
    rsv = ar.carve("scale_v", 4 * B * HKV, align=4, role="in", kind="fp32")
    rsk.load(sk)
    rsv.load(sv)
    rtab = ar.carve("block_table", 4 * B * M, align=4, role="in", kind="int32")
    rtab.load(table.to(DEV))
    rcu = ar.carve("cu_seqlens", 4 * (B + 1), align=4, role="in", kind="int32")
    rcu.load(torch.tensor(cu, dtype=torch.int32, device=DEV))
    cos, sin, rcos, rsin, tr = _carve_tables(ar, D, tview)
    rsl = ar.carve("seqlens", 4 * B, align=4, role="scratch")
    nb = P.pool_bytes(num_pages, HKV, ps, D)
    rik = ar.carve("k_pool", nb, align=16, row_bytes=D, role="scratch")
    riv = ar.carve("v_pool", nb, align=16, row_bytes=D, role="scratch")
    s2 = (ctypes.c_longlong * 2)(*strides[:2])
    # the header's rules, literally
    pos = [min(max(p, 0), CAP) for p in lens]
    end = [min(pos[b] + counts[b], CAP) for b in range(B)]
    mine = torch.zeros(num_pages, HKV, ps, dtype=torch.bool, device=DEV)
    for b in range(B):
        js = torch.arange(pos[b], end[b])
        mine[table[b].long()[js // ps].to(DEV), :, (js % ps).to(DEV)] = True
    runs = []
    for hostile, fill in ((True, 0xA5), (False, P.NAN_BYTE[fmt])):
        ar.set_input_guards(hostile)
        rk.load_view(k, strides, hostile=hostile)
        rv.load_view(v, strides, hostile=hostile)
        rcos.load_view(cos, (tr, 1), hostile=hostile)
        rsin.load_view(sin, (tr, 1), hostile=hostile)
        rik.fill(fill)
        riv.fill(fill)
        rsl.interior.view(torch.int32).copy_(torch.tensor(lens, dtype=torch.int32))
        rc = L.qattn_paged_kv_cache_append_varlen_rope_fp8(rk.ptr, rv.ptr, _native.fmt_of(dtype), s2, s2, rik.ptr, riv.ptr, rsk.ptr, rsv.ptr, rtab.ptr,
                                                           M, rsl.ptr, rcu.ptr, advance, B, HKV, total, num_pages, ps, M, D, _native.fmt_of(fp8),
                                                           rcos.ptr, rsin.ptr, tr, CAP, il, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.qattn_strerror(rc))
        A.assert_guards_intact(ar)
        assert rsl.interior.view(torch.int32).tolist() == (end if advance else lens)
        rows = []
        for reg, layout in ((rik, KC.KFRAG), (riv, KC.VFRAG)):
            got = KC.from_image(reg.interior, layout, num_pages, HKV, ps, D)
            other = got[~mine]
            assert (other == fill).all(), (f"{reg.name}: {(other != fill).any(-1).sum().item()} keys the call does not append lost their "
                                           f"pre-fill 0x{fill:02x}")
            rows.append(got[mine].clone())
        runs.append(rows)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])   # no appended byte depends on what the pools or the guards held
    # ... and they are the bytes of the ordinary call (the binding on torch tensors) from the same starting state ...
    kp, vp = (torch.full((nb,), P.NAN_BYTE[fmt], dtype=torch.uint8, device=DEV) for _ in range(2))
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    _native.paged_kv_cache_append_varlen_rope_fp8(kp, vp, sk, sv, table.to(DEV), sl, k, v, cu_t, cos, sin, num_pages=num_pages, page_size=ps,
                                                  fp8_dtype=fp8, interleaved=bool(il), advance=bool(advance))
    assert torch.equal(kp, rik.interior) and torch.equal(vp, riv.interior) and sl.tolist() == (end if advance else lens)
    # ... which are THE RULE's: the rotation in torch at the header's positions, then the plain packed append
    kq, vq = (torch.full((nb,), P.NAN_BYTE[fmt], dtype=torch.uint8, device=DEV) for _ in range(2))
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    k_rot = RC.rotate_at(k, RC.positions(counts, lens, total, rows=CAP, cap=CAP), cos, sin, bool(il))
    _native.paged_kv_cache_append_varlen_fp8(kq, vq, sk, sv, table.to(DEV), sl, k_rot, v, cu_t, num_pages=num_pages, page_size=ps, fp8_dtype=fp8,
                                             advance=bool(advance))
    assert torch.equal(kq, rik.interior) and torch.equal(vq, riv.interior)


@pytest.mark.parametrize("appended", [0, 1], ids=["before-append", "after-append"])
@pytest.mark.parametrize("D,dtype,fmt,ps,counts,lens,view,tview,il", CASES, ids=IDS)
def test_rope_paged_varlen(D, dtype, fmt, ps, counts, lens, view, tview, il, appended):
    L = _native.lib()
    H = 4
    g = torch.Generator().manual_seed(2000 * sum(counts) + D)
    total = sum(counts)
    bucket = total + 3                                   # rows behind cu[B]: neither read nor written
    cu = RC.cu_list(counts)
    x = (torch.randn(bucket, H, D, generator=g) * 3).to(dtype).to(DEV)
    x[total:] = float("nan")
    strides, span = _view(view, bucket, H, D)
    kind = A.KIND_OF_DTYPE[dtype]
    ar = A.Arena(DEV)
    rx = ar.carve("x16", span * 2, align=16, row_bytes=2 * D, role="in", kind=kind)
    rcu = ar.carve("cu_seqlens", 4 * (B + 1), align=4, role="in", kind="int32")
    rcu.load(torch.tensor(cu, dtype=torch.int32, device=DEV))
    rsl = ar.carve("seqlens", 4 * B, align=4, role="in", kind="int32")
    rsl.load(torch.tensor(lens, dtype=torch.int32, device=DEV))
    cos, sin, rcos, rsin, tr = _carve_tables(ar, D, tview)
    rout = ar.carve("out16", 2 * bucket * H * D, align=16, row_bytes=2 * D, role="out", kind=kind)
    s2 = (ctypes.c_longlong * 2)(*strides[:2])
    want = RC.rotate_at(x[:total], RC.positions(counts, lens, total, rows=CAP, cap=CAP, appended=bool(appended)), cos, sin, bool(il))
    runs = []
    for hostile in (True, False):
        ar.set_input_guards(hostile)
        rx.load_view(x, strides, hostile=hostile)
        rcos.load_view(cos, (tr, 1), hostile=hostile)
        rsin.load_view(sin, (tr, 1), hostile=hostile)
        rout.fill_poison()
        rc = L.qattn_rope_paged_varlen(rx.ptr, _native.fmt_of(dtype), s2, rout.ptr, rcu.ptr, rsl.ptr, appended, B, H, total + 3, CAP, D, rcos.ptr,
                                       rsin.ptr, tr, CAP, il, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.qattn_strerror(rc))
        A.assert_guards_intact(ar)
        got = rout.view(dtype, (bucket, H, D))
        assert torch.equal(got[:total].view(torch.int16), want.view(torch.int16))
        tail = rout.interior[2 * total * H * D:]
        assert rout.poison_left(tail) == 3 * H * D, "a row behind cu_seqlens[B] was written"
        runs.append(got[:total].clone())
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16))
    # the ordinary call (the binding on torch tensors)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    mine = _native.rope_paged_varlen(x, sl, torch.tensor(cu, dtype=torch.int32, device=DEV), cos, sin, capacity=CAP, interleaved=bool(il),
                                     appended=bool(appended))
    assert torch.equal(mine[:total].view(torch.int16), runs[0].view(torch.int16))

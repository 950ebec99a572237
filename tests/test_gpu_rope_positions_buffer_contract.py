"""Buffer contract of qattn_paged_kv_cache_append_varlen_rope_pos_fp8 and qattn_rope_packed_positions
(include/qattn_paged_varlen_rope_pos.h), held the way tests/test_gpu_paged_varlen_rope_buffer_contract.py holds their siblings: the C
entries through ctypes, every caller-provided buffer carved from a guarded arena (tests/arena.py) of EXACTLY the documented size at the
documented alignment -- positions: exactly `total` 64-bit words at 8 bytes; k16 / v16 / x16 of exactly `total` rows; cos / sin of exactly
T rows at 16 bytes.  After the call every guard is intact, the outputs are bit-equal to the ordinary call's and to THE RULE's, every other
pool byte holds its pre-fill, and no bit depends on what the guards, the pads of a strided view or the pools held.  The positions repeat,
descend and leave [0, T): the clamp keeps every table read inside the carved tables.  The argument checks return before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from quantumattention_amd import _native
from tests import arena as A
from tests import kvcache_cases as KC
from tests import paged_cases as P
from tests import paged_varlen_rope_cases as RC
from tests.test_gpu_buffer_contract import _stream
from tests.test_gpu_paged_varlen_rope_buffer_contract import B, CAP, CASES, HKV, IDS, _carve_tables, _view

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _positions(total, seed):
    rng = np.random.RandomState(seed)
    pos = rng.randint(-40, CAP + 40, total).astype(np.int64)
    if total > 8:
        pos[2:5] = pos[1]                  # siblings
        pos[5], pos[6], pos[7] = -(1 << 62), (1 << 62), CAP
    return pos


def _carve_positions(ar, pos):
    r = ar.carve("positions", 8 * len(pos), align=8, role="in", kind="int32")
    r.load(torch.from_numpy(pos).to(DEV).view(torch.int32))
    return r


@pytest.mark.parametrize("advance", [1, 0], ids=["advance", "no-advance"])
@pytest.mark.parametrize("D,dtype,fmt,ps,counts,lens,view,tview,il", CASES, ids=IDS)
def test_paged_kv_cache_append_varlen_rope_pos_fp8(D, dtype, fmt, ps, counts, lens, view, tview, il, advance):
    L = _native.lib()
    fp8 = P.FP8[fmt]
    M = CAP // ps
    g = torch.Generator().manual_seed(1000 * sum(counts) + D)
    num_pages = B * M + 2
    table = torch.randperm(num_pages, generator=g)[:B * M].view(B, M).to(torch.int32)
    total = sum(counts)
    cu = RC.cu_list(counts)
    k, v = ((torch.randn(total, HKV, D, generator=g) * 3).to(dtype).to(DEV) for _ in range(2))
    sk = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    sv = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    pos = _positions(total, D + total)
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
    rpos = _carve_positions(ar, pos)
    cos, sin, rcos, rsin, tr = _carve_tables(ar, D, tview)
    rsl = ar.carve("seqlens", 4 * B, align=4, role="scratch")
    nb = P.pool_bytes(num_pages, HKV, ps, D)
    rik = ar.carve("k_pool", nb, align=16, row_bytes=D, role="scratch")
    riv = ar.carve("v_pool", nb, align=16, row_bytes=D, role="scratch")
    s2 = (ctypes.c_longlong * 2)(*strides[:2])
    # where the keys go is the packed append's rule, literally
    start = [min(max(p, 0), CAP) for p in lens]
    end = [min(start[b] + counts[b], CAP) for b in range(B)]
    mine = torch.zeros(num_pages, HKV, ps, dtype=torch.bool, device=DEV)
    for b in range(B):
        js = torch.arange(start[b], end[b])
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
        rc = L.qattn_paged_kv_cache_append_varlen_rope_pos_fp8(rk.ptr, rv.ptr, _native.fmt_of(dtype), s2, s2, rik.ptr, riv.ptr, rsk.ptr, rsv.ptr,
                                                               rtab.ptr, M, rsl.ptr, rcu.ptr, advance, B, HKV, total, num_pages, ps, M, D,
                                                               _native.fmt_of(fp8), rcos.ptr, rsin.ptr, tr, CAP, il, rpos.ptr, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.qattn_strerror(rc))
        A.assert_guards_intact(ar)
        assert rsl.interior.view(torch.int32).tolist() == (end if advance else lens)
        rows = []
        for reg, layout in ((rik, KC.KFRAG), (riv, KC.VFRAG)):
            got = KC.from_image(reg.interior, layout, num_pages, HKV, ps, D)
            other = got[~mine]
            assert (other == fill).all(), f"{reg.name}: keys the call does not append lost their pre-fill 0x{fill:02x}"
            rows.append(got[mine].clone())
        runs.append(rows)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # the ordinary call (the binding on torch tensors) from the same starting state ...
    kp, vp = (torch.full((nb,), P.NAN_BYTE[fmt], dtype=torch.uint8, device=DEV) for _ in range(2))
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    _native.paged_kv_cache_append_varlen_rope_pos_fp8(kp, vp, sk, sv, table.to(DEV), sl, k, v, cu_t, torch.from_numpy(pos).to(DEV), cos, sin,
                                                      num_pages=num_pages, page_size=ps, fp8_dtype=fp8, interleaved=bool(il), advance=bool(advance))
    assert torch.equal(kp, rik.interior) and torch.equal(vp, riv.interior) and sl.tolist() == (end if advance else lens)
    # ... which are THE RULE's: the rotation in torch at the clamped positions, then the plain packed append
    kq, vq = (torch.full((nb,), P.NAN_BYTE[fmt], dtype=torch.uint8, device=DEV) for _ in range(2))
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    k_rot = RC.rotate_at(k, np.clip(pos, 0, CAP - 1).tolist(), cos, sin, bool(il))
    _native.paged_kv_cache_append_varlen_fp8(kq, vq, sk, sv, table.to(DEV), sl, k_rot, v, cu_t, num_pages=num_pages, page_size=ps, fp8_dtype=fp8,
                                             advance=bool(advance))
    assert torch.equal(kq, rik.interior) and torch.equal(vq, riv.interior)


@pytest.mark.parametrize("D,dtype,fmt,ps,counts,lens,view,tview,il", CASES, ids=IDS)
def test_rope_packed_positions(D, dtype, fmt, ps, counts, lens, view, tview, il):
    L = _native.lib()
    H = 4
    g = torch.Generator().manual_seed(2000 * sum(counts) + D)
    total = sum(counts)
    x = (torch.randn(total, H, D, generator=g) * 3).to(dtype).to(DEV)
    pos = _positions(total, D + 7)
    strides, span = _view(view, total, H, D)
    kind = A.KIND_OF_DTYPE[dtype]
    ar = A.Arena(DEV)
    rx = ar.carve("x16", span * 2, align=16, row_bytes=2 * D, role="in", kind=kind)
    rpos = _carve_positions(ar, pos)
    cos, sin, rcos, rsin, tr = _carve_tables(ar, D, tview)
    rout = ar.carve("out16", 2 * total * H * D, align=16, row_bytes=2 * D, role="out", kind=kind)
    s2 = (ctypes.c_longlong * 2)(*strides[:2])
    want = RC.rotate_at(x, np.clip(pos, 0, CAP - 1).tolist(), cos, sin, bool(il))
    runs = []
    for hostile in (True, False):
        ar.set_input_guards(hostile)
        rx.load_view(x, strides, hostile=hostile)
        rcos.load_view(cos, (tr, 1), hostile=hostile)
        rsin.load_view(sin, (tr, 1), hostile=hostile)
        rout.fill_poison()
        rc = L.qattn_rope_packed_positions(rx.ptr, _native.fmt_of(dtype), s2, rout.ptr, rpos.ptr, H, total, D, rcos.ptr, rsin.ptr, tr, CAP, il,
                                           _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.qattn_strerror(rc))
        A.assert_guards_intact(ar)
        got = rout.view(dtype, (total, H, D))
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert rout.poison_left(rout.interior) == 0, "a row was left unwritten"
        runs.append(got.clone())
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16))
    mine = _native.rope_packed_positions(x, torch.from_numpy(pos).to(DEV), cos, sin, interleaved=bool(il))
    assert torch.equal(mine.view(torch.int16), runs[0].view(torch.int16))


def test_the_argument_checks_return_their_codes_before_any_launch():
    L = _native.lib()
    p = 0x1000
    s2 = (ctypes.c_longlong * 2)(2 * 128, 128)
    e4 = _native.fmt_of(torch.float8_e4m3fn)

    def app(positions=p, cos=p, tr=64, T=512, il=0, D=128, total=10, k=p, table=p):
        return L.qattn_paged_kv_cache_append_varlen_rope_pos_fp8(k, p, _native.FMT_BF16, s2, s2, p, p, p, p, table, 8, p, p, 1, 4, 2, total, 34, 64, 8, D,
                                                                 e4, cos, p, tr, T, il, positions, None)
    INVALID = app(table=None)
    assert INVALID != 0
    for kw in (dict(positions=None), dict(positions=p + 4), dict(positions=p + 1), dict(cos=None), dict(cos=p + 4), dict(tr=6), dict(T=0), dict(il=2),
               dict(k=None), dict(total=-1)):
        assert app(**kw) == INVALID, kw
    assert app(D=96) not in (0, INVALID)
    assert app(total=0) == 0                                            # nothing launched

    def rot(positions=p, x=p, out=p, H=4, total=10, D=128, cos=p, tr=64, T=512, il=0, fmt=_native.FMT_BF16):
        return L.qattn_rope_packed_positions(x, fmt, s2, out, positions, H, total, D, cos, p, tr, T, il, None)
    for kw in (dict(positions=None), dict(positions=p + 4), dict(x=None), dict(out=None), dict(out=p + 8), dict(H=0), dict(total=-1), dict(cos=p + 8),
               dict(tr=-4), dict(T=0), dict(il=3)):
        assert rot(**kw) == INVALID, kw
    assert rot(D=96) == app(D=96) and rot(fmt=e4) not in (0, INVALID, rot(D=96))
    assert rot(total=0) == 0                                            # nothing launched

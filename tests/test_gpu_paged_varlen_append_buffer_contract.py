"""Buffer contract of qattn_paged_kv_cache_append_varlen_fp8 (include/qattn_paged_varlen_append.h), held the way
tests/test_gpu_paged_buffer_contract.py holds the padded append: the C entry through ctypes, every caller-provided buffer carved from a
guarded arena (tests/arena.py) of EXACTLY the documented size at the documented alignment -- k16 / v16 of exactly `total` rows (the last
row of a strided view ends where the buffer ends), cu_seqlens of exactly B + 1 ints.  After the call every guard is intact, the appended
keys hold the reference quantiser's bytes (which the ordinary call is held to as well), every other pool byte its pre-fill, and no bit
depends on what the guards, the pads of a strided view or the pools held.  Every table entry is a valid page."""
import ctypes

import pytest
import torch

from quantumattention_amd import _native
from tests import arena as A
from tests import kvcache_cases as KC
from tests import paged_cases as P
from tests.test_gpu_buffer_contract import _stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
HKV, CAP = 2, 512
CASES = [   # D, dtype, fp8 format, page size, counts, seqlens, input view
    (64, torch.bfloat16, "e4m3", 64, [7, 0, 1, 64], [0, 61, 125, 64], "dense"),
    (128, torch.bfloat16, "e4m3", 64, [130, 1, 1, 0], [5, 66, 511, 3], "qkv"),
    (128, torch.float16, "e5m2", 128, [1, 1, 1, 1], [63, 127, 512, 0], "padded"),           # slot 2 is full: its token is dropped
    (256, torch.bfloat16, "e4m3", 256, [0, 3, 65, 0], [255, 2, 500, 9], "qkv"),              # slot 2 overflows: 12 of 65 stored
    (128, torch.bfloat16, "e5m2", 256, [70, 2, 1, 5], [-5, 1300, 200, 64], "dense"),         # seqlens outside [0, capacity]: clamped
]
IDS = ["d64-ps64", "d128-ps64-chunk-and-decodes-qkv", "d128-fp16-e5m2-ps128-decode", "d256-ps256-overflow-qkv", "d128-e5m2-clamped-seqlens"]
B = 4


def _view(kind, total, D):
    """(element strides {token, head, 1}, span in elements) of a [total, HKV, D] view whose last row ends the buffer"""
    if kind == "dense":
        ts, hs = HKV * D, D
    elif kind == "qkv":
        ts, hs = (4 + 2 * HKV) * D, D          # the K slice of a [total, (Hq + 2 Hkv) D] projection, Hq 4
    else:
        hs = D + 8
        ts = HKV * hs + 16
    return (ts, hs, 1), (total - 1) * ts + (HKV - 1) * hs + D


@pytest.mark.parametrize("advance", [1, 0], ids=["advance", "no-advance"])
@pytest.mark.parametrize("D,dtype,fmt,ps,counts,lens,view", CASES, ids=IDS)
def test_paged_kv_cache_append_varlen_fp8(D, dtype, fmt, ps, counts, lens, view, advance):
    L = _native.lib()
    fp8 = P.FP8[fmt]
    M = CAP // ps
    g = torch.Generator().manual_seed(1000 * sum(counts) + D)
    num_pages = B * M + 2
    table = torch.randperm(num_pages, generator=g)[:B * M].view(B, M).to(torch.int32)       # every sequence owns all its pages: private, shuffled
    total = sum(counts)
    cu = [0]
    for n in counts:
        cu.append(cu[-1] + n)
    k, v = ((torch.randn(total, HKV, D, generator=g) * 3).to(dtype).to(DEV) for _ in range(2))
    sk = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    sv = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    strides, span = _view(view, total, D)
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
    rsl = ar.carve("seqlens", 4 * B, align=4, role="scratch")
    nb = P.pool_bytes(num_pages, HKV, ps, D)
    assert nb == L.qattn_fp8_tensor_bytes(_native.LAYOUT_KFRAG, num_pages, HKV, ps, D) == L.qattn_fp8_tensor_bytes(_native.LAYOUT_VFRAG, num_pages, HKV, ps, D)
    rik = ar.carve("k_pool", nb, align=16, row_bytes=D, role="scratch")
    riv = ar.carve("v_pool", nb, align=16, row_bytes=D, role="scratch")
    s2 = (ctypes.c_longlong * 2)(*strides[:2])
    # the header's rules, literally
    pos = [min(max(p, 0), CAP) for p in lens]
    end = [min(pos[b] + counts[b], CAP) for b in range(B)]
    mine = torch.zeros(num_pages, HKV, ps, dtype=torch.bool, device=DEV)
    at = [None] * B                                                         # (pages, slots) of sequence b's appended keys, in order
    for b in range(B):
        js = torch.arange(pos[b], end[b])
        at[b] = (table[b].long()[js // ps].to(DEV), (js % ps).to(DEV))
        mine[at[b][0], :, at[b][1]] = True
    pad = lambda x: torch.stack([torch.cat([x[cu[b]:cu[b + 1]], x.new_zeros((max(counts) - counts[b], HKV, D))]).transpose(0, 1) for b in range(B)])
    qk, qv = KC.quant_ref(pad(k), sk, fp8), KC.quant_ref(pad(v), sv, fp8)      # [B, HKV, T, D]
    runs = []
    for hostile, fill in ((True, 0xA5), (False, P.NAN_BYTE[fmt])):
        ar.set_input_guards(hostile)
        rk.load_view(k, strides, hostile=hostile)
        rv.load_view(v, strides, hostile=hostile)
        rik.fill(fill)
        riv.fill(fill)
        rsl.interior.view(torch.int32).copy_(torch.tensor(lens, dtype=torch.int32))
        rc = L.qattn_paged_kv_cache_append_varlen_fp8(rk.ptr, rv.ptr, _native.fmt_of(dtype), s2, s2, rik.ptr, riv.ptr, rsk.ptr, rsv.ptr, rtab.ptr, M,
                                                      rsl.ptr, rcu.ptr, advance, B, HKV, total, num_pages, ps, M, D, _native.fmt_of(fp8), _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.qattn_strerror(rc))
        A.assert_guards_intact(ar)
        assert rsl.interior.view(torch.int32).tolist() == (end if advance else lens)
        rows = []
        for reg, layout, qx in ((rik, KC.KFRAG, qk), (riv, KC.VFRAG, qv)):
            got = KC.from_image(reg.interior, layout, num_pages, HKV, ps, D)
            other = got[~mine]
            assert (other == fill).all(), (f"{reg.name}: {(other != fill).any(-1).sum().item()} keys the call does not append lost their "
                                           f"pre-fill 0x{fill:02x}")
            for b in range(B):
                n = end[b] - pos[b]
                if n:
                    assert torch.equal(got[at[b][0], :, at[b][1]], qx[b, :, :n].transpose(0, 1)), (reg.name, b)
            rows.append(got[mine].clone())
        runs.append(rows)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])   # no appended byte depends on what the pools or the guards held
    # ... and they are the bytes of the ordinary call (the binding on torch tensors) from the same starting state
    kp, vp = (torch.full((nb,), P.NAN_BYTE[fmt], dtype=torch.uint8, device=DEV) for _ in range(2))
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    _native.paged_kv_cache_append_varlen_fp8(kp, vp, sk, sv, table.to(DEV), sl, k, v, torch.tensor(cu, dtype=torch.int32, device=DEV),
                                             num_pages=num_pages, page_size=ps, fp8_dtype=fp8, advance=bool(advance))
    assert torch.equal(kp, rik.interior) and torch.equal(vp, riv.interior) and sl.tolist() == (end if advance else lens)

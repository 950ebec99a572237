"""Buffer contract of qattn_kv_cache_append_fp8 (include/qattn_kvcache.h; sizes, alignment and written bytes: include/qattn_buffers.h): the C
entry through ctypes, every buffer carved from a guarded arena (tests/arena.py) of EXACTLY the documented size at the documented alignment.
After the call every guard is intact; with the images pre-filled once with 0xA5 and once with NaN bytes (0x7f), every byte that does not
belong to an appended key still holds the pre-fill, the appended keys' bytes are the oracle's and the same in both runs, and seqlens is
written only under `advance`.  The inputs are read through strides with hostile pads between their rows."""
import ctypes

import pytest
import torch

from quantumattention_amd import _native
from tests import arena as A
from tests import kvcache_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV, CAP = 2, 2, 200
CASES = [   # D, dtype, fp8 format, T, seqlens, new_lens, input view
    (64, torch.bfloat16, "e4m3", 7, [0, 61], None, "dense"),
    (128, torch.bfloat16, "e4m3", 130, [5, 66], None, "bthd"),
    (128, torch.float16, "e5m2", 1, [63, 199], None, "padded"),
    (256, torch.bfloat16, "e4m3", 4, [127, 2], [0, 3], "bthd"),
    (64, torch.float16, "e4m3", 16, [190, 200], None, "padded"),
    (128, torch.bfloat16, "e5m2", 70, [-5, 250], [70, 70], "dense"),      # seqlens outside [0, capacity]: clamped
]
IDS = ["d64-T7-group-split", "d128-T130-bthd", "d128-fp16-e5m2-T1-padded", "d256-new-lens", "d64-fp16-overflow", "d128-e5m2-clamped-seqlens"]


def _view(kind, T, D):
    """(element strides, span in elements) of a [B, HKV, T, D] view"""
    if kind == "dense":
        return (HKV * T * D, T * D, D, 1), B * HKV * T * D
    if kind == "bthd":
        return (T * HKV * D, D, HKV * D, 1), B * T * HKV * D
    rs = D + 8
    hs = T * rs + 16
    return (HKV * hs, hs, rs, 1), B * HKV * hs


@pytest.mark.parametrize("advance", [1, 0], ids=["advance", "no-advance"])
@pytest.mark.parametrize("D,dtype,fmt,T,lens,new_lens,view", CASES, ids=IDS)
def test_kv_cache_append_fp8(D, dtype, fmt, T, lens, new_lens, view, advance):
    L = _native.lib()
    fp8 = C.FP8[fmt]
    g = torch.Generator().manual_seed(1000 * T + D)
    k, v = ((torch.randn(B, HKV, T, D, generator=g) * 3).to(dtype).to(DEV) for _ in range(2))
    sk = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    sv = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    strides, span = _view(view, T, D)
    ar = A.Arena(DEV)
    rk = ar.carve("k16", span * 2, align=16, row_bytes=2 * D, role="in", kind=A.KIND_OF_DTYPE[dtype])
    rv = ar.carve("v16", span * 2, align=16, row_bytes=2 * D, role="in", kind=A.KIND_OF_DTYPE[dtype])
    rsk = ar.carve("scale_k", 4 * B * HKV, align=4, role="in", kind="fp32")
    rsv = ar.carve("scale_v", 4 * B * HKV, align=4, role="in", kind="fp32")
    rsk.load(sk)
    rsv.load(sv)
    rnl = None
    if new_lens is not None:
        rnl = ar.carve("new_lens", 4 * B, align=4, role="in", kind="int32")
        rnl.load(torch.tensor(new_lens, dtype=torch.int32, device=DEV))
    rsl = ar.carve("seqlens", 4 * B, align=4, role="scratch")
    nk = L.qattn_fp8_tensor_bytes(_native.LAYOUT_KFRAG, B, HKV, CAP, D)
    nv = L.qattn_fp8_tensor_bytes(_native.LAYOUT_VFRAG, B, HKV, CAP, D)
    rik = ar.carve("k8_kfrag", nk, align=16, row_bytes=D, role="scratch")
    riv = ar.carve("v8_vfrag", nv, align=16, row_bytes=D, role="scratch")
    s3 = (ctypes.c_longlong * 3)(*strides[:3])
    # the header's rules, literally
    pos = [min(max(p, 0), CAP) for p in lens]
    cnt = [T if new_lens is None else min(max(new_lens[b], 0), T) for b in range(B)]
    end = [min(pos[b] + cnt[b], CAP) for b in range(B)]
    Sp = (CAP + 63) // 64 * 64
    mine = torch.zeros(B, HKV, Sp, dtype=torch.bool, device=DEV)
    for b in range(B):
        mine[b, :, pos[b]:end[b]] = True
    qk, qv = C.quant_ref(k, sk, fp8), C.quant_ref(v, sv, fp8)
    runs = []
    for hostile, fill in ((True, 0xA5), (False, 0x7F)):
        ar.set_input_guards(hostile)
        rk.load_view(k, strides, hostile=hostile)
        rv.load_view(v, strides, hostile=hostile)
        rik.fill(fill)
        riv.fill(fill)
        rsl.interior.view(torch.int32).copy_(torch.tensor(lens, dtype=torch.int32))
        rc = L.qattn_kv_cache_append_fp8(rk.ptr, rv.ptr, _native.fmt_of(dtype), s3, s3, rik.ptr, riv.ptr, rsk.ptr, rsv.ptr, rsl.ptr,
                                         None if rnl is None else rnl.ptr, advance, B, HKV, T, CAP, D, _native.fmt_of(fp8),
                                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.qattn_strerror(rc))
        A.assert_guards_intact(ar)
        assert rsl.interior.view(torch.int32).tolist() == (end if advance else lens)
        rows = []
        for reg, layout, q in ((rik, C.KFRAG, qk), (riv, C.VFRAG, qv)):
            got = C.from_image(reg.interior, layout, B, HKV, CAP, D)
            other = got[~mine]
            assert (other == fill).all(), (f"{reg.name}: {(other != fill).any(-1).sum().item()} keys the call does not append lost their "
                                           f"pre-fill 0x{fill:02x}")
            for b in range(B):
                assert torch.equal(got[b, :, pos[b]:end[b]], q[b, :, :end[b] - pos[b]]), (reg.name, b)
            rows.append(got[mine].clone())
        runs.append(rows)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])   # no appended byte depends on what the images held

"""Buffer contract of the two paged entries (include/qattn_paged.h; sizes, alignment and written bytes: include/qattn_buffers.h), held the way
tests/test_gpu_splitkv_buffer_contract.py and tests/test_gpu_kvcache_buffer_contract.py hold the contiguous ones: the C entries through
ctypes, every caller-provided buffer carved from a guarded arena (tests/arena.py) of EXACTLY the documented size at the documented
alignment.  After the call every guard is intact, every output is bit-equal to the ordinary call, the workspace size function suffices and
no bit depends on what the workspace (or, for the append, the pool) held.  The tables are the shared ones of tests/paged_cases.py: every
entry is a valid page, the unread ones point at the NaN page."""
import ctypes

import pytest
import torch

from quantumattention_amd import _native
from tests import arena as A
from tests import kvcache_cases as KC
from tests import paged_cases as P
from tests.test_gpu_buffer_contract import ALIGN1, ALIGN4, ALIGN16, Plan, _kind, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV, CAP = P.B, P.HKV, P.CAP
CFGS = [   # D, dtype, fp8 format, page size, shared table, G, Sq, causal, precision
    (64, torch.bfloat16, "e4m3", 64, 0, 2, 5, True, "accurate"),
    (128, torch.bfloat16, "e4m3", 128, 1, 4, 1, False, "fast"),
    (128, torch.float16, "e5m2", 256, 2, 1, 3, True, "fast"),
    (256, torch.bfloat16, "e4m3", 64, 3, 1, 1, False, "accurate"),
]
CFG_IDS = ["d64-ps64-gqa", "d128-ps128-decode", "d128-fp16-e5m2-ps256", "d256-ps64"]


def _pools(t, D, fmt, seed):
    rk, rv = P.random_rows(t.num_pages, t.page_size, D, fmt, seed, DEV)
    rk[P.POISON], rv[P.POISON] = P.NAN_BYTE[fmt], P.NAN_BYTE[fmt]
    fp8 = P.FP8[fmt]
    return _native.pack_fp8(rk.view(fp8), _native.LAYOUT_KFRAG), _native.pack_fp8(rv.view(fp8), _native.LAYOUT_VFRAG)


@pytest.mark.parametrize("ns", [1, 3, 9])
@pytest.mark.parametrize("D,dtype,fmt,ps,ti,G,Sq,causal,precision", CFGS, ids=CFG_IDS)
def test_fp8_attention_paged_splitkv_forward(D, dtype, fmt, ps, ti, G, Sq, causal, precision, ns):
    L = _native.lib()
    t = P.shared_tables(ps)[ti]
    kp, vp = _pools(t, D, fmt, 1000 * Sq + D)
    Hq = HKV * G
    g = torch.Generator().manual_seed(10 * D + Sq)
    q = (torch.randn(B, Hq, Sq, D, generator=g) * 1.5).to(dtype).to(DEV)
    sk = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    sv = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    table = torch.tensor(t.table, dtype=torch.int32, device=DEV)
    su = torch.tensor(t.lens, dtype=torch.int32, device=DEV)
    w = _native.fp8_attention_paged_splitkv(q, kp, vp, sk, sv, table, su, Skv=CAP, num_pages=t.num_pages, page_size=ps, fp8_dtype=P.FP8[fmt],
                                            is_causal=causal, precision=precision, num_splits=ns, return_lse=True, return_partials=True,
                                            return_quant=True, return_path=True)
    wo, wl, wpo, wpl, wpp, wq8, wsq, wpath = w
    rows = B * Hq * Sq
    p = Plan()
    pq = p.inp("q", q, row_bytes=2 * D)
    assert kp.numel() == L.qattn_fp8_tensor_bytes(_native.LAYOUT_KFRAG, t.num_pages, HKV, ps, D) == P.pool_bytes(t.num_pages, HKV, ps, D)
    pk = p.inp("k_pool", kp, row_bytes=D)
    pv = p.inp("v_pool", vp, row_bytes=D)
    ptab = p.inp("block_table", table, align=ALIGN4)
    psk, psv = p.inp("scale_k", sk, align=ALIGN4), p.inp("scale_v", sv, align=ALIGN4)
    psu = p.inp("seqused_k", su, align=ALIGN4)
    po = p.out("out", 2 * rows * D, _kind(dtype), row_bytes=2 * D)
    pl = p.out("lse", 4 * rows, "fp32", align=ALIGN4)
    pq8 = p.out("q8", L.qattn_fp8_tensor_bytes(_native.LAYOUT_ROWMAJOR, B, Hq, Sq, D), "fp8", row_bytes=D)
    psq = p.out("scale_q", 4 * B * Hq, "fp32", align=ALIGN4)
    ppath = p.out("row_path", rows, "path", align=ALIGN1)
    expected = {"out": wo, "lse": wl, "q8": wq8, "scale_q": wsq, "row_path": wpath}
    ppo = ppl = ppp = None
    if ns > 1:
        ppo = p.out("partial_o", 4 * ns * rows * D, "fp32", row_bytes=4 * D)
        ppl = p.out("partial_lse", 4 * ns * rows, "fp32", align=ALIGN4)
        ppp = p.out("partial_path", ns * rows, "path", align=ALIGN1)
        expected.update(partial_o=wpo, partial_lse=wpl, partial_path=wpp)
    wb = L.qattn_fp8_attention_paged_splitkv_workspace_bytes(B, Hq, HKV, Sq, CAP, D, ns)
    pw = p.scratch("workspace", wb, align=ALIGN16)
    p.check(lambda: L.qattn_fp8_attention_paged_splitkv_forward(
        pq, _native.fmt_of(dtype), pk, pv, ptab, t.M, t.num_pages, ps, t.M, psk, psv, po, pl, psu, B, Hq, HKV, Sq, CAP, D, _native.fmt_of(P.FP8[fmt]),
        0, int(causal), 0.0, _native.PRECISION[precision], ns, pq8, psq, ppath, ppo, ppl, ppp, pw, wb, _stream()), expected)


APPEND_CASES = [   # D, dtype, fp8 format, page size, T, seqlens, new_lens, input view
    (64, torch.bfloat16, "e4m3", 64, 7, [0, 61, 125], None, "dense"),
    (128, torch.bfloat16, "e4m3", 64, 130, [5, 66, 1000], None, "bthd"),
    (128, torch.float16, "e5m2", 128, 1, [63, 127, 1279], None, "padded"),
    (256, torch.bfloat16, "e4m3", 256, 4, [255, 2, 510], [0, 3, 4], "bthd"),
    (64, torch.float16, "e4m3", 128, 16, [1270, 1280, 100], None, "padded"),
    (128, torch.bfloat16, "e5m2", 256, 70, [-5, 1300, 200], [70, 70, 1], "dense"),      # seqlens outside [0, capacity]: clamped
]
APPEND_IDS = ["d64-ps64-T7", "d128-ps64-T130-bthd", "d128-fp16-e5m2-ps128-T1", "d256-ps256-new-lens", "d64-fp16-overflow", "d128-e5m2-clamped-seqlens"]


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
@pytest.mark.parametrize("D,dtype,fmt,ps,T,lens,new_lens,view", APPEND_CASES, ids=APPEND_IDS)
def test_paged_kv_cache_append_fp8(D, dtype, fmt, ps, T, lens, new_lens, view, advance):
    L = _native.lib()
    fp8 = P.FP8[fmt]
    M = CAP // ps
    t = P.Tables(ps, (CAP,) * B, seed=T, need=[M] * B)                     # every sequence owns all its pages: private, shuffled
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
    rtab = ar.carve("block_table", 4 * B * M, align=4, role="in", kind="int32")
    rtab.load(torch.tensor(t.table, dtype=torch.int32, device=DEV))
    rnl = None
    if new_lens is not None:
        rnl = ar.carve("new_lens", 4 * B, align=4, role="in", kind="int32")
        rnl.load(torch.tensor(new_lens, dtype=torch.int32, device=DEV))
    rsl = ar.carve("seqlens", 4 * B, align=4, role="scratch")
    nb = P.pool_bytes(t.num_pages, HKV, ps, D)
    assert nb == L.qattn_fp8_tensor_bytes(_native.LAYOUT_KFRAG, t.num_pages, HKV, ps, D) == L.qattn_fp8_tensor_bytes(_native.LAYOUT_VFRAG, t.num_pages, HKV, ps, D)
    rik = ar.carve("k_pool", nb, align=16, row_bytes=D, role="scratch")
    riv = ar.carve("v_pool", nb, align=16, row_bytes=D, role="scratch")
    s3 = (ctypes.c_longlong * 3)(*strides[:3])
    # the header's rules, literally
    pos = [min(max(p, 0), CAP) for p in lens]
    cnt = [T if new_lens is None else min(max(new_lens[b], 0), T) for b in range(B)]
    end = [min(pos[b] + cnt[b], CAP) for b in range(B)]
    mine = torch.zeros(t.num_pages, HKV, ps, dtype=torch.bool, device=DEV)
    at = [[], [], []]                                                       # (pages, slots) of sequence b's appended keys, in order
    for b in range(B):
        js = torch.arange(pos[b], end[b])
        at[b] = (torch.tensor(t.table[b], dtype=torch.long)[js // ps].to(DEV), (js % ps).to(DEV))
        mine[at[b][0], :, at[b][1]] = True
    qk, qv = KC.quant_ref(k, sk, fp8), KC.quant_ref(v, sv, fp8)
    runs = []
    for hostile, fill in ((True, 0xA5), (False, P.NAN_BYTE[fmt])):
        ar.set_input_guards(hostile)
        rk.load_view(k, strides, hostile=hostile)
        rv.load_view(v, strides, hostile=hostile)
        rik.fill(fill)
        riv.fill(fill)
        rsl.interior.view(torch.int32).copy_(torch.tensor(lens, dtype=torch.int32))
        rc = L.qattn_paged_kv_cache_append_fp8(rk.ptr, rv.ptr, _native.fmt_of(dtype), s3, s3, rik.ptr, riv.ptr, rsk.ptr, rsv.ptr, rtab.ptr, M, rsl.ptr,
                                               None if rnl is None else rnl.ptr, advance, B, HKV, T, t.num_pages, ps, M, D, _native.fmt_of(fp8),
                                               _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.qattn_strerror(rc))
        A.assert_guards_intact(ar)
        assert rsl.interior.view(torch.int32).tolist() == (end if advance else lens)
        rows = []
        for reg, layout, qx in ((rik, KC.KFRAG, qk), (riv, KC.VFRAG, qv)):
            got = KC.from_image(reg.interior, layout, t.num_pages, HKV, ps, D)
            other = got[~mine]
            assert (other == fill).all(), (f"{reg.name}: {(other != fill).any(-1).sum().item()} keys the call does not append lost their "
                                           f"pre-fill 0x{fill:02x}")
            for b in range(B):
                n = end[b] - pos[b]
                if n:
                    assert torch.equal(got[at[b][0], :, at[b][1]], qx[b, :, :n].transpose(0, 1)), (reg.name, b)
            rows.append(got[mine].clone())
        runs.append(rows)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])   # no appended byte depends on what the pools held

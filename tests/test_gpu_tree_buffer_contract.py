"""Buffer contract of the two entries of include/qattn_paged_varlen_tree.h, held the way tests/test_gpu_paged_buffer_contract.py holds the
paged ones: the C entries through ctypes, every caller-provided buffer carved from a guarded arena (tests/arena.py) of EXACTLY the size
the header states at the alignment it states (tree_mask: 8 bytes; the int32 tensors: 4; pools, q, out, workspace: 16).  After the call
every guard is intact, every output is bit-equal to the ordinary call, nothing the contract says is written is left unwritten, and no bit
depends on what the workspace held or on bytes outside the inputs.  Shapes, tables and trees: tests/tree_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

from quantumattention_amd import _native
from tests import arena as A
from tests import paged_cases as P
from tests import paged_varlen_cases as V
from tests import tree_cases as T
from tests.test_gpu_buffer_contract import ALIGN1, ALIGN4, ALIGN16, Plan, _kind, _stream
from tests.test_gpu_paged_buffer_contract import _pools

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV, CAP = T.B, T.HKV, T.CAP
ALIGN8 = 8
CFGS = [   # case, D, dtype, fp8 format, page size, tree, precision
    ("A", 128, torch.bfloat16, "e4m3", 64, "random", "fast"),
    ("B", 64, torch.float16, "e5m2", 128, "binary", "accurate"),
    ("C", 128, torch.bfloat16, "e4m3", 256, "star", "accurate"),
    ("D", 256, torch.bfloat16, "e4m3", 64, "random", "fast"),
]
CFG_IDS = ["A-d128-ps64", "B-d64-fp16-e5m2-ps128", "C-d128-ps256-g1", "D-d256-ps64"]


def _i32(x):
    return torch.tensor(np.asarray(x), dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("name,D,dtype,fmt,ps,kind,precision", CFGS, ids=CFG_IDS)
def test_fp8_attention_paged_varlen_tree_forward(name, D, dtype, fmt, ps, kind, precision, ns):
    L = _native.lib()
    G, sq, lens = T.CASES[name]
    t = T.tables(name, ps, 3)
    kp, vp = _pools(t, D, fmt, 1000 + D)
    Hq, total, mx = HKV * G, sum(sq), max(sq)
    g = torch.Generator().manual_seed(10 * D + ns)
    q = (torch.randn(total, Hq, D, generator=g) * 1.5).to(dtype).to(DEV)
    sk = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    sv = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    table, su, cu = _i32(t.table), _i32(lens), _i32(V.cu_of(sq))
    words = torch.from_numpy(T.as_int64(T.words_of(kind, sq, 5)[0])).to(DEV)
    w = _native.fp8_attention_paged_varlen(q, kp, vp, sk, sv, table, su, cu, max_seqlen_q=mx, Skv=CAP, num_pages=t.num_pages, page_size=ps,
                                           fp8_dtype=P.FP8[fmt], precision=precision, num_splits=ns, return_lse=True, return_partials=True,
                                           return_quant=True, return_path=True, tree_mask=words)
    wo, wl, wpo, wpl, wpp, wq8, wsq, wpath = w
    rows = Hq * total
    p = Plan()
    pq = p.inp("q", q, row_bytes=2 * D)
    pk, pv = p.inp("k_pool", kp, row_bytes=D), p.inp("v_pool", vp, row_bytes=D)
    ptab = p.inp("block_table", table, align=ALIGN4)
    psk, psv = p.inp("scale_k", sk, align=ALIGN4), p.inp("scale_v", sv, align=ALIGN4)
    psu, pcu = p.inp("seqused_k", su, align=ALIGN4), p.inp("cu_seqlens_q", cu, align=ALIGN4)
    pw64 = p.inp("tree_mask", words.view(torch.int32), align=ALIGN8)          # [total_q] 64-bit words: 8 total_q bytes at 8-byte alignment
    po = p.out("out", 2 * rows * D, _kind(dtype), row_bytes=2 * D)
    pl = p.out("lse", 4 * rows, "fp32", align=ALIGN4)
    pq8 = p.out("q8", rows * D, "fp8", row_bytes=D)
    psq = p.out("scale_q", 4 * B * Hq, "fp32", align=ALIGN4)
    ppath = p.out("row_path", rows, "path", align=ALIGN1)
    expected = {"out": wo, "lse": wl, "q8": wq8, "scale_q": wsq, "row_path": wpath}
    ppo = ppl = ppp = None
    if ns > 1:
        ppo = p.out("partial_o", 4 * ns * rows * D, "fp32", row_bytes=4 * D)
        ppl = p.out("partial_lse", 4 * ns * rows, "fp32", align=ALIGN4)
        ppp = p.out("partial_path", ns * rows, "path", align=ALIGN1)
        expected.update(partial_o=wpo, partial_lse=wpl, partial_path=wpp)
    wb = L.qattn_fp8_attention_paged_varlen_workspace_bytes(B, Hq, HKV, total, CAP, D, ns)
    pw = p.scratch("workspace", wb, align=ALIGN16)
    s2 = (ctypes.c_longlong * 2)(Hq * D, D)
    p.check(lambda: L.qattn_fp8_attention_paged_varlen_tree_forward(
        pq, s2, _native.fmt_of(dtype), pk, pv, ptab, t.M, t.num_pages, ps, t.M, psk, psv, po, pl, pcu, psu, B, Hq, HKV, total, mx, CAP, D,
        _native.fmt_of(P.FP8[fmt]), 0, pw64, 0.0, _native.PRECISION[precision], ns, pq8, psq, ppath, ppo, ppl, ppp, pw, wb, _stream()), expected)


@pytest.mark.parametrize("accept", ["path", "wild"])
@pytest.mark.parametrize("name,D,dtype,fmt,ps,kind,precision", CFGS, ids=CFG_IDS)
def test_paged_kv_cache_compact_fp8(name, D, dtype, fmt, ps, kind, precision, accept):
    """the pools and seqlens are read AND written: carved as scratch, loaded before each run, compared byte for byte with the ordinary call
    on the same contents -- which the tests of tests/test_gpu_tree.py hold to the rule"""
    L = _native.lib()
    G, sq, lens = T.CASES[name]
    t = T.tables(name, ps, 4)
    kp, vp = _pools(t, D, fmt, 2000 + D)
    cu = V.cu_of(sq)
    idx, cnt = T.accept_lists(sq, 7, accept)
    table = _i32(t.table)
    wk, wv, wl = kp.clone(), vp.clone(), _i32(lens)
    _native.paged_kv_cache_compact_fp8(wk, wv, table, wl, _i32(cu), _i32(idx), _i32(cnt), Hkv=HKV, D=D, num_pages=t.num_pages, page_size=ps)
    assert wl.tolist() != list(lens) or all(not (1 <= n <= 64 and Lb >= n) for n, Lb in zip(sq, lens))
    ar = A.Arena(DEV)
    rtab = ar.carve("block_table", 4 * B * t.M, align=4, role="in", kind="int32")
    rtab.load(table)
    rcu = ar.carve("cu_seqlens", 4 * (B + 1), align=4, role="in", kind="int32")
    rcu.load(_i32(cu))
    rai = ar.carve("accept_index", 4 * sum(sq), align=4, role="in", kind="int32")
    rai.load(_i32(idx))
    ral = ar.carve("accept_lens", 4 * B, align=4, role="in", kind="int32")
    ral.load(_i32(cnt))
    rsl = ar.carve("seqlens", 4 * B, align=4, role="scratch")
    nb = P.pool_bytes(t.num_pages, HKV, ps, D)
    assert nb == kp.numel() == vp.numel()
    rk = ar.carve("k_pool", nb, align=16, row_bytes=D, role="scratch")
    rv = ar.carve("v_pool", nb, align=16, row_bytes=D, role="scratch")
    for hostile in (True, False):
        ar.set_input_guards(hostile)
        rk.load(kp)
        rv.load(vp)
        rsl.load(_i32(lens))
        rc = L.qattn_paged_kv_cache_compact_fp8(rk.ptr, rv.ptr, rtab.ptr, t.M, rsl.ptr, rcu.ptr, rai.ptr, ral.ptr, B, HKV, sum(sq), t.num_pages, ps, t.M,
                                                D, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.qattn_strerror(rc))
        A.assert_guards_intact(ar)
        assert rsl.interior.view(torch.int32).tolist() == wl.tolist()
        assert torch.equal(rk.interior, wk) and torch.equal(rv.interior, wv), hostile

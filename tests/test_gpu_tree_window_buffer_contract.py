"""Buffer contract of qattn_fp8_attention_paged_varlen_tree_window_forward (include/qattn_paged_varlen_tree_window.h), held the way
tests/test_gpu_tree_buffer_contract.py holds the tree entry: the C entry through ctypes, every caller-provided buffer carved from a
guarded arena (tests/arena.py) of EXACTLY the size the header states at the alignment it states (tree_mask: 8 bytes; sinks and the int32
tensors: 4; pools, q, out, workspace: 16).  After the call every guard is intact, every output is bit-equal to the ordinary call, nothing
the contract says is written is left unwritten, and no bit depends on what the workspace held or on bytes outside the inputs.  The
argument checks return their codes before any launch.  Shapes, tables and trees: tests/tree_window_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

from quantumattention_amd import _native
from tests import paged_cases as P
from tests import paged_varlen_cases as V
from tests import tree_cases as T
from tests import tree_window_cases as W
from tests.test_gpu_buffer_contract import ALIGN1, ALIGN4, ALIGN16, Plan, _kind, _stream
from tests.test_gpu_paged_buffer_contract import _pools

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV, CAP = W.B, W.HKV, W.CAP
ALIGN8 = 8
CFGS = [   # case, D, dtype, fp8 format, page size, tree, precision, window, sinks
    ("A", 128, torch.bfloat16, "e4m3", 64, "random", "fast", (127, 0), True),
    ("B", 64, torch.float16, "e5m2", 128, "binary", "accurate", (63, 0), False),
    ("C", 128, torch.bfloat16, "e4m3", 256, "star", "accurate", (-1, 0), True),
    ("E", 256, torch.bfloat16, "e4m3", 64, "random", "fast", (1100, 0), False),
    ("E", 64, torch.bfloat16, "e4m3", 128, "binary", "accurate", (127, 0), True),
]
CFG_IDS = ["A-d128-ps64-w127-sinks", "B-d64-fp16-e5m2-ps128-w63", "C-d128-ps256-g1-full-sinks", "E-d256-ps64-w1100", "E-d64-ps128-w127-sinks"]


def _i32(x):
    return torch.tensor(np.asarray(x), dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("name,D,dtype,fmt,ps,kind,precision,window,with_sinks", CFGS, ids=CFG_IDS)
def test_fp8_attention_paged_varlen_tree_window_forward(name, D, dtype, fmt, ps, kind, precision, window, with_sinks, ns):
    L = _native.lib()
    G, sq, lens = W.CASES[name]
    t = W.tables(name, ps, 3)
    kp, vp = _pools(t, D, fmt, 1000 + D)
    Hq, total, mx = HKV * G, sum(sq), max(sq)
    g = torch.Generator().manual_seed(10 * D + ns)
    q = (torch.randn(total, Hq, D, generator=g) * 1.5).to(dtype).to(DEV)
    sk = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    sv = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    sinks = (torch.randn(Hq, generator=g) * 1.5).to(DEV) if with_sinks else None
    table, su, cu = _i32(t.table), _i32(lens), _i32(V.cu_of(sq))
    words = torch.from_numpy(T.as_int64(T.words_of(kind, sq, 5)[0])).to(DEV)
    w = _native.fp8_attention_paged_varlen(q, kp, vp, sk, sv, table, su, cu, max_seqlen_q=mx, Skv=CAP, num_pages=t.num_pages, page_size=ps,
                                           fp8_dtype=P.FP8[fmt], precision=precision, num_splits=ns, return_lse=True, return_partials=True,
                                           return_quant=True, return_path=True, tree_mask=words, window=window, sinks=sinks)
    wo, wl, wpo, wpl, wpp, wq8, wsq, wpath = w
    rows = Hq * total
    p = Plan()
    pq = p.inp("q", q, row_bytes=2 * D)
    pk, pv = p.inp("k_pool", kp, row_bytes=D), p.inp("v_pool", vp, row_bytes=D)
    ptab = p.inp("block_table", table, align=ALIGN4)
    psk, psv = p.inp("scale_k", sk, align=ALIGN4), p.inp("scale_v", sv, align=ALIGN4)
    psu, pcu = p.inp("seqused_k", su, align=ALIGN4), p.inp("cu_seqlens_q", cu, align=ALIGN4)
    pw64 = p.inp("tree_mask", words.view(torch.int32), align=ALIGN8)          # [total_q] 64-bit words: 8 total_q bytes at 8-byte alignment
    psn = p.inp("sinks", sinks, align=ALIGN4) if with_sinks else None          # [Hq] fp32: 4 Hq bytes at 4-byte alignment
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
    p.check(lambda: L.qattn_fp8_attention_paged_varlen_tree_window_forward(
        pq, s2, _native.fmt_of(dtype), pk, pv, ptab, t.M, t.num_pages, ps, t.M, psk, psv, po, pl, pcu, psu, B, Hq, HKV, total, mx, CAP, D,
        _native.fmt_of(P.FP8[fmt]), 0, pw64, window[0], window[1], psn, 0.0, _native.PRECISION[precision], ns, pq8, psq, ppath, ppo, ppl, ppp, pw,
        wb, _stream()), expected)


def test_the_argument_checks_return_their_codes_before_any_launch():
    """null-page addresses that are never dereferenced: a failing check returns first, and a call that passes every check without a
    workspace returns QATTN_ERR_WORKSPACE -- still before any device call"""
    L = _native.lib()
    p = 0x1000
    s2 = (ctypes.c_longlong * 2)(8 * 128, 128)

    def att(tree_mask=p, left=127, right=0, sinks=None, block_table=p, page_size=64, Hq=8, D=128, num_splits=1, q=p):
        return L.qattn_fp8_attention_paged_varlen_tree_window_forward(q, s2, _native.FMT_BF16, p, p, block_table, 20, 62, page_size, 20, p, p, p, None,
                                                                      p, p, 3, Hq, 2, 10, 4, 1280, D, _native.fmt_of(torch.float8_e4m3fn), 0,
                                                                      tree_mask, left, right, sinks, 0.0, 2, num_splits, None, None, None, None,
                                                                      None, None, None, 0, None)
    INVALID = att(block_table=None)
    assert INVALID != 0
    for kw in (dict(tree_mask=None), dict(tree_mask=p + 4), dict(left=62), dict(left=0), dict(left=-2), dict(right=1), dict(right=-1),
               dict(sinks=p + 2), dict(sinks=p + 1, left=-1), dict(page_size=96), dict(num_splits=65), dict(q=None)):
        assert att(**kw) == INVALID, kw
    assert att(D=96) not in (0, INVALID) and att(Hq=7) == att(D=96)     # QATTN_ERR_UNSUPPORTED_DIM
    for kw in (dict(), dict(left=63), dict(left=-1), dict(sinks=p), dict(left=1 << 30)):
        assert att(**kw) not in (0, INVALID, att(D=96)), kw             # QATTN_ERR_WORKSPACE

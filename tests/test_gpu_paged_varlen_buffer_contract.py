"""Buffer contract of qattn_fp8_attention_paged_varlen_forward (include/qattn_paged_varlen.h; sizes, alignment and written bytes:
include/qattn_buffers.h), held the way tests/test_gpu_paged_buffer_contract.py holds the dense paged entry: the C entry through ctypes,
every caller-provided buffer carved from a guarded arena (tests/arena.py) of EXACTLY the documented size at the documented alignment.
After the call every guard is intact, every output is bit-equal to the ordinary call, every described element is written, the workspace
size function suffices and no bit depends on what the workspace held.  Tables and cu_seqlens_q are consistent (cu[B] = total_q): every
token belongs to a sequence.  The tables are the shared ones of tests/paged_cases.py, the query counts tests/paged_varlen_cases.py's."""
import ctypes

import pytest
import torch

from quantumattention_amd import _native
from tests import paged_cases as P
from tests import paged_varlen_cases as V
from tests.test_gpu_buffer_contract import ALIGN1, ALIGN4, ALIGN16, Plan, _kind, _stream
from tests.test_gpu_paged_buffer_contract import _pools

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV, CAP = P.B, P.HKV, P.CAP
CFGS = [   # D, dtype, fp8 format, page size, shared table, query pair, causal, precision, q view
    (64, torch.bfloat16, "e4m3", 64, 0, 2, True, "accurate", "dense"),
    (128, torch.bfloat16, "e4m3", 128, 1, 0, False, "fast", "qkv"),
    (128, torch.float16, "e5m2", 256, 2, 1, True, "fast", "dense"),
    (256, torch.bfloat16, "e4m3", 64, 3, 3, True, "accurate", "qkv"),
]
CFG_IDS = ["d64-ps64-gqa-two-tiles", "d128-ps128-idle-slot-strided", "d128-fp16-e5m2-ps256-g1", "d256-ps64-equal-strided"]


@pytest.mark.parametrize("ns", [1, 3, 9])
@pytest.mark.parametrize("D,dtype,fmt,ps,ti,qi,causal,precision,view", CFGS, ids=CFG_IDS)
def test_fp8_attention_paged_varlen_forward(D, dtype, fmt, ps, ti, qi, causal, precision, view, ns):
    L = _native.lib()
    t = P.shared_tables(ps)[ti]
    G, sq = V.QCASES[qi]
    Hq, total = HKV * G, sum(sq)
    kp, vp = _pools(t, D, fmt, 1000 * qi + D)
    g = torch.Generator().manual_seed(10 * D + qi)
    q = (torch.randn(total, Hq, D, generator=g) * 1.5).to(dtype).to(DEV)
    sk = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    sv = (torch.rand(B, HKV, generator=g) * 0.02 + 0.005).to(DEV)
    table = torch.tensor(t.table, dtype=torch.int32, device=DEV)
    su = torch.tensor(t.lens, dtype=torch.int32, device=DEV)
    cu = torch.tensor(V.cu_of(sq), dtype=torch.int32, device=DEV)
    w = _native.fp8_attention_paged_varlen(q, kp, vp, sk, sv, table, su, cu, max_seqlen_q=max(sq), Skv=CAP, num_pages=t.num_pages, page_size=ps,
                                           fp8_dtype=P.FP8[fmt], is_causal=causal, precision=precision, num_splits=ns, return_lse=True,
                                           return_partials=True, return_quant=True, return_path=True)
    wo, wl, wpo, wpl, wpp, wq8, wsq, wpath = w
    rows = Hq * total
    p = Plan()
    if view == "dense":
        pq, s2 = p.inp("q", q, row_bytes=2 * D), None
    else:                      # the q slice of a [total_q, 3, Hq, D] projection: only q's rows are the call's to read
        strides = (3 * Hq * D, D, 1)
        pq = p.inp_view("q", q, strides, (total - 1) * 3 * Hq * D + Hq * D, row_bytes=2 * D)
        s2 = (ctypes.c_longlong * 2)(*strides[:2])
    pk = p.inp("k_pool", kp, row_bytes=D)
    pv = p.inp("v_pool", vp, row_bytes=D)
    ptab = p.inp("block_table", table, align=ALIGN4)
    psk, psv = p.inp("scale_k", sk, align=ALIGN4), p.inp("scale_v", sv, align=ALIGN4)
    psu = p.inp("seqused_k", su, align=ALIGN4)
    pcu = p.inp("cu_seqlens_q", cu, align=ALIGN4)
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
    assert wb > 0
    pw = p.scratch("workspace", wb, align=ALIGN16)
    p.check(lambda: L.qattn_fp8_attention_paged_varlen_forward(
        pq, s2, _native.fmt_of(dtype), pk, pv, ptab, t.M, t.num_pages, ps, t.M, psk, psv, po, pl, pcu, psu, B, Hq, HKV, total, max(sq), CAP, D,
        _native.fmt_of(P.FP8[fmt]), 0, int(causal), 0.0, _native.PRECISION[precision], ns, pq8, psq, ppath, ppo, ppl, ppp, pw, wb, _stream()),
        expected)

"""Buffer contract of the three soft-cap C entries (include/qattn_softcap.h; sizes, alignment and written bytes: include/qattn_buffers.h),
held the way tests/test_gpu_sinks_buffer_contract.py holds the sink entries: the C entry through ctypes, every caller-provided buffer carved
from a guarded arena (tests/arena.py) of EXACTLY the documented size at the documented alignment -- softcap itself travels by value.  After
the call every guard is intact, every output is bit-equal to the ordinary call, every described element is written, the siblings'
workspace size functions suffice and no bit depends on what lies outside the described inputs."""
import ctypes
import gc

import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import paged_cases as P
from tests import paged_varlen_cases as V
from tests.test_gpu_buffer_contract import ALIGN4, ALIGN16, Plan, _stream
from tests.test_gpu_paged_buffer_contract import _pools
from tests.test_gpu_splitkv_window_buffer_contract import _outs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """This module's device memory goes back to the driver when its last test is done: tests later in the suite measure a call's
    peak allocation against the caching allocator's state (tests/test_gpu_window.py), and cached blocks of this module's sizes would be
    handed out whole to their smaller requests."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

DEV = "cuda"
B, HKV, CAP = P.B, P.HKV, P.CAP


CONTIG = [   # D, dtype, B, Hq, Hkv, Sq, Skv, used, window, precision, softcap
    (64, torch.bfloat16, 2, 4, 2, 5, 1100, [1100, 65], (127, 0), "accurate", 2.0),
    (128, torch.bfloat16, 1, 8, 2, 1, 1100, None, (-1, 0), "fast", 30.0),
    (128, torch.float16, 2, 4, 4, 130, 1100, [1036, 0], (200, 37), "fast", 0.5),
    (256, torch.bfloat16, 1, 8, 1, 130, 130, [77], (0, 0), "accurate", 50.0),
]
CONTIG_IDS = ["d64-gqa-seqused-window", "d128-decode-full-layer-grok", "d128-fp16-two-tiles-band", "d256-gemma2-one-key-rows-without-key"]


@pytest.mark.parametrize("ns", [1, 3, 9])
@pytest.mark.parametrize("D,dtype,Bn,Hq,Hkv,Sq,Skv,used,window,precision,cap", CONTIG, ids=CONTIG_IDS)
def test_fp8_attention_splitkv_softcap_forward(D, dtype, Bn, Hq, Hkv, Sq, Skv, used, window, precision, cap, ns):
    L = _native.lib()
    g = torch.Generator().manual_seed(1000 * Sq + 10 * Skv + D)
    q = torch.randn(Bn, Hq, Sq, D, generator=g).to(dtype).to(DEV)
    k, v = (torch.randn(Bn, Hkv, Skv, D, generator=g).to(dtype).to(DEV) for _ in range(2))
    kv = qa.prepare_kv_fp8(k, v)
    su = None if used is None else torch.tensor(used, dtype=torch.int32, device=DEV)
    w = _native.fp8_attention_splitkv(q, kv.k, kv.v, kv.scale_k, kv.scale_v, Skv=Skv, window=window, softcap=cap, precision=precision, num_splits=ns,
                                      seqused_k=su, return_lse=True, return_partials=True, return_quant=True, return_path=True)
    rows = Bn * Hq * Sq
    p = Plan()
    pq = p.inp("q", q, row_bytes=2 * D)
    pk = p.inp("k8", kv.k, row_bytes=D)
    pv = p.inp("v8", kv.v, row_bytes=D)
    psk, psv = p.inp("scale_k", kv.scale_k, align=ALIGN4), p.inp("scale_v", kv.scale_v, align=ALIGN4)
    psu = None if su is None else p.inp("seqused_k", su, align=ALIGN4)
    po, pl, pq8, psq, ppath, ppo, ppl, ppp, expected = _outs(p, dtype, rows, D, L.qattn_fp8_tensor_bytes(_native.LAYOUT_ROWMAJOR, Bn, Hq, Sq, D),
                                                             Bn * Hq, ns, w)
    wb = L.qattn_fp8_attention_splitkv_workspace_bytes(Bn, Hq, Hkv, Sq, Skv, D, ns)
    pw = p.scratch("workspace", wb, align=ALIGN16)
    p.check(lambda: L.qattn_fp8_attention_splitkv_softcap_forward(
        pq, _native.fmt_of(dtype), pk, pv, psk, psv, po, pl, psu, Bn, Hq, Hkv, Sq, Skv, D, _native.FMT_E4M3, 0, window[0], window[1], cap, 0.0,
        _native.PRECISION[precision], ns, pq8, psq, ppath, ppo, ppl, ppp, pw, wb, _stream()), expected)


PAGED = [   # D, dtype, fp8 format, page size, shared table, G, Sq, window, precision, softcap
    (64, torch.bfloat16, "e4m3", 64, 0, 2, 5, (127, 0), "accurate", 2.0),
    (128, torch.bfloat16, "e4m3", 128, 1, 4, 1, (-1, 0), "fast", 30.0),
    (128, torch.float16, "e5m2", 256, 2, 1, 3, (840, 5), "fast", 0.5),
    (256, torch.bfloat16, "e4m3", 64, 3, 4, 40, (200, 0), "accurate", 50.0),
]
PAGED_IDS = ["d64-ps64-window", "d128-ps128-decode-full-layer-grok", "d128-fp16-e5m2-ps256-edge-on-page", "d256-ps64-gemma2-tile-crosses-heads"]


@pytest.mark.parametrize("ns", [1, 3, 9])
@pytest.mark.parametrize("D,dtype,fmt,ps,ti,G,Sq,window,precision,cap", PAGED, ids=PAGED_IDS)
def test_fp8_attention_paged_splitkv_softcap_forward(D, dtype, fmt, ps, ti, G, Sq, window, precision, cap, ns):
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
                                            window=window, softcap=cap, precision=precision, num_splits=ns, return_lse=True, return_partials=True,
                                            return_quant=True, return_path=True)
    rows = B * Hq * Sq
    p = Plan()
    pq = p.inp("q", q, row_bytes=2 * D)
    pk = p.inp("k_pool", kp, row_bytes=D)
    pv = p.inp("v_pool", vp, row_bytes=D)
    ptab = p.inp("block_table", table, align=ALIGN4)
    psk, psv = p.inp("scale_k", sk, align=ALIGN4), p.inp("scale_v", sv, align=ALIGN4)
    psu = p.inp("seqused_k", su, align=ALIGN4)
    po, pl, pq8, psq, ppath, ppo, ppl, ppp, expected = _outs(p, dtype, rows, D, L.qattn_fp8_tensor_bytes(_native.LAYOUT_ROWMAJOR, B, Hq, Sq, D),
                                                             B * Hq, ns, w)
    wb = L.qattn_fp8_attention_paged_splitkv_workspace_bytes(B, Hq, HKV, Sq, CAP, D, ns)
    assert wb > 0
    pw = p.scratch("workspace", wb, align=ALIGN16)
    p.check(lambda: L.qattn_fp8_attention_paged_splitkv_softcap_forward(
        pq, _native.fmt_of(dtype), pk, pv, ptab, t.M, t.num_pages, ps, t.M, psk, psv, po, pl, psu, B, Hq, HKV, Sq, CAP, D,
        _native.fmt_of(P.FP8[fmt]), 0, window[0], window[1], cap, 0.0, _native.PRECISION[precision], ns, pq8, psq, ppath, ppo, ppl, ppp, pw, wb,
        _stream()), expected)


PACKED = [   # D, dtype, fp8 format, page size, shared table, query pair, window, precision, q view, softcap
    (64, torch.bfloat16, "e4m3", 64, 0, 2, (127, 0), "accurate", "dense", 2.0),
    (128, torch.bfloat16, "e4m3", 128, 1, 0, (-1, 0), "fast", "qkv", 30.0),
    (128, torch.float16, "e5m2", 256, 2, 1, (840, 5), "fast", "dense", 0.5),
    (256, torch.bfloat16, "e4m3", 64, 3, 3, (200, 0), "accurate", "qkv", 50.0),
]
PACKED_IDS = ["d64-ps64-gqa-two-tiles", "d128-ps128-idle-slot-strided", "d128-fp16-e5m2-ps256-g1", "d256-ps64-equal-strided"]


@pytest.mark.parametrize("ns", [1, 3, 9])
@pytest.mark.parametrize("D,dtype,fmt,ps,ti,qi,window,precision,view,cap", PACKED, ids=PACKED_IDS)
def test_fp8_attention_paged_varlen_softcap_forward(D, dtype, fmt, ps, ti, qi, window, precision, view, cap, ns):
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
                                           fp8_dtype=P.FP8[fmt], window=window, softcap=cap, precision=precision, num_splits=ns, return_lse=True,
                                           return_partials=True, return_quant=True, return_path=True)
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
    po, pl, pq8, psq, ppath, ppo, ppl, ppp, expected = _outs(p, dtype, rows, D, rows * D, B * Hq, ns, w)
    wb = L.qattn_fp8_attention_paged_varlen_workspace_bytes(B, Hq, HKV, total, CAP, D, ns)
    assert wb > 0
    pw = p.scratch("workspace", wb, align=ALIGN16)
    p.check(lambda: L.qattn_fp8_attention_paged_varlen_softcap_forward(
        pq, s2, _native.fmt_of(dtype), pk, pv, ptab, t.M, t.num_pages, ps, t.M, psk, psv, po, pl, pcu, psu, B, Hq, HKV, total, max(sq), CAP, D,
        _native.fmt_of(P.FP8[fmt]), 0, window[0], window[1], cap, 0.0, _native.PRECISION[precision], ns, pq8, psq, ppath, ppo, ppl, ppp, pw, wb,
        _stream()), expected)

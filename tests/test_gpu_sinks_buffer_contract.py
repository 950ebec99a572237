"""Buffer contract of the four learned-sink C entries (include/qattn_sinks.h; sizes, alignment and written bytes: include/qattn_buffers.h),
held the way tests/test_gpu_splitkv_window_buffer_contract.py holds the window siblings: the C entry through ctypes, every caller-provided
buffer carved from a guarded arena (tests/arena.py) of EXACTLY the documented size at the documented alignment -- `sinks` exactly Hq floats
on 4 bytes.  After the call every guard is intact, every output is bit-equal to the ordinary call, every described element is written,
the siblings' workspace size functions suffice and no bit depends on what lies outside the described inputs."""
import ctypes
import math

import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import arena as A
from tests import paged_cases as P
from tests import paged_varlen_cases as V
from tests.test_gpu_buffer_contract import ALIGN4, ALIGN16, Plan, _stream
from tests.test_gpu_paged_buffer_contract import _pools
from tests.test_gpu_splitkv_window_buffer_contract import _outs

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV, CAP = P.B, P.HKV, P.CAP


def _sinks(Hq, seed):
    """finite sinks around the key LSEs of these shapes, one head without a sink"""
    s = torch.randn(Hq, generator=torch.Generator().manual_seed(seed)) * 2 + 5
    s[Hq // 2] = -math.inf
    return s.to(DEV)


CONTIG = [   # D, dtype, B, Hq, Hkv, Sq, Skv, used, window, precision
    (64, torch.bfloat16, 2, 4, 2, 5, 1100, [1100, 65], (127, 0), "accurate"),
    (128, torch.bfloat16, 1, 8, 2, 1, 1100, None, (-1, 0), "fast"),
    (128, torch.float16, 2, 4, 4, 130, 1100, [1036, 0], (200, 37), "fast"),
    (256, torch.bfloat16, 1, 8, 1, 130, 130, [77], (0, 0), "accurate"),
]
CONTIG_IDS = ["d64-gqa-seqused-gpt-oss-window", "d128-decode-full-layer", "d128-fp16-two-tiles-band", "d256-one-key-rows-without-key"]


@pytest.mark.parametrize("ns", [1, 3, 9])
@pytest.mark.parametrize("D,dtype,Bn,Hq,Hkv,Sq,Skv,used,window,precision", CONTIG, ids=CONTIG_IDS)
def test_fp8_attention_splitkv_sink_forward(D, dtype, Bn, Hq, Hkv, Sq, Skv, used, window, precision, ns):
    L = _native.lib()
    g = torch.Generator().manual_seed(1000 * Sq + 10 * Skv + D)
    q = torch.randn(Bn, Hq, Sq, D, generator=g).to(dtype).to(DEV)
    k, v = (torch.randn(Bn, Hkv, Skv, D, generator=g).to(dtype).to(DEV) for _ in range(2))
    kv = qa.prepare_kv_fp8(k, v)
    su = None if used is None else torch.tensor(used, dtype=torch.int32, device=DEV)
    snk = _sinks(Hq, D + Sq)
    w = _native.fp8_attention_splitkv(q, kv.k, kv.v, kv.scale_k, kv.scale_v, Skv=Skv, window=window, sinks=snk, precision=precision, num_splits=ns,
                                      seqused_k=su, return_lse=True, return_partials=True, return_quant=True, return_path=True)
    rows = Bn * Hq * Sq
    p = Plan()
    pq = p.inp("q", q, row_bytes=2 * D)
    pk = p.inp("k8", kv.k, row_bytes=D)
    pv = p.inp("v8", kv.v, row_bytes=D)
    psk, psv = p.inp("scale_k", kv.scale_k, align=ALIGN4), p.inp("scale_v", kv.scale_v, align=ALIGN4)
    psu = None if su is None else p.inp("seqused_k", su, align=ALIGN4)
    psn = p.inp("sinks", snk, align=ALIGN4)
    po, pl, pq8, psq, ppath, ppo, ppl, ppp, expected = _outs(p, dtype, rows, D, L.qattn_fp8_tensor_bytes(_native.LAYOUT_ROWMAJOR, Bn, Hq, Sq, D),
                                                             Bn * Hq, ns, w)
    wb = L.qattn_fp8_attention_splitkv_workspace_bytes(Bn, Hq, Hkv, Sq, Skv, D, ns)
    pw = p.scratch("workspace", wb, align=ALIGN16)
    p.check(lambda: L.qattn_fp8_attention_splitkv_sink_forward(
        pq, _native.fmt_of(dtype), pk, pv, psk, psv, po, pl, psu, Bn, Hq, Hkv, Sq, Skv, D, _native.FMT_E4M3, 0, window[0], window[1], psn, 0.0,
        _native.PRECISION[precision], ns, pq8, psq, ppath, ppo, ppl, ppp, pw, wb, _stream()), expected)


PAGED = [   # D, dtype, fp8 format, page size, shared table, G, Sq, window, precision
    (64, torch.bfloat16, "e4m3", 64, 0, 2, 5, (127, 0), "accurate"),
    (128, torch.bfloat16, "e4m3", 128, 1, 4, 1, (-1, 0), "fast"),
    (128, torch.float16, "e5m2", 256, 2, 1, 3, (840, 5), "fast"),
    (256, torch.bfloat16, "e4m3", 64, 3, 4, 40, (200, 0), "accurate"),
]
PAGED_IDS = ["d64-ps64-gpt-oss-window", "d128-ps128-decode-full-layer", "d128-fp16-e5m2-ps256-edge-on-page", "d256-ps64-tile-crosses-heads"]


@pytest.mark.parametrize("ns", [1, 3, 9])
@pytest.mark.parametrize("D,dtype,fmt,ps,ti,G,Sq,window,precision", PAGED, ids=PAGED_IDS)
def test_fp8_attention_paged_splitkv_sink_forward(D, dtype, fmt, ps, ti, G, Sq, window, precision, ns):
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
    snk = _sinks(Hq, D + Sq)
    w = _native.fp8_attention_paged_splitkv(q, kp, vp, sk, sv, table, su, Skv=CAP, num_pages=t.num_pages, page_size=ps, fp8_dtype=P.FP8[fmt],
                                            window=window, sinks=snk, precision=precision, num_splits=ns, return_lse=True, return_partials=True,
                                            return_quant=True, return_path=True)
    rows = B * Hq * Sq
    p = Plan()
    pq = p.inp("q", q, row_bytes=2 * D)
    pk = p.inp("k_pool", kp, row_bytes=D)
    pv = p.inp("v_pool", vp, row_bytes=D)
    ptab = p.inp("block_table", table, align=ALIGN4)
    psk, psv = p.inp("scale_k", sk, align=ALIGN4), p.inp("scale_v", sv, align=ALIGN4)
    psu = p.inp("seqused_k", su, align=ALIGN4)
    psn = p.inp("sinks", snk, align=ALIGN4)
    po, pl, pq8, psq, ppath, ppo, ppl, ppp, expected = _outs(p, dtype, rows, D, L.qattn_fp8_tensor_bytes(_native.LAYOUT_ROWMAJOR, B, Hq, Sq, D),
                                                             B * Hq, ns, w)
    wb = L.qattn_fp8_attention_paged_splitkv_workspace_bytes(B, Hq, HKV, Sq, CAP, D, ns)
    assert wb > 0
    pw = p.scratch("workspace", wb, align=ALIGN16)
    p.check(lambda: L.qattn_fp8_attention_paged_splitkv_sink_forward(
        pq, _native.fmt_of(dtype), pk, pv, ptab, t.M, t.num_pages, ps, t.M, psk, psv, po, pl, psu, B, Hq, HKV, Sq, CAP, D,
        _native.fmt_of(P.FP8[fmt]), 0, window[0], window[1], psn, 0.0, _native.PRECISION[precision], ns, pq8, psq, ppath, ppo, ppl, ppp, pw, wb,
        _stream()), expected)


PACKED = [   # D, dtype, fp8 format, page size, shared table, query pair, window, precision, q view
    (64, torch.bfloat16, "e4m3", 64, 0, 2, (127, 0), "accurate", "dense"),
    (128, torch.bfloat16, "e4m3", 128, 1, 0, (-1, 0), "fast", "qkv"),
    (128, torch.float16, "e5m2", 256, 2, 1, (840, 5), "fast", "dense"),
    (256, torch.bfloat16, "e4m3", 64, 3, 3, (200, 0), "accurate", "qkv"),
]
PACKED_IDS = ["d64-ps64-gqa-two-tiles", "d128-ps128-idle-slot-strided", "d128-fp16-e5m2-ps256-g1", "d256-ps64-equal-strided"]


@pytest.mark.parametrize("ns", [1, 3, 9])
@pytest.mark.parametrize("D,dtype,fmt,ps,ti,qi,window,precision,view", PACKED, ids=PACKED_IDS)
def test_fp8_attention_paged_varlen_sink_forward(D, dtype, fmt, ps, ti, qi, window, precision, view, ns):
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
    snk = _sinks(Hq, D + qi)
    w = _native.fp8_attention_paged_varlen(q, kp, vp, sk, sv, table, su, cu, max_seqlen_q=max(sq), Skv=CAP, num_pages=t.num_pages, page_size=ps,
                                           fp8_dtype=P.FP8[fmt], window=window, sinks=snk, precision=precision, num_splits=ns, return_lse=True,
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
    psn = p.inp("sinks", snk, align=ALIGN4)
    po, pl, pq8, psq, ppath, ppo, ppl, ppp, expected = _outs(p, dtype, rows, D, rows * D, B * Hq, ns, w)
    wb = L.qattn_fp8_attention_paged_varlen_workspace_bytes(B, Hq, HKV, total, CAP, D, ns)
    assert wb > 0
    pw = p.scratch("workspace", wb, align=ALIGN16)
    p.check(lambda: L.qattn_fp8_attention_paged_varlen_sink_forward(
        pq, s2, _native.fmt_of(dtype), pk, pv, ptab, t.M, t.num_pages, ps, t.M, psk, psv, po, pl, pcu, psu, B, Hq, HKV, total, max(sq), CAP, D,
        _native.fmt_of(P.FP8[fmt]), 0, window[0], window[1], psn, 0.0, _native.PRECISION[precision], ns, pq8, psq, ppath, ppo, ppl, ppp, pw, wb,
        _stream()), expected)


@pytest.mark.parametrize("D, S, n, out_dtype", [(64, 67, 1, torch.bfloat16), (128, 300, 3, torch.float32), (256, 1, 8, torch.float16)])
def test_attention_state_merge_sink(D, S, n, out_dtype):
    """as tests/test_gpu_merge.py holds the merge entry: out B H S D elements on 16 bytes, lse_out B H S floats on 4, sink H floats on 4; the
    inputs are padded views whose pads and guards hold NaN in one run and zeros in the other"""
    from tests.test_gpu_merge_sink import B as Bn, H, states
    outs, lses = states(n, S, D, 17)
    fmts = [o.dtype for o in outs]
    snk = _sinks(H, D) - 5
    want = qa.merge_attn_states_with_sinks(outs, lses, snk, out_dtype=out_dtype)
    ar = A.Arena(DEV)
    es = out_dtype.itemsize
    r_out = ar.carve("out", Bn * H * S * D * es, align=16, row_bytes=D * es, role="out", kind=A.KIND_OF_DTYPE[out_dtype])
    r_lse = ar.carve("lse_out", Bn * H * S * 4, align=4, row_bytes=4, role="out", kind="fp32")
    ll, vp = ctypes.c_longlong, ctypes.c_void_p
    results = []
    for hostile in (True, False):
        o_ptrs, l_ptrs, o_str, l_str = [], [], [], []
        for i, (o, l) in enumerate(zip(outs, lses)):
            per16 = 16 // o.element_size()
            so = (H * S * (D + per16) + per16, S * (D + per16), D + per16)
            sl = (H * (S + 3) + 1, S + 3, 1)
            ro = ar.carve(f"o{i}_{hostile}", ((Bn - 1) * so[0] + (H - 1) * so[1] + (S - 1) * so[2] + D) * o.element_size(), align=16,
                          row_bytes=D * o.element_size(), role="in", kind=A.KIND_OF_DTYPE[o.dtype])
            rl = ar.carve(f"lse{i}_{hostile}", ((Bn - 1) * sl[0] + (H - 1) * sl[1] + (S - 1) * sl[2] + 1) * 4, align=4, row_bytes=4, role="in", kind="fp32")
            ro.set_guards(hostile)
            rl.set_guards(hostile)
            ro.load_view(o, so + (1,), hostile)
            rl.load_view(l, sl, hostile)
            o_ptrs.append(ro.ptr); l_ptrs.append(rl.ptr); o_str += so; l_str += sl
        rs = ar.carve(f"sink_{hostile}", H * 4, align=4, row_bytes=4, role="in", kind="fp32")
        rs.set_guards(hostile)
        rs.load_view(snk, (1,), hostile)
        r_out.fill_poison()
        r_lse.fill_poison()
        rc = _native.lib().qattn_attention_state_merge_sink(
            n, (vp * n)(*o_ptrs), (ctypes.c_int * n)(*[_native._MERGE_FMT[d] for d in fmts]), (ll * (3 * n))(*o_str), (vp * n)(*l_ptrs),
            (ll * (3 * n))(*l_str), r_out.ptr, _native._MERGE_FMT[out_dtype], (ll * 3)(H * S * D, S * D, D), r_lse.ptr, (ll * 3)(H * S, S, 1),
            Bn, H, S, D, torch.cuda.current_stream().cuda_stream, rs.ptr)
        assert rc == 0, rc
        torch.cuda.synchronize()
        A.assert_guards_intact(ar)
        assert r_out.poison_left() == 0 and r_lse.poison_left() == 0, "every output byte is written"
        results.append((r_out.interior.clone(), r_lse.interior.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), "no dependence on bytes outside the inputs"
    assert torch.equal(results[0][0].view(out_dtype).view(Bn, H, S, D), want[0]) and torch.equal(results[0][1].view(torch.float32).view(Bn, H, S), want[1])

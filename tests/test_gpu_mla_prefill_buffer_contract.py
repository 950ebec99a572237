"""Buffer contract of qattn_fp8_mla_prefill_varlen_forward (include/qattn_mla_prefill.h), held the way tests/test_gpu_mla_buffer_contract.py
holds the decode entries: the C entry through ctypes on guarded arenas (tests/arena.py).  k_nope and v are the two halves of ONE
[total_k, H, 256] buffer, q a slice of a wider one, k_pe rows 72 elements apart; each buffer ends with its last row's last used element.  The
pads of the views, the keys behind seqused_k and the tokens behind the last sequence -- INSIDE the buffers -- hold NaN in two runs and
zeros in the third.  out, lse, q8 and scale_q are written for the rows of sequences and for no other (the rows behind cu_seqlens_q[B] keep
their pre-fill), scale_k and scale_v everywhere; the workspace has exactly the stated bytes and is pre-filled 0x00, then 0xFF."""
import numpy as np
import pytest
import torch

from quantumattention_amd import _native
from tests.test_gpu_buffer_contract import ALIGN4, _kind, _stream
from tests.test_gpu_mla_buffer_contract import DEV, FP8, P0, SM_SCALE, MPlan, _caller, _gen, _i32, _ll

pytestmark = pytest.mark.gpu

LQ = (0, 1, 130, 200)                             # an empty sequence, one row, a tile and two rows, two tiles
LK = (0, 1, 130, 200)
USED = (0, 1, 100, 200)                           # sequence 2: 30 keys behind the used length
B = len(LQ)
TAIL_Q, TAIL_K = 6, 5                             # tokens behind the last sequence


@pytest.mark.parametrize("with_used", [False, True], ids=["whole-extents", "seqused_k"])
@pytest.mark.parametrize("H,dtype,fmt,causal", [(2, torch.bfloat16, "e4m3", True), (3, torch.float16, "e5m2", False), (2, torch.bfloat16, "e5m2", True),
                                                (3, torch.float16, "e4m3", False)],
                         ids=["h2-bf16-e4m3-causal", "h3-fp16-e5m2", "h2-bf16-e5m2-causal", "h3-fp16-e4m3"])
def test_fp8_mla_prefill_varlen_forward(H, dtype, fmt, causal, with_used):
    L = _native.lib()
    live_q, live_k = sum(LQ), sum(LK)
    total_q, total_k = live_q + TAIL_Q, live_k + TAIL_K
    g = _gen(H + 10 * causal)
    q = (torch.randn(total_q, H, 192, generator=g) * 1.5).to(dtype).to(DEV)
    kv = (torch.randn(total_k, H, 256, generator=g) * 1.5).to(dtype).to(DEV)
    kpe = (torch.randn(total_k, 64, generator=g) * 1.5).to(dtype).to(DEV)
    cu_q, cu_k = _i32(np.concatenate([[0], np.cumsum(LQ)])), _i32(np.concatenate([[0], np.cumsum(LK)]))
    used = _i32(USED) if with_used else None
    dead_k = torch.ones(total_k, dtype=torch.bool, device=DEV)
    for k0, n in zip(np.cumsum((0,) + LK[:-1]).tolist(), USED if with_used else LK):
        dead_k[k0:k0 + n] = False
    q[live_q:], kv[dead_k], kpe[dead_k] = 0, 0, 0
    wo, wl, wq8, wsq, wsk, wsv = _native.fp8_mla_prefill_varlen(q, kv[..., :128], kpe, kv[..., 128:], cu_q, cu_k, used, is_causal=causal,
                                                                sm_scale=SM_SCALE, fp8_dtype=FP8[fmt], return_quantized=True)
    p = MPlan()
    qstr, kvstr, pestr = (H * 256 + 8, 256, 1), (H * 256 + 8, 256, 1), (72, 1)
    pq = p.inp_view("q", q, qstr, row_bytes=2 * 192)
    pkv = p.inp_view("k_nope | v", kv, kvstr, row_bytes=2 * 256)
    ppe = p.inp_view("k_pe", kpe, pestr, row_bytes=2 * 72)
    p.never_read(q, slice(live_q, None))
    p.never_read(kv, dead_k)
    p.never_read(kpe, dead_k)
    pcq, pck = p.inp("cu_seqlens_q", cu_q, align=ALIGN4), p.inp("cu_seqlens_k", cu_k, align=ALIGN4)
    pus = p.inp("seqused_k", used, align=ALIGN4) if with_used else None
    rows = lambda width: (lambda b: b[:live_q * width])                                      # the rows of sequences: the leading ones
    po = p.out("out", 2 * total_q * H * 128, _kind(dtype), row_bytes=2 * 128, logical=rows(2 * H * 128))
    pl = p.out("lse", 4 * H * total_q, "fp32", align=ALIGN4,
               logical=lambda b: b.view(torch.float32).view(H, total_q)[:, :live_q].contiguous().view(-1).view(torch.uint8))
    pq8 = p.out("q8", total_q * H * 192, "fp8", row_bytes=192, logical=rows(H * 192))
    psq = p.out("scale_q", 4 * total_q * H, "fp32", align=ALIGN4, logical=rows(4 * H))
    psk, psv = p.out("scale_k", 4 * B * H, "fp32", align=ALIGN4), p.out("scale_v", 4 * B * H, "fp32", align=ALIGN4)
    wb = L.qattn_fp8_mla_prefill_varlen_workspace_bytes(B, H, total_q, total_k)
    assert wb > 0
    pw = p.scratch("workspace", wb)
    s7 = _ll(qstr[0], qstr[1], kvstr[0], kvstr[1], pestr[0], kvstr[0], kvstr[1])
    first = p.check(lambda: L.qattn_fp8_mla_prefill_varlen_forward(pq, pkv, ppe, pkv + 2 * 128, s7, _native.fmt_of(dtype), po, pl, pcq, pck, pus, B, H,
                                                                   total_q, total_k, _native.fmt_of(FP8[fmt]), int(causal), SM_SCALE, pq8, psq, psk, psv,
                                                                   pw, wb, _stream()),
                    {"out": wo[:live_q], "lse": wl[:, :live_q], "q8": wq8[:live_q], "scale_q": wsq[:live_q], "scale_k": wsk, "scale_v": wsv})
    assert torch.isfinite(first["lse"].view(torch.float32).view(H, live_q)[:, -1]).all()      # the last row of the last sequence sees keys


def test_the_argument_checks_of_qattn_mla_prefill_h_return_their_codes_before_any_launch():
    """beyond tests/test_cpu_mla_prefill.py: each 16-byte pointer class, a negative stride, a short and a misaligned workspace.  A call that
    passed every other check here would still return QATTN_ERR_WORKSPACE before any device call."""
    L = _native.lib()
    names = ("q", "kn", "kp", "v", "st", "in_fmt", "out", "lse", "cq", "ck", "used", "B", "H", "tq", "tk", "fmt", "causal", "scale", "q8", "sq", "sk",
             "sv", "ws", "wsb", "stream")
    call = _caller(L.qattn_fp8_mla_prefill_varlen_forward, names,
                   dict(q=P0, kn=P0, kp=P0, v=P0, in_fmt=_native.FMT_BF16, out=P0, cq=P0, ck=P0, B=2, H=2, tq=5, tk=7, fmt=_native.FMT_E4M3, causal=1,
                        scale=0.07, wsb=0))
    for kw in (dict(kn=P0 + 8), dict(kp=P0 + 8), dict(v=P0 + 8), dict(out=P0 + 8), dict(q8=P0 + 8), dict(kn=None), dict(kp=None), dict(v=None),
               dict(out=None), dict(cq=None), dict(ck=None), dict(st=_ll(384, 192, 256, 128, 64, 256, -128)), dict(st=_ll(384, 192, 256, 128, 64, 260, 128)),
               dict(B=0), dict(tq=-1), dict(tk=-1), dict(scale=float("nan"))):
        assert call(**kw) == -1, kw
    need = L.qattn_fp8_mla_prefill_varlen_workspace_bytes(2, 2, 5, 7)
    assert call(ws=P0, wsb=need - 1) == -4 and call(ws=P0 + 8, wsb=need) == -4 and call(ws=None, wsb=need) == -4

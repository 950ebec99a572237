"""Buffer contract of the two RoPE entries (include/qattn_rope.h; sizes, alignment and written bytes: include/qattn_buffers.h), held the way
tests/test_gpu_buffer_contract.py holds every other entry: each caller-provided buffer -- the cos / sin tables included -- is carved from
a guarded arena (tests/arena.py) of EXACTLY the documented size at the documented alignment and no more; after the call every guard is
intact, every output is bit-equal to the ordinary call (the `_native` wrappers tests/test_gpu_rope.py grades), nothing is left unwritten,
and no bit depends on what the workspace held or on the bytes around the inputs (hostile NaN guards and view pads, then benign ones).
The tables hold exactly S rows: a table row read for a padding row of the last 64-row tile would come out of a NaN guard."""
import pytest
import torch

from quantumattention_amd import _native
from tests.test_gpu_buffer_contract import ALIGN4, ALIGN16, Plan, _c3, _kind, _strided_rows, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HQ, HKV = 1, 4, 2
CFGS = [(64, torch.bfloat16, "head-wise"), (64, torch.bfloat16, "token-wise"), (128, torch.bfloat16, "head-wise"),
        (128, torch.float16, "head-wise"), (256, torch.bfloat16, "head-wise")]
CFG_IDS = ["d64", "d64-token", "d128", "d128-fp16", "d256"]
SHAPES = [(1, 1), (257, 63), (1089, 1089)]
OFF = 77   # the keys' position offset: k has tables of its own


def _qkv(Sq, Skv, D, dtype):
    g = torch.Generator().manual_seed(1000 * Sq + 10 * Skv + D)
    q = torch.randn(B, HQ, Sq, D, generator=g)
    k, v = (torch.randn(B, HKV, Skv, D, generator=g) for _ in range(2))
    return tuple(t.to(dtype).to(DEV) for t in (q, k, v))


def _tables(S, half, offset):
    """exactly S rows, dense"""
    inv = 10000.0 ** (-torch.arange(half, dtype=torch.float64) / half)
    ang = (torch.arange(S, dtype=torch.float64) + offset)[:, None] * inv
    return torch.cos(ang).to(torch.float32).to(DEV), torch.sin(ang).to(torch.float32).to(DEV)


def _inputs(p, q, k, strided):
    """q and k into the arena, dense or as views with padded rows and heads; returns (pq, pk, strides or None)"""
    D = q.shape[3]
    if not strided:
        return p.inp("q", q, row_bytes=2 * D), p.inp("k", k, row_bytes=2 * D), None
    (sq, nq), (sk, nk) = _strided_rows("q", q), _strided_rows("k", k)
    return p.inp_view("q", q, sq, nq, row_bytes=2 * D), p.inp_view("k", k, sk, nk, row_bytes=2 * D), _c3([sq, sk])


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("il", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("Sq,Skv", SHAPES)
@pytest.mark.parametrize("D,dtype,scaling", CFGS, ids=CFG_IDS)
def test_rope_quant_qk_fp8(D, dtype, scaling, Sq, Skv, il, strided):
    L = _native.lib()
    q, k, _ = _qkv(Sq, Skv, D, dtype)
    cq, sq_ = _tables(Sq, D // 2, 0)
    ck, sk_ = _tables(Skv, D // 2, OFF)
    mode = _native._scale_mode(scaling)
    wq8, wsq = _native.rope_quant_fp8(q, cq, sq_, interleaved=il, scaling=scaling)
    wk8, wsk = _native.rope_quant_fp8(k, ck, sk_, interleaved=il, scaling=scaling, layout=_native.LAYOUT_KFRAG)
    p = Plan()
    pq, pk, strides = _inputs(p, q, k, strided)
    tabs = [p.inp(n, t, row_bytes=2 * D) for n, t in (("cos_q", cq), ("sin_q", sq_), ("cos_k", ck), ("sin_k", sk_))]
    pq8 = p.out("q8", L.qattn_fp8_tensor_bytes(_native.LAYOUT_ROWMAJOR, B, HQ, Sq, D), "fp8", row_bytes=D)
    pk8 = p.out("k8", L.qattn_fp8_tensor_bytes(_native.LAYOUT_KFRAG, B, HKV, Skv, D), "fp8", row_bytes=D)
    psq, psk = (p.out(n, 4 * w.numel(), "fp32", align=ALIGN4) for n, w in (("scale_q", wsq), ("scale_k", wsk)))
    wb = L.qattn_rope_quant_qk_workspace_bytes(B, HQ, HKV)
    pw = p.scratch("workspace", wb, align=ALIGN4)
    half = D // 2
    p.check(lambda: L.qattn_rope_quant_qk_fp8(pq, pk, strides, _native.fmt_of(dtype), tabs[0], tabs[1], 0, half, tabs[2], tabs[3], 0, half, int(il),
                                              pq8, pk8, _native.LAYOUT_KFRAG, psq, psk, B, HQ, HKV, Sq, Skv, D, _native.FMT_E4M3, mode, 0,
                                              pw, wb, _stream()),
            {"q8": wq8, "k8": wk8, "scale_q": wsq, "scale_k": wsk})


@pytest.mark.parametrize("v16", [False, True], ids=["fp8v-neox", "v16-gptj"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Sq,Skv", [(65, 65), (257, 63), (1089, 1089)])
@pytest.mark.parametrize("D,dtype,scaling", CFGS, ids=CFG_IDS)
def test_fp8_rope_quant_attention_forward(D, dtype, scaling, Sq, Skv, causal, v16):
    L = _native.lib()
    il = v16
    q, k, v = _qkv(Sq, Skv, D, dtype)
    cq, sq_ = _tables(Sq, D // 2, 0)
    ck, sk_ = _tables(Skv, D // 2, OFF)
    mode = _native._scale_mode(scaling)
    wo, wl, w = _native.fp8_rope_quant_attention(q, k, v, cq, sq_, ck, sk_, interleaved=il, is_causal=causal, scaling=scaling, pv_16bit=v16,
                                                 return_lse=True, return_quant=True)
    p = Plan()
    pq, pk, strides = _inputs(p, q, k, strided=causal)      # (the causal cases also take q and k as padded views)
    pv = p.inp("v", v, row_bytes=2 * D)
    tabs = [p.inp(n, t, row_bytes=2 * D) for n, t in (("cos_q", cq), ("sin_q", sq_), ("cos_k", ck), ("sin_k", sk_))]
    po = p.out("out", 2 * B * HQ * Sq * D, _kind(dtype), row_bytes=2 * D)
    pl = p.out("lse", 4 * B * HQ * L.qattn_lse_row_stride(Sq, _native.LSE_NATURAL), "fp32", align=ALIGN4)
    pq8 = p.out("q8", L.qattn_fp8_tensor_bytes(_native.LAYOUT_ROWMAJOR, B, HQ, Sq, D), "fp8", row_bytes=D)
    pk8 = p.out("k8", L.qattn_fp8_tensor_bytes(_native.LAYOUT_KFRAG, B, HKV, Skv, D), "fp8", row_bytes=D)
    psq, psk = (p.out(n, 4 * w[n].numel(), "fp32", align=ALIGN4) for n in ("scale_q", "scale_k"))
    expected = {"out": wo, "lse": wl, "q8": w["q8"], "k8": w["k8"], "scale_q": w["scale_q"], "scale_k": w["scale_k"]}
    pv8 = psv = None
    if not v16:
        pv8 = p.out("v8", L.qattn_fp8_tensor_bytes(_native.LAYOUT_VFRAG, B, HKV, Skv, D), "fp8", row_bytes=D)
        psv = p.out("scale_v", 4 * B * HKV, "fp32", align=ALIGN4)
        expected.update(v8=w["v8"], scale_v=w["scale_v"])
    wb = L.qattn_fp8_rope_quant_attention_workspace_bytes(B, HQ, HKV, Sq, Skv, D)
    pw = p.scratch("workspace", wb, align=ALIGN16)
    f16, f8, half = _native.fmt_of(dtype), _native.FMT_E4M3, D // 2
    p.check(lambda: L.qattn_fp8_rope_quant_attention_forward(
        pq, pk, pv, strides, f16, tabs[0], tabs[1], 0, half, tabs[2], tabs[3], 0, half, int(il), po, pl, pq8, pk8, pv8, psq, psk, psv,
        B, HQ, HKV, Sq, Skv, D, f8, f16 if v16 else f8, mode, 0, int(causal), 0.0, _native.PRECISION["auto"], _native.LSE_NATURAL,
        pw, wb, _stream()), expected)

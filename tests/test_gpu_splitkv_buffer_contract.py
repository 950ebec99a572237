"""Buffer contract of qattn_fp8_attention_splitkv_forward (include/qattn_splitkv.h; sizes, alignment and written bytes:
include/qattn_buffers.h), held the way tests/test_gpu_buffer_contract.py holds every other entry: each caller-provided buffer is carved
from a guarded arena (tests/arena.py) of EXACTLY the documented size at the documented alignment and no more; after the call every guard
is intact, every output is bit-equal to the ordinary call (the `_native` wrapper tests/test_gpu_splitkv.py grades), nothing described is
left unwritten, and no bit depends on what the workspace held or on the bytes around the inputs.  Then: no bit depends on the bytes of the
prepared K / V behind seqused_k -- NaN bytes and the largest finite value, inside the chunk that holds key L_b and in the chunks behind it."""
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests.test_gpu_buffer_contract import ALIGN1, ALIGN4, ALIGN16, Plan, _kind, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
CFGS = [   # D, dtype, B, Hq, Hkv, Sq, Skv, used, causal, precision
    (64, torch.bfloat16, 2, 4, 2, 5, 1100, [1100, 65], True, "accurate"),
    (128, torch.bfloat16, 1, 8, 2, 1, 1100, None, False, "fast"),
    (128, torch.float16, 2, 4, 4, 130, 1100, [1036, 0], True, "fast"),
    (256, torch.bfloat16, 1, 8, 1, 130, 130, [77], False, "accurate"),
]
CFG_IDS = ["d64-gqa-seqused", "d128-decode", "d128-fp16-two-tiles", "d256-ragged-tiles"]


def _qkv(B, Hq, Hkv, Sq, Skv, D, dtype):
    g = torch.Generator().manual_seed(1000 * Sq + 10 * Skv + D)
    q = torch.randn(B, Hq, Sq, D, generator=g)
    k, v = (torch.randn(B, Hkv, Skv, D, generator=g) for _ in range(2))
    return tuple(t.to(dtype).to(DEV) for t in (q, k, v))


@pytest.mark.parametrize("ns", [1, 3, 9])
@pytest.mark.parametrize("D,dtype,B,Hq,Hkv,Sq,Skv,used,causal,precision", CFGS, ids=CFG_IDS)
def test_fp8_attention_splitkv_forward(D, dtype, B, Hq, Hkv, Sq, Skv, used, causal, precision, ns):
    L = _native.lib()
    q, k, v = _qkv(B, Hq, Hkv, Sq, Skv, D, dtype)
    kv = qa.prepare_kv_fp8(k, v)
    su = None if used is None else torch.tensor(used, dtype=torch.int32, device=DEV)
    w = _native.fp8_attention_splitkv(q, kv.k, kv.v, kv.scale_k, kv.scale_v, Skv=Skv, is_causal=causal, precision=precision, num_splits=ns,
                                      seqused_k=su, return_lse=True, return_partials=True, return_quant=True, return_path=True)
    wo, wl, wpo, wpl, wpp, wq8, wsq, wpath = w
    rows = B * Hq * Sq
    p = Plan()
    pq = p.inp("q", q, row_bytes=2 * D)
    pk = p.inp("k8", kv.k, row_bytes=D)
    pv = p.inp("v8", kv.v, row_bytes=D)
    psk, psv = p.inp("scale_k", kv.scale_k, align=ALIGN4), p.inp("scale_v", kv.scale_v, align=ALIGN4)
    psu = None if su is None else p.inp("seqused_k", su, align=ALIGN4)
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
    wb = L.qattn_fp8_attention_splitkv_workspace_bytes(B, Hq, Hkv, Sq, Skv, D, ns)
    pw = p.scratch("workspace", wb, align=ALIGN16)
    p.check(lambda: L.qattn_fp8_attention_splitkv_forward(
        pq, _native.fmt_of(dtype), pk, pv, psk, psv, po, pl, psu, B, Hq, Hkv, Sq, Skv, D, _native.FMT_E4M3, 0, int(causal), 0.0,
        _native.PRECISION[precision], ns, pq8, psq, ppath, ppo, ppl, ppp, pw, wb, _stream()), expected)


@pytest.mark.parametrize("D", [64, 128, 256])
def test_bytes_of_the_prepared_k_and_v_behind_seqused_k_influence_no_bit(D):
    """the row-major fp8 bytes behind L_b replaced by NaN bytes (0x7f) and by the largest finite value (e4m3 0x7e = 448, times the scale far
    above every real key), then re-laid into the images: L_b = 1036 leaves 52 such keys inside the chunk that holds key L_b (their scores
    are masked, their V bytes must not reach the matrix pipe) and a whole chunk behind it (never read); L_b = 65 leaves whole blocks"""
    B, Hq, Hkv, Sq, Skv = 2, 4, 2, 5, 1100
    used = [1036, 65]
    q, k, v = _qkv(B, Hq, Hkv, Sq, Skv, D, torch.bfloat16)
    k8, sk = _native.quant_fp8(k, scaling="head-wise")
    v8, sv = _native.quant_fp8(v, scaling="head-wise")
    su = torch.tensor(used, dtype=torch.int32, device=DEV)

    def prepared(poison):
        kb, vb = k8.view(torch.uint8).clone(), v8.view(torch.uint8).clone()
        if poison is not None:
            for b, n in enumerate(used):
                kb[b, :, n:] = poison
                vb[b, :, n:] = poison
        kf = _native.pack_fp8(kb.view(torch.float8_e4m3fn), _native.LAYOUT_KFRAG)
        vf = _native.pack_fp8(vb.view(torch.float8_e4m3fn), _native.LAYOUT_VFRAG)
        return qa.PreparedKV(kf, vf, sk, sv, k.shape, "e4m3", k.dtype, "compiled", "frag")

    clean = prepared(None)
    ref = qa.prepare_kv_fp8(k, v)
    assert torch.equal(clean.k, ref.k) and torch.equal(clean.v, ref.v) and torch.equal(sk, ref.scale_k) and torch.equal(sv, ref.scale_v)
    for ns in (1, 3, 9):
        for precision in ("accurate", "fast"):
            for causal in (False, True):
                for lse in (True, False):
                    call = lambda kv: qa.fp8_attn_splitkv_func(q, kv, causal=causal, seqused_k=su, num_splits=ns, precision=precision, return_lse=lse)
                    want = call(clean)
                    for poison in (0x7F, 0x7E):
                        got = call(prepared(poison))
                        for a, b in zip(got if lse else (got,), want if lse else (want,)):
                            assert not torch.isnan(a.float()).any() and torch.equal(a, b), (ns, precision, causal, lse, hex(poison))

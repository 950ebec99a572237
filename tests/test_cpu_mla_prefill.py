"""CPU tests of the non-absorbed MLA prefill entry (include/qattn_mla_prefill.h): the eager definition -- the specification -- against the fp64
reference of tests/mla_prefill_cases.py, the rejection reasons, and the C names in the export list.

Bounds: out per element 2^-6 max(1, |ref| / 2) and lse 2e-3, the figures of the GPU test; the eager definition is fp32 softmax on the same
de-quantised operands, so it sits far inside both (its only error against fp64 is the rounding of out to 16 bits)."""
import ctypes

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import mla_prefill_cases as C
from tests.gpu_utils import assert_within_bound
from tests.mla_cases import LSE_TOL


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("fmt,dtype,H", [("e4m3", torch.bfloat16, 3), ("e5m2", torch.float16, 1)])
def test_eager_definition_against_the_fp64_reference(causal, fmt, dtype, H):
    q, kv, k_pe = C.make_inputs(H, dtype)
    cu_q, cu_k = C.tables()
    with qa.config.patch({"attention.fp8_format": fmt}):
        out, lse, q8, sq, sk, sv = qa.fp8_mla_prefill_varlen_func(q, kv[..., :128], k_pe, kv[..., 128:], cu_q, cu_k, 130, 200, scale=C.SM_SCALE,
                                                                  causal=causal, return_lse=True, return_quantized=True)
    assert out.shape == (q.shape[0], H, 128) and out.dtype == dtype and lse.shape == (H, q.shape[0]) and q8.dtype == torch.float8_e4m3fn
    fmax = torch.finfo(C.TDT[fmt]).max
    assert (sk[3] >= C.PE_PEAK / fmax * (1 - 2.0 ** -20)).all() and (sk[6] == 2.0 ** -23).all()   # k_pe's peak sets K's scale; no key: eps
    kd, vd = C.dequantised_kv(kv, k_pe, sk, sv, fmt)
    ref_o, ref_l = C.reference((q8.double() * sq.double()[..., None]).numpy(), kd, vd, causal)
    fin = np.isfinite(ref_l)
    assert_within_bound(out.float().numpy(), ref_o, what=(causal, fmt, H))
    assert np.array_equal(np.isneginf(lse.numpy()), ~fin) and (out.float().numpy()[~fin.T] == 0).all()
    assert (~fin).sum() == H * ((5 + 40) if causal else 5)      # the sequence without keys; causal: and the first L_q - L_k rows of (70, 30)
    assert np.abs(lse.numpy()[fin] - ref_l[fin]).max() <= LSE_TOL


def test_rejection_reasons():
    q, kv, k_pe = C.make_inputs(3, torch.bfloat16)
    cu_q, cu_k = C.tables()
    kn, v = kv[..., :128], kv[..., 128:]
    why = lambda *a, scale=C.SM_SCALE: qa.mla_prefill_input_reason(*a, cu_q, cu_k, 130, 200, scale=scale)
    assert why(q, kn, k_pe, v) is None
    assert "head dimensions" in why(q[..., :128], kn, k_pe, v) and "head dimensions" in why(q, kn, k_pe, kv)      # wrong head dims
    assert "share a dtype" in why(q, kn.half(), k_pe, v)                                                           # mixed dtypes
    assert "scale is required" in why(q, kn, k_pe, v, scale=None) and "finite number" in why(q, kn, k_pe, v, scale=0.0)
    assert "dense channels" in why(q, kv[..., ::2], k_pe, v)                                                       # channels not dense
    assert "dense channels" in why(q, kn, torch.zeros((441, 68), dtype=torch.bfloat16)[:, 4:], v)                  # rows not 16-byte aligned
    assert "one head count" in why(q, kn[:, :2], k_pe, v[:, :2])                                                   # H mismatch
    assert "same tokens" in why(q, kn, k_pe[:-1], v)
    with pytest.raises(ValueError, match="scale is required"):
        qa.fp8_mla_prefill_varlen_func(q, kn, k_pe, v, cu_q, cu_k, 130, 200)


def test_exports_and_argument_codes():
    assert {"qattn_fp8_mla_prefill_varlen_workspace_bytes", "qattn_fp8_mla_prefill_varlen_forward"} <= set(_native.EXPORTS)
    assert "fp8_mla_prefill_varlen_func" not in qa.__all__ and "mla_prefill_input_reason" not in qa.__all__
    L = _native.lib()
    assert L.qattn_fp8_mla_prefill_varlen_workspace_bytes(0, 3, 10, 10) == 0 and L.qattn_fp8_mla_prefill_varlen_workspace_bytes(7, 3, 398, 441) > 0
    # the argument checks come before any device call (include/qattn.h: QATTN_ERR_INVALID_ARG -1, _UNSUPPORTED_FMT -3, _WORKSPACE -4)
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = buf.data_ptr() + (-buf.data_ptr()) % 16
    names = ("q", "kn", "kp", "v", "st", "in_fmt", "out", "lse", "cq", "ck", "used", "B", "H", "tq", "tk", "fmt", "causal", "scale", "q8", "sq",
             "sk", "sv", "ws", "wsb", "stream")
    good = dict.fromkeys(names) | dict(q=p, kn=p, kp=p, v=p, in_fmt=_native.FMT_BF16, out=p, cq=p, ck=p, B=1, H=1, tq=1, tk=1, fmt=_native.FMT_E4M3,
                                       causal=1, scale=0.07, wsb=0)
    call = lambda **kw: L.qattn_fp8_mla_prefill_varlen_forward(*(good | kw).values())
    assert call(q=None) == -1 and call(scale=0.0) == -1 and call(q=p + 2) == -1 and call(H=0) == -1
    assert call(st=(ctypes.c_longlong * 7)(192, 192, 128, 128, 60, 128, 128)) == -1      # a stride that is no multiple of 8
    assert call(in_fmt=_native.FMT_E4M3) == -3 and call(fmt=_native.FMT_BF16) == -3
    assert call() == -4

"""CPU-only tests of the variable-length entry (quantumattention_amd.fp8_attn_varlen_func, include/qattn_varlen.h): the public signature,
the validation reasons, the C entry's argument codes before any device call, the op's fake implementation, and the eager restatement
behind config.attention.force_eager_fallback."""
import ctypes
import inspect
import math

import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, varlen


def _fake(*shape, dtype=torch.bfloat16):
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        return torch.empty(*shape, dtype=dtype, device="cuda")


def test_signature_follows_flash_attn_varlen_and_all_is_unchanged():
    assert list(inspect.signature(qa.fp8_attn_varlen_func).parameters) == [
        "q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k", "dropout_p", "softmax_scale", "causal",
        "seqused_k", "return_lse"]
    params = inspect.signature(qa.fp8_attn_varlen_func).parameters
    assert params["dropout_p"].default == 0.0 and params["softmax_scale"].default is None and params["causal"].default is False
    for n in ("seqused_k", "return_lse"):
        assert params[n].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["seqused_k"].default is None and params["return_lse"].default is False
    assert qa.fp8_attn_varlen_func is varlen.fp8_attn_varlen_func
    assert "fp8_attn_varlen_func" not in qa.__all__ and len(qa.__all__) == 7


def test_validation_rules_give_their_reasons():
    r = varlen.varlen_input_reason
    q, k = _fake(300, 8, 128), _fake(400, 2, 128)
    cu = _fake(4, dtype=torch.int32)
    assert r(q, k, k, cu, cu, 128, 128) is None
    assert r(q, k, k, cu, cu, 128, 128, seqused_k=_fake(3, dtype=torch.int32), softmax_scale=0.1) is None
    assert r(q, k, k, cu, cu, 128, 128, dropout_p=0.1) == "NYI: dropout_p must be 0.0"
    assert "3-D" in r(_fake(1, 300, 8, 128), k, k, cu, cu, 128, 128)
    assert "dtype" in r(_fake(300, 8, 128, dtype=torch.float32), k, k, cu, cu, 128, 128)
    assert "share a dtype" in r(q, _fake(400, 2, 128, dtype=torch.float16), k, cu, cu, 128, 128)
    assert "same head dimension" in r(q, _fake(400, 2, 64), _fake(400, 2, 64), cu, cu, 128, 128)
    assert r(_fake(300, 8, 96), _fake(400, 2, 96), _fake(400, 2, 96), cu, cu, 128, 128) == "Unsupported head dimension: 96"
    assert "same shape" in r(q, k, _fake(399, 2, 128), cu, cu, 128, 128)
    assert "multiple of the key/value heads" in r(q, _fake(400, 3, 128), _fake(400, 3, 128), cu, cu, 128, 128)
    cpu = torch.empty(300, 8, 128, dtype=torch.bfloat16)
    assert r(cpu, cpu, cpu, cu, cu, 1, 1) == "Expected query, key, and value to be on a CUDA device"
    assert "int32" in r(q, k, k, _fake(4, dtype=torch.int64), cu, 128, 128)
    assert "int32" in r(q, k, k, cu, _fake(4, 1, dtype=torch.int32), 128, 128)
    assert "int32" in r(q, k, k, _fake(1, dtype=torch.int32), cu, 128, 128)
    assert "same length" in r(q, k, k, cu, _fake(5, dtype=torch.int32), 128, 128)
    assert "on cuda" in r(q, k, k, torch.zeros(4, dtype=torch.int32), cu, 128, 128)
    assert "seqused_k" in r(q, k, k, cu, cu, 128, 128, seqused_k=_fake(4, dtype=torch.int32))
    assert "seqused_k" in r(q, k, k, cu, cu, 128, 128, seqused_k=_fake(3, dtype=torch.float32))
    assert "max_seqlen" in r(q, k, k, cu, cu, -1, 128)
    assert "max_seqlen" in r(q, k, k, cu, cu, 1.5, 128)
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert "softmax_scale" in r(q, k, k, cu, cu, 128, 128, softmax_scale=bad)
    # the public function raises them as ValueError, before any launch; then the device gate (no gfx950 on this box)
    with pytest.raises(ValueError, match="dropout_p"):
        qa.fp8_attn_varlen_func(q, k, k, cu, cu, 128, 128, dropout_p=0.5)
    with pytest.raises(ValueError, match="gfx950"):
        qa.fp8_attn_varlen_func(q, k, k, cu, cu, 128, 128)


def test_c_entry_rejects_bad_arguments_before_any_device_call():
    L = _native.lib()
    one = ctypes.c_void_p(256)   # any non-NULL, 16-byte aligned pointer: the checks come first
    ws = 1 << 40

    def call(q=one, out=one, cu=one, B=2, Hq=4, Hkv=2, tq=100, tk=100, D=128, in_fmt=2, fp8=0, numerics=0, strides=None, workspace=one, wsb=ws):
        return L.qattn_fp8_quant_attention_varlen_forward(q, one, one, strides, in_fmt, out, None, cu, one, None, B, Hq, Hkv, tq, tk, D, fp8,
                                                          numerics, 0, 0.0, None, None, None, None, workspace, wsb, None)

    assert call(q=None) == -1 and call(out=None) == -1 and call(cu=None) == -1
    assert call(B=0) == -1 and call(Hq=0) == -1 and call(tq=-1) == -1
    assert call(D=96) == -2 and call(Hq=3) == -2
    assert call(in_fmt=0) == -3 and call(fp8=2) == -3
    assert call(numerics=5) == -1
    assert call(strides=(ctypes.c_longlong * 6)(512, 128, 4, 128, 256, 128)) == -1   # a stride not a multiple of 8
    assert call(q=ctypes.c_void_p(264)) == -1                                        # a base off 16 bytes
    assert call(workspace=None) == -4
    need = L.qattn_fp8_quant_attention_varlen_workspace_bytes(2, 4, 2, 100, 100, 128)
    assert need > 0 and call(wsb=need - 1) == -4
    assert call(tq=0, wsb=need) == 0   # no query row: nothing to launch
    # sizes: q8 slabs H total D, KFRAG images H D (total + 64 B)
    assert L.qattn_varlen_tensor_bytes(_native.LAYOUT_ROWMAJOR, 3, 4, 100, 128) == 4 * 100 * 128
    assert L.qattn_varlen_tensor_bytes(_native.LAYOUT_KFRAG, 3, 4, 100, 128) == 4 * 128 * (100 + 192)
    assert L.qattn_varlen_tensor_bytes(_native.LAYOUT_VFRAG, 3, 4, 100, 128) == 0
    assert L.qattn_fp8_quant_attention_varlen_workspace_bytes(0, 4, 2, 100, 100, 128) == 0


def test_fake_impl_of_the_varlen_op():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from quantumattention_amd import ops  # noqa: F401  (registers the ops)

    with FakeTensorMode():
        q, k = torch.empty(300, 8, 64, dtype=torch.float16, device="cuda"), torch.empty(500, 2, 64, dtype=torch.float16, device="cuda")
        cu = torch.empty(4, dtype=torch.int32, device="cuda")
        out, lse = torch.ops.quantumattention_amd.fp8_varlen_attention_forward(q, k, k, cu, cu, None, 200, 200, True, "e4m3", "compiled", True)
        assert out.shape == (300, 8, 64) and out.dtype == torch.float16 and out.device.type == "cuda"
        assert lse.shape == (8, 300) and lse.dtype == torch.float32
        _, lse = torch.ops.quantumattention_amd.fp8_varlen_attention_forward(q, k, k, cu, cu, None, 200, 200)
        assert lse.shape == (0,)


def _loop_eager(q, k, v, lq, lk, causal, scale):
    """the eager fp8 definition (nn._fp8_attention_eager) called on every sequence, trimmed to its used keys"""
    outs = []
    cq = [0]
    for n in lq:
        cq.append(cq[-1] + n)
    for i, (a, b) in enumerate(zip(cq[:-1], cq[1:])):
        qi = q[a:b].transpose(0, 1)[None]
        ki, vi = (t[i][:lk[i]].transpose(0, 1)[None] for t in (k, v))
        outs.append(qa.nn._fp8_attention_eager(qi, ki, vi, causal, scale, None, None, "head-wise")[0].transpose(0, 1))
    return torch.cat(outs)


def test_force_eager_fallback_is_the_per_sequence_loop_and_ignores_unused_keys():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    lq, lk, S_pad, H, D = [5, 17, 9], [7, 12, 3], 16, 2, 64
    q = torch.randn(sum(lq), H, D, dtype=torch.bfloat16)
    k, v = (torch.randn(len(lk), S_pad, H, D, dtype=torch.bfloat16) for _ in range(2))
    cu_q = torch.tensor([0, 5, 22, 31], dtype=torch.int32)
    cu_k = torch.arange(len(lk) + 1, dtype=torch.int32) * S_pad
    used = torch.tensor(lk, dtype=torch.int32)
    with qa.config.patch({"attention.force_eager_fallback": True, "attention.skip_supported_check": True}):
        for causal in (False, True):
            out, lse = qa.fp8_attn_varlen_func(q, k.flatten(0, 1), v.flatten(0, 1), cu_q, cu_k, 17, S_pad, causal=causal, seqused_k=used,
                                               return_lse=True)
            assert out.shape == q.shape and lse.shape == (H, sum(lq)) and torch.isfinite(lse).all()
            assert torch.equal(out, _loop_eager(q, k, v, lq, lk, causal, None))
            k2, v2 = k.clone(), v.clone()
            for i, n in enumerate(lk):
                k2[i, n:], v2[i, n:] = 1e4, float("nan")
            assert torch.equal(qa.fp8_attn_varlen_func(q, k2.flatten(0, 1), v2.flatten(0, 1), cu_q, cu_k, 17, S_pad, causal=causal,
                                                       seqused_k=used), out)
        # a sequence without keys: zero rows and an LSE of -inf
        out, lse = qa.fp8_attn_varlen_func(q, k.flatten(0, 1), v.flatten(0, 1), cu_q, cu_k, 17, S_pad, seqused_k=torch.tensor([7, 0, 3], dtype=torch.int32),
                                           return_lse=True)
        assert (out[5:22] == 0).all() and (lse[:, 5:22] == -math.inf).all() and torch.isfinite(lse[:, :5]).all()

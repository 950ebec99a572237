"""CPU-only tests of the packed entry's FP8 P.V mode (fp8_attn_varlen_pv_func(..., pv_precision="fp8"),
qattn_fp8_quant_attention_varlen_forward_fp8pv in include/qattn_varlen.h): the function's literal signature beside the unchanged
fp8_attn_varlen_func, the new symbols, the workspace queries, the C entry's argument codes before any device call, the public function's
argument errors, the op's fake implementation and the eager definition with the per-sequence FP8 V restated, held against the fp64 oracle."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import oracle
import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import gpu_utils

NEW = ("qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes", "qattn_fp8_quant_attention_varlen_fp8pv_smooth_workspace_bytes",
       "qattn_fp8_quant_attention_varlen_forward_fp8pv")
VARLEN_PARAMS = ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k", "dropout_p", "softmax_scale", "causal",
                 "seqused_k", "return_lse"]


def test_signature_is_literal_and_the_released_surface_is_unchanged():
    assert list(inspect.signature(qa.fp8_attn_varlen_func).parameters) == VARLEN_PARAMS
    params = inspect.signature(qa.fp8_attn_varlen_pv_func).parameters
    assert list(params) == VARLEN_PARAMS + ["pv_precision", "precision"]
    for name in ("seqused_k", "return_lse", "pv_precision", "precision"):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    for name in VARLEN_PARAMS[:10]:
        assert params[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, name
    assert params["pv_precision"].default == "16bit" and params["precision"].default == "accurate"
    assert params["dropout_p"].default == 0.0 and params["softmax_scale"].default is None and params["causal"].default is False
    assert params["seqused_k"].default is None and params["return_lse"].default is False
    assert len(qa.__all__) == 7 and "fp8_attn_varlen_pv_func" not in qa.__all__


def test_new_symbols_exist_and_the_abi_stays_8():
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW:
        assert name in _native.EXPORTS and getattr(raw, name) is not None
    assert _native.lib().qattn_abi_version() == _native.ABI_VERSION == 8


def test_workspace_queries_are_monotone_and_zero_for_bad_arguments():
    L = _native.lib()
    plain, smooth = L.qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes, L.qattn_fp8_quant_attention_varlen_fp8pv_smooth_workspace_bytes
    base = dict(B=3, Hq=4, Hkv=2, total_q=300, total_k=500, D=128)
    order = ("B", "Hq", "Hkv", "total_q", "total_k", "D")
    for f in (plain, smooth):
        assert f(0, 4, 2, 300, 500, 128) == 0 and f(3, 0, 2, 300, 500, 128) == 0 and f(3, 4, 0, 300, 500, 128) == 0
        assert f(3, 4, 2, -1, 500, 128) == 0 and f(3, 4, 2, 300, -1, 128) == 0 and f(3, 4, 2, 300, 500, 96) == 0
        need = f(*[base[n] for n in order])
        assert need > 0 and need % 16 == 0
        for name, bigger in (("B", 4), ("Hq", 8), ("Hkv", 4), ("total_q", 301), ("total_k", 501), ("D", 256)):
            args = dict(base, **{name: bigger})
            assert f(*[args[n] for n in order]) >= need, name
        for name, bigger in (("B", 40), ("Hq", 8), ("Hkv", 4), ("total_q", 3000), ("total_k", 5000), ("D", 256)):
            args = dict(base, **{name: bigger})
            assert f(*[args[n] for n in order]) > need, name
    need = plain(3, 4, 2, 300, 500, 128)
    # at least: q8 and the KFRAG and VFRAG images (64 keys of padding per sequence)
    assert need >= 4 * 300 * 128 + 2 * (2 * 128 * (500 + 64 * 3))
    assert smooth(3, 4, 2, 300, 500, 128) > need
    # the FP8 V images on top of what the 16-bit-PV entry needs
    assert need > L.qattn_fp8_quant_attention_varlen_workspace_bytes(3, 4, 2, 300, 500, 128)


def test_c_entry_rejects_bad_arguments_before_any_device_call():
    L = _native.lib()
    one = ctypes.c_void_p(256)   # any non-NULL, 16-byte aligned pointer: the checks come first
    ws = 1 << 40

    def call(q=one, k=one, v=one, out=one, cu_q=one, cu_k=one, B=2, Hq=4, Hkv=2, total_q=300, total_k=300, D=128, in_fmt=2, fp8=0, numerics=0,
             precision=2, strides=None, k_mean=None, workspace=one, wsb=ws):
        return L.qattn_fp8_quant_attention_varlen_forward_fp8pv(q, k, v, strides, in_fmt, out, None, cu_q, cu_k, None, B, Hq, Hkv, total_q, total_k,
                                                                D, fp8, numerics, 0, 0.0, precision, None, None, None, None, None, None, None,
                                                                k_mean, workspace, wsb, None)

    assert call(q=None) == -1 and call(k=None) == -1 and call(v=None) == -1 and call(out=None) == -1
    assert call(cu_q=None) == -1 and call(cu_k=None) == -1
    assert call(B=0) == -1 and call(Hq=0) == -1 and call(Hkv=0) == -1 and call(total_q=-1) == -1 and call(total_k=-1) == -1
    assert call(D=96) == -2 and call(Hq=3) == -2
    assert call(in_fmt=0) == -3 and call(fp8=2) == -3
    assert call(numerics=5) == -1
    assert call(precision=0) == -1 and call(precision=3) == -1 and call(precision=-1) == -1   # AUTO and unknown enums: no rescue pass here
    assert call(strides=(ctypes.c_longlong * 6)(512, 128, 256, 128, 256, -8)) == -1   # a negative stride
    assert call(strides=(ctypes.c_longlong * 6)(512, 128, 256, 128, 260, 128)) == -1  # rows off 16 bytes
    assert call(q=ctypes.c_void_p(264)) == -1                        # a base off 16 bytes
    assert call(k_mean=ctypes.c_void_p(264)) == -1                   # k_mean off 16 bytes
    assert call(workspace=None) == -4
    need = L.qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes(2, 4, 2, 300, 300, 128)
    for precision in (1, 2):
        assert need > 0 and call(precision=precision, wsb=need - 1) == -4
    need_s = L.qattn_fp8_quant_attention_varlen_fp8pv_smooth_workspace_bytes(2, 4, 2, 300, 300, 128)
    assert call(k_mean=one, wsb=need_s - 1) == -4   # with smoothing the larger workspace is asked for
    assert call(total_q=0, wsb=L.qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes(2, 4, 2, 0, 300, 128)) == 0   # no query row: nothing to do


def _packed(lens_q, lens_k, Hq, Hkv, D, dtype):
    q = torch.randn(sum(lens_q), Hq, D).to(dtype)
    k, v = (torch.randn(sum(lens_k), Hkv, D).to(dtype) for _ in range(2))
    cu = lambda lens: torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    return q, k, v, cu(lens_q), cu(lens_k)


def test_public_function_rejects_auto_and_unknown_modes():
    q, k, v, cu_q, cu_k = _packed([5, 9], [5, 9], 2, 2, 64, torch.bfloat16)
    args = (q, k, v, cu_q, cu_k, 9, 9)
    with qa.config.patch({"attention.force_eager_fallback": True, "attention.skip_supported_check": True}):
        with pytest.raises(ValueError, match="precision"):
            qa.fp8_attn_varlen_pv_func(*args, pv_precision="fp8", precision="auto")
        with pytest.raises(ValueError, match="precision"):
            qa.fp8_attn_varlen_pv_func(*args, pv_precision="fp8", precision="exact")
        with pytest.raises(ValueError, match="pv_precision"):
            qa.fp8_attn_varlen_pv_func(*args, pv_precision="auto")
        with pytest.raises(ValueError, match="pv_precision"):
            qa.fp8_attn_varlen_pv_func(*args, pv_precision="fp16")
        with pytest.raises(ValueError, match="precision"):
            qa.fp8_attn_varlen_pv_func(*args, pv_precision="16bit", precision="fast")
        with pytest.raises(ValueError, match="precision"):
            qa.fp8_attn_varlen_pv_func(*args, precision="auto")
        # the default call is the released function
        for causal in (False, True):
            a = qa.fp8_attn_varlen_pv_func(*args, causal=causal, return_lse=True)
            b = qa.fp8_attn_varlen_func(*args, causal=causal, return_lse=True)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="precision"):
        _native.fp8_quant_attention_varlen_fp8pv(q, k, v, cu_q, cu_k, precision="auto")


def test_fake_impl_of_the_new_op():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from quantumattention_amd import ops  # noqa: F401  (registers the ops)

    with FakeTensorMode():
        q, k = torch.empty(300, 8, 64, dtype=torch.float16, device="cuda"), torch.empty(500, 2, 64, dtype=torch.float16, device="cuda")
        cu = torch.empty(4, dtype=torch.int32, device="cuda")
        op = torch.ops.quantumattention_amd.fp8_varlen_attention_forward_fp8pv
        out, lse = op(q, k, k, cu, cu, None, 300, 500, True, "e4m3", "compiled", True, False, "fast")
        assert out.shape == (300, 8, 64) and out.dtype == torch.float16 and out.device.type == "cuda" and out.is_contiguous()
        assert lse.shape == (8, 300) and lse.dtype == torch.float32 and lse.stride() == (300, 1)
        out, lse = op(q, k, k, cu, cu, scale=0.3)
        assert out.shape == (300, 8, 64) and lse.shape == (0,)
    # the first op's schema is the released one
    schema = str(torch.ops.quantumattention_amd.fp8_varlen_attention_forward.default._schema)
    assert "precision" not in schema and schema.count("Tensor") == 8, schema


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("fp8,dtype", [("e4m3", torch.bfloat16), ("e5m2", torch.float16)])
def test_eager_definition_agrees_with_the_fp64_oracle_on_the_fp8_v_of_the_used_keys(fp8, dtype, causal):
    """force_eager_fallback with pv_precision="fp8": fp32 attention on the eager quantiser's q, k AND head-wise FP8 V of each sequence's
    used keys, against oracle.attention_forward (fp64) on those same quantised tensors; the bound is the fp8-V bound of tests/gpu_utils.py
    (grade with a plain array).  Sequence 1 uses fewer keys than its slot holds, with NaN behind them."""
    torch.manual_seed(2)
    torch.set_num_threads(4)
    Hq, Hkv, D = 4, 2, 64
    lq, slots, used = [70, 130, 3], [90, 200, 40], [90, 150, 40]
    q, k, v, cu_q, cu_k = _packed(lq, slots, Hq, Hkv, D, dtype)
    k[cu_k[1] + used[1]:cu_k[2]] = float("nan")
    v[cu_k[1] + used[1]:cu_k[2]] = float("nan")
    su = torch.tensor(used, dtype=torch.int32)
    with qa.config.patch({"attention.force_eager_fallback": True, "attention.skip_supported_check": True, "attention.fp8_format": fp8}):
        out, lse = qa.fp8_attn_varlen_pv_func(q, k, v, cu_q, cu_k, max(lq), max(slots), softmax_scale=0.2, causal=causal, seqused_k=su,
                                              return_lse=True, pv_precision="fp8", precision="fast")
        out16 = qa.fp8_attn_varlen_func(q, k, v, cu_q, cu_k, max(lq), max(slots), softmax_scale=0.2, causal=causal, seqused_k=su)
    assert out.shape == q.shape and out.dtype == dtype and lse.shape == (Hq, sum(lq))
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    assert not torch.equal(out, out16), "the FP8 V must show in the result"
    tdt, f, b8 = gpu_utils.TDT[fp8], gpu_utils.FMT[fp8], gpu_utils.bits8
    for i, (n, m) in enumerate(zip(lq, used)):
        a, b = int(cu_q[i]), int(cu_k[i])
        seq = lambda t, s, c: t[s:s + c].transpose(0, 1)[None]
        q8, sq = qa.nn._dynamically_quantize_fp8(seq(q, a, n), reduction_dim=[2, 3], fp8_dtype=tdt)
        k8, sk = qa.nn._dynamically_quantize_fp8(seq(k, b, m), reduction_dim=[2, 3], fp8_dtype=tdt)
        v8, sv = qa.nn._dynamically_quantize_fp8(seq(v, b, m), reduction_dim=[2, 3], fp8_dtype=tdt)
        ref, ref_lse = oracle.attention_forward(b8(q8), b8(k8), b8(v8), f, f, f, sq.numpy(), sk.numpy(), sv.numpy(), causal=causal, sm_scale=0.2,
                                                return_lse=True)
        gpu_utils.assert_within_bound(out[a:a + n].transpose(0, 1)[None].float().numpy(), ref, what=i)
        assert np.abs(lse[:, a:a + n][None].numpy() - ref_lse).max() < 2e-3, i
    assert math.isfinite(float(lse.max()))

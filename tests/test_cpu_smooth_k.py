"""Key smoothing (config.attention.smooth_k, include/qattn_smooth.h) without a GPU: the flag, the boundary, and the eager restatement
(force_eager_fallback's function) on keys with a large per-channel offset shared by all tokens of a head -- the keys of image / video DiTs.

Accuracy bar: the reference's own (tests/test_interface.py): RMSE < 1e-2 against the unquantised computation, here fp64 SDPA on the
16-bit inputs."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, nn
from tests.conftest import ROOT

BAR = 1e-2


def _offset_inputs(seed, dtype, offset_sigma=16.0, B=1, H=4, S=2048, D=128):
    torch.manual_seed(seed)
    q = torch.randn(B, H, S, D)
    k = torch.randn(B, H, S, D) + offset_sigma * torch.randn(B, H, 1, D)
    v = torch.randn(B, H, S, D)
    return q.to(dtype), k.to(dtype), v.to(dtype)


def _rmse_vs_fp64(out, q, k, v):
    ref = torch.nn.functional.scaled_dot_product_attention(q.double(), k.double(), v.double())
    return (out.double() - ref).pow(2).mean().sqrt().item()


def _eager(q, k, v, smooth):
    with qa.config.patch({"attention.smooth_k": smooth}):
        return nn._fp8_attention_eager(q, k, v, False, None, None, None, "head-wise")


def test_flag_is_off_by_default_and_patchable():
    assert qa.config.attention.smooth_k is False
    with qa.config.patch({"attention.smooth_k": True}):
        assert qa.config.attention.smooth_k is True
    assert qa.config.attention.smooth_k is False


def test_public_surface_is_unchanged():
    sdpa = ["query", "key", "value", "attn_mask", "dropout_p", "is_causal", "scale"]
    extra = ["scale_q", "scale_k", "scaling_method", "amax_q", "amax_k", "ssq_q", "ssq_k"]
    assert list(inspect.signature(qa.fp8_attn_func).parameters) == sdpa + extra
    assert list(inspect.signature(qa.nn.fp8_attention).parameters) == sdpa + extra
    assert list(inspect.signature(qa.fp8_token_wise_attn_func).parameters) == sdpa + ["scale_q", "scale_k"]
    assert "smooth_k" not in " ".join(qa.__all__)
    # the op: a trailing keyword whose default keeps every existing call valid
    schema = str(torch.ops.quantumattention_amd.fp8_quant_attention_forward.default._schema)
    assert schema.split("*", 1)[1].count("bool smooth_k=False") == 1, schema


def test_header_functions_are_exported_with_matching_argtypes():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qattn_smooth.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(qattn_[a-z0-9_]+)\s*\(([^)]*)\)", text))
    assert sorted(protos) == ["qattn_fp8_quant_attention_forward_smooth", "qattn_fp8_quant_attention_smooth_workspace_bytes"]
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()

    def ctype(arg):
        arg = arg.strip()
        if "*" in arg:
            return ctypes.c_void_p
        return {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}[arg.rsplit(" ", 1)[0].strip()]

    for name, args in protos.items():
        assert name in _native.EXPORTS and getattr(raw, name) is not None
        assert getattr(L, name).argtypes == [ctype(a) for a in args.split(",")], name
    # the fused entry: qattn_fp8_quant_attention_forward_strided's argument list plus `float* k_mean`
    assert L.qattn_fp8_quant_attention_forward_smooth.argtypes[:-1] == L.qattn_fp8_quant_attention_forward_strided.argtypes
    assert L.qattn_abi_version() == 8
    assert L.qattn_fp8_quant_attention_smooth_workspace_bytes(4, 32, 32, 4096, 4096, 128) > L.qattn_fp8_quant_attention_workspace_bytes(4, 32, 32, 4096)
    assert L.qattn_fp8_quant_attention_smooth_workspace_bytes(1, 1, 1, 1, 1, 96) == 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_eager_path_clears_the_bar_on_offset_keys_only_with_smoothing(seed, dtype):
    q, k, v = _offset_inputs(seed, dtype)
    on = _rmse_vs_fp64(_eager(q, k, v, True), q, k, v)
    off = _rmse_vs_fp64(_eager(q, k, v, False), q, k, v)
    print(f"seed {seed} {dtype}: rmse smooth_k on {on:.5f} off {off:.5f}")
    assert on < BAR, on
    assert off > BAR, off   # guards that the inputs are hard: without smoothing they miss the bar


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_eager_path_on_offset_free_keys_is_fine_either_way(dtype):
    q, k, v = _offset_inputs(0, dtype, offset_sigma=0.0)
    on = _rmse_vs_fp64(_eager(q, k, v, True), q, k, v)
    off = _rmse_vs_fp64(_eager(q, k, v, False), q, k, v)
    print(f"{dtype}: rmse smooth_k on {on:.5f} off {off:.5f}")
    assert on < BAR and off < BAR, (on, off)


@pytest.mark.parametrize("name", ["amax_k", "ssq_k"])
def test_figures_of_the_unsmoothed_key_are_refused_with_the_flag_on(name):
    q, k, v = (torch.randn(1, 2, 64, 128, dtype=torch.bfloat16) for _ in range(3))
    kw = {"amax_k": {"amax_k": torch.ones(1, 2)}, "ssq_k": {"ssq_q": torch.ones(1, 2), "ssq_k": torch.ones(1, 2)}}[name]
    with qa.config.patch({"attention.smooth_k": True, "attention.skip_supported_check": True}):
        with pytest.raises(ValueError, match="unsmoothed key"):
            qa.fp8_attn_func(q, k, v, **kw)
        with pytest.raises(ValueError, match="unsmoothed key"):
            nn._fp8_attention_wrapper(q, k, v, scaling_method="head-wise", **kw)
    with pytest.raises(ValueError, match="unsmoothed key"):   # the binding, whoever calls it
        _native.fp8_quant_attention_forward(q, k, v, is_causal=False, smooth_k=True, **kw)


def test_compiled_region_hands_over_no_figures_of_the_key():
    """Under torch.compile the abs-max of query is still traced into the caller's graph; K's figures are those of key - mean, which only the
    op knows, and the flag itself is an argument of the op (baked in at trace time)."""
    import torch._dynamo

    x, k, v = (torch.randn(1, 2, 128, 128, dtype=torch.bfloat16) for _ in range(3))
    for smooth in (False, True):
        torch._dynamo.reset()
        with qa.config.patch({"attention.skip_supported_check": True, "attention.smooth_k": smooth}):
            gm = torch._dynamo.export(lambda x_, k_, v_: qa.fp8_attn_func(x_ * 1.5, k_, v_))(x, k, v).graph_module
        op = [n for n in gm.graph.nodes if n.op == "call_function" and "fp8_quant_attention_forward" in str(n.target)]
        assert len(op) == 1
        names = "query key value is_causal scaling_method fp8_format numerics precision amax_q amax_k ssq_q ssq_k amax_v".split()
        args = dict(zip(names, op[0].args), **op[0].kwargs)
        assert bool(args.get("smooth_k", False)) is smooth
        assert args.get("amax_q") is not None
        assert (args.get("amax_k") is None) == smooth and (args.get("ssq_k") is None) == smooth and (args.get("ssq_q") is None) == smooth
    torch._dynamo.reset()

"""CPU-only tests of the block-sparse entry (quantumattention_amd.fp8_block_sparse_attn_func, include/qattn_block_sparse.h): the public
surface, the validation reasons, the C entry's argument codes before any device call, the op's fake implementation, and the eager
definition behind config.attention.force_eager_fallback."""
import ctypes
import inspect
import math

import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, block_sparse


def _fake(*shape, dtype=torch.bfloat16):
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        return torch.empty(*shape, dtype=dtype, device="cuda")


def test_public_surface_and_all_is_unchanged():
    assert qa.BLOCK_M == 128 and qa.BLOCK_N == 128 and _native.BLOCK_SPARSE_BLOCK == 128
    assert qa.fp8_block_sparse_attn_func is block_sparse.fp8_block_sparse_attn_func
    params = inspect.signature(qa.fp8_block_sparse_attn_func).parameters
    assert list(params) == ["q", "k", "v", "block_mask", "scale", "return_lse"]
    for n in ("scale", "return_lse"):
        assert params[n].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["scale"].default is None and params["return_lse"].default is False
    assert "fp8_block_sparse_attn_func" not in qa.__all__ and "BLOCK_M" not in qa.__all__ and len(qa.__all__) == 7


def test_validation_rules_give_their_reasons():
    r = block_sparse.block_sparse_input_reason
    q, k = _fake(2, 8, 1000, 128), _fake(2, 2, 999, 128)
    m = _fake(2, 8, 8, 8, dtype=torch.bool)
    assert r(q, k, k, m) is None
    assert r(q, k, k, _fake(1, 1, 8, 8, dtype=torch.bool), scale=0.1) is None      # broadcast over batch and heads
    assert r(q, k, k, _fake(8, 8, dtype=torch.bool)) is None                         # fewer dimensions broadcast too
    assert r(q, k, k, _fake(2, 8, 1, 8, dtype=torch.bool)) is None
    # mask dtype, shape / broadcast, device
    assert "torch.bool" in r(q, k, k, _fake(2, 8, 8, 8, dtype=torch.uint8))
    assert "torch.bool" in r(q, k, k, [[True]])
    for bad in ((2, 8, 7, 8), (2, 8, 8, 9), (3, 8, 8, 8), (2, 4, 8, 8), (1, 2, 8, 8, 8)):
        assert "broadcast to [B, Hq, ceil(Sq/128), ceil(Skv/128)] = [2, 8, 8, 8]" in r(q, k, k, _fake(*bad, dtype=torch.bool)), bad
    assert "block_mask to be on cuda" in r(q, k, k, torch.zeros(2, 8, 8, 8, dtype=torch.bool))
    # tensors
    assert r(_fake(300, 8, 128), k, k, m).startswith("NYI: query, key and value must be 4-D")
    assert r(q, k, k, m, scale=None) is None
    assert r(_fake(2, 8, 1000, 96), _fake(2, 2, 999, 96), _fake(2, 2, 999, 96), m) == "Unsupported head dimension: 96"
    assert "same head dimension" in r(q, _fake(2, 2, 999, 64), _fake(2, 2, 999, 64), m)
    assert "multiple of the key/value heads" in r(q, _fake(2, 3, 999, 128), _fake(2, 3, 999, 128), m)
    assert "dtype" in r(_fake(2, 8, 1000, 128, dtype=torch.float32), k, k, m)
    assert "share a dtype" in r(q, _fake(2, 2, 999, 128, dtype=torch.float16), k, m)
    assert "same shape" in r(q, k, _fake(2, 2, 998, 128), m)
    assert "batch size" in r(q, _fake(1, 2, 999, 128), _fake(1, 2, 999, 128), m)
    assert "non-empty" in r(_fake(2, 8, 0, 128), k, k, _fake(2, 8, 0, 8, dtype=torch.bool))
    qg = torch.empty(1, 2, 256, 64, dtype=torch.bfloat16, requires_grad=True)
    assert "leaf tensors" in r(qg, qg.detach(), qg.detach(), torch.ones(1, 1, 2, 2, dtype=torch.bool))
    cpu = torch.empty(1, 2, 256, 64, dtype=torch.bfloat16)
    assert r(cpu, cpu, cpu, torch.ones(1, 1, 2, 2, dtype=torch.bool)) == "Expected query, key, and value to be on a CUDA device"
    for bad in (0.0, -1.0, math.inf, math.nan, True):
        assert "scale must be a finite number > 0" in r(q, k, k, m, scale=bad), bad
    # the public function raises them as ValueError before any launch; then the device gate (no gfx950 on this box)
    with pytest.raises(ValueError, match="torch.bool"):
        qa.fp8_block_sparse_attn_func(q, k, k, _fake(2, 8, 8, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="gfx950"):
        qa.fp8_block_sparse_attn_func(q, k, k, m)


def test_c_entry_rejects_bad_arguments_before_any_device_call():
    L = _native.lib()
    one = ctypes.c_void_p(256)   # any non-NULL, 16-byte aligned pointer: the checks come first
    ws = 1 << 40

    def call(q=one, out=one, mask=one, B=2, Hq=4, Hkv=2, Sq=300, Skv=300, D=128, in_fmt=2, fp8=0, numerics=0, strides=None, workspace=one,
             wsb=ws):
        return L.qattn_fp8_block_sparse_attention_forward(q, one, one, in_fmt, out, None, mask, strides, B, Hq, Hkv, Sq, Skv, D, fp8, numerics,
                                                          0.0, None, None, None, None, workspace, wsb, None)

    assert call(q=None) == -1 and call(out=None) == -1 and call(mask=None) == -1
    assert call(B=0) == -1 and call(Hq=0) == -1 and call(Sq=0) == -1 and call(Skv=-1) == -1
    assert call(D=96) == -2 and call(Hq=3) == -2
    assert call(in_fmt=0) == -3 and call(fp8=2) == -3
    assert call(numerics=5) == -1
    assert call(strides=(ctypes.c_longlong * 4)(0, 0, 3, -1)) == -1   # a negative stride (0: broadcast, accepted)
    assert call(q=ctypes.c_void_p(264)) == -1                        # a base off 16 bytes
    assert call(D=256, Skv=1 << 20) == -2                            # the key list does not fit the LDS behind the D = 256 ring
    assert call(workspace=None) == -4
    need = L.qattn_fp8_block_sparse_attention_workspace_bytes(2, 4, 2, 300, 300, 128)
    assert need > 0 and call(wsb=need - 1) == -4
    assert L.qattn_fp8_block_sparse_attention_workspace_bytes(0, 4, 2, 300, 300, 128) == 0
    assert L.qattn_fp8_block_sparse_attention_workspace_bytes(2, 4, 2, 300, 300, 96) == 0


def test_fake_impl_of_the_block_sparse_op():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from quantumattention_amd import ops  # noqa: F401  (registers the ops)

    with FakeTensorMode():
        q, k = torch.empty(2, 8, 300, 64, dtype=torch.float16, device="cuda"), torch.empty(2, 2, 500, 64, dtype=torch.float16, device="cuda")
        m = torch.empty(1, 1, 3, 4, dtype=torch.bool, device="cuda").expand(2, 8, 3, 4)
        out, lse = torch.ops.quantumattention_amd.fp8_block_sparse_attention_forward(q, k, k, m, "e4m3", "compiled", True)
        assert out.shape == (2, 8, 300, 64) and out.dtype == torch.float16 and out.device.type == "cuda"
        assert lse.shape == (2, 8, 300) and lse.dtype == torch.float32
        out, lse = torch.ops.quantumattention_amd.fp8_block_sparse_attention_forward(q, k, k, m, scale=0.3)
        assert out.shape == (2, 8, 300, 64) and lse.shape == (0,)
        bf = torch.empty(1, 4, 129, 256, dtype=torch.bfloat16, device="cuda")
        out, lse = torch.ops.quantumattention_amd.fp8_block_sparse_attention_forward(bf, bf, bf, torch.empty(1, 4, 2, 2, dtype=torch.bool,
                                                                                                                   device="cuda"))
        assert out.shape == (1, 4, 129, 256) and out.dtype == torch.bfloat16 and lse.shape == (0,)


def test_force_eager_fallback_skips_masked_blocks_and_gives_zero_rows():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    B, Hq, Hkv, Sq, Skv, D = 1, 4, 2, 300, 260, 64
    q = torch.randn(B, Hq, Sq, D, dtype=torch.bfloat16)
    k, v = (torch.randn(B, Hkv, Skv, D, dtype=torch.bfloat16) for _ in range(2))
    mask = torch.tensor([[True, False, True], [False, False, False], [False, True, False]])   # query block 1 lists no key block
    with qa.config.patch({"attention.force_eager_fallback": True, "attention.skip_supported_check": True}):
        out, lse = qa.fp8_block_sparse_attn_func(q, k, v, mask, return_lse=True)
        assert out.shape == q.shape and out.dtype == q.dtype and lse.shape == (B, Hq, Sq)
        assert (out[:, :, 128:256] == 0).all() and (lse[:, :, 128:256] == -math.inf).all()
        assert torch.isfinite(out).all() and torch.isfinite(lse[:, :, :128]).all() and torch.isfinite(lse[:, :, 256:]).all()
        # keys of blocks a query block does not list change none of its rows (the K scale aside: k keeps its abs-max)
        k2, v2 = k.clone(), v.clone()
        k2[:, :, 128:256] = k2[:, :, 128:256].flip(2)
        v2[:, :, 128:256] = 1e4   # (finite: the eager definition's P.V is one matrix product, in which 0 * NaN would still be NaN)
        out2 = qa.fp8_block_sparse_attn_func(q, k2, v2, mask)
        assert torch.equal(out2[:, :, :128], out[:, :, :128])
        # an all-true mask is dense attention on the de-quantised q and k
        dense = qa.fp8_block_sparse_attn_func(q, k, v, torch.ones(3, 3, dtype=torch.bool), scale=0.2)
        q8, sq = qa.nn._dynamically_quantize_fp8(q, reduction_dim=[2, 3])
        k8, sk = qa.nn._dynamically_quantize_fp8(k, reduction_dim=[2, 3])
        dq, dk = q8.float() * sq[..., None, None], (k8.float() * sk[..., None, None]).repeat_interleave(2, dim=1)
        ref = torch.softmax((dq @ dk.transpose(-1, -2)) * 0.2, dim=-1) @ v.float().repeat_interleave(2, dim=1)
        assert (dense.float() - ref).abs().max() < 2 ** -7

"""CPU-only tests of the sliding-window entries (quantumattention_amd.fp8_attn_varlen_window_func / fp8_window_attn_func,
include/qattn_window.h): the public signatures, the window_size reasons, the C entry's argument codes before any device call, the op's
fake implementation, the exported symbols, and the eager restatement behind config.attention.force_eager_fallback against a per-row
masked fp32 softmax written out here."""
import ctypes
import inspect
import math
import os

import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, varlen


def _fake(*shape, dtype=torch.bfloat16):
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        return torch.empty(*shape, dtype=dtype, device="cuda")


def test_signatures_and_all_is_unchanged():
    params = inspect.signature(qa.fp8_attn_varlen_window_func).parameters
    assert list(params) == ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k", "window_size", "dropout_p",
                            "softmax_scale", "seqused_k", "return_lse"]
    assert params["window_size"].default is inspect.Parameter.empty
    assert params["dropout_p"].default == 0.0 and params["softmax_scale"].default is None
    for n in ("seqused_k", "return_lse"):
        assert params[n].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["seqused_k"].default is None and params["return_lse"].default is False
    dense = inspect.signature(qa.fp8_window_attn_func).parameters
    assert list(dense) == ["q", "k", "v", "window_size", "scale", "return_lse"]
    assert dense["scale"].kind is inspect.Parameter.KEYWORD_ONLY and dense["scale"].default is None
    assert dense["return_lse"].kind is inspect.Parameter.KEYWORD_ONLY and dense["return_lse"].default is False
    assert qa.fp8_attn_varlen_window_func is varlen.fp8_attn_varlen_window_func and qa.fp8_window_attn_func is varlen.fp8_window_attn_func
    assert "fp8_attn_varlen_window_func" not in qa.__all__ and "fp8_window_attn_func" not in qa.__all__ and len(qa.__all__) == 7


def test_window_size_reasons():
    r = varlen.window_size_reason
    for ok in ((0, 0), (-1, -1), [64, 0], (5, -1), (2 ** 40, 3)):
        assert r(ok) is None
    for bad in (7, None, (1,), (1, 2, 3), "ab"):
        assert "a pair (left, right)" in r(bad)
    for bad in ((1.0, 0), (True, 0), (0, None), ("1", "2"), (torch.tensor(1), 0)):
        assert "host ints" in r(bad)
    for bad in ((-2, 0), (0, -2), (-5, -5)):
        assert ">= -1" in r(bad)
    # the public functions raise them as ValueError before any launch; the packed entry's own rules come first, the device gate last
    q, k = _fake(300, 8, 128), _fake(400, 2, 128)
    cu = _fake(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="a pair"):
        qa.fp8_attn_varlen_window_func(q, k, k, cu, cu, 128, 128, 5)
    with pytest.raises(ValueError, match="host ints"):
        qa.fp8_attn_varlen_window_func(q, k, k, cu, cu, 128, 128, (1.5, 0))
    with pytest.raises(ValueError, match=">= -1"):
        qa.fp8_attn_varlen_window_func(q, k, k, cu, cu, 128, 128, (-2, 0))
    with pytest.raises(ValueError, match="dropout_p"):
        qa.fp8_attn_varlen_window_func(q, k, k, cu, cu, 128, 128, (-2, 0), dropout_p=0.5)
    with pytest.raises(ValueError, match="gfx950"):
        qa.fp8_attn_varlen_window_func(q, k, k, cu, cu, 128, 128, (64, 0))
    with pytest.raises(ValueError, match="4-D"):
        qa.fp8_window_attn_func(q, k, k, (64, 0))
    with pytest.raises(ValueError, match=">= -1"):
        qa.fp8_window_attn_func(_fake(2, 8, 100, 64), _fake(2, 2, 100, 64), _fake(2, 2, 100, 64), (0, -3))


def test_c_entry_rejects_bad_arguments_before_any_device_call():
    L = _native.lib()
    one = ctypes.c_void_p(256)   # any non-NULL, 16-byte aligned pointer: the checks come first
    ws = 1 << 40

    def call(q=one, out=one, cu=one, B=2, Hq=4, Hkv=2, tq=100, tk=100, D=128, in_fmt=2, fp8=0, numerics=0, left=64, right=0, strides=None,
             workspace=one, wsb=ws, k_mean=None):
        return L.qattn_fp8_quant_attention_varlen_window_forward(q, one, one, strides, in_fmt, out, None, cu, one, None, B, Hq, Hkv, tq, tk, D,
                                                                 fp8, numerics, left, right, 0.0, None, None, None, None, workspace, wsb, None,
                                                                 k_mean)

    assert call(left=-2) == -1 and call(right=-2) == -1 and call(left=-7, right=-7) == -1
    assert call(q=None) == -1 and call(out=None) == -1 and call(cu=None) == -1
    assert call(B=0) == -1 and call(Hq=0) == -1 and call(tq=-1) == -1
    assert call(D=96) == -2 and call(Hq=3) == -2
    assert call(in_fmt=0) == -3 and call(fp8=2) == -3
    assert call(numerics=5) == -1
    assert call(strides=(ctypes.c_longlong * 6)(512, 128, 4, 128, 256, 128)) == -1   # a stride not a multiple of 8
    assert call(q=ctypes.c_void_p(264)) == -1                                        # a base off 16 bytes
    assert call(k_mean=ctypes.c_void_p(264)) == -1                                   # a misaligned k_mean
    assert call(workspace=None) == -4
    need = L.qattn_fp8_quant_attention_varlen_window_workspace_bytes(2, 4, 2, 100, 100, 128)
    assert need == L.qattn_fp8_quant_attention_varlen_smooth_workspace_bytes(2, 4, 2, 100, 100, 128) > 0
    assert call(wsb=need - 1, k_mean=one) == -4
    # no query row: nothing to launch -- with any legal window, values beyond every length included
    for left, right in ((-1, -1), (0, 0), (2 ** 31 - 1, 2 ** 31 - 1), (-1, 0)):
        assert call(tq=0, wsb=need, left=left, right=right) == 0
    assert L.qattn_fp8_quant_attention_varlen_window_workspace_bytes(0, 4, 2, 100, 100, 128) == 0
    assert L.qattn_fp8_quant_attention_varlen_window_workspace_bytes(2, 4, 2, 100, 100, 96) == 0


def test_new_header_functions_are_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qattn_window.h")).read()
    L = _native.lib()
    for name in ("qattn_fp8_quant_attention_varlen_window_workspace_bytes", "qattn_fp8_quant_attention_varlen_window_forward"):
        assert name + "(" in header and name in _native.EXPORTS
        assert getattr(L, name) is not None
    assert L.qattn_abi_version() == _native.ABI_VERSION   # an addition found by symbol: the ABI number stays


def test_fake_impl_of_the_window_op():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from quantumattention_amd import ops  # noqa: F401  (registers the ops)

    with FakeTensorMode():
        q, k = torch.empty(300, 8, 64, dtype=torch.float16, device="cuda"), torch.empty(500, 2, 64, dtype=torch.float16, device="cuda")
        cu = torch.empty(4, dtype=torch.int32, device="cuda")
        out, lse = torch.ops.quantumattention_amd.fp8_varlen_window_attention_forward(q, k, k, cu, cu, None, 200, 200, 64, 0, "e4m3", "compiled", True)
        assert out.shape == (300, 8, 64) and out.dtype == torch.float16 and out.device.type == "cuda"
        assert lse.shape == (8, 300) and lse.dtype == torch.float32
        _, lse = torch.ops.quantumattention_amd.fp8_varlen_window_attention_forward(q, k, k, cu, cu, None, 200, 200, -1, 5)
        assert lse.shape == (0,)


def _quant(x, fp8_dtype=torch.float8_e4m3fn):
    """the reference's dynamically_quantize_fp8 over the last two dims of [H, L, D], restated"""
    q_max = torch.finfo(fp8_dtype).max
    scale = x.abs().amax((-2, -1), keepdim=True).mul(1.0 / q_max).clamp_min(torch.finfo(torch.float32).eps)
    return (x / scale).clamp(-q_max, q_max).to(fp8_dtype).float() * scale.float()


def _rowwise_reference(q, k, v, lq, lk_pad, lk_used, window, scale=None):
    """Row by row: de-quantised q and used keys of the row's sequence, the keys of the row's window picked by index, fp32 softmax."""
    left, right = window
    Hq, Hkv, D = q.shape[1], k.shape[1], q.shape[2]
    sm = 1.0 / math.sqrt(D) if scale is None else scale
    out = torch.zeros(q.shape, dtype=torch.float32)
    lse = torch.full((Hq, q.shape[0]), -math.inf)
    q0 = k0 = 0
    for n_q, n_pad, n_k in zip(lq, lk_pad, lk_used):
        if n_q and n_k:
            dq = _quant(q[q0:q0 + n_q].transpose(0, 1))
            dk = _quant(k[k0:k0 + n_k].transpose(0, 1))
            vv = v[k0:k0 + n_k].transpose(0, 1).float()
            for r in range(n_q):
                c = r + n_k - n_q
                lo = 0 if left < 0 else max(0, c - left)
                hi = n_k - 1 if right < 0 else min(n_k - 1, c + right)
                if lo > hi:
                    continue
                for h in range(Hq):
                    g = h // (Hq // Hkv)
                    s = (dk[g, lo:hi + 1] @ dq[h, r]) * sm
                    m = s.max()
                    e = torch.exp(s - m)
                    out[q0 + r, h] = (e / e.sum()) @ vv[g, lo:hi + 1]
                    lse[h, q0 + r] = m + torch.log(e.sum())
        q0 += n_q
        k0 += n_pad
    return out, lse


@pytest.mark.parametrize("window", [(0, 0), (3, 0), (-1, 0), (2, 5), (4, -1), (-1, -1), (100, 100)])
def test_force_eager_fallback_is_the_per_row_window_softmax(window):
    torch.manual_seed(1)
    torch.set_num_threads(4)
    # L_q < L_k, L_q > L_k (rows without a key under (.., 0)), equal, and a sequence whose used keys are fewer than its slot
    lq, lk_pad, lk_used, Hq, Hkv, D = [5, 17, 9, 6], [12, 7, 9, 16], [12, 7, 9, 3], 4, 2, 64
    q = torch.randn(sum(lq), Hq, D, dtype=torch.bfloat16)
    k, v = (torch.randn(sum(lk_pad), Hkv, D, dtype=torch.bfloat16) for _ in range(2))
    cu_q = torch.tensor([0, 5, 22, 31, 37], dtype=torch.int32)
    cu_k = torch.tensor([0, 12, 19, 28, 44], dtype=torch.int32)
    used = torch.tensor(lk_used, dtype=torch.int32)
    k2, v2 = k.clone(), v.clone()
    k2[28 + 3:], v2[28 + 3:] = 1e4, float("nan")   # the unused keys of the last sequence
    ref, ref_lse = _rowwise_reference(q, k, v, lq, lk_pad, lk_used, window)
    with qa.config.patch({"attention.force_eager_fallback": True, "attention.skip_supported_check": True}):
        out, lse = qa.fp8_attn_varlen_window_func(q, k2, v2, cu_q, cu_k, 17, 16, window, seqused_k=used, return_lse=True)
        assert torch.equal(qa.fp8_attn_varlen_window_func(q, k2, v2, cu_q, cu_k, 17, 16, window, seqused_k=used), out)
    assert out.shape == q.shape and out.dtype == q.dtype and lse.shape == (Hq, sum(lq)) and lse.dtype == torch.float32
    empty = torch.isinf(ref_lse)
    if window[1] == 0:   # delta = -10 in sequence 1, -3 in sequence 3: their first rows have no key
        assert empty[:, 5:15].all() and not empty[:, 15:22].any() and empty[:, 31:34].all() and not empty[:, :5].any()
    else:
        assert empty.any() == (window == (2, 5))   # (rows 0 .. 4 of sequence 1 end before key 0 under right = 5)
    assert torch.equal(torch.isinf(lse), empty) and (lse[empty] == -math.inf).all()
    assert (out.transpose(0, 1)[empty] == 0).all()
    # fp32 against fp32 on the same de-quantised operands: summation order and the bf16 rounding of `out` are all that differ
    assert torch.allclose(lse[~empty], ref_lse[~empty], rtol=0, atol=2e-5)
    assert torch.allclose(out.float(), ref, rtol=2.0 ** -8, atol=2.0 ** -8)


def test_eager_fallback_window_follows_smooth_k_and_the_dense_shape():
    torch.manual_seed(2)
    torch.set_num_threads(4)
    B, Hq, Hkv, S, D = 2, 4, 2, 40, 64
    q = torch.randn(B, S, Hq, D, dtype=torch.bfloat16).transpose(1, 2)           # [B, H, S, D] views of [B, S, H, D] memory
    k = (torch.randn(B, S, Hkv, D) + 8.0).to(torch.bfloat16).transpose(1, 2)     # offset keys: smoothing changes the quantisation
    v = torch.randn(B, S, Hkv, D, dtype=torch.bfloat16).transpose(1, 2)
    cu = torch.arange(B + 1, dtype=torch.int32) * S
    pk = lambda t: t.transpose(1, 2).reshape(B * S, t.shape[1], D)
    with qa.config.patch({"attention.force_eager_fallback": True, "attention.skip_supported_check": True}):
        out, lse = qa.fp8_window_attn_func(q, k, v, (7, 2), return_lse=True)
        po, pl = qa.fp8_attn_varlen_window_func(pk(q), pk(k), pk(v), cu, cu, S, S, (7, 2), return_lse=True)
        with qa.config.patch({"attention.smooth_k": True}):
            so, sl = qa.fp8_window_attn_func(q, k, v, (7, 2), return_lse=True)
    assert out.shape == (B, Hq, S, D) and lse.shape == (B, Hq, S)
    assert torch.equal(out, po.view(B, S, Hq, D).permute(0, 2, 1, 3)) and torch.equal(lse, pl.view(Hq, B, S).permute(1, 0, 2))
    # smoothing is a change of quantisation only: against the unquantised fp32 window attention it lands closer than the plain call on
    # these offset keys, in `out` and -- the LSE being corrected back to the true scores -- in the LSE
    d = torch.arange(S)[None, :] - torch.arange(S)[:, None]
    s = (q.float() @ k.float().repeat_interleave(Hq // Hkv, 1).transpose(-1, -2)) / math.sqrt(D)
    s = s.masked_fill(~((d >= -7) & (d <= 2)), -math.inf)
    exact, exact_lse = torch.softmax(s, -1) @ v.float().repeat_interleave(Hq // Hkv, 1), torch.logsumexp(s, -1)
    assert not torch.equal(so, out)
    assert (so.float() - exact).abs().max() < (out.float() - exact).abs().max()
    assert (sl - exact_lse).abs().max() < (lse - exact_lse).abs().max()

"""CPU-only tests of the sliding-window entry's FP8 P.V mode (fp8_attn_varlen_window_pv_func / fp8_window_attn_pv_func with
pv_precision="fp8", qattn_fp8_quant_attention_varlen_window_forward_fp8pv in include/qattn_window.h): the literal signatures beside the
unchanged released window functions, the new symbol, the C entry's argument codes before any device call, the public functions' argument
errors, the op's fake implementation, the eager definition held against an fp64 windowed softmax written here, the literal FAST rule
against the packed entry's table, and the teeth of the membership-probe cases tests/test_gpu_window_fp8.py runs."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import gpu_utils
from tests import probes as P
from tests import window_fp8_cases as W

NEW = "qattn_fp8_quant_attention_varlen_window_forward_fp8pv"
WINDOW_PARAMS = ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k", "window_size", "dropout_p", "softmax_scale",
                 "seqused_k", "return_lse"]
DENSE_PARAMS = ["q", "k", "v", "window_size", "scale", "return_lse"]


def test_signatures_are_literal_and_the_released_surface_is_unchanged():
    assert list(inspect.signature(qa.fp8_attn_varlen_window_func).parameters) == WINDOW_PARAMS
    assert list(inspect.signature(qa.fp8_window_attn_func).parameters) == DENSE_PARAMS
    params = inspect.signature(qa.fp8_attn_varlen_window_pv_func).parameters
    assert list(params) == WINDOW_PARAMS + ["pv_precision", "precision"]
    for name in ("seqused_k", "return_lse", "pv_precision", "precision"):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    for name in WINDOW_PARAMS[:10]:
        assert params[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, name
    assert params["window_size"].default is inspect.Parameter.empty
    assert params["pv_precision"].default == "16bit" and params["precision"].default == "accurate"
    assert params["dropout_p"].default == 0.0 and params["softmax_scale"].default is None
    assert params["seqused_k"].default is None and params["return_lse"].default is False
    dense = inspect.signature(qa.fp8_window_attn_pv_func).parameters
    assert list(dense) == DENSE_PARAMS + ["pv_precision", "precision"]
    for name in ("scale", "return_lse", "pv_precision", "precision"):
        assert dense[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert dense["scale"].default is None and dense["return_lse"].default is False
    assert dense["pv_precision"].default == "16bit" and dense["precision"].default == "accurate"
    assert len(qa.__all__) == 7 and "fp8_attn_varlen_window_pv_func" not in qa.__all__ and "fp8_window_attn_pv_func" not in qa.__all__


def test_new_symbol_exists_and_the_abi_stays_8():
    raw = ctypes.CDLL(_native.LIB_PATH)
    assert NEW in _native.EXPORTS and getattr(raw, NEW) is not None
    assert _native.lib().qattn_abi_version() == _native.ABI_VERSION == 8


def test_c_entry_rejects_bad_arguments_before_any_device_call():
    L = _native.lib()
    one = ctypes.c_void_p(256)   # any non-NULL, 16-byte aligned pointer: the checks come first
    ws = 1 << 40

    def call(q=one, k=one, v=one, out=one, cu_q=one, cu_k=one, B=2, Hq=4, Hkv=2, total_q=300, total_k=300, D=128, in_fmt=2, fp8=0, numerics=0,
             left=16, right=0, precision=2, strides=None, k_mean=None, workspace=one, wsb=ws):
        return getattr(L, NEW)(q, k, v, strides, in_fmt, out, None, cu_q, cu_k, None, B, Hq, Hkv, total_q, total_k, D, fp8, numerics, left, right,
                               0.0, precision, None, None, None, None, None, None, None, k_mean, workspace, wsb, None)

    assert call(left=-2) == -1 and call(right=-2) == -1 and call(left=-2 ** 31) == -1 and call(right=-7) == -1
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
    # the workspace is the packed FP8-PV entry's: sized by its two functions
    need = L.qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes(2, 4, 2, 300, 300, 128)
    for precision in (1, 2):
        for window in ((-1, -1), (0, 0), (2 ** 31 - 1, 5)):
            assert need > 0 and call(precision=precision, left=window[0], right=window[1], wsb=need - 1) == -4
    need_s = L.qattn_fp8_quant_attention_varlen_fp8pv_smooth_workspace_bytes(2, 4, 2, 300, 300, 128)
    assert call(k_mean=one, wsb=need_s - 1) == -4   # with smoothing the larger workspace is asked for
    assert call(total_q=0, wsb=L.qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes(2, 4, 2, 0, 300, 128)) == 0   # no query row: nothing to do


def _packed(lens_q, lens_k, Hq, Hkv, D, dtype):
    q = torch.randn(sum(lens_q), Hq, D).to(dtype)
    k, v = (torch.randn(sum(lens_k), Hkv, D).to(dtype) for _ in range(2))
    cu = lambda lens: torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    return q, k, v, cu(lens_q), cu(lens_k)


def test_public_functions_reject_auto_and_unknown_modes():
    q, k, v, cu_q, cu_k = _packed([5, 9], [5, 9], 2, 2, 64, torch.bfloat16)
    args = (q, k, v, cu_q, cu_k, 9, 9, (3, 0))
    dq, dk = torch.randn(2, 2, 7, 64).bfloat16(), torch.randn(2, 2, 9, 64).bfloat16()
    with qa.config.patch({"attention.force_eager_fallback": True, "attention.skip_supported_check": True}):
        for f, a in ((qa.fp8_attn_varlen_window_pv_func, args), (qa.fp8_window_attn_pv_func, (dq, dk, dk, (3, 0)))):
            with pytest.raises(ValueError, match="precision"):
                f(*a, pv_precision="fp8", precision="auto")
            with pytest.raises(ValueError, match="precision"):
                f(*a, pv_precision="fp8", precision="exact")
            with pytest.raises(ValueError, match="pv_precision"):
                f(*a, pv_precision="auto")
            with pytest.raises(ValueError, match="pv_precision"):
                f(*a, pv_precision="fp16")
            with pytest.raises(ValueError, match="precision"):
                f(*a, pv_precision="16bit", precision="fast")
            with pytest.raises(ValueError, match="precision"):
                f(*a, precision="auto")
        # the default call is the released function
        a = qa.fp8_attn_varlen_window_pv_func(*args, return_lse=True)
        b = qa.fp8_attn_varlen_window_func(*args, return_lse=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        a = qa.fp8_window_attn_pv_func(dq, dk, dk, (3, 0), return_lse=True)
        b = qa.fp8_window_attn_func(dq, dk, dk, (3, 0), return_lse=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        # the dense form is the packed sibling on views
        a = qa.fp8_window_attn_pv_func(dq, dk, dk, (3, 1), return_lse=True, pv_precision="fp8", precision="fast")
        steps = torch.arange(3, dtype=torch.int32)
        pk = dk.permute(0, 2, 1, 3).reshape(18, 2, 64)
        b = qa.fp8_attn_varlen_window_pv_func(dq.permute(0, 2, 1, 3).reshape(14, 2, 64), pk, pk, steps * 7, steps * 9, 7, 9, (3, 1), return_lse=True,
                                              pv_precision="fp8", precision="fast")
        assert torch.equal(a[0], b[0].view(2, 7, 2, 64).permute(0, 2, 1, 3)) and torch.equal(a[1], b[1].view(2, 2, 7).permute(1, 0, 2))
    # window_size_reason applies unchanged
    with qa.config.patch({"attention.force_eager_fallback": True}):
        with pytest.raises(ValueError, match="window_size"):
            qa.fp8_window_attn_pv_func(dq, dk, dk, (3, -2), pv_precision="fp8")
    with pytest.raises(ValueError, match="precision"):
        _native.fp8_quant_attention_varlen_window_fp8pv(q, k, v, cu_q, cu_k, precision="auto")
    with pytest.raises(ValueError, match="window"):
        _native.fp8_quant_attention_varlen_window_fp8pv(q, k, v, cu_q, cu_k, window_left=-2)


def test_fake_impl_of_the_new_op():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from quantumattention_amd import ops  # noqa: F401  (registers the ops)

    with FakeTensorMode():
        q, k = torch.empty(300, 8, 64, dtype=torch.float16, device="cuda"), torch.empty(500, 2, 64, dtype=torch.float16, device="cuda")
        cu = torch.empty(4, dtype=torch.int32, device="cuda")
        op = torch.ops.quantumattention_amd.fp8_varlen_window_attention_forward_fp8pv
        out, lse = op(q, k, k, cu, cu, None, 300, 500, 16, 0, "e4m3", "compiled", True, False, "fast")
        assert out.shape == (300, 8, 64) and out.dtype == torch.float16 and out.device.type == "cuda" and out.is_contiguous()
        assert lse.shape == (8, 300) and lse.dtype == torch.float32 and lse.stride() == (300, 1)
        out, lse = op(q, k, k, cu, cu, scale=0.3)
        assert out.shape == (300, 8, 64) and lse.shape == (0,)
    # the first window op's schema is the released one
    schema = str(torch.ops.quantumattention_amd.fp8_varlen_window_attention_forward.default._schema)
    assert "precision" not in schema and schema.count("Tensor") == 8, schema


# ---- the eager definition -------------------------------------------------------------------------------------------------------------------
LQ, LK = [300, 1, 70], [260, 5, 70]    # L_q > L_k (40 leading rows without a key under right = 0), L_q < L_k, L_q = L_k
EAGER_WINDOWS = [(0, 0), (16, 0), (5, -1), (-1, 0)]


def _deq(t8, s):
    return t8.float().double().numpy()[0] * s.double().numpy()[0][:, None, None]


def _eager_reference(q, k, v, lq, used, starts_k, window, scale, tdt, smooth=False):
    """fp64 windowed softmax (W.window_softmax64, numpy) on the eager quantiser's q, k and fp8 V of the used keys.  smooth: k quantised as
    fp32(k) - the fp32 channel mean of the used keys, the LSE of a row with keys raised by scale * q.mean (the caller's 16-bit q)"""
    outs, lses, a = [], [], 0
    for n, m, b in zip(lq, used, starts_k):
        seq = lambda t, s, c: t[s:s + c].transpose(0, 1)[None]
        if n and m:
            q8, sq = qa.nn._dynamically_quantize_fp8(seq(q, a, n), reduction_dim=[2, 3], fp8_dtype=tdt)
            ki = seq(k, b, m)
            if smooth:
                ki = ki.float()
                mean = ki.mean(dim=-2, keepdim=True)
                ki = ki - mean
            k8, sk = qa.nn._dynamically_quantize_fp8(ki, reduction_dim=[2, 3], fp8_dtype=tdt)
            v8, sv = qa.nn._dynamically_quantize_fp8(seq(v, b, m), reduction_dim=[2, 3], fp8_dtype=tdt)
            o, l = W.window_softmax64(_deq(q8, sq), _deq(k8, sk), _deq(v8, sv), window, scale)
            if smooth:
                mq = np.repeat(mean.double().numpy()[0], q.shape[1] // k.shape[1], 0)           # [Hq, 1, D]
                l = l + scale * (seq(q, a, n).double().numpy()[0] * mq).sum(-1)                # (-inf stays -inf)
        else:
            o, l = np.zeros((q.shape[1], n, q.shape[2])), np.full((q.shape[1], n), -np.inf)
        outs.append(o.transpose(1, 0, 2))
        lses.append(l)
        a += n
    return np.concatenate(outs, 0), np.concatenate(lses, 1)


@pytest.mark.parametrize("window", EAGER_WINDOWS)
@pytest.mark.parametrize("fp8,dtype", [("e4m3", torch.bfloat16), ("e5m2", torch.float16)])
def test_eager_definition_agrees_with_an_fp64_windowed_softmax_on_the_fp8_v_of_the_used_keys(fp8, dtype, window):
    """force_eager_fallback with pv_precision="fp8"; bound: the fp8-V bound of tests/gpu_utils.py (grade with a plain array), LSE 2e-3.
    Sequence 0 has 40 more queries than keys: under right = 0 its first 40 rows have no key -- zeros, -inf, no NaN."""
    torch.manual_seed(3)
    torch.set_num_threads(4)
    Hq, Hkv, D, scale = 4, 2, 64, 0.2
    q, k, v, cu_q, cu_k = _packed(LQ, LK, Hq, Hkv, D, dtype)
    with qa.config.patch({"attention.force_eager_fallback": True, "attention.skip_supported_check": True, "attention.fp8_format": fp8}):
        out, lse = qa.fp8_attn_varlen_window_pv_func(q, k, v, cu_q, cu_k, max(LQ), max(LK), window, softmax_scale=scale, return_lse=True,
                                                     pv_precision="fp8", precision="fast")
        out16 = qa.fp8_attn_varlen_window_func(q, k, v, cu_q, cu_k, max(LQ), max(LK), window, softmax_scale=scale)
    assert out.shape == q.shape and out.dtype == dtype and lse.shape == (Hq, sum(LQ))
    assert torch.isfinite(out.float()).all() and not torch.isnan(lse).any()
    assert not torch.equal(out, out16), "the FP8 V must show in the result"
    ref, ref_lse = _eager_reference(q, k, v, LQ, LK, [int(x) for x in cu_k[:-1]], window, scale, gpu_utils.TDT[fp8])
    dead = np.isneginf(ref_lse)
    if window[1] == 0:
        assert dead[:, :40].all() and not dead[:, 40:].any()
    else:
        assert not dead.any()
    assert np.array_equal(np.isneginf(lse.numpy()), dead)
    assert (out.float().numpy()[dead.T] == 0).all()
    gpu_utils.assert_within_bound(out.float().numpy(), ref, what=window)
    assert np.abs(lse.numpy()[~dead] - ref_lse[~dead]).max() < 2e-3


def test_eager_definition_with_seqused_k_and_nan_behind_it():
    torch.manual_seed(4)
    torch.set_num_threads(4)
    Hq, Hkv, D, scale, window = 4, 2, 64, 0.2, (16, 0)
    slots, used = [300, 9, 130], [260, 5, 70]
    q, k, v, cu_q, cu_k = _packed(LQ, slots, Hq, Hkv, D, torch.bfloat16)
    for i, (m, a) in enumerate(zip(used, slots)):
        k[cu_k[i] + m:cu_k[i] + a] = float("nan")
        v[cu_k[i] + m:cu_k[i] + a] = float("nan")
    su = torch.tensor(used, dtype=torch.int32)
    for smooth in (False, True):
        with qa.config.patch({"attention.force_eager_fallback": True, "attention.skip_supported_check": True, "attention.smooth_k": smooth}):
            out, lse = qa.fp8_attn_varlen_window_pv_func(q, k, v, cu_q, cu_k, max(LQ), max(slots), window, softmax_scale=scale, seqused_k=su,
                                                         return_lse=True, pv_precision="fp8")
        assert not torch.isnan(out.float()).any() and not torch.isnan(lse).any()
        ref, ref_lse = _eager_reference(q, k, v, LQ, used, [int(x) for x in cu_k[:-1]], window, scale, torch.float8_e4m3fn, smooth)
        dead = np.isneginf(ref_lse)
        assert dead[:, :40].all() and np.array_equal(np.isneginf(lse.numpy()), dead)
        gpu_utils.assert_within_bound(out.float().numpy(), ref, what=("seqused", smooth))
        assert np.abs(lse.numpy()[~dead] - ref_lse[~dead]).max() < 2e-3


# ---- the literal FAST rule ------------------------------------------------------------------------------------------------------------------
def _packed_rule(n_q, m, causal, precision):
    """tests/test_gpu_varlen_fp8.py's _expected_path formula, written out: tile t sees n = used L_k keys (causal: min(L_k, 128 (t + 1)));
    ACCURATE two-term everywhere, FAST one-term iff n >= 1024; no used key: the one-term code"""
    r = np.arange(n_q)
    n = np.minimum(m, 128 * (r // 128 + 1)) if causal else np.full(n_q, m)
    one = (n == 0) | ((n >= 1024) if precision == "fast" else False)
    return np.where(one, 0, 1).astype(np.uint8)


@pytest.mark.parametrize("precision", ["accurate", "fast"])
def test_the_literal_fast_rule_gives_the_packed_rules_table_where_the_masks_agree(precision):
    lens = [1, 63, 128, 129, 1023, 1024, 1025, 1100, 1300, 2304]
    for n in lens:
        # (-1, 0) on equal lengths: the causal rule, n = min(L_k, 128 (t + 1))
        assert np.array_equal(W.expected_path([n], [n], 1, (-1, 0), precision)[0], _packed_rule(n, n, True, precision)), n
        for t in range((n + 127) // 128):
            assert W.tile_interval(n, n, -1, 0, t) == (0, min(n, 128 * (t + 1)) - 1)
        # (-1, -1): the non-causal rule, n = L_k, at any pair of lengths
        for m in (0, 1, 1023, 1024, 1300):
            assert np.array_equal(W.expected_path([n], [m], 1, (-1, -1), precision)[0], _packed_rule(n, m, False, precision)), (n, m)
            if m:
                assert W.tile_interval(n, m, -1, -1, 0) == (0, m - 1)
    # finite windows: (1024, 0) reaches 1024 keys from tile 7 on (klo = 0, khi = 1023); (600, 500) and (512, 512) in the interior
    p = W.expected_path([2304], [2304], 1, (1024, 0), "fast")[0]
    first = np.argmax(p == W.ONE)
    assert (p[:first] == W.TWO).all() and (p[first:] == W.ONE).all() and first == 128 * 7   # tile 7: klo = 0, khi = 1023
    assert W.tile_interval(2304, 2304, 1024, 0, 7) == (0, 1023) and W.tile_interval(2304, 2304, 1024, 0, 9) == (128, 1279)
    assert (W.expected_path([2304], [2304], 1, (1024, 0), "accurate") == W.TWO).all()
    p = W.expected_path([1300], [1300], 1, (600, 500), "fast")[0]
    assert (p == W.ONE).any() and (p == W.TWO).any()
    p = W.expected_path([2304], [2304], 1, (512, 512), "fast")[0]   # interior tiles: 512 + 128 + 512 = 1152 keys
    assert (p[:384] == W.TWO).all() and (p[384:1792] == W.ONE).all() and (p[-128:] == W.TWO).all()
    # every row of a one-term tile attends at least n - 127 keys (the causal rule's own worst case)
    for window, n, m in (((1024, 0), 2304, 2304), ((600, 500), 1300, 1300), ((-1, 0), 1300, 1500), ((900, 300), 700, 1300)):
        ok = W.alive(n, m, window)
        for t in range((n + 127) // 128):
            iv = W.tile_interval(n, m, window[0], window[1], t)
            rows = ok[128 * t:128 * (t + 1)]
            if iv is None:
                assert not rows.any()
                continue
            cols = np.nonzero(rows.any(0))[0]
            assert (cols[0], cols[-1]) == iv, (window, t)
            keyed = rows.sum(1)[rows.any(1)]
            assert keyed.min() >= min(iv[1] - iv[0] + 1 - 127, keyed.max())
    # L_q > L_k with right = 0: leading tiles without a key carry the one-term code under both precisions
    p = W.expected_path([400], [100], 1, (16, 0), precision)[0]
    assert (p[:256] == W.ONE).all() and (p[256:] == W.TWO).all()


# ---- the teeth of the probe cases the GPU file runs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128, 256])
def test_teeth_of_the_probe_cases_against_the_fp8_v_bound(D):
    """one wrongly admitted or dropped key moves the output by >= 4x P.project_bound(ref, False) on every case of W.probe_cases (which
    names what was left out and why)"""
    worst = {}
    for probe, window, lq, lk in W.probe_cases(D):
        teeth = W.case_teeth(W.make_probe(probe, D, window, lq, lk))
        assert teeth, (probe, window)
        worst[(probe, window, tuple(lq))] = min(teeth.values())
        assert all(t >= P.TEETH for t in teeth.values()), (probe, window, lq, {k: v for k, v in teeth.items() if v < P.TEETH})
    print(f"D {D}: least teeth {min(worst.values()):.2f} over {len(worst)} cases")

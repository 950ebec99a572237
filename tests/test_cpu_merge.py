"""Merging of attention states without a GPU (include/qattn_merge.h, quantumattention_amd/merge.py): the eager definition against an
fp64 merge written independently (tests/merge_ref.py), the call surface and its errors, the C entry's argument checks (they return before
any device call), the export, the ops' schemas -- and TEETH: three plausible wrong merges that the bounds of merge_ref must reject."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, merge
from tests import merge_ref as R
from tests.conftest import ROOT

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
INF = math.inf


# ---- the eager definition against the fp64 merge ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n, dtypes, out_dtype", [(2, (BF, BF), BF), (3, (HF, HF, HF), HF), (2, (F32, BF), F32), (8, (BF,) * 8, F32),
                                                  (11, (BF,) * 11, BF)])
@pytest.mark.parametrize("packed", [False, True])
def test_eager_definition_meets_the_bounds_of_the_fp64_merge(n, dtypes, out_dtype, packed):
    B, H, S, D = 2, 3, 37, 64
    shape_o, shape_l = ((B * S, H, D), (H, B * S)) if packed else ((B, H, S, D), (B, H, S))
    outs, lses = R.draw_states(n, shape_o, shape_l, dtypes, seed=n)
    out, lse = qa.merge_attn_states(outs, lses, out_dtype=out_dtype)
    assert out.dtype == out_dtype and lse.dtype == F32 and out.shape == shape_o and lse.shape == shape_l
    ref = R.reference_of(outs, lses)
    r_out, r_lse = R.worst_ratios(out, lse, ref, out_dtype)
    print(f"eager n={n} {dtypes[0]}..{dtypes[-1]}->{out_dtype} packed={packed}: worst out {r_out:.3f} lse {r_lse:.3f} of the bound")
    assert r_out <= 1.0 and r_lse <= 1.0
    empty = ~np.isfinite(ref[1])
    assert empty.any() and not R.f64(out)[R.rows_of(empty, packed)[..., 0]].any(), "rows empty in every partial are zero rows"


def test_minus_inf_partial_leaves_the_bits_of_the_merge_without_it():
    outs, lses = R.draw_states(3, (2, 3, 20, 64), (2, 3, 20), (BF, BF, BF), seed=5, empty_rows=False)
    want = qa.merge_attn_states([outs[0], outs[2]], [lses[0], lses[2]])
    lses[1][:] = -INF
    outs[1][:] = float("nan")
    got = qa.merge_attn_states(outs, lses)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_inf_and_nan_lse_propagate_as_nan():
    outs, lses = R.draw_states(2, (1, 1, 4, 64), (1, 1, 4), (BF, BF), seed=1, empty_rows=False)
    lses[0][0, 0, 1] = INF
    lses[1][0, 0, 2] = float("nan")
    out, lse = qa.merge_attn_states(outs, lses)
    assert out[0, 0, 1].isnan().all() and out[0, 0, 2].isnan().all() and lse[0, 0, 1].isnan() and lse[0, 0, 2].isnan()
    assert not out[0, 0, 0].isnan().any() and not out[0, 0, 3].isnan().any()


def test_single_state_inplace_and_return_forms():
    outs, lses = R.draw_states(2, (1, 2, 9, 64), (1, 2, 9), (F32, BF), seed=2)
    one = qa.merge_attn_states(outs[:1], lses[:1])
    assert one[0] is outs[0] and one[1] is lses[0]
    assert qa.merge_attn_states(outs[:1], lses[:1], out_dtype=BF, return_lse=False).dtype == BF
    want = qa.merge_attn_states(outs, lses)
    assert isinstance(qa.merge_attn_states(outs, lses, return_lse=False), torch.Tensor)
    got = qa.merge_attn_states(outs, lses, inplace=True)
    assert got[0] is outs[0] and got[1] is lses[0] and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- signatures and validation --------------------------------------------------------------------------------------------------
def test_signatures():
    def sig(f):
        return [(p.name, p.kind, p.default) for p in inspect.signature(f).parameters.values()]
    P, K, E = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty
    assert sig(qa.merge_attn_states) == [("outs", P, E), ("lses", P, E), ("out_dtype", K, None), ("return_lse", K, True), ("inplace", K, False)]
    assert sig(qa.fp8_attn_lse_func) == [("query", P, E), ("key", P, E), ("value", P, E), ("is_causal", P, False), ("scale", K, None)]
    assert sig(qa.fp8_attn_multi_kv_func) == [("query", P, E), ("kvs", P, E), ("scale", K, None), ("return_lse", K, False)]
    assert sig(_native.attention_state_merge) == [("outs", P, E), ("lses", P, E), ("out", K, None), ("lse_out", K, None), ("out_dtype", K, None),
                                                  ("return_lse", K, True)]
    for name in ("merge_attn_states", "fp8_attn_lse_func", "fp8_attn_multi_kv_func"):
        assert name not in qa.__all__, "package attributes beyond the reference's exported names"


def test_merge_validation_errors():
    o = lambda *s, dt=BF: torch.zeros(*s, dtype=dt)
    good_o, good_l = o(1, 2, 5, 64), o(1, 2, 5, dt=F32)
    with pytest.raises(ValueError, match="same length"):
        qa.merge_attn_states([good_o, good_o], [good_l])
    with pytest.raises(ValueError, match="same length"):
        qa.merge_attn_states([], [])
    with pytest.raises(TypeError):
        qa.merge_attn_states(good_o, good_l)
    with pytest.raises(ValueError, match="mixes"):
        qa.merge_attn_states([good_o, o(5, 2, 64)], [good_l, o(2, 5, dt=F32)])
    with pytest.raises(ValueError, match="do not match"):
        qa.merge_attn_states([good_o, o(1, 2, 6, 64)], [good_l, o(1, 2, 6, dt=F32)])
    with pytest.raises(ValueError, match="do not match"):
        qa.merge_attn_states([good_o, good_o], [good_l, o(1, 2, 4, dt=F32)])
    with pytest.raises(ValueError, match="float32"):
        qa.merge_attn_states([good_o, good_o], [good_l, good_l.to(BF)])
    with pytest.raises(ValueError, match="bf16, fp16 or fp32"):
        qa.merge_attn_states([good_o, good_o.to(torch.float64)], [good_l, good_l])
    with pytest.raises(ValueError, match="out_dtype"):
        qa.merge_attn_states([good_o, good_o], [good_l, good_l], out_dtype=torch.float64)
    with pytest.raises(ValueError, match="inplace"):
        qa.merge_attn_states([good_o, good_o], [good_l, good_l], out_dtype=F32, inplace=True)
    with pytest.raises(ValueError, match="dimensions"):
        qa.merge_attn_states([good_o, good_o], [good_l[0, 0], good_l[0, 0]])


def test_lse_and_multi_kv_validation_errors():
    q = torch.zeros(1, 2, 8, 64, dtype=BF)
    with pytest.raises(ValueError):      # no gfx950 device under the tensors: the fused step has no CPU path of its own
        qa.fp8_attn_lse_func(q, q, q)
    with pytest.raises(ValueError, match="non-empty sequence"):
        qa.fp8_attn_multi_kv_func(q, [])
    with pytest.raises(ValueError, match=r"kvs\[1\]"):
        qa.fp8_attn_multi_kv_func(q, [(q, q), (q,)])
    with pytest.raises(ValueError, match=r"kvs\[0\]"):
        qa.fp8_attn_multi_kv_func(q, [q])
    with pytest.raises(TypeError):
        qa.fp8_attn_multi_kv_func(q, [(q, q)], True)      # return_lse is keyword-only


def test_eager_fallback_of_the_lse_step_and_multi_kv_on_cpu():
    """With the supported check skipped and force_eager_fallback the whole composition runs in torch ops: two sources merged = SDPA over the
    concatenation, to the fp8 quantisation error (the project's RMSE bar, 1e-2)."""
    g = torch.Generator().manual_seed(0)
    q = torch.randn(1, 4, 33, 64, generator=g).to(BF)
    k1, v1, k2, v2 = (torch.randn(1, 2, s, 64, generator=g).to(BF) for s in (50, 50, 70, 70))
    with qa.config.patch({"attention.skip_supported_check": True, "attention.force_eager_fallback": True}):
        out, lse = qa.fp8_attn_multi_kv_func(q, [(k1, v1), (k2, v2)], return_lse=True)
        one, lse1 = qa.fp8_attn_lse_func(q, k1, v1)
    k, v = (torch.cat(p, dim=2).float().repeat_interleave(2, dim=1) for p in ((k1, k2), (v1, v2)))
    ref = torch.nn.functional.scaled_dot_product_attention(q.float(), k, v)
    ref_lse = torch.logsumexp(q.float() @ k.transpose(-1, -2) / 8.0, dim=-1)
    assert (out.float() - ref).pow(2).mean().sqrt() < 1e-2 and (lse - ref_lse).abs().max() < 5e-2
    assert one.shape == q.shape and lse1.shape == (1, 4, 33) and lse1.dtype == F32


def test_path_table_answers_where_the_lse_request_keeps_the_bits_of_out():
    assert [merge.lse_request_keeps_out_bits(D) for D in (64, 128, 256)] == [False, True, False]
    assert merge.lse_request_keeps_out_bits(128, HF, 20000)


# ---- the C entry: export and argument errors (before any device call) -----------------------------------------------------------------
def test_export_is_found_by_symbol_and_abi_stays_8():
    raw = ctypes.CDLL(_native.LIB_PATH)
    assert "qattn_attention_state_merge" in _native.EXPORTS and raw.qattn_attention_state_merge is not None
    assert _native.lib().qattn_abi_version() == _native.ABI_VERSION == 8
    header = open(os.path.join(ROOT, "include", "qattn_merge.h")).read()
    assert "qattn_attention_state_merge(" in header and "#define QATTN_FMT_FP32 4" in header
    assert "QATTN_ABI_VERSION 8" in open(os.path.join(ROOT, "include", "qattn.h")).read()


def _c_merge(n=2, fmts=None, o_ptrs=None, lse_ptrs=None, o_str=None, l_str=None, out=0x10000, out_fmt=_native.FMT_BF16, out_str=None,
             lse_out=0x20000, lout_str="dense", B=2, H=3, S=5, D=64, tables=True):
    """qattn_attention_state_merge on made-up (never dereferenced) device addresses: every case here must be refused on the host."""
    ll, vp = ctypes.c_longlong, ctypes.c_void_p
    m = max(n, 1)
    dense_o, dense_l = [H * S * D, S * D, D], [H * S, S, 1]
    fmts = fmts or [_native.FMT_BF16] * m
    o_ptrs = o_ptrs or [0x100000 * (i + 1) for i in range(m)]
    lse_ptrs = lse_ptrs or [0x1000000 + 0x1000 * i for i in range(m)]
    o_str = o_str or dense_o * m
    l_str = l_str or dense_l * m
    arr = lambda ty, xs: (ty * len(xs))(*xs)
    return _native.lib().qattn_attention_state_merge(
        n, arr(vp, o_ptrs) if tables else None, arr(ctypes.c_int, fmts), arr(ll, o_str), arr(vp, lse_ptrs), arr(ll, l_str), out, out_fmt,
        arr(ll, out_str or dense_o), lse_out, None if lout_str is None else arr(ll, dense_l if lout_str == "dense" else lout_str), B, H, S, D, None)


def test_c_entry_refuses_bad_arguments_before_any_device_call():
    INVALID, DIM, FMT = -1, -2, -3          # QATTN_ERR_INVALID_ARG, _UNSUPPORTED_DIM, _UNSUPPORTED_FMT (include/qattn.h)
    assert _c_merge(n=1) == INVALID and _c_merge(n=9) == INVALID and _c_merge(n=0) == INVALID
    assert _c_merge(D=96) == DIM and _c_merge(D=32) == DIM
    assert _c_merge(B=0) == INVALID and _c_merge(S=-1) == INVALID and _c_merge(H=70000) == INVALID
    assert _c_merge(fmts=[_native.FMT_BF16, _native.FMT_E4M3]) == FMT and _c_merge(out_fmt=7) == FMT
    assert _c_merge(tables=False) == INVALID
    assert _c_merge(o_ptrs=[0x100000, 0]) == INVALID and _c_merge(lse_ptrs=[0, 0x1000]) == INVALID and _c_merge(out=0) == INVALID
    assert _c_merge(o_ptrs=[0x100000, 0x200008]) == INVALID, "a base off 16 bytes"
    assert _c_merge(lse_ptrs=[0x1000, 0x1002]) == INVALID, "an LSE off 4 bytes"
    assert _c_merge(o_str=[960, 320, 64, 3 * 5 * 68, 5 * 68, 68]) == INVALID, "bf16 rows 136 bytes apart are not 16-byte aligned"
    assert _c_merge(o_str=[960, 320, 64, 960, -320, 64]) == INVALID, "a negative stride"
    assert _c_merge(out_str=[0, 320, 64]) == INVALID, "out cannot be a broadcast view"
    assert _c_merge(out_str=[960, 320, 32]) == INVALID, "output rows closer than D overlap"
    assert _c_merge(out_str=[640, 64, 192]) == INVALID, "[B,S,H,D] with a batch stride that does not cover its 5 rows of 192"
    assert _c_merge(lout_str=None) == INVALID, "lse_out without its strides"
    assert _c_merge(lout_str=[15, 5, 0]) == INVALID and _c_merge(lout_str=[15, 4, 1]) == INVALID, "lse_out rows that collide"


# ---- the ops ---------------------------------------------------------------------------------------------------------------------
def test_ops_are_registered_with_fake_implementations():
    ops = torch.ops.quantumattention_amd
    assert str(ops.attention_state_merge.default._schema) == \
        "quantumattention_amd::attention_state_merge(Tensor[] outs, Tensor[] lses, ScalarType? out_dtype=None) -> (Tensor, Tensor)"
    assert str(ops.attention_state_merge_.default._schema) == \
        "quantumattention_amd::attention_state_merge_(Tensor(a0!) acc, Tensor(a1!) acc_lse, Tensor[] outs, Tensor[] lses) -> ()"
    o = [torch.empty(7, 3, 128, dtype=BF, device="meta").transpose(0, 1).transpose(0, 1) for _ in range(2)]
    l = [torch.empty(3, 7, dtype=F32, device="meta") for _ in range(2)]
    out, lse = ops.attention_state_merge(o, l, F32)
    assert out.shape == (7, 3, 128) and out.dtype == F32 and lse.shape == (3, 7) and lse.dtype == F32 and out.device.type == "meta"
    assert ops.attention_state_merge(o, l)[0].dtype == BF


# ---- teeth: wrong merges the bounds must reject -----------------------------------------------------------------------------------
def _teeth_case(lse_level=0.0):
    outs, lses = R.draw_states(3, (2, 3, 40, 64), (2, 3, 40), (BF, BF, BF), seed=9)
    lses = [l + lse_level for l in lses]
    return outs, lses, R.reference_of(outs, lses)


def _passes(out, lse, ref, dtype=F32):
    r_out, r_lse = R.worst_ratios(out, lse, ref, dtype)
    return r_out <= 1.0 and r_lse <= 1.0


def test_teeth_the_right_merge_passes_where_the_wrong_ones_below_fail():
    for level in (0.0, 90.0 + 64.0):
        outs, lses, ref = _teeth_case(level)
        assert _passes(*merge.merge_attn_states_eager(outs, lses, F32), ref)


def test_teeth_a_plain_average_fails():
    outs, lses, ref = _teeth_case()
    avg = torch.stack([torch.nan_to_num(o.float()) for o in outs]).mean(0)
    lse = torch.logsumexp(torch.stack(lses), dim=0)
    assert not _passes(avg, lse, ref)
    assert R.worst_ratios(avg, lse, ref, F32)[0] > 100


def test_teeth_weights_without_the_max_shift_fail_on_lse_near_90():
    outs, lses, ref = _teeth_case(90.0 + 64.0)      # the LSEs of the case sit in [-64, 64]: lifted, the row maxima are >= 90
    w = [torch.exp(l) for l in lses]                # exp(90) is past fp32's range
    den = sum(w)
    out = sum(wi[..., None] * torch.where(wi[..., None] != 0, o.float(), torch.zeros(())) for wi, o in zip(w, outs)) / den[..., None]
    assert not _passes(out, torch.log(den), ref)


def test_teeth_nan_to_num_after_the_fact_fails():
    outs, lses, ref = _teeth_case()
    L = torch.stack(lses)
    m = L.max(0).values
    e = torch.exp(L - m)                                            # rows empty everywhere: -inf - -inf = NaN
    out = sum(e[i][..., None] * outs[i].float() for i in range(3)) / e.sum(0)[..., None]     # 0 * NaN = NaN on the rows partial 1 skipped
    out, lse = torch.nan_to_num(out, nan=0.0), torch.nan_to_num(m + torch.log(e.sum(0)), nan=-INF)
    assert not out.isnan().any() and not _passes(out, lse, ref), "zeroing the NaN rows loses the partials that did attend keys"


# ---- the compiled unit ----------------------------------------------------------------------------------------------------------
def test_merge_unit_compiles_without_scratch_spills_or_lds():
    """tools/kernel_resources.py on the -save-temps output of the product build: 3 head dims x 7 values of N, none with a spill, scratch
    or LDS, all at 5 or more waves per SIMD (at most 96 VGPRs)."""
    import sys

    from quantumattention_amd import build as hip_build

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    d = hip_build.build(save_temps=True)   # no-op when the objects and their .s files are current
    rows = kernel_resources.parse(os.path.join(d, "qattn_merge-hip-amdgcn-amd-amdhsa-gfx950.s"))
    assert len(rows) == 21 and all("merge_states_kernel" in r["name"] for r in rows), [r["name"] for r in rows]
    for r in rows:
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, r
        assert r.get("group_segment_fixed_size", 0) == 0 and r["vgpr_count"] <= 96, r


def test_correct_rounding_alone_exceeds_the_flat_half_ulp_figure():
    """Why the 16-bit bound takes half an ulp from the FORMAT: the fp64 reference itself, rounded once and correctly to bf16 / fp16, sits
    within merge_ref's bound and up to twice above `2^-9 |ref|` / `2^-12 |ref|` -- those are half an ulp only at the top of a binade."""
    outs, lses, ref = _teeth_case()
    exact = torch.from_numpy(ref[0])
    lse = torch.from_numpy(ref[1]).to(F32)
    for dtype in (BF, HF):
        rounded = exact.to(dtype)
        assert R.worst_ratios(rounded, lse, ref, dtype)[0] <= 1.0
        flat = R.flat_ratio(rounded, ref, dtype)
        print(f"fp64 merge rounded to {dtype}: {flat:.3f} of the flat figure")
        assert 1.5 < flat <= 2.0

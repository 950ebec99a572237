"""GPU tests of the RoPE-fused quant pre-pass (include/qattn_rope.h, quantumattention_amd/rope.py).

The contract is ONE bit-identity: the fused path equals the unfused composition -- `apply_rope_eager` (torch on the CPU: the definition),
then the existing quantiser and the existing attention entry -- so every grading rule the project has for those applies through it:

  1. rope_quantize_fp8 / the C entry's KFRAG image  ==  _native.quant_fp8 on the eagerly rotated tensor (payload, scale, padding bytes);
  2. fp8_attn_rope_func out / lse  ==  _native.quant_qkv_fp8 + _native.fp8_attention_forward on the eagerly rotated q and k;
  3. the quarter-turn probe (tests/rope_probe.py) through both entry points: the exact signed permutation, the probe's fp64 answer;
  4. strided views, sliced tables, distinct k tables, batched tables, the identity table;
  5. sanity against the mathematics: RMSE < 1e-2 against fp32 SDPA on the fp64-rotated, unquantised inputs (the reference's bar);
  6. HIP-graph capture and replay equals eager bit for bit.

Shapes: B 2, Hq / Hkv 4 / 2, Sq 200, Skv 333 (no multiple of 64, more than one 64-row tile and more than one abs-max block per head at
D = 256), one case at 1100 keys (the one-term sweep starts at 1024).  Inputs are finite N(0, 1) draws."""
import functools
import math

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import rope_probe as RP

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HQ, HKV, SQ, SKV = 2, 4, 2, 200, 333
BF16, FP16 = torch.bfloat16, torch.float16
DT = {"bf16": BF16, "fp16": FP16}
FP8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
# (D, dtype, scaling, interleaved): the full grid
GRID = [(D, dt, sc, il) for D in (64, 128, 256) for dt in ("bf16", "fp16") for sc in ("head-wise", "token-wise") for il in (False, True)]
GRID_IDS = [f"d{D}-{dt}-{sc.split('-')[0]}-{'gptj' if il else 'neox'}" for D, dt, sc, il in GRID]


@functools.lru_cache(maxsize=None)
def _inputs(Sq, Skv, D, dt, seed=0):
    """(q, k, v) on the CPU: finite N(0,1) draws"""
    g = torch.Generator().manual_seed(100003 * seed + 1000 * Sq + 10 * Skv + D)
    q = torch.randn(B, HQ, Sq, D, generator=g).to(DT[dt])
    k, v = (torch.randn(B, HKV, Skv, D, generator=g).to(DT[dt]) for _ in range(2))
    return q, k, v


@functools.lru_cache(maxsize=None)
def _tables(T, half, batched=False):
    """cos / sin of the usual frequencies 10000^(-i / half) at positions 0 .. T-1 (batched: each batch element its own position offset)"""
    inv = 10000.0 ** (-torch.arange(half, dtype=torch.float64) / half)
    pos = torch.arange(T, dtype=torch.float64)
    if batched:
        pos = pos[None, :] + torch.tensor([0.0, 1234.0], dtype=torch.float64)[:, None]
    ang = pos[..., None] * inv
    return torch.cos(ang).to(torch.float32), torch.sin(ang).to(torch.float32)


@functools.lru_cache(maxsize=None)
def _rotated(Sq, Skv, D, dt, il, k_off=0, batched=False):
    """the eagerly rotated (q, k) on the device: computed once on the CPU by the definition, shared, never modified"""
    q, k, _ = _inputs(Sq, Skv, D, dt)
    cos, sin = _tables(max(Sq, Skv + k_off) + 5, D // 2, batched)
    ck, sk = (t[..., k_off:k_off + Skv, :] for t in (cos, sin))
    return qa.apply_rope_eager(q, cos, sin, interleaved=il).to(DEV), qa.apply_rope_eager(k, ck, sk, interleaved=il).to(DEV)


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


def _same(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _kfrag_from_c_entry(k, cos, sin, il, scaling, fp8):
    return _native.rope_quant_fp8(k, cos, sin, interleaved=il, scaling=scaling, fp8_dtype=fp8, layout=_native.LAYOUT_KFRAG)


# ------------------------------------------------------------------------------------------------------------ 1. the pre-pass alone
def _check_quant(Sq, Skv, D, dt, scaling, il, fp8="e4m3", numerics="compiled"):
    q, k, _ = _inputs(Sq, Skv, D, dt)
    cos, sin = _dev(*_tables(max(Sq, Skv) + 5, D // 2))
    qr, kr = _rotated(Sq, Skv, D, dt, il)
    got8, gots = qa.rope_quantize_fp8(q.to(DEV), cos, sin, interleaved=il, scaling=scaling, fp8_dtype=FP8[fp8], numerics=numerics)
    want8, wants = _native.quant_fp8(qr, scaling=scaling, fp8_dtype=FP8[fp8], numerics=numerics)
    assert got8.dtype == FP8[fp8] and _same(gots, wants), "scale_q differs from the quantiser on the eagerly rotated tensor"
    assert _same(got8, want8), "q8 differs from the quantiser on the eagerly rotated tensor"
    gotk, gotks = _kfrag_from_c_entry(k.to(DEV), cos, sin, il, scaling, FP8[fp8]) if numerics == "compiled" else (None, None)
    if gotk is not None:
        wantk, wantks = _native.quant_fp8(kr, scaling=scaling, fp8_dtype=FP8[fp8], layout=_native.LAYOUT_KFRAG)
        assert gotk.numel() == B * HKV * ((Skv + 63) // 64 * 64) * D
        assert _same(gotks, wantks) and _same(gotk, wantk), "the KFRAG image (padding bytes included) differs"


@pytest.mark.parametrize("D,dt,scaling,il", GRID, ids=GRID_IDS)
def test_rope_quantize_equals_the_quantiser_on_the_rotated_tensor(D, dt, scaling, il):
    _check_quant(SQ, SKV, D, dt, scaling, il)


@pytest.mark.parametrize("fp8,numerics,Skv", [("e5m2", "compiled", SKV), ("e4m3", "eager", SKV), ("e4m3", "compiled", 1100)],
                         ids=["e5m2", "eager-numerics", "s1100"])
def test_rope_quantize_other_formats_and_sizes(fp8, numerics, Skv):
    for il in (False, True):
        _check_quant(SQ, Skv, 128, "bf16", "head-wise", il, fp8=fp8, numerics=numerics)


# --------------------------------------------------------------------------------------------------------------- 2. the whole step
@functools.lru_cache(maxsize=None)
def _fused(Sq, Skv, D, dt, scaling, il, causal=False, pv="fp8", precision="auto", fp8="e4m3"):
    q, k, v = _dev(*_inputs(Sq, Skv, D, dt))
    cos, sin = _dev(*_tables(max(Sq, Skv) + 5, D // 2))
    with qa.config.patch({"attention.fp8_format": fp8}):
        return qa.fp8_attn_rope_func(q, k, v, cos, sin, interleaved=il, is_causal=causal, scaling=scaling, pv_precision=pv,
                                     precision=precision, return_lse=True)


def _composition(qr, kr, v, scaling, causal, pv, precision, fp8="e4m3"):
    """the separate calls on already rotated tensors: what fp8_attn_rope_func must equal bit for bit"""
    q8, kf, vf, sq, sk, sv = _native.quant_qkv_fp8(qr, kr, v, scaling=scaling, fp8_dtype=FP8[fp8])
    v16 = pv == "16bit"
    return _native.fp8_attention_forward(q8, kf, v if v16 else vf, sq, sk, None if v16 else sv, Hkv=kr.shape[1], Skv=kr.shape[2],
                                         out_dtype=qr.dtype, is_causal=causal, scaling=scaling, return_lse=True, precision=precision)


def _check_attention(Sq, Skv, D, dt, scaling, il, causal=False, pv="fp8", precision="auto", fp8="e4m3"):
    out, lse = _fused(Sq, Skv, D, dt, scaling, il, causal, pv, precision, fp8)
    qr, kr = _rotated(Sq, Skv, D, dt, il)
    want, want_lse = _composition(qr, kr, _inputs(Sq, Skv, D, dt)[2].to(DEV), scaling, causal, pv, precision, fp8)
    assert out.dtype == DT[dt] and out.shape == (B, HQ, Sq, D) and lse.shape == (B, HQ, Sq) and lse.dtype == torch.float32
    assert torch.isfinite(out.float()).all()
    assert _same(out, want), "out differs from the composition on the eagerly rotated tensors"
    assert _same(lse, want_lse), "lse differs from the composition on the eagerly rotated tensors"


@pytest.mark.parametrize("D,dt,scaling,il", GRID, ids=GRID_IDS)
def test_attention_equals_the_composition(D, dt, scaling, il):
    _check_attention(SQ, SKV, D, dt, scaling, il)


# causal at Sq = Skv, the 16-bit V, the other precisions, e5m2, and 1100 keys (the one-term sweep)
EXTRA = [
    (SQ, SQ, 64, "bf16", "head-wise", False, True, "fp8", "auto", "e4m3"),
    (SQ, SQ, 128, "fp16", "head-wise", True, True, "fp8", "auto", "e4m3"),
    (SQ, SQ, 128, "bf16", "token-wise", True, True, "16bit", "auto", "e4m3"),
    (SQ, SQ, 256, "bf16", "head-wise", False, True, "fp8", "accurate", "e4m3"),
    (SQ, SKV, 128, "bf16", "head-wise", False, False, "16bit", "auto", "e4m3"),
    (SQ, SKV, 64, "fp16", "token-wise", True, False, "16bit", "auto", "e4m3"),
    (SQ, SKV, 128, "bf16", "head-wise", True, False, "fp8", "fast", "e4m3"),
    (SQ, SKV, 128, "bf16", "head-wise", True, False, "fp8", "auto", "e5m2"),
    (SQ, 1100, 128, "bf16", "head-wise", True, False, "fp8", "auto", "e4m3"),
    (1100, 1100, 128, "bf16", "head-wise", False, True, "fp8", "fast", "e4m3"),
]


@pytest.mark.parametrize("case", EXTRA, ids=[f"{c[0]}x{c[1]}-d{c[2]}-{c[3]}-{c[4].split('-')[0]}-{'gptj' if c[5] else 'neox'}-"
                                             f"{'causal' if c[6] else 'full'}-pv{c[7]}-{c[8]}-{c[9]}" for c in EXTRA])
def test_attention_equals_the_composition_other_paths(case):
    _check_attention(*case)


# --------------------------------------------------------------------------------------------------------- 3. the quarter-turn probe
@functools.lru_cache(maxsize=None)
def _probe(D, il, causal):
    return RP.Probe(B, HQ, HKV, SQ, SQ if causal else SKV, D, il, k_offset=0 if causal else 77, causal=causal, seed=2)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("il", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("D,dt", [(64, "bf16"), (128, "fp16"), (256, "bf16")])
def test_quarter_turn_probe(D, dt, il, causal):
    p = _probe(D, il, causal)
    q, k, v = p.tensors(DT[dt], DEV)
    cos, sin = _dev(p.cos, p.sin)
    ck, sk = _dev(*p.k_tables())
    # the exact signed permutation before quantisation: the probe's values are exact in fp8, so the dequantised bytes ARE the rotated tensor
    for scaling in ("head-wise", "token-wise"):
        for x, c, s, want in ((q, cos, sin, p.q_rot), (k, ck, sk, p.k_rot)):
            x8, sc = qa.rope_quantize_fp8(x, c, s, interleaved=il, scaling=scaling)
            deq = x8.to(torch.float64) * sc.to(torch.float64).reshape(sc.shape + (1,) * (4 - sc.dim()))
            err = (deq.cpu().numpy() - want).__abs__().max()
            assert err <= 2.0 ** -20, (scaling, err)
            assert np.array_equal(np.sign(x8.to(torch.float32).cpu().numpy()), np.sign(want))
    # the probe's attention answer: fp64 attention on the exactly rotated tensors, the project's bounds
    for pv, tol in (("fp8", RP.TOL), ("16bit", RP.TOL_V16)):
        out, lse = qa.fp8_attn_rope_func(q, k, v, cos, sin, cos_k=ck, sin_k=sk, interleaved=il, is_causal=causal, pv_precision=pv, return_lse=True)
        err = np.abs(out.double().cpu().numpy() - p.ref).max()
        print(f"probe d{D} {dt} il={il} causal={causal} pv={pv}: max |out - ref| = {err:.3e} (bound {tol:.3e})")
        assert err <= tol, (pv, err, tol)
        assert np.abs(lse.double().cpu().numpy() - p.ref_lse).max() <= 2e-2
    # teeth on the device: q's table applied to k (the keys' offset lost) moves every row by more than TEETH x the bound
    if not causal:
        bad = qa.fp8_attn_rope_func(q, k, v, cos, sin, interleaved=il)
        moved = np.abs(bad.double().cpu().numpy() - p.ref).max(-1)
        assert moved.min() > RP.TEETH * RP.TOL, float(moved.min())


# ------------------------------------------------------------------------------------- 4. views, slices, other tables, the identity
@pytest.mark.parametrize("il", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("D,dt,scaling", [(64, "fp16", "token-wise"), (128, "bf16", "head-wise"), (256, "bf16", "head-wise")])
def test_transposed_views_give_the_dense_bits(D, dt, scaling, il):
    q, k, v = _dev(*_inputs(SQ, SKV, D, dt))
    cos, sin = _dev(*_tables(SKV + 5, D // 2))
    qv, kv = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (q, k))        # [B,S,H,D]-backed
    assert not qv.is_contiguous() and not kv.is_contiguous() and _native._strided_ok(qv)
    out, lse = qa.fp8_attn_rope_func(qv, kv, v, cos, sin, interleaved=il, scaling=scaling, return_lse=True)
    want, want_lse = _fused(SQ, SKV, D, dt, scaling, il)
    assert _same(out, want) and _same(lse, want_lse)
    got8, gots = qa.rope_quantize_fp8(qv, cos, sin, interleaved=il, scaling=scaling)
    want8, wants = qa.rope_quantize_fp8(q, cos, sin, interleaved=il, scaling=scaling)
    assert _same(got8, want8) and _same(gots, wants)
    gk, gks = _kfrag_from_c_entry(kv, cos, sin, il, scaling, FP8["e4m3"])
    wk, wks = _kfrag_from_c_entry(k, cos, sin, il, scaling, FP8["e4m3"])
    assert _same(gk, wk) and _same(gks, wks)


@pytest.mark.parametrize("il", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("batched", [False, True], ids=["shared-table", "batched-table"])
@pytest.mark.parametrize("D,dt,scaling", [(128, "bf16", "head-wise"), (64, "fp16", "token-wise")])
def test_sliced_and_distinct_key_tables(D, dt, scaling, batched, il):
    """k positions offset by 77: cos_k / sin_k are SLICES of the tables (views, read in place), q keeps rows 0 .. Sq-1"""
    OFF = 77
    q, k, v = _dev(*_inputs(SQ, SKV, D, dt))
    cos, sin = _dev(*_tables(SKV + OFF + 5, D // 2, batched))
    ck, sk = cos[..., OFF:OFF + SKV, :], sin[..., OFF:OFF + SKV, :]
    assert ck.data_ptr() != cos.data_ptr()
    out, lse = qa.fp8_attn_rope_func(q, k, v, cos, sin, cos_k=ck, sin_k=sk, interleaved=il, scaling=scaling, return_lse=True)
    qr, kr = _rotated(SQ, SKV, D, dt, il, OFF, batched)
    want, want_lse = _composition(qr, kr, v, scaling, False, "fp8", "auto")
    assert _same(out, want) and _same(lse, want_lse)
    # and the keys' offset matters: q's table on k gives other bits
    assert not _same(out, qa.fp8_attn_rope_func(q, k, v, cos, sin, interleaved=il, scaling=scaling))
    # 16-bit tables are up-cast in the wrapper (exact): the bits of fp32 tables holding the same values
    c16, s16 = cos.to(torch.bfloat16), sin.to(torch.bfloat16)
    assert _same(qa.fp8_attn_rope_func(q, k, v, c16, s16, interleaved=il, scaling=scaling),
                 qa.fp8_attn_rope_func(q, k, v, c16.float(), s16.float(), interleaved=il, scaling=scaling))


@pytest.mark.parametrize("D,dt,scaling", [(64, "bf16", "head-wise"), (128, "fp16", "token-wise"), (256, "bf16", "head-wise")])
def test_identity_table_gives_the_unrotated_composition(D, dt, scaling):
    q, k, v = _dev(*_inputs(SQ, SKV, D, dt))
    one, zero = torch.ones(SKV, D // 2, device=DEV), torch.zeros(SKV, D // 2, device=DEV)
    want, want_lse = _composition(q, k, v, scaling, False, "fp8", "auto")
    for il in (False, True):
        out, lse = qa.fp8_attn_rope_func(q, k, v, one, zero, interleaved=il, scaling=scaling, return_lse=True)
        assert _same(out, want) and _same(lse, want_lse)


# ------------------------------------------------------------------------------------------------ 5. sanity against the mathematics
@pytest.mark.parametrize("D,dt,scaling,il", GRID, ids=GRID_IDS)
def test_rmse_against_fp32_sdpa_on_fp64_rotated_inputs(D, dt, scaling, il):
    """the reference's bar (RMSE < 1e-2, as tests/test_gpu_attention.py) against attention in fp32 on inputs rotated in fp64 and NOT quantised"""
    out, _ = _fused(SQ, SKV, D, dt, scaling, il)
    q, k, v = _inputs(SQ, SKV, D, dt)
    cos, sin = (t.double() for t in _tables(SKV + 5, D // 2))

    def rot64(x):
        S, h = x.shape[2], D // 2
        c, s, x = cos[:S], sin[:S], x.double()
        a, b = (x[..., 0::2], x[..., 1::2]) if il else (x[..., :h], x[..., h:])
        y0, y1 = a * c - b * s, b * c + a * s
        return torch.stack((y0, y1), -1).flatten(-2) if il else torch.cat((y0, y1), -1)

    qr, kr = rot64(q).float().to(DEV), rot64(k).float().to(DEV)
    rep = HQ // HKV
    ref = torch.nn.functional.scaled_dot_product_attention(qr, kr.repeat_interleave(rep, 1), v.float().to(DEV).repeat_interleave(rep, 1))
    rmse = (out.float() - ref).pow(2).mean().sqrt().item()
    print(f"rmse d{D} {dt} {scaling} il={il}: {rmse:.3e}")
    assert rmse < 1e-2, rmse


# ------------------------------------------------------------------------------------------------------------------ 6. HIP graphs
def test_graph_capture_and_replay_equal_eager():
    D, dt, il = 128, "bf16", True
    q, k, v = _dev(*_inputs(SQ, SKV, D, dt))
    cos, sin = _dev(*_tables(SKV + 5, D // 2))
    call = lambda: qa.fp8_attn_rope_func(q, k, v, cos, sin, interleaved=il, return_lse=True)
    want, want_lse = call()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, lse = call()
    g.replay()
    torch.cuda.synchronize()
    assert _same(out, want) and _same(lse, want_lse)
    # new inputs in the captured buffers: the replay follows them
    q2, k2, _ = _dev(*_inputs(SQ, SKV, D, dt, seed=1))
    q.copy_(q2); k.copy_(k2)
    g.replay()
    torch.cuda.synchronize()
    want2, want_lse2 = call()
    assert _same(out, want2) and _same(lse, want_lse2) and not _same(want2, want)

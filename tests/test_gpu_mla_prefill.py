"""GPU tests of the non-absorbed MLA prefill entry (include/qattn_mla_prefill.h): the sweep against the plain fp64 reference of
tests/mla_prefill_cases.py, the pre-pass and the in-kernel q quantiser against the eager definition bit for bit, the bytes no sequence uses,
strided views, chunked prefill through `merge_attn_states`, and a replayed graph.

Bounds: out per element 2^-6 max(1, |ref| / 2) (tests/gpu_utils.py: the bound of every FP8-P.V entry with two-term P; the reference shares the
quantised operands) and lse 2e-3 (mla_cases.LSE_TOL, the FP8-P.V siblings')."""
import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from tests import mla_prefill_cases as C
from tests.gpu_utils import assert_within_bound
from tests.mla_cases import LSE_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
bits = lambda t: t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.uint8)


def _call(q, kv, k_pe, cu_q, cu_k, fmt="e4m3", **kw):
    with qa.config.patch({"attention.fp8_format": fmt}):
        return qa.fp8_mla_prefill_varlen_func(q, kv[..., :128], k_pe, kv[..., 128:], cu_q, cu_k, 130, 200, scale=C.SM_SCALE, **kw)


@pytest.mark.parametrize("H", C.HEADS)
@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("causal", [True, False])
def test_sweep_against_the_fp64_reference(causal, dtype, fmt, H):
    q, kv, k_pe = C.make_inputs(H, dtype)
    cu_q, cu_k = C.tables()
    out, lse, q8, sq, sk, sv = _call(q.to(DEV), kv.to(DEV), k_pe.to(DEV), cu_q.to(DEV), cu_k.to(DEV), fmt, causal=causal, return_lse=True,
                                     return_quantized=True)
    kd, vd = C.dequantised_kv(kv, k_pe, sk.cpu(), sv.cpu(), fmt)
    ref_o, ref_l = C.reference((q8.double() * sq.double()[..., None]).cpu().numpy(), kd, vd, causal)
    got_o, got_l, fin = out.float().cpu().numpy(), lse.cpu().numpy(), np.isfinite(ref_l)
    what = (causal, dtype, fmt, H)
    print(what, "max |err| out", np.abs(got_o - ref_o).max(), "lse", np.abs(got_l[fin] - ref_l[fin]).max())
    assert_within_bound(got_o, ref_o, what=what)
    assert np.array_equal(np.isneginf(got_l), ~fin), what                # a row without a key: LSE -inf exactly ...
    assert (got_o[~fin.T] == 0).all(), what                              # ... and a zero row
    assert np.abs(got_l[fin] - ref_l[fin]).max() <= LSE_TOL, what


@pytest.mark.parametrize("fmt,dtype", [("e4m3", torch.bfloat16), ("e5m2", torch.float16)])
def test_quantisers_equal_the_eager_definition_bit_for_bit(fmt, dtype):
    q, kv, k_pe = C.make_inputs(3, dtype)
    cu_q, cu_k = C.tables()
    eager = _call(q, kv, k_pe, cu_q, cu_k, fmt, return_quantized=True)[1:]
    got = _call(q.to(DEV), kv.to(DEV), k_pe.to(DEV), cu_q.to(DEV), cu_k.to(DEV), fmt, return_quantized=True)[1:]
    for name, g, e in zip(("q8", "scale_q", "scale_k", "scale_v"), got, eager):
        assert torch.equal(bits(g).cpu(), bits(e)), name
    peak = torch.tensor(C.PE_PEAK, dtype=dtype).float() * torch.tensor(1.0 / torch.finfo(C.TDT[fmt]).max, dtype=torch.float32)
    assert (got[2][3].cpu() == peak).all()      # sequence 3's largest |k| sits in k_pe: every head's K scale is that value's


@pytest.mark.parametrize("causal", [True, False])
def test_unused_bytes_change_no_output_bit(causal):
    """keys behind seqused_k, and tokens behind the last sequence, hold zeros in one call and NaN in the other"""
    q, kv, k_pe = (t.to(DEV) for t in C.make_inputs(3, torch.bfloat16, pad=9))
    cu_q, cu_k = (t.to(DEV) for t in C.tables())
    used = torch.tensor([1, 60, 129, 131, 30, 0, 0], dtype=torch.int32, device=DEV)
    dead = torch.ones(kv.shape[0], dtype=torch.bool, device=DEV)
    for k0, n in zip(cu_k.tolist(), used.tolist()):
        dead[k0:k0 + n] = False
    res = []
    for fill in (0.0, float("nan")):
        kv[dead], k_pe[dead], q[-9:] = fill, fill, fill
        res.append(_call(q, kv, k_pe, cu_q, cu_k, causal=causal, seqused_k=used, return_lse=True, return_quantized=True))
    tq = q.shape[0]
    live = lambda t: t[:-9] if t.shape[0] == tq else t[:, :-9] if t.shape[1] == tq else t      # the rows of sequences ([B, H] scales: all)
    for name, a, b in zip(("out", "lse", "q8", "scale_q", "scale_k", "scale_v"), *res):
        assert torch.equal(live(bits(a)), live(bits(b))), name
    assert torch.isfinite(live(res[1][0]).float()).all()


def test_strided_views_equal_contiguous_copies():
    q, kv, k_pe = (t.to(DEV) for t in C.make_inputs(3, torch.float16))
    cu_q, cu_k = (t.to(DEV) for t in C.tables())
    wide_q = torch.zeros((q.shape[0], 3, 256), dtype=q.dtype, device=DEV)
    wide_q[..., :192] = q
    wide_pe = torch.zeros((k_pe.shape[0], 128), dtype=q.dtype, device=DEV)
    wide_pe[:, 64:] = k_pe
    with qa.config.patch({"attention.fp8_format": "e4m3"}):
        a = qa.fp8_mla_prefill_varlen_func(wide_q[..., :192], kv[..., :128], wide_pe[:, 64:], kv[..., 128:], cu_q, cu_k, 130, 200,
                                           scale=C.SM_SCALE, return_lse=True, return_quantized=True)
        b = qa.fp8_mla_prefill_varlen_func(q, kv[..., :128].contiguous(), k_pe, kv[..., 128:].contiguous(), cu_q, cu_k, 130, 200,
                                           scale=C.SM_SCALE, return_lse=True, return_quantized=True)
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))


def test_chunked_prefill_merges_to_the_single_call():
    """The (130, 200) sequence: keys 0..69 as context (causal=False) + keys 70..199 as the chunk (causal=True), merged by their LSEs.  Equal
    maxima (+-4 over data clamped to +-3) are planted in both key ranges, so the three calls quantise K and V with the same scales and the
    comparison is of the sweeps and the merge, not of two quantisations."""
    lens = ((130, 200),)
    q, kv, k_pe = C.make_inputs(3, torch.bfloat16, lens=lens, seed=3)
    kv, k_pe = kv.clamp(-3, 3), k_pe.clamp(-3, 3)
    for r in (0, 70):
        kv[r, :, 5], kv[r, :, 128 + 5], k_pe[r, 5] = 4.0, -4.0, 4.0
    q, kv, k_pe = q.to(DEV), kv.to(DEV), k_pe.to(DEV)
    cu = lambda *x: torch.tensor(x, dtype=torch.int32, device=DEV)
    one_o, one_l = _call(q, kv, k_pe, cu(0, 130), cu(0, 200), causal=True, return_lse=True)
    ctx = _call(q, kv[:70], k_pe[:70], cu(0, 130), cu(0, 70), causal=False, return_lse=True)
    new = _call(q, kv[70:], k_pe[70:], cu(0, 130), cu(0, 130), causal=True, return_lse=True)
    out, lse = qa.merge_attn_states([ctx[0], new[0]], [ctx[1], new[1]])
    print("max |diff| out", (out.float() - one_o.float()).abs().max().item(), "lse", (lse - one_l).abs().max().item())
    assert_within_bound(out.float().cpu().numpy(), one_o.float().cpu().numpy())
    assert (lse - one_l).abs().max().item() <= LSE_TOL


def test_captured_call_follows_the_tables():
    q, kv, k_pe = (t.to(DEV) for t in C.make_inputs(3, torch.bfloat16))
    cu_q, cu_k0 = (t.to(DEV) for t in C.tables())
    cu_k = cu_k0.clone()
    used = torch.tensor([b for _, b in C.LENS], dtype=torch.int32, device=DEV)
    step = lambda: _call(q, kv, k_pe, cu_q, cu_k, causal=True, seqused_k=used, return_lse=True)
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_lse = step()
    shifted = cu_k0.clone()
    shifted[1:4] += torch.tensor([3, 2, 1], dtype=torch.int32, device=DEV)       # sequences 0..2 grow, 1..3 start later, total unchanged
    for table, lens in ((cu_k0, (1, 64, 100, 7, 30, 17, 0)), (shifted, (4, 63, 128, 199, 0, 9, 0)), (cu_k0, [b for _, b in C.LENS])):
        cu_k.copy_(table)
        used.copy_(torch.tensor(lens, dtype=torch.int32))
        graph.replay()
        got = (g_out.clone(), g_lse.clone())
        e_out, e_lse = step()
        assert torch.equal(bits(got[0]), bits(e_out)) and torch.equal(bits(got[1]), bits(e_lse)), lens

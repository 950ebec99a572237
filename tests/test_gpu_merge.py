"""The merge kernel (include/qattn_merge.h) against the fp64 merge of the SAME inputs (tests/merge_ref.py: the reference and the bounds, with
their derivation).  Every case prints its worst |error| / bound; profiles/merge/pytest_gpu_merge.log keeps a run.

Bounds: fp32 output 2^-16 sum_i w_i |O_i|; 16-bit output that plus half an ulp of the output format at |ref|; LSE 2^-15 max(1, |L_ref|).  Half
an ulp is taken from the format (merge_ref.half_ulp), between 2^-9 |ref| and 2^-8 |ref| for bf16: the flat 2^-9 |ref| (2^-12 |ref| for fp16)
is half an ulp only at the top of a binade -- the correctly rounded fp64 result itself is off by up to twice that everywhere else
(tests/test_cpu_merge.py::test_correct_rounding_alone_exceeds_the_flat_half_ulp_figure).  Every 16-bit case prints its ratio to that flat
figure too.  Measured on the MI355X (profiles/merge/pytest_gpu_merge.log): up to 1.98 for bf16 -- the rounded reference's own 1.92 -- and
up to 76.8 for fp16, on results below fp16's normal range, where half an ulp is 2^-25 whatever |ref| is; the fp32 outputs of the same
inputs sit at 0.07 of their bound, so what exceeds the flat figure is the output rounding and nothing else."""
import ctypes
import math

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import arena as A
from tests import merge_ref as R

pytestmark = pytest.mark.gpu

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
DEV = "cuda"
B, H = 2, 3
FORMATS = {"bf16": lambda n: (BF,) * n, "fp16": lambda n: (HF,) * n, "fp32acc+bf16": lambda n: (F32,) + (BF,) * (n - 1)}


def _grade(out, lse, ref, out_dtype, what):
    r_out, r_lse = R.worst_ratios(out, lse, ref, out_dtype)
    flat = "" if out_dtype == F32 else f" (against the flat 2^{-9 if out_dtype == BF else -12} |ref| figure: {R.flat_ratio(out, ref, out_dtype):.3f})"
    print(f"{what}: worst out {r_out:.3f} lse {r_lse:.4f} of the bound{flat}")
    assert not out.isnan().any() and not lse.isnan().any(), what
    assert r_out <= 1.0 and r_lse <= 1.0, (what, r_out, r_lse)
    return r_out, r_lse


@pytest.mark.parametrize("n", [2, 3, 8, 11])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_kernel_meets_the_bounds_of_the_fp64_merge(D, n):
    """S 1 / 67 / 300 (no multiple of the 8 / 16 / 32 rows of a workgroup; more than one workgroup), all-bf16, all-fp16 and an fp32
    accumulator + bf16 partials, into bf16, fp16 and fp32; n = 11 takes the chained path (8, then accumulator + 3).  Every case holds rows
    that one partial skipped (LSE -inf, NaN in its O rows) and rows empty in all partials."""
    worst = (0.0, 0.0)
    for S in (1, 67, 300):
        for name, fmts in FORMATS.items():
            outs, lses = R.draw_states(n, (B, H, S, D), (B, H, S), fmts(n), seed=1000 * n + S, device=DEV)
            ref = R.reference_of(outs, lses)
            for out_dtype in (BF, HF, F32):
                out, lse = qa.merge_attn_states(outs, lses, out_dtype=out_dtype)
                assert out.dtype == out_dtype and out.shape == (B, H, S, D) and lse.shape == (B, H, S) and lse.dtype == F32
                r = _grade(out, lse, ref, out_dtype, f"D={D} n={n} S={S} {name}->{out_dtype}")
                worst = (max(worst[0], r[0]), max(worst[1], r[1]))
                empty = torch.from_numpy(~np.isfinite(ref[1])).to(DEV)
                assert not out[empty].any() and (lse[empty] == -math.inf).all(), "rows empty in every partial: zero rows, LSE -inf"
    print(f"D={D} n={n}: worst ratio over the sweep: out {worst[0]:.3f} lse {worst[1]:.4f}")


def _views(kind, o, l):
    """The state (o [B,H,S,D], l [B,H,S]) re-housed in a layout the library returns, pads filled with NaN; no copy is made afterwards."""
    Bq, Hq, S, D = o.shape
    nan = float("nan")
    if kind == "packed":           # the packed entries: [total, H, D] / [H, total]
        return o.permute(0, 2, 1, 3).reshape(Bq * S, Hq, D).contiguous(), l.permute(1, 0, 2).reshape(Hq, Bq * S).contiguous()
    if kind == "window":           # fp8_window_attn_func: permuted views of the packed buffers
        ob = o.permute(0, 2, 1, 3).contiguous()                         # [B, S, H, D]
        lb = l.permute(1, 0, 2).contiguous()                            # [H, B, S]
        return ob.permute(0, 2, 1, 3), lb.permute(1, 0, 2)
    if kind == "padded":           # QATTN_LSE_REFERENCE's padded rows, and O rows with a pad between them
        ld = _native.lib().qattn_lse_row_stride(S, _native.LSE_REFERENCE)
        lb = torch.full((Bq, Hq, ld + 4), nan, dtype=F32, device=o.device)
        lb[..., :S] = l
        ob = torch.full((Bq, Hq, S, D + 16), nan, dtype=o.dtype, device=o.device)
        ob[..., :D] = o
        return ob[..., :D], lb[..., :S]
    return o, l


@pytest.mark.parametrize("kind", ["packed", "window", "padded"])
def test_layouts_go_to_the_kernel_as_they_are(kind):
    S, D, n = 67, 128, 3
    outs, lses = R.draw_states(n, (B, H, S, D), (B, H, S), (F32, BF, BF), seed=7, device=DEV)
    want = qa.merge_attn_states(outs, lses, out_dtype=BF)
    vo, vl = zip(*(_views(kind, o, l) for o, l in zip(outs, lses)))
    assert all(_native.merge_addressable(o) for o in vo), "the views are addressed through their strides: no copy"
    if kind != "packed":
        assert not any(o.is_contiguous() for o in vo)
    got = qa.merge_attn_states(list(vo), list(vl), out_dtype=BF)
    if kind == "packed":
        got = (got[0].view(B, S, H, D).permute(0, 2, 1, 3), got[1].view(H, B, S).permute(1, 0, 2))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    _grade(got[0], got[1], R.reference_of(outs, lses), BF, f"layout {kind}")
    # in place on the views: the same bits, written through the views' strides
    acc, acc_l = vo[0].clone(memory_format=torch.preserve_format), vl[0].clone(memory_format=torch.preserve_format)
    want32 = qa.merge_attn_states(list(vo), list(vl))
    res = qa.merge_attn_states([acc] + list(vo[1:]), [acc_l] + list(vl[1:]), inplace=True)
    assert res[0] is acc and res[1] is acc_l and torch.equal(acc, want32[0]) and torch.equal(acc_l, want32[1])


def test_minus_inf_partial_with_nan_rows_gives_the_bits_of_the_merge_without_it():
    S, D = 67, 128
    for fmts in ((BF, BF, BF), (F32, BF, BF)):
        outs, lses = R.draw_states(3, (B, H, S, D), (B, H, S), fmts, seed=3, empty_rows=False, device=DEV)
        want = qa.merge_attn_states([outs[0], outs[2]], [lses[0], lses[2]])
        rows = torch.arange(S, device=DEV) % 3 != 1
        lses[1][..., rows] = -math.inf
        outs[1][..., rows, :] = float("nan")
        got = qa.merge_attn_states(outs, lses)
        assert torch.equal(got[0][..., rows, :], want[0][..., rows, :]) and torch.equal(got[1][..., rows], want[1][..., rows])
        assert not got[0].isnan().any() and not got[1].isnan().any()
        lses[0][..., rows] = -math.inf
        lses[2][..., rows] = -math.inf
        got = qa.merge_attn_states(outs, lses)
        assert not got[0][..., rows, :].any() and (got[1][..., rows] == -math.inf).all() and not got[0].isnan().any()


@pytest.mark.parametrize("n", [2, 8, 11])
def test_inplace_gives_the_bits_of_the_out_of_place_call(n):
    S, D = 300, 64
    outs, lses = R.draw_states(n, (B, H, S, D), (B, H, S), (F32,) + (BF,) * (n - 1), seed=n, device=DEV)
    want = qa.merge_attn_states(outs, lses)
    acc, acc_l = outs[0].clone(), lses[0].clone()
    got = qa.merge_attn_states([acc] + outs[1:], [acc_l] + lses[1:], inplace=True)
    assert got[0] is acc and got[1] is acc_l
    assert torch.equal(acc, want[0]) and torch.equal(acc_l, want[1])


def test_graph_capture_and_replay_give_the_bits_of_the_eager_call():
    S, D, n = 300, 128, 4
    outs, lses = R.draw_states(n, (B, H, S, D), (B, H, S), (BF,) * n, seed=11, device=DEV)
    want = qa.merge_attn_states(outs, lses)
    qa.merge_attn_states(outs, lses)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, lse = qa.merge_attn_states(outs, lses)
    out.zero_()
    lse.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want[0]) and torch.equal(lse, want[1])
    outs2, lses2 = R.draw_states(n, (B, H, S, D), (B, H, S), (BF,) * n, seed=12, device=DEV)
    want2 = qa.merge_attn_states(outs2, lses2)
    for a, b in zip(outs + lses, outs2 + lses2):
        a.copy_(b)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want2[0]) and torch.equal(lse, want2[1]), "a replay follows the buffers' new contents"


def test_compiled_call_traces_the_op():
    S, D = 67, 64
    outs, lses = R.draw_states(3, (B, H, S, D), (B, H, S), (BF,) * 3, seed=13, device=DEV)
    want = qa.merge_attn_states(outs, lses, out_dtype=HF)
    f = torch.compile(lambda o, l: torch.ops.quantumattention_amd.attention_state_merge(o, l, HF), fullgraph=True, backend="aot_eager")
    got = f(outs, lses)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("D, S, out_dtype", [(64, 67, BF), (128, 300, F32), (256, 1, HF)])
def test_buffer_contract_of_the_c_entry(D, S, out_dtype):
    """Guarded buffers (tests/arena.py) of exactly the documented sizes at exactly the documented alignments: out B H S D elements on 16
    bytes, lse_out B H S floats on 4; the inputs are padded views whose pads and guards hold NaN in one run and zeros in the other.
    Guards intact, every output byte written, the same bits whatever lies outside the described inputs."""
    n = 3
    fmts = (F32, BF, HF)
    outs, lses = R.draw_states(n, (B, H, S, D), (B, H, S), fmts, seed=17, device=DEV)
    ar = A.Arena(DEV)
    es = out_dtype.itemsize
    r_out = ar.carve("out", B * H * S * D * es, align=16, row_bytes=D * es, role="out", kind=A.KIND_OF_DTYPE[out_dtype])
    r_lse = ar.carve("lse_out", B * H * S * 4, align=4, row_bytes=4, role="out", kind="fp32")
    ll, vp = ctypes.c_longlong, ctypes.c_void_p
    results = []
    for hostile in (True, False):
        o_ptrs, l_ptrs, o_str, l_str = [], [], [], []
        for i, (o, l) in enumerate(zip(outs, lses)):
            per16 = 16 // o.element_size()
            so = (H * S * (D + per16) + per16, S * (D + per16), D + per16)          # rows a 16-byte pad apart, batches one more
            sl = (H * (S + 3) + 1, S + 3, 1)
            name_o, name_l = f"o{i}_{hostile}", f"lse{i}_{hostile}"
            ro = ar.carve(name_o, ((B - 1) * so[0] + (H - 1) * so[1] + (S - 1) * so[2] + D) * o.element_size(), align=16,
                          row_bytes=D * o.element_size(), role="in", kind=A.KIND_OF_DTYPE[o.dtype])
            rl = ar.carve(name_l, ((B - 1) * sl[0] + (H - 1) * sl[1] + (S - 1) * sl[2] + 1) * 4, align=4, row_bytes=4, role="in", kind="fp32")
            ro.set_guards(hostile)
            rl.set_guards(hostile)
            ro.load_view(o, so + (1,), hostile)
            rl.load_view(l, sl, hostile)
            o_ptrs.append(ro.ptr); l_ptrs.append(rl.ptr); o_str += so; l_str += sl
        r_out.fill_poison()
        r_lse.fill_poison()
        rc = _native.lib().qattn_attention_state_merge(
            n, (vp * n)(*o_ptrs), (ctypes.c_int * n)(*[_native._MERGE_FMT[d] for d in fmts]), (ll * (3 * n))(*o_str), (vp * n)(*l_ptrs),
            (ll * (3 * n))(*l_str), r_out.ptr, _native._MERGE_FMT[out_dtype], (ll * 3)(H * S * D, S * D, D), r_lse.ptr, (ll * 3)(H * S, S, 1),
            B, H, S, D, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        A.assert_guards_intact(ar)
        assert r_out.poison_left() == 0 and r_lse.poison_left() == 0, "every output byte is written"
        results.append((r_out.interior.clone(), r_lse.interior.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), "no dependence on bytes outside the inputs"
    out = results[0][0].view(out_dtype).view(B, H, S, D)
    lse = results[0][1].view(F32).view(B, H, S)
    _grade(out, lse, R.reference_of(outs, lses), out_dtype, f"arena D={D} S={S}")

"""The state merge with a learned sink (qattn_attention_state_merge_sink, include/qattn_sinks.h; `merge_attn_states_with_sinks`) against the
fp64 merge of the SAME inputs with the sink as one more state -- lse = sink_h, an O row of zeros -- under tests/merge_ref.py's bounds, the
existing merge tests' own: n = 1 .. 8 in one launch and 9 / 11 / 16 chained (the sink in the last launch alone), mixed bf16 / fp16 / fp32
partials, the dense and the packed stride conventions, in place through the C entry, rows empty in every partial (a zero row with
lse = sink_h exactly) and -inf sinks (the bits of the merge without a sink)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import merge_ref as R

pytestmark = pytest.mark.gpu

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
DEV = "cuda"
B, H = 2, 3
SINKS = (-45.0, -math.inf, 10.0)          # inside the LSEs' range [-64, 64], none, above most rows
MIXED = (F32, BF, HF)


def states(n, S, D, seed, fmts=None, packed=False):
    """tests/merge_ref.draw_states for n >= 1 (it draws at least two): rows that partial 1 skipped, rows empty in every partial"""
    m = max(n, 2)
    fmts = ((MIXED * 6)[:m]) if fmts is None else tuple(fmts) + (BF,) * (m - len(fmts))
    shape_o, shape_l = ((B * S, H, D), (H, B * S)) if packed else ((B, H, S, D), (B, H, S))
    outs, lses = R.draw_states(m, shape_o, shape_l, fmts, seed=seed, device=DEV)
    return outs[:n], lses[:n]


def reference_with_sink(outs, lses, sinks):
    packed = lses[0].dim() == 2
    s = sinks.to(DEV).float()
    sink_lse = (s[:, None] if packed else s[None, :, None]).expand_as(lses[0]).contiguous()
    return R.reference_of(list(outs) + [torch.zeros_like(outs[0], dtype=F32)], list(lses) + [sink_lse])


def _grade(out, lse, ref, out_dtype, what):
    r_out, r_lse = R.worst_ratios(out, lse, ref, out_dtype)
    print(f"{what}: worst out {r_out:.3f} lse {r_lse:.4f} of the bound")
    assert r_out <= 1.0 and r_lse <= 1.0, (what, r_out, r_lse)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 16])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_kernel_meets_the_bounds_of_the_fp64_merge_with_the_sink_as_one_more_state(D, n):
    snk = torch.tensor(SINKS, device=DEV)
    for S in (1, 67, 300):
        for packed in (False, True):
            outs, lses = states(n, S, D, 1000 * n + S, packed=packed)
            ref = reference_with_sink(outs, lses, snk)
            for out_dtype in (BF, F32) if S != 67 else (BF, HF, F32):
                out, lse = qa.merge_attn_states_with_sinks(outs, lses, snk, out_dtype=out_dtype)
                assert out.dtype == out_dtype and out.shape == outs[0].shape and lse.shape == lses[0].shape and lse.dtype == F32
                _grade(out, lse, ref, out_dtype, f"D={D} n={n} S={S} packed={packed}->{out_dtype}")
                # rows empty in every partial: a zero row, lse = sink_h exactly
                empty = torch.stack([torch.isneginf(l) for l in lses]).all(0)
                want = (snk[:, None] if packed else snk[None, :, None]).expand_as(lse)
                assert empty.any() and torch.equal(lse[empty], want[empty])
                assert not out[empty.t() if packed else empty].any()
            # -inf sinks: the merge without a sink, bit for bit
            if n > 1:
                a = qa.merge_attn_states_with_sinks(outs, lses, torch.full((H,), -math.inf, device=DEV), out_dtype=BF)
                b = qa.merge_attn_states(outs, lses, out_dtype=BF)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_sixteen_bit_sinks_are_up_cast_and_a_nan_or_inf_sink_poisons_its_head_alone():
    outs, lses = states(3, 67, 128, 5)
    snk = torch.tensor(SINKS, device=DEV)
    want = qa.merge_attn_states_with_sinks(outs, lses, snk)
    for dt in (BF, HF):
        got = qa.merge_attn_states_with_sinks(outs, lses, snk.to(dt))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for poison in (math.nan, math.inf):
        bad = snk.clone()
        bad[2] = poison
        out, lse = qa.merge_attn_states_with_sinks(outs, lses, bad)
        assert out[:, 2].isnan().all() and lse[:, 2].isnan().all()
        assert torch.equal(out[:, :2], want[0][:, :2]) and torch.equal(lse[:, :2], want[1][:, :2])


@pytest.mark.parametrize("n", [1, 4, 8])
def test_in_place_through_the_c_entry_gives_the_bits_of_the_out_of_place_call(n):
    """out = o[0] and lse_out = lse[0] with equal strides: the aliasing the merge entry allows"""
    S, D = 300, 64
    outs, lses = states(n, S, D, n, fmts=(F32,))
    snk = torch.tensor(SINKS, device=DEV)
    want = qa.merge_attn_states_with_sinks(outs, lses, snk)
    acc, acc_l = outs[0].clone(), lses[0].clone()
    got = _native.attention_state_merge_sink([acc] + outs[1:], [acc_l] + lses[1:], snk, out=acc, lse_out=acc_l)
    assert got[0] is acc and got[1] is acc_l and torch.equal(acc, want[0]) and torch.equal(acc_l, want[1])


def test_graph_capture_follows_rewritten_sinks_and_the_compiled_op_traces():
    S, D, n = 67, 128, 3
    outs, lses = states(n, S, D, 11)
    snk = torch.tensor(SINKS, device=DEV)
    qa.merge_attn_states_with_sinks(outs, lses, snk)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, lse = qa.merge_attn_states_with_sinks(outs, lses, snk)
    for new in ((0.0, 1.0, -70.0), (-math.inf,) * 3, SINKS):
        snk.copy_(torch.tensor(new))
        g.replay()
        torch.cuda.synchronize()
        want = qa.merge_attn_states_with_sinks(outs, lses, torch.tensor(new, device=DEV))
        assert torch.equal(out, want[0]) and torch.equal(lse, want[1]), new
    f = torch.compile(lambda o, l, s: torch.ops.quantumattention_amd.attention_state_merge_sink(o, l, s, HF), fullgraph=True, backend="aot_eager")
    got, want = f(outs, lses, snk), qa.merge_attn_states_with_sinks(outs, lses, snk, out_dtype=HF)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_the_c_entry_refuses_what_it_documents():
    L = _native.lib()
    outs, lses = states(2, 5, 64, 1, fmts=(BF, BF))
    snk = torch.tensor(SINKS, device=DEV)
    out, lse = torch.empty_like(outs[0]), torch.empty_like(lses[0])
    ll, vp = ctypes.c_longlong, ctypes.c_void_p

    def rc(n, sink_ptr):
        m = max(n, 1)
        return L.qattn_attention_state_merge_sink(
            n, (vp * m)(*[outs[i % 2].data_ptr() for i in range(m)]), (ctypes.c_int * m)(*[_native.FMT_BF16] * m), (ll * (3 * m))(*[H * 5 * 64, 5 * 64, 64] * m),
            (vp * m)(*[lses[i % 2].data_ptr() for i in range(m)]), (ll * (3 * m))(*[H * 5, 5, 1] * m), out.data_ptr(), _native.FMT_BF16,
            (ll * 3)(H * 5 * 64, 5 * 64, 64), lse.data_ptr(), (ll * 3)(H * 5, 5, 1), B, H, 5, 64, torch.cuda.current_stream().cuda_stream, sink_ptr)

    assert rc(1, snk.data_ptr()) == 0 and rc(8, snk.data_ptr()) == 0
    assert rc(0, snk.data_ptr()) == -1 and rc(9, snk.data_ptr()) == -1 and rc(2, None) == -1 and rc(2, snk.data_ptr() + 2) == -1
    torch.cuda.synchronize()
    assert np.isfinite(lse.cpu().numpy()[:, [0, 2]]).all()

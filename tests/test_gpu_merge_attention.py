"""Merged attention states through the real kernels: partial calls over pieces of K / V merged into the result over all keys
(quantumattention_amd/merge.py).  The merge is graded twice: against the fp64 merge of the kernels' OWN partials with the bounds of
tests/merge_ref.py (that isolates the merge), and against fp32 SDPA of the unquantised inputs over all keys with the bar the project
takes from the reference, RMSE < 1e-2."""
import math

import numpy as np
import pytest
import torch

import oracle
import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import merge_ref as R
from tests.gpu_utils import bits16

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
RMSE_BAR = 1e-2
# LSE of the dense fused step against the fp64 LSE of the quantised scores, per row path (restated from tests/test_gpu_attention.py):
# one-term rows of the head_dim-128 kernel (sums of e4m3 weights) 2e-2, other one-term / two-term rows 2e-3, 16-bit-V rows 4e-3
LSE_TOL_ONE_TERM_D128, LSE_TOL_EXACT, LSE_TOL_V16 = 2e-2, 2e-3, 4e-3
PATH_ONE_TERM, PATH_V16 = 0, 2


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(BF).to(DEV)


def _sdpa(q, k, v, causal=False):
    g = q.shape[1] // k.shape[1]
    return torch.nn.functional.scaled_dot_product_attention(q.float(), k.float().repeat_interleave(g, dim=1),
                                                            v.float().repeat_interleave(g, dim=1), is_causal=causal)


def _rmse(a, b):
    return float((a.float() - b.float()).pow(2).mean().sqrt())


def _grade_merge(parts, got, what):
    outs, lses = [p[0] for p in parts], [p[1] for p in parts]
    r_out, r_lse = R.worst_ratios(got[0], got[1], R.reference_of(outs, lses), got[0].dtype)
    print(f"{what}: merge vs the fp64 merge of the kernels' partials: worst out {r_out:.3f} lse {r_lse:.4f} of the bound")
    assert r_out <= 1.0 and r_lse <= 1.0, (what, r_out, r_lse)


# ---- (a) K / V split ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 64])
def test_kv_split_through_the_packed_and_the_block_sparse_entries(D):
    Sq, pieces, Hq, Hkv = 300, (40, 260, 800), 4, 2
    q, k, v = _randn(1, Hq, Sq, D, seed=1), _randn(1, Hkv, sum(pieces), D, seed=2), _randn(1, Hkv, sum(pieces), D, seed=3)
    ref = _sdpa(q, k, v)
    cuts = np.cumsum((0,) + pieces)
    # packed entry: one sequence per call
    qp = q[0].transpose(0, 1).contiguous()
    i32 = lambda *x: torch.tensor(x, dtype=torch.int32, device=DEV)
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        kp, vp = (t[0, :, a:b].transpose(0, 1).contiguous() for t in (k, v))
        parts.append(qa.fp8_attn_varlen_func(qp, kp, vp, i32(0, Sq), i32(0, b - a), Sq, int(b - a), return_lse=True))
    got = qa.merge_attn_states([p[0] for p in parts], [p[1] for p in parts])
    assert got[0].shape == (Sq, Hq, D) and got[1].shape == (Hq, Sq)
    _grade_merge(parts, got, f"packed D={D}")
    rmse = _rmse(got[0].transpose(0, 1)[None], ref)
    print(f"packed D={D}: RMSE against SDPA over all keys {rmse:.5f}")
    assert rmse < RMSE_BAR
    # block-sparse entry under an all-true mask
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        mask = torch.ones(1, Hq, -(-Sq // 128), -(-int(b - a) // 128), dtype=torch.bool, device=DEV)
        parts.append(qa.fp8_block_sparse_attn_func(q, k[:, :, a:b].contiguous(), v[:, :, a:b].contiguous(), mask, return_lse=True))
    got = qa.merge_attn_states([p[0] for p in parts], [p[1] for p in parts])
    _grade_merge(parts, got, f"block-sparse D={D}")
    rmse = _rmse(got[0], ref)
    print(f"block-sparse D={D}: RMSE against SDPA over all keys {rmse:.5f}")
    assert rmse < RMSE_BAR


# ---- (b) several sources ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(1100, 200), (1100, 200, 64)])
def test_multi_kv_func(lens):
    Sq, Hq, Hkv, D = 300, 4, 2, 128
    q = _randn(1, Hq, Sq, D, seed=10)
    kvs = [(_randn(1, Hkv, n, D, seed=20 + i), _randn(1, Hkv, n, D, seed=30 + i)) for i, n in enumerate(lens)]
    out, lse = qa.fp8_attn_multi_kv_func(q, kvs, return_lse=True)
    assert out.shape == q.shape and out.dtype == BF and lse.shape == (1, Hq, Sq)
    assert torch.equal(qa.fp8_attn_multi_kv_func(q, kvs), out)
    states = [qa.fp8_attn_lse_func(q, k, v) for k, v in kvs]
    want = qa.merge_attn_states([s[0] for s in states], [s[1] for s in states])
    assert torch.equal(out, want[0]) and torch.equal(lse, want[1]), "the function IS one lse call per pair and one merge"
    k, v = (torch.cat([kv[i] for kv in kvs], dim=2) for i in (0, 1))
    rmse = _rmse(out, _sdpa(q, k, v))
    ref_lse = torch.logsumexp(q.float() @ k.float().repeat_interleave(Hq // Hkv, dim=1).transpose(-1, -2) / math.sqrt(D), dim=-1)
    print(f"multi_kv {lens}: RMSE against SDPA over the concatenation {rmse:.5f}, LSE max error {float((lse - ref_lse).abs().max()):.4f}")
    assert rmse < RMSE_BAR      # (the LSE figure is printed only: the kernels' own LSE tolerances are held in test_fp8_attn_lse_func)


# ---- (c) ring rehearsal on one GPU --------------------------------------------------------------------------------------------------
def test_ring_rehearsal_causal_over_three_shards():
    """What rank r of a sequence-parallel ring computes, one rank after the other: full attention over the key shards before its own,
    bottom-right causal attention over its own, nothing for the later ones -- accumulated IN PLACE in an fp32 state that starts empty."""
    H, D, lens = 4, 128, (384, 384, 332)
    S = sum(lens)
    q, k, v = _randn(1, H, S, D, seed=40), _randn(1, H, S, D, seed=41), _randn(1, H, S, D, seed=42)
    cuts = np.cumsum((0,) + lens)
    shard = lambda t, r: t[:, :, cuts[r]:cuts[r + 1]].contiguous()
    out = torch.empty(1, H, S, D, dtype=F32, device=DEV)
    for r in range(3):
        acc = torch.zeros(1, H, lens[r], D, dtype=F32, device=DEV)
        acc_lse = torch.full((1, H, lens[r]), -math.inf, dtype=F32, device=DEV)
        for s in range(r + 1):
            if s < r:
                part = qa.fp8_attn_lse_func(shard(q, r), shard(k, s), shard(v, s))
            else:
                part = qa.fp8_window_attn_func(shard(q, r), shard(k, s), shard(v, s), (-1, 0), return_lse=True)
            res = qa.merge_attn_states([acc, part[0]], [acc_lse, part[1]], inplace=True)
            assert res[0] is acc and res[1] is acc_lse
        assert not acc.isnan().any() and torch.isfinite(acc_lse).all()
        out[:, :, cuts[r]:cuts[r + 1]] = acc
    rmse = _rmse(out, _sdpa(q, k, v, causal=True))
    print(f"ring rehearsal: RMSE against full causal SDPA {rmse:.5f}")
    assert rmse < RMSE_BAR
    v0 = v[0, :, 0].float()
    assert ((out[0, :, 0] - v0).abs() <= 2.0 ** -7 * v0.abs()).all(), "the first row attends key 0 alone: V[0] to within one bf16 step"


# ---- (d) empty rows through real kernels ----------------------------------------------------------------------------------------------
def test_rows_a_window_left_empty_take_the_other_partial_exactly():
    """300 queries over 200 keys under (-1, 0): delta = -100, rows 0 .. 99 attend nothing (zero rows, LSE -inf).  Merged with a second bf16
    partial into bf16, those rows ARE the second partial: one contributing partial has weight exp(0) = 1 and a sum of weights of 1."""
    H, D, Sq = 4, 128, 300
    q = _randn(1, H, Sq, D, seed=50)
    k1, v1, k2, v2 = _randn(1, H, 200, D, seed=51), _randn(1, H, 200, D, seed=52), _randn(1, H, 260, D, seed=53), _randn(1, H, 260, D, seed=54)
    win = qa.fp8_window_attn_func(q, k1, v1, (-1, 0), return_lse=True)
    assert (win[1][..., :100] == -math.inf).all() and not win[0][..., :100, :].any() and torch.isfinite(win[1][..., 100:]).all()
    other = qa.fp8_attn_lse_func(q, k2, v2)
    for order in ((win, other), (other, win)):
        out, lse = qa.merge_attn_states([order[0][0], order[1][0]], [order[0][1], order[1][1]])
        assert torch.equal(out[..., :100, :], other[0][..., :100, :]) and torch.equal(lse[..., :100], other[1][..., :100])
        assert not out.isnan().any() and not lse.isnan().any()
        _grade_merge(order, (out, lse), "window + dense")


# ---- (e) the dense step with its LSE ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D, causal", [(128, False), (128, True), (64, False)])
def test_fp8_attn_lse_func(D, causal):
    Hq, Hkv, Sq, Skv = 4, 2, 1300, 1300
    q, k, v = _randn(1, Hq, Sq, D, seed=60), _randn(1, Hkv, Skv, D, seed=61), _randn(1, Hkv, Skv, D, seed=62)
    out, lse = qa.fp8_attn_lse_func(q, k, v, causal)
    plain = qa.fp8_attn_func(q, k, v, is_causal=causal)
    keeps = qa.merge.lse_request_keeps_out_bits(D, BF, Skv)
    assert keeps == (D == 128), "include/qattn.h PATH TABLE: only the head_dim-128 kernel sums the weights it already has"
    if keeps:
        assert torch.equal(out, plain), "the path table promises the bits of fp8_attn_func"
    rmse = _rmse(out, _sdpa(q, k, v, causal))
    print(f"lse_func D={D} causal={causal}: RMSE against SDPA {rmse:.5f}; out == fp8_attn_func: {torch.equal(out, plain)}")
    assert rmse < RMSE_BAR and _rmse(out, plain) < RMSE_BAR
    # the LSE against the fp64 LSE of the quantised scores, per row path (the same C call reports it)
    _, lse_c, path = _native.fp8_quant_attention_forward(q, k, v, is_causal=causal, return_lse=True, return_path=True)
    assert torch.equal(lse_c, lse)
    q8, sq = oracle.quantize_fp8(bits16(q), oracle.FMT_BF16, "head")
    k8, sk = oracle.quantize_fp8(bits16(k), oracle.FMT_BF16, "head")
    _, ref_lse = oracle.attention_forward(q8, k8, bits16(v), 0, 0, oracle.FMT_BF16, sq, sk, None, causal=causal, return_lse=True)
    path = path.cpu().numpy()
    tol = np.where(path == PATH_ONE_TERM, LSE_TOL_ONE_TERM_D128 if D == 128 else LSE_TOL_EXACT,
                   np.where(path == PATH_V16, LSE_TOL_V16, LSE_TOL_EXACT))
    err = np.abs(lse.cpu().numpy() - ref_lse)
    print(f"lse_func D={D} causal={causal}: worst LSE error / tolerance {float((err / tol).max()):.3f}")
    assert (err < tol).all(), float((err / tol).max())

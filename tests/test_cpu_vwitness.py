"""No GPU: the constant-V witness of tests/vwitness.py has teeth ("V-format witness").

separation     every witness channel's fp8 reading is >= 5x the 16-bit-V bound away from its 16-bit value (e4m3 and e5m2, bf16 and fp16,
               D = 64, 128, 256), and the block-scaled and head-scaled readings are one vector.
independence   oracle.attention_forward on the witness V returns the constant vector of each query head's OWN kv head within 1e-6, on the
               16-bit V and on the fp8 V, causal or not, on flat and on mixed scores: the output does not depend on P.
teeth          rows swapped between the two references change label, exactly those; a row of the other kv head is "neither"; gpu_utils.grade
               with one row's path flipped fails by >= 5x on the witness V -- and the same flip on an N(0,1) V is printed: the hole.
non-vacuity    every mixed case of the GPU test holds >= 32 severe and >= 32 moderate rows outside the early query blocks."""
import numpy as np
import pytest
import torch

import oracle
from tests import vwitness as W
from tests.vwitness import FMT, FP8, NEITHER, V16, bits16, fmt16

DTYPES = [torch.bfloat16, torch.float16]
B, HQ, HKV = 1, 4, 2


# ---- separation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("fp8", ["e4m3", "e5m2"])
def test_every_witness_channel_is_five_bounds_from_its_fp8_reading(fp8, dtype, D):
    v16, vfp8 = W.witness_vectors(HKV, D, dtype, fp8)
    assert (v16[:, 0] == W.TOP).all() and (vfp8[:, 0] == W.TOP).all()
    ratio = (np.abs(vfp8 - v16) / W.bound_v16(v16))[:, 1:]
    print(f"{fp8} D {D}: |fp8 reading - value| / (2^-7 max(1, |v|)) over the witness channels: {ratio.min():.2f} .. {ratio.max():.2f} "
          f"({len(W.witness_values(fp8))} values)")
    assert ratio.min() >= W.SEPARATION
    assert not np.array_equal(v16[0], v16[1]), "the kv heads carry different vectors"
    # the whole tensor, at a key count that is no multiple of 64: block reading == head reading == the vector (asserted inside)
    v = W.witness_v(B, HKV, 1023, D, dtype, fp8)
    assert v.shape == (B, HKV, 1023, D) and (v == v[:, :, :1]).all(), "constant along the key axis"


def test_the_values_the_issue_names_are_found_by_the_search():
    """e4m3: 1.0546875, 1.0703125, 1.1796875, 1.1953125 (non-tie) and the tie 1.0625; e5m2: 1.1171875, 1.1328125"""
    assert set((1.0546875, 1.0703125, 1.1796875, 1.1953125, 1.0625)) <= set(W.witness_values("e4m3"))
    assert set((1.1171875, 1.1328125)) <= set(W.witness_values("e5m2"))


# ---- independence from P --------------------------------------------------------------------------------------------------------------
S_CPU = 320


def _oracle_pair(q, k, v, dtype, fp8, causal, scaling="head"):
    """(out on the block-scaled fp8 V, out on the head-scaled fp8 V, out on the 16-bit V): fp64 SDPA on the quantised q, k"""
    f = FMT[fp8]
    q8, sq = oracle.quantize_fp8(bits16(q.to(dtype)), fmt16(dtype), scaling, f)
    k8, sk = oracle.quantize_fp8(bits16(k.to(dtype)), fmt16(dtype), scaling, f)
    vb = bits16(v)
    _, _, vdq = oracle.quantize_v_block(vb, fmt16(dtype), f)
    v8, sv = oracle.quantize_fp8(vb, fmt16(dtype), "head", f, "compiled")
    run = lambda vv, vf, s: oracle.attention_forward(q8, k8, vv, f, f, vf, sq, sk, s, scale_mode=scaling, causal=causal)
    return run(vdq, oracle.FMT_BF16, None), run(v8, f, sv), run(vb, fmt16(dtype), None)


@pytest.mark.parametrize("kind", ["flat", "mixed"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("fp8,dtype", [("e4m3", torch.bfloat16), ("e4m3", torch.float16), ("e5m2", torch.bfloat16)])
def test_the_oracle_returns_the_constant_vector_whatever_the_weights(fp8, dtype, causal, kind):
    D = 64
    q, k = W.scores_case(S_CPU, D, kind, 3, causal)
    v = W.witness_v(B, HKV, S_CPU, D, dtype, fp8)
    v16, vfp8 = (W.per_q_head(t, HQ)[None, :, None, :] for t in W.witness_vectors(HKV, D, dtype, fp8))
    out_block, out_head, out16 = _oracle_pair(q, k, v, dtype, fp8, causal)
    for name, out, vec in (("block-scaled fp8 V", out_block, vfp8), ("head-scaled fp8 V", out_head, vfp8), ("16-bit V", out16, v16)):
        assert np.abs(out - vec).max() <= 1e-6, (name, float(np.abs(out - vec).max()))     # (GQA: each query head its own kv head's vector)
    assert (W.classify(out16, v16, vfp8)[0] == V16).all() and (W.classify(out_block, v16, vfp8)[0] == FP8).all()


# ---- classifier teeth -----------------------------------------------------------------------------------------------------------------
def _flip_ratios(out8, out16):
    """per row: what gpu_utils.grade's worst |err| / bound becomes when the row's path is reported wrongly -- an fp8 row reported V16
    (graded against the 16-bit oracle at 2^-7 max(1, |ref|)) and a V16 row reported fp8 (against the fp8 oracle at 2^-6 max(1, |ref|/2))"""
    d = np.abs(np.asarray(out8, np.float64) - np.asarray(out16, np.float64))
    return (d / W.bound_v16(out16)).max(-1), (d / W.bound_fp8(out8)).max(-1)


def test_classifier_and_grader_teeth_on_oracle_outputs():
    from tests.gpu_utils import PATH_ONE_TERM, PATH_TWO_TERM, PATH_V16, PathRef, grade   # (imports the product's binding: no device call)

    D, dtype, fp8 = 64, torch.bfloat16, "e4m3"
    q, k = W.scores_case(S_CPU, D, "flat", 5)
    v = W.witness_v(B, HKV, S_CPU, D, dtype, fp8)
    v16, vfp8 = (W.per_q_head(t, HQ)[None, :, None, :] for t in W.witness_vectors(HKV, D, dtype, fp8))
    out8, _, out16 = _oracle_pair(q, k, v, dtype, fp8, False)
    rng = np.random.default_rng(0)
    # k rows swapped between the two references: exactly those rows change label
    swap = np.zeros((B, HQ, S_CPU), bool)
    swap.reshape(-1)[rng.choice(swap.size, 37, replace=False)] = True
    mixed = np.where(swap[..., None], out16, out8)
    labels, worst = W.classify(mixed, v16, vfp8)
    assert np.array_equal(labels == V16, swap) and np.array_equal(labels == FP8, ~swap)
    assert worst[V16] <= 1e-6 and worst[FP8] <= 1e-6
    # a row of the OTHER kv head (query head 0 reads kv head 0, query head 2 kv head 1), in either format: neither
    for src in (out16, out8):
        wrong = mixed.copy()
        wrong[0, 0, 11], wrong[0, 3, 200] = src[0, 2, 11], src[0, 1, 200]
        lab = W.classify(wrong, v16, vfp8)[0]
        assert lab[0, 0, 11] == NEITHER and lab[0, 3, 200] == NEITHER and (lab == NEITHER).sum() == 2
    # W.require reports the factor
    with pytest.raises(AssertionError, match="bound = "):
        W.require(labels, mixed, v16, vfp8, np.full(S_CPU, FP8, object), "all rows fp8")
    W.require(labels, mixed, v16, vfp8, np.where(swap, V16, FP8), "the true labels")
    # the grader of the parity tests, the true path and one flipped row of each kind
    ref = PathRef(out8, out16)
    path = np.where(swap, PATH_V16, PATH_ONE_TERM).astype(np.uint8)
    assert grade(mixed, ref, path)[2] < 1e-3
    as16, as8 = _flip_ratios(out8, out16)
    print(f"witness V: an fp8 row reported V16 misses by {as16.min():.2f}x .. {as16.max():.2f}x; a V16 row reported fp8 by {as8.min():.2f}x .. {as8.max():.2f}x")
    assert as16.min() >= W.SEPARATION


@pytest.mark.parametrize("fp8", ["e4m3", "e5m2"])
def test_grade_with_a_flipped_path_fails_by_five_on_the_witness_v_and_the_hole_on_gaussian_v(fp8):
    """gpu_utils.grade with ONE row's path flipped fails on the witness V and passes with the true path.
    An fp8-V row reported as V16 is held against the 16-bit vector at 2^-7 max(1, |v|): >= 5x, by construction of the witness values.
    A V16 row reported as fp8 is held against the fp8 vector at 2^-6 (|v| < 2), a bound twice as wide: e5m2 (grid 0.25 under the
    2^-15 scale) still misses by >= 5x; e4m3 (grid 0.125 under 2^-8) can move a value by at most half a step, 2^-4 = 4.0 bounds, reached
    on the tie values, which the flipped row carries -- asserted as 4.0x exactly.  The same flips on an N(0,1) V of the same shape are the hole being closed: printed
    (DESIGN.md), not asserted."""
    from tests.gpu_utils import PATH_ONE_TERM, PATH_V16, PathRef, grade

    S, causal = W.SHAPE_FULL
    D, dtype = 64, torch.bfloat16
    q, k = W.scores_case(S, D, "flat", 5)
    v = W.witness_v(B, HKV, S, D, dtype, fp8)
    out8, _, out16 = _oracle_pair(q, k, v, dtype, fp8, causal)
    vn = torch.from_numpy(np.random.default_rng(9).standard_normal((B, HKV, S, D)).astype(np.float32)).to(dtype)
    n8, _, n16 = _oracle_pair(q, k, vn, dtype, fp8, causal)
    res = {}
    for true, flipped, need in ((PATH_ONE_TERM, PATH_V16, W.SEPARATION), (PATH_V16, PATH_ONE_TERM, W.SEPARATION if fp8 == "e5m2" else 4.0)):
        path = np.full((B, HQ, S), true, np.uint8)
        got, gotn = (out16, n16) if true == PATH_V16 else (out8, n8)
        assert grade(got, PathRef(out8, out16), path)[2] < 1e-3, "the true path passes"
        path[0, 1, 700] = flipped
        witness = grade(got, PathRef(out8, out16), path)[2]
        assert witness >= need - 1e-3, (true, flipped, witness)
        if need == 4.0:   # e4m3, a V16 row reported fp8: half a step of the 2^-3 grid against 2^-6, no more and no less
            assert abs(witness - 4.0) <= 1e-3, witness
        res[(true, flipped)] = (witness, grade(gotn, PathRef(n8, n16), path)[2])
    as16, as8 = _flip_ratios(n8, n16)
    (w1, g1), (w2, g2) = res[(PATH_ONE_TERM, PATH_V16)], res[(PATH_V16, PATH_ONE_TERM)]
    print(f"{fp8} S {S} D {D}, one flipped row: fp8 reported V16 -- witness V {w1:.2f}x its bound, N(0,1) V {g1:.3f}x; V16 reported fp8 -- witness V "
          f"{w2:.2f}x, N(0,1) V {g2:.3f}x.  ANY row flipped on the N(0,1) V: worst {as16.max():.3f}x (median {np.median(as16):.3f}x) as V16, worst "
          f"{as8.max():.3f}x as fp8; max |fp8 oracle - 16-bit oracle| {np.abs(n8 - n16).max():.5f}")


# ---- non-vacuity of the mixed cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,scaling,dtype,fp8", W.MIXED, ids=lambda x: str(x).replace("torch.", ""))
def test_mixed_cases_hold_enough_severe_and_moderate_rows(D, scaling, dtype, fp8):
    for S, causal in (W.SHAPE_FULL, W.SHAPE_CAUSAL):
        q, k = W.scores_case(S, D, "mixed", W.MIXED_SEED, causal)
        severe, moderate = W.peaked_rows(q, k, dtype, fp8, scaling, causal)
        late = ~W.early_rows(S, S, causal)
        n_sev, n_mod = int(severe[..., late].sum()), int(moderate[..., late].sum())
        planted = int(S * W.PLANTED_SHARE) * HQ
        print(f"mixed S {S} causal {causal} D {D} {scaling} {fp8}: {n_sev} severe (R <= 4), {n_mod} moderate (10 <= R <= 20) rows outside the early blocks")
        assert n_sev >= W.MIN_ROWS and n_mod >= W.MIN_ROWS, (S, causal, n_sev, n_mod)
        assert W.PLANTED_SHARE <= 0.10 and n_sev <= planted // 2, "at most 10 % of the rows are planted, half of them severe (a flat row may be moderate by chance)"
        # no head starts in the precise mode: the per-head mean square of q stays that of N(0,1) (the moments the starting mode reads)
        msq = (q.double() ** 2).mean(dim=(2, 3))
        assert ((msq > 0.95) & (msq < 1.05)).all(), msq

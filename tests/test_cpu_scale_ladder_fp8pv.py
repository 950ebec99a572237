"""The scale ladder for the FP8-PV family on the CPU ("Scale ladder for the FP8-PV and split-KV entries"): on the very cases
and used lengths tests/test_gpu_scale_ladder_fp8pv.py runs, every named way of reading a head-wise scale at the wrong index moves the fp64
reference by >= TEETH = 4 x the bound the GPU test applies.  The teeth are CONDITIONS on the inputs; every figure is printed.

What is new against tests/test_cpu_scale_ladder.py: one mask per batch entry (seqused_k, bottom-right causal), one fp8 V scale per head
on every case, and the TILE mutants -- the split-KV kernels pack the rows of a kv head's G query heads into 128-row tiles, so `g` (and
scale_q) differs per lane.  "Every row of a tile reads the scale_q of the tile's first row" stays BELOW the teeth on the head ladder
(F_HEAD only makes a std-0.25 head look like a std-1 head: nothing collapses) -- the last test shows that hole -- and is reached by
`group_ladder`, whose scale_q inside a GQA group differs by x4 with the larger scale on the group's first head."""
import numpy as np
import pytest
import torch

from tests import scale_ladder as L
from tests.scale_ladder import B, HQ, TEETH
from tests.test_cpu_scale_ladder import JUDGED_KEYS, V_SHARE

FLAT_W, FLAT_KEYS = 1.0 / 16, 128     # group ladder, EVERY judged row: the sparse heads' scores lie on a lattice, their rows are a little
                                      # less flat than the dense ones (L.FLAT_W, L.FLAT_KEYS hold for >= L.FLAT_SHARE of the rows)
IDS = [L.case_id(c) for c in L.FP8PV_CASES]
PACKED_IDS = [f"D{c[0]}_S{c[1]}_{L.NAME[c[2]]}_{c[3]}" for c in L.PACKED_CASES]


def judged_rows(mask):
    """bool [B, 1 or HQ, Sq, Skv] -> [B, HQ, Sq]: rows that attend at least one 64-key chunk"""
    return np.broadcast_to(mask.sum(-1) >= JUDGED_KEYS, (B, HQ, mask.shape[2]))


def too_large(qz, rs, cs, mask):
    return np.stack([L.too_large(qz, rs, cs, mask[b])[b] for b in range(B)])


def scale_teeth(qz, sc, ref, mutants, mask):
    """tests/test_cpu_scale_ladder.scale_teeth (head-level rule) with one mask per batch entry: the best, over the (batch, head) groups
    whose every judged row gets a score scale >= LARGE x too large, of the group's WORST row"""
    judged = judged_rows(mask)
    res = {}
    for name, (rs, cs) in mutants.items():
        large = too_large(qz, rs, cs, mask) & judged
        mv = L.moved(ref, sc.softmax(rs, cs)[0])
        groups = [(b, h) for b in range(B) for h in range(HQ) if large[b, h].any() and (large[b, h] == judged[b, h]).all()]
        assert groups, (name, "the mutant makes no group's scores >= 4 x too large: the ladder does not reach it")
        res[name] = max(float(mv[b, h][judged[b, h]].min()) for b, h in groups)
    return res


def vhead_teeth(qz, sc, ref, mask, what):
    """tests/test_cpu_scale_ladder.vhead_teeth with one mask per batch entry"""
    judged = judged_rows(mask)
    for name, (v, lg) in L.vhead_mutants(qz).items():
        mv = L.moved(ref, sc.softmax(v=v)[0])
        share = {(b, h): float((mv[b, h][judged[b, h]] >= TEETH).mean()) for b in range(B) for h in range(HQ) if lg[b, L.kv_of(h)] != 0}
        assert share, name
        print(f"V head ladder {what}: {name}: best touched group {100 * max(share.values()):.1f} % of its rows by >= {TEETH:.0f} x the bound")
        assert max(share.values()) >= V_SHARE, (name, share)


def masks_of(case):
    """{name: mask [B, 1 or HQ, Sq, Skv]} a case is run under on the GPU"""
    D, Sq, Skv, causal = case[:4]
    return {"used": L.used_mask(Sq, Skv, L.used_lengths(Skv), causal)}


def packed_masks(S):
    used = L.used_lengths(S)
    rep = lambda m: np.broadcast_to(m, (B,) + m.shape).copy()
    return {"full, seqused_k": L.used_mask(S, S, used, False), "causal (top-left), seqused_k": L.used_mask(S, S, used, True, top_left=True),
            "window": rep(L.mask_of(S, S, window=L.WINDOW)), "window (-1, 0)": L.used_mask(S, S, [S, S], True),
            "all tiles": rep(L.mask_of(S, S)), "sparse tiles": rep(L.mask_of(S, S, tiles=L.sparse_tiles(S)))}


def head_teeth(what, D, Sq, Skv, dtype, fp8, masks):
    """the head mutants on the plain-V head ladder and the V mutants on the V head ladder, under every mask"""
    qz = L.quantise(L.head_ladder_plain_v(D, Sq, Skv), dtype, fp8, "head", v_block=False)
    qv = L.quantise(L.head_ladder(D, Sq, Skv, v_head=True), dtype, fp8, "head", v_block=False)
    for name, mask in masks.items():
        sc = L.UsedScores(qz, mask)
        res = scale_teeth(qz, sc, sc.softmax()[0], L.head_mutants(qz, packed=True), mask)
        for mut, t in res.items():
            print(f"head ladder, plain V, {what} {name}: {mut}: teeth {t:.2f} x the bound")
        assert min(res.values()) >= TEETH, (name, res)
        sv = L.UsedScores(qv, mask)
        vhead_teeth(qv, sv, sv.softmax()[0], mask, f"{what} {name}")


def test_the_reference_with_one_mask_per_batch_entry_is_the_oracles():
    """UsedScores.softmax (the reference of the GPU tests, the teeth's) against oracle.attention_forward per batch entry, causal with
    q_offset = L_b - Sq (tests/test_gpu_splitkv.py grades with that call), on a case whose second entry ends inside a key block"""
    import oracle
    D, Sq, Skv, causal, dtype, fp8 = L.FP8PV_CASES[4]
    qz = L.quantise(L.group_ladder(D, Sq, Skv), dtype, fp8, "head", v_block=False)
    used = L.used_lengths(Skv)
    out, lse = L.UsedScores(qz, L.used_mask(Sq, Skv, used, causal)).softmax()
    f = L.FMT[fp8]
    for b, n in enumerate(used):
        ref, ref_lse = oracle.attention_forward(qz.q8[b:b + 1], qz.k8[b:b + 1, :, :n], qz.v8[b:b + 1, :, :n], f, f, f, qz.sq[b:b + 1], qz.sk[b:b + 1],
                                                qz.sv[b:b + 1], causal=causal, q_offset=n - Sq, return_lse=True)
        assert np.abs(out[b] - ref[0]).max() < 2e-6 * max(1.0, np.abs(ref).max()) and np.abs(lse[b] - ref_lse[0]).max() < 1e-5


# ---- the head ladder ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.FP8PV_CASES, ids=IDS)
def test_head_and_v_head_ladder_teeth_on_the_split_kv_cases_at_their_used_lengths(case):
    D, Sq, Skv, causal, dtype, fp8 = case
    head_teeth(L.case_id(case), D, Sq, Skv, dtype, fp8, masks_of(case))


@pytest.mark.parametrize("case", L.PACKED_CASES, ids=PACKED_IDS)
def test_head_and_v_head_ladder_teeth_on_the_fp8pv_siblings(case):
    """block-sparse (all tiles, sparse tiles), packed (causal and not, with seqused_k) and window FP8-PV: fp8 P on the head's fp8 V"""
    D, S, dtype, fp8 = case
    head_teeth(f"D {D} S {S}", D, S, S, dtype, fp8, packed_masks(S))


@pytest.mark.parametrize("case", L.FP8PV_CASES, ids=IDS)
def test_the_ladders_quantise_exactly(case):
    """bytes 0 or +- the largest code; every scale an exact power of two times the plain scale (that of a tensor whose abs-max is 1)"""
    D, Sq, Skv, causal, dtype, fp8 = case
    top = L.TOP_CODE[fp8]
    for lad in (L.group_ladder(D, Sq, Skv), L.head_ladder_plain_v(D, Sq, Skv), L.head_ladder(D, Sq, Skv, v_head=True)):
        qz = L.quantise(lad, dtype, fp8, "head", v_block=False)
        one = L.quantise(L.head_ladder(D, Sq, Skv, gains=False), dtype, fp8, "head", v_block=False)
        assert len(set(one.sq.ravel()) | set(one.sk.ravel()) | set(one.sv.ravel())) == 1, "the plain scale: one number"
        for x8, s, e in ((qz.q8, qz.sq, lad.e_q), (qz.k8, qz.sk, lad.e_k), (qz.v8, qz.sv, lad.e_v)):
            assert np.isin(x8 & 0x7F, (0, top)).all()
            assert np.array_equal(s, one.sq[0, 0] * np.exp2(e).astype(np.float32))
    lad = L.group_ladder(D, Sq, Skv)
    nz = (lad.q != 0).sum(-1)
    assert (nz[:, lad.sparse] == D // L.SPARSE_SHARE).all() and (nz[:, ~lad.sparse] == D).all()
    plain = L.quantise(L.group_ladder(D, Sq, Skv, gains=False), dtype, fp8, "head", v_block=False)
    qz = L.quantise(lad, dtype, fp8, "head", v_block=False)
    assert np.array_equal(qz.q8, plain.q8) and np.array_equal(qz.k8, plain.k8) and np.array_equal(qz.v8, plain.v8)
    assert np.array_equal(qz.sq[:, :, None] * qz.sk[:, L.kv_of(), None], plain.sq[:, :, None] * plain.sk[:, L.kv_of(), None]), "scale_q scale_k does not move with e"


# ---- the group ladder and the tile mutants -------------------------------------------------------------------------------------------------
def tile_moves(qz, sc, sq_per_sequence, mask):
    """{mutant: the moves [n] of the judged rows it touches}"""
    ref = sc.softmax()[0]
    judged = judged_rows(mask)
    res = {}
    for name, (rs, cs) in L.tile_mutants(qz, sq_per_sequence).items():
        touched = (rs != qz.row_scale()) & judged
        res[name] = L.moved(ref, sc.softmax(rs, cs)[0])[touched]
    return res


@pytest.mark.parametrize("case", L.FP8PV_CASES, ids=IDS)
def test_group_ladder_rows_are_flat_and_both_tile_mutants_move_every_touched_row(case):
    D, Sq, Skv, causal, dtype, fp8 = case
    qz = L.quantise(L.group_ladder(D, Sq, Skv), dtype, fp8, "head", v_block=False)
    mask = masks_of(case)["used"]
    sc = L.UsedScores(qz, mask)
    top, eff = sc.weights_summary()
    judged = judged_rows(mask)
    s = np.stack([sc._scaled(b, *(torch.from_numpy(np.array(x)) for x in (qz.row_scale(), qz.col_scale()))).numpy() for b in range(B)])
    std = np.array([[s[b, h][np.isfinite(s[b, h])].std() for h in range(HQ)] for b in range(B)])
    print(f"group ladder {L.case_id(case)}: largest weight {top[judged].max():.4f}, smallest effective key count {eff[judged].min():.0f}, "
          f"{100 * ((top < L.FLAT_W) & (eff >= L.FLAT_KEYS))[judged].mean():.2f} % of the rows within (1 / 24, 192); score std per head {std.min():.3f} .. {std.max():.3f}")
    assert (top[judged] < FLAT_W).all() and (eff[judged] >= FLAT_KEYS).all()
    assert (np.abs(std - 1) < 0.1).all(), "every legitimate row keeps a score standard deviation of 1"
    moves = tile_moves(qz, sc, [Sq, Sq], mask)
    first = moves["scale_q of the tile's first row"]
    assert first.size and moves["g computed with max_seqlen_q"].size == 0, "equal query counts: the second mutant is the identity"
    print(f"group ladder {L.case_id(case)}: scale_q of the tile's first row: {first.size} touched judged rows, moved by {first.min():.1f} .. {first.max():.1f} x the bound")
    assert first.min() >= TEETH
    res = scale_teeth(qz, sc, sc.softmax()[0], L.head_mutants(qz, packed=True), mask)
    print(f"group ladder {L.case_id(case)}: head mutants " + ", ".join(f"{k}: {v:.1f}" for k, v in res.items()))
    assert min(res.values()) >= TEETH, res
    if Sq == L.PACKED_SQ[0]:     # packed queries over the paged cache: sequences of 130 and 5 rows
        pm = L.used_mask(Sq, Skv, L.used_lengths(Skv), causal, L.PACKED_SQ)
        for name, mv in tile_moves(qz, L.UsedScores(qz, pm), L.PACKED_SQ, pm).items():
            print(f"group ladder {L.case_id(case)}, packed queries {L.PACKED_SQ}: {name}: {mv.size} touched judged rows, moved by {mv.min():.1f} .. {mv.max():.1f} x the bound")
            assert mv.size and mv.min() >= TEETH, name


# ---- the hole ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.FP8PV_CASES, ids=IDS)
def test_on_the_head_ladder_the_tile_mutant_stays_below_the_teeth(case):
    """why group_ladder exists: on the head ladder the tile's first head is the f = 0 one, and a std-0.25 head that reads its scale_q
    becomes a std-1 head -- a flat row stays flat.  Measured over the five cases: the least moved touched judged row (the statistic the
    teeth ask >= 4 of) moves by 1.80 .. 2.82 x the bound, the most moved one by 3.07 .. 7.18 x"""
    D, Sq, Skv, causal, dtype, fp8 = case
    qz = L.quantise(L.head_ladder_plain_v(D, Sq, Skv), dtype, fp8, "head", v_block=False)
    mask = masks_of(case)["used"]
    mv = tile_moves(qz, L.UsedScores(qz, mask), [Sq, Sq], mask)["scale_q of the tile's first row"]
    print(f"the hole, head ladder {L.case_id(case)}: scale_q of the tile's first row moves its {mv.size} touched judged rows by "
          f"{mv.min():.2f} .. {mv.max():.2f} x the bound (asked of a ladder: every such row >= {TEETH:.0f})")
    assert mv.size and mv.min() < TEETH, "the statistic asked >= TEETH of a ladder is the WORST (least moved) touched row"

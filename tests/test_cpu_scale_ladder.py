"""The scale ladder of tests/scale_ladder.py on the CPU ("Scale ladder"): the constructions are exact in every format, the rows
are flat, and -- on the very cases tests/test_gpu_scale_ladder.py runs -- every named way of reading a scale at the wrong index moves
the fp64 reference by >= TEETH = 4 x the bound the GPU test applies.  The teeth are CONDITIONS on the inputs.  The last test runs the
same mutants on N(0,1) inputs: there they move 4 .. 100 % of the rows by 1 .. 4 bounds at 1100 keys (head tables least, token and V
tables most) -- the size of the kernels' own error, shrinking with 1 / sqrt(keys) -- and none reaches the ladder's 4 x."""
import numpy as np
import pytest
import torch

import oracle
from tests import scale_ladder as L
from tests.scale_ladder import B, HKV, HQ, TEETH

JUDGED_KEYS = 64              # teeth are asked on the rows that attend at least one 64-key chunk (row 0 of a causal case attends ONE key:
                              # its output is that key's V whatever the scales are)
FLAT_KEYS_SEEN = L.EARLY_KEYS # flatness is asked on the rows that attend >= 1024 keys: the rows the FP8 sweep serves
V_SHARE = 0.90                # V chunk mutants: this share of the rows of every head


def judged_rows(mask, keys=JUDGED_KEYS):
    """bool [1 or HQ, Sq] -> [B, HQ, Sq]: rows that attend at least `keys` keys"""
    return np.broadcast_to(mask.sum(-1) >= keys, (HQ, mask.shape[1]))[None].repeat(B, 0)


def agree_with_oracle(sc, qz, causal, v="fp8"):
    """softmax64 (the teeth's reference) is oracle.attention_forward (the GPU test's) on the same quantised operands"""
    out, lse = sc.softmax(v=qz.v16 if v == "v16" else None)
    ref, ref_lse = L.oracle_reference(qz, causal, v, return_lse=True)
    assert np.abs(out - ref).max() < 2e-6 * max(1.0, np.abs(ref).max()) and np.abs(lse - ref_lse).max() < 1e-5
    return out


def scale_teeth(qz, sc, ref, mutants, mask, v=None, head_level=True):
    """{mutant: (teeth, share of the judged rows it makes flatter)}.  teeth: head-level mutants -- the best, over the (batch, head) groups
    whose every judged row gets a score scale >= LARGE x too large, of the group's WORST row; token-level -- the worst of all such rows"""
    judged = judged_rows(mask)
    res = {}
    for name, (rs, cs) in mutants.items():
        large = L.too_large(qz, rs, cs, mask) & judged
        mv = L.moved(ref, sc.softmax(rs, cs, v)[0])
        hid = float((L.flatter(qz, rs, cs) & judged).sum() / judged.sum())
        if head_level:
            groups = [(b, h) for b in range(B) for h in range(HQ) if large[b, h].any() and (large[b, h] == judged[b, h]).all()]
            assert groups, (name, "the mutant makes no group's scores >= 4 x too large: the ladder does not reach it")
            res[name] = (max(float(mv[b, h][judged[b, h]].min()) for b, h in groups), hid)
        else:
            assert large.any(), name
            res[name] = (float(mv[large].min()), hid)
    return res


def vhead_teeth(qz, sc, ref, mask, what):
    """the V head ladder: a head's bytes de-quantised with another head's scale_v must move >= V_SHARE of the judged rows of at least one
    (batch, head) group it touches by >= TEETH x the bound (O scales with the gain: a group whose V is 2^-3 cannot show an error of its own size)"""
    judged = judged_rows(mask)
    for name, (v, lg) in L.vhead_mutants(qz).items():
        mv = L.moved(ref, sc.softmax(v=v)[0])
        share = {(b, h): float((mv[b, h][judged[b, h]] >= TEETH).mean()) for b in range(B) for h in range(HQ) if lg[b, L.kv_of(h)] != 0}
        assert share, name
        print(f"V head ladder {what}: {name}: best touched group {100 * max(share.values()):.1f} % of its rows by >= {TEETH:.0f} x the bound; "
              f"per touched group " + ", ".join(f"{k}: {100 * x:.0f} %" for k, x in share.items()))
        assert max(share.values()) >= V_SHARE, (name, share)


def show(what, res):
    for name, (t, hid) in res.items():
        print(f"{what}: {name}: teeth {t:.2f} x the bound; {100 * hid:.0f} % of the judged rows only get flatter (not counted)")


# ---- exactness ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.TOKEN_CASES, ids=L.case_id)
def test_token_ladder_quantises_exactly_and_its_rows_are_flat(case):
    D, Sq, Skv, causal, dtype, fp8, side = case
    lad = L.token_ladder(D, Sq, Skv, side)
    for t in (torch.bfloat16, torch.float16):
        for f in ("e4m3", "e5m2"):
            qz = L.quantise(lad, t, f, "token")
            x8, s = (qz.k8, qz.sk) if side == "k" else (qz.q8, qz.sq)
            assert np.isin(x8 & 0x7F, (0, L.TOP_CODE[f])).all(), "bytes are 0 or +- the format's largest code"
            base = s[lad.e == 0]
            assert (base == base[0]).all() and np.array_equal(s, np.exp2(lad.e).astype(np.float32) * base[0]), "scale of token j = 2^(e_j) x one number"
            deq = oracle.fp8_to_f32(x8, L.FMT[f]).astype(np.float64) * s.astype(np.float64)[..., None]
            want = lad.k if side == "k" else lad.q      # (fp32(1 / fmax) x fmax is one rounding off 1: the scale, not the byte, carries it)
            assert np.abs(deq - want).max() <= 2.0 ** -23 * np.abs(want).max(), "token-wise quantisation returns the ladder"
    qz = L.quantise(lad, dtype, fp8, "token")
    mask = L.mask_of(Sq, Skv, causal)
    top, eff = L.Scores(qz, mask).weights_summary()
    rows = judged_rows(mask, FLAT_KEYS_SEEN)
    ok = (top < L.FLAT_W) & (eff >= L.FLAT_KEYS)
    print(f"token ladder {L.case_id(case)}: largest weight {top[rows].max():.4f}, smallest effective key count {eff[rows].min():.0f}, "
          f"{100 * ok[rows].mean():.2f} % of the rows with >= {FLAT_KEYS_SEEN} keys are flat")
    assert ok[rows].mean() >= L.FLAT_SHARE


@pytest.mark.parametrize("case", L.HEAD_CASES, ids=L.case_id)
def test_head_ladder_moves_the_scales_by_exact_powers_of_two_and_no_byte(case):
    """the quantiser echo and the exact equivariance, as the CPU quantiser has them"""
    D, Sq, Skv, causal, dtype, fp8 = case
    plain = L.quantise(L.head_ladder(D, Sq, Skv, gains=False), dtype, fp8, "head")
    lad = L.head_ladder(D, Sq, Skv)
    qz = L.quantise(lad, dtype, fp8, "head")
    assert np.array_equal(qz.q8, plain.q8) and np.array_equal(qz.k8, plain.k8) and np.array_equal(qz.v8, plain.v8)
    assert np.array_equal(qz.sq, plain.sq * np.exp2(lad.e_q).astype(np.float32)) and np.array_equal(qz.sk, plain.sk * np.exp2(lad.e_k).astype(np.float32))
    if qz.v_block:
        assert np.array_equal(qz.ve.astype(np.int64), plain.ve.astype(np.int64) + lad.g)
    else:
        assert np.array_equal(qz.sv, plain.sv * np.exp2(lad.e_v).astype(np.float32))
    e_only = L.quantise(L.head_ladder(D, Sq, Skv, f=False), dtype, fp8, "head")
    assert np.array_equal(e_only.sq[:, :, None] * e_only.sk[:, L.kv_of(), None], plain.sq[:, :, None] * plain.sk[:, L.kv_of(), None]), \
        "f = 0: scale_q scale_k is the plain inputs' product bit for bit"
    s = (torch.from_numpy(qz.qf[0, :, :64]) @ torch.from_numpy(qz.kf[0]).repeat_interleave(HQ // HKV, 0).transpose(-1, -2)).numpy()
    s = s * (qz.sq[0, :, None, None] * qz.sk[0, L.kv_of(), None, None]).astype(np.float64) / np.sqrt(D)
    want = np.exp2(L.F_HEAD)
    assert (np.abs(s.std((-1, -2)) / want - 1) < 0.05).all(), "scores keep a standard deviation of 1 (f = 0) or 0.25 (f = -2) whatever e"


# ---- teeth -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.HEAD_CASES, ids=L.case_id)
def test_head_ladder_teeth_on_the_fused_cases(case):
    D, Sq, Skv, causal, dtype, fp8 = case
    qz = L.quantise(L.head_ladder(D, Sq, Skv), dtype, fp8, "head")
    mask = L.mask_of(Sq, Skv, causal)
    sc = L.Scores(qz, mask)
    ref = agree_with_oracle(sc, qz, causal)
    res = scale_teeth(qz, sc, ref, L.head_mutants(qz), mask)
    show(f"head ladder {L.case_id(case)}", res)
    assert min(t for t, _ in res.values()) >= TEETH, res
    if not qz.v_block:
        return
    # the V chunk ladder: the rows that read the fp8 V (every precision attends the 16-bit V on the early blocks)
    late = np.broadcast_to(~L.early_rows(Sq, Skv, causal), (B, HQ, Sq))
    for name, v in L.vchunk_mutants(qz).items():
        mv = L.moved(ref, sc.softmax(v=v)[0])
        share = np.array([[(mv[b, h][late[b, h]] >= TEETH).mean() for h in range(HQ)] for b in range(B)])
        print(f"V chunk ladder {L.case_id(case)}: {name}: moves {100 * share.min():.1f} % .. {100 * share.max():.1f} % of a head's fp8-V rows by >= {TEETH:.0f} x the "
              f"bound (smallest move {mv[late].min():.2f} x, {int(late[0, 0].sum())} rows per head)")
        if "alone" not in name:     # (the last partial chunk alone: reported without a condition)
            assert share.min() >= V_SHARE, (name, share)


@pytest.mark.parametrize("case", L.TOKEN_CASES, ids=L.case_id)
def test_token_ladder_teeth_on_the_fused_cases(case):
    D, Sq, Skv, causal, dtype, fp8, side = case
    qz = L.quantise(L.token_ladder(D, Sq, Skv, side), dtype, fp8, "token")
    mask = L.mask_of(Sq, Skv, causal)
    sc = L.Scores(qz, mask)
    ref = agree_with_oracle(sc, qz, causal)
    res = scale_teeth(qz, sc, ref, L.token_mutants(qz, side), mask, head_level=False)
    show(f"token ladder {L.case_id(case)}", res)
    assert min(t for t, _ in res.values()) >= TEETH, res


@pytest.mark.parametrize("case", L.VHEAD_TOKEN, ids=L.case_id)
def test_v_head_ladder_teeth_on_the_token_wise_cases(case):
    D, Sq, Skv, causal, dtype, fp8, side = case
    qz = L.quantise(L.token_ladder(D, Sq, Skv, side, v_head=True), dtype, fp8, "token")
    mask = L.mask_of(Sq, Skv, causal)
    sc = L.Scores(qz, mask)
    vhead_teeth(qz, sc, agree_with_oracle(sc, qz, causal), mask, L.case_id(case))


@pytest.mark.parametrize("case", L.SEPARATE_HEAD, ids=L.case_id)
def test_v_head_ladder_teeth_on_the_separate_calls(case):
    """the separate C calls and the pre-quantised entry keep ONE fp8 V scale per head: the head ladder's q, k with the V head ladder (the
    q / k scale mutants have their teeth on the chunk-ladder V: test_head_ladder_teeth_on_the_fused_cases)"""
    D, Sq, Skv, causal, dtype, fp8 = case
    qz = L.quantise(L.head_ladder(D, Sq, Skv, v_head=True), dtype, fp8, "head", v_block=False)
    mask = L.mask_of(Sq, Skv, causal)
    sc = L.Scores(qz, mask)
    ref = agree_with_oracle(sc, qz, causal)
    vhead_teeth(qz, sc, ref, mask, "separate calls " + L.case_id(case))


@pytest.mark.parametrize("case", L.PACKED_CASES, ids=lambda c: f"D{c[0]}_S{c[1]}_{L.NAME[c[2]]}_{c[3]}")
def test_head_ladder_teeth_on_the_16bit_v_entries(case):
    """packed (a batch entry is a sequence; causal and not), window, block-sparse: 16-bit P on the caller's 16-bit V on every row"""
    D, S, dtype, fp8 = case
    qz = L.quantise(L.head_ladder(D, S, S), dtype, fp8, "head")
    for what, kw in (("full", {}), ("causal", {"causal": True}), ("window", {"window": L.WINDOW}), ("tiles", {"tiles": L.sparse_tiles(S)})):
        mask = L.mask_of(S, S, **kw)
        sc = L.Scores(qz, mask)
        ref = agree_with_oracle(sc, qz, what == "causal", "v16") if what in ("full", "causal") else sc.softmax(v=qz.v16)[0]
        res = scale_teeth(qz, sc, ref, L.head_mutants(qz, packed=what != "tiles"), mask, v=qz.v16)
        show(f"head ladder D {D} S {S} {what}", res)
        assert min(t for t, _ in res.values()) >= TEETH, (what, res)


# ---- the hole ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaling", ["head", "token"])
def test_the_same_mutants_on_normal_inputs_never_reach_the_ladders_margin(scaling):
    """An N(0,1) bf16 case of tests/test_gpu_attention.py's kind (no ladder; the scales of a tensor agree to ~10 %), D 128, 1100 keys.  Per
    mutant: the share of the rows it moves by >= 1 x the bound, the median row's move, and the statistic the teeth tests ask >= TEETH = 4
    of, over the rows the mutant changes at all (head tables: the worst row of the best (batch, head) group; token and V tables: the worst row).
    As computed, the premise "a wrong scale hides on N(0,1) data" holds only in part at this length (share of the rows moved by >= 1 x the
    bound / median row / the statistic): head tables 4 .. 44 % / 0.1 .. 0.7 x / 0.30 .. 0.71 -- no group is sure to show; rolled K token
    tables 100 % / 3.8 x / 1.18 .. 1.50; Q token tables 63 % / 1.4 x / 0.03; V chunk tables 50 % / 0.4 .. 0.7 x / 0.88 .. 1.38; the head's
    V scale for every chunk 100 % / 2.8 x / 1.67; a wrong per-head scale_v 17 .. 36 % / 0.1 .. 0.8 x / 0.24 .. 0.30.  So the rows that move
    move by 1 .. 4 bounds, against a kernel error of up to ~0.7 bounds of either sign: such a mistake may or may not fail a test, and the
    move shrinks with 1 / sqrt(keys).  What is asserted is the difference to the ladder: no mutant reaches 4 x here on the rows it
    touches, every mutant does there (5 .. 37 x, at 1100, 2304 and 16448 keys)."""
    D, S = 128, 1100
    qz = L.quantise(L.normal_case(D, S, S), torch.bfloat16, "e4m3", scaling)
    mask = L.mask_of(S, S)
    sc = L.Scores(qz, mask)
    ref = sc.softmax()[0]
    muts = L.head_mutants(qz, packed=True) if scaling == "head" else {**L.token_mutants(qz, "k"), **L.token_mutants(qz, "q")}
    muts = {name: sc.softmax(rs, cs)[0] for name, (rs, cs) in muts.items()}
    muts.update({name: sc.softmax(v=v)[0] for name, v in L.vchunk_mutants(qz).items()} if qz.v_block else
                {name: sc.softmax(v=v)[0] for name, (v, _) in L.vhead_mutants(qz).items()})
    worst = 0.0
    for name, out in muts.items():
        mv = L.moved(ref, out)
        touched = mv > 0                      # rows the mutant changes at all (a rolled table leaves rows whose two scales are equal alone)
        assert touched.any(), name
        if scaling == "head" and "chunk" not in name:
            stat = max(float(mv[b, h][touched[b, h]].min()) for b in range(B) for h in range(HQ) if touched[b, h].any())
        else:
            stat = float(mv[touched].min())
        worst = max(worst, stat)
        print(f"no ladder, {scaling}-wise N(0,1) D {D} S {S}: {name}: {100 * float((mv >= 1.0).mean()):.2f} % of the rows move by >= 1 x the bound, "
              f"median row {float(np.median(mv)):.2f} x; the statistic asked >= {TEETH:.0f} of the ladder: {stat:.3f}")
    assert worst < TEETH, worst

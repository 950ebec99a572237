"""The scale ladder of the MLA entries on the CPU: on the very case tables tests/test_gpu_mla_scale_ladder.py runs,
every named way of reading a scale at the wrong index moves the fp64 reference -- on EVERY row where it makes a score scale or an output
scale >= LARGE = 4 times too large -- by >= TEETH = 4 x the bound the GPU test applies to an element, or by >= 4 x LSE_TOL in the row's LSE.
(A row with ONE distinct key can show a score mutant in its LSE alone, by (ratio - 1) |s|: the few whose one score is too near 0 for that are
counted, printed and held below mla_scale_ladder.LONE_SHARE of the judged rows.)  No (mutant, case) pair is skipped: a mutant without such a
row fails, and the pairs that are not in the table are named in mla_scale_ladder.NOT_LISTED.  The product's eager definitions -- CPU tensors
-- pass the GPU file's oracle grading, echo (the eager appends write the plain inputs' bytes; scale_q, scale_k and scale_v are exactly 2^e
times the plain ones) and exact-equivariance checks on the same inputs."""
import numpy as np
import pytest
import torch

from tests import mla_cases as C
from tests import mla_index_cases as X
from tests import mla_prefill_cases as PF
from tests import mla_scale_ladder as L
from tests import mla_sparse_cases as S

DECODE_IDS = [L.decode_id(c) for c in L.DECODE_CASES]


def report(what, res):
    for name, rows in res.items():
        rows, lone = rows if isinstance(rows, tuple) else (rows, 0)
        print(f"{what}: {name}: {rows} rows with a scale >= {L.LARGE:.0f} x too large, shown at >= {L.TEETH:.0f} bounds but for {lone} one-key rows")


def test_the_ladders_are_what_the_design_says():
    assert (np.diff(np.sort(L.E_SLOT)) >= 2).all() and L.E_SLOT.max() == 0
    for Sq, (even, odd) in L.F_ROWS.items():
        f = L.f_rows(4, Sq).reshape(-1)                                   # packed rows r = h Sq + i of four heads: every neighbour >= x4 apart
        assert (np.abs(np.diff(f)) >= 2).all() and (np.abs(np.array(even) - np.array(odd)) >= 2).all(), Sq
    f = L.f_tokens(6, 6)
    assert (np.abs(np.diff(f, axis=0)) >= 2).all() and (np.abs(np.diff(f, axis=1)) >= 2).all()
    assert (np.abs(np.diff(L.EK)) >= 2).all() and (np.abs(np.diff(L.EV, axis=0)) >= 2).all() and L.EV.max() == 0 and set(L.GH) == {0, 2}
    lat = L.decode_inputs(16, 1, torch.bfloat16, False, False).lat.double()
    assert float((lat ** 2).mean().sqrt()) <= 1.0                         # the normalised latent: rms <= 1


@pytest.mark.parametrize("lens", C.LENS)
@pytest.mark.parametrize("case", L.DECODE_CASES, ids=DECODE_IDS)
def test_decode_mutants_show_on_the_dense_cases(case, lens):
    Hq, Sq, _, dtype = case
    report(f"dense {L.decode_id(case)} {lens}", L.decode_teeth(L.decode_inputs(Hq, Sq, dtype), lens))


@pytest.mark.parametrize("topk", L.SPARSE_TOPKS)
@pytest.mark.parametrize("lens", C.LENS)
@pytest.mark.parametrize("case", L.DECODE_CASES, ids=DECODE_IDS)
def test_decode_mutants_show_on_the_sparse_cases(case, lens, topk):
    Hq, Sq, _, dtype = case
    idx = S.draw_indices(Sq, topk, seed=1000 * topk + Sq)
    report(f"sparse {L.decode_id(case)} {lens} topk {topk}", L.decode_teeth(L.decode_inputs(Hq, Sq, dtype), lens, idx))


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Hq", L.VARLEN_HEADS)
def test_packed_sparse_mutants_show(Hq, causal):
    report(f"packed sparse Hq {Hq} causal {causal}", L.varlen_teeth(L.varlen_inputs(Hq, torch.bfloat16), causal))


@pytest.mark.parametrize("case", L.INDEX_CASES, ids=[f"Hi{c[0]}_Sq{c[1]}_{c[3]}" for c in L.INDEX_CASES])
def test_index_mutants_show_and_the_fp32_sums_are_exact(case):
    Hi, Sq, page, fmt, dtype = case
    p = L.index_inputs(Hi, Sq, dtype)
    for lens in X.LENS:
        icache = L.make_icache(p, page, lens, fmt, "cpu")
        for causal in (True, False):
            ref, mag = L.index_reference(p, icache, lens, causal)
            assert L.fp32_exact(ref), (lens, causal)                      # the plain-weights ladder: the GPU test compares bit for bit
            report(f"index Hi {Hi} {lens} causal {causal}", L.index_teeth(ref, mag, L.index_mutants(p, icache, lens, causal)))


@pytest.mark.parametrize("case", L.INDEX_VARLEN_CASES, ids=[f"{c[0]}_Hi{c[1]}_{c[3]}" for c in L.INDEX_VARLEN_CASES])
def test_packed_index_mutants_show_and_the_fp32_sums_are_exact(case):
    shape, Hi, page, fmt, dtype = case
    p = L.index_varlen_inputs(shape, Hi, dtype)
    icache = L.make_icache(p, page, p.lens, fmt, "cpu")
    for causal in (True, False):
        ref, mag = L.index_varlen_reference(p, icache, causal)
        assert L.fp32_exact(ref), causal
        report(f"packed index {shape} Hi {Hi} causal {causal}", L.index_teeth(ref, mag, L.index_varlen_mutants(p, icache, causal)))


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("fmt,dtype", L.PREFILL_CASES)
def test_prefill_mutants_show(fmt, dtype, causal):
    p = L.prefill_inputs(dtype)
    sk, sv = L.prefill_scales(p, fmt)
    base = L.prefill_scales(L.prefill_inputs(dtype, False), fmt)
    keys = torch.tensor([lk > 0 for _, lk in PF.LENS])[:, None]
    assert torch.equal(sk, torch.where(keys, base[0] * L.t2(p.e_k), base[0])) and torch.equal(sv, torch.where(keys, base[1] * L.t2(p.e_v), base[1]))
    report(f"prefill {fmt} causal {causal}", L.prefill_teeth(p, fmt, causal))


# ---- the eager definitions on the same inputs: oracle grading, echo, exact equivariance -------------------------------------------------------
@pytest.mark.parametrize("case", L.DECODE_CASES, ids=DECODE_IDS)
def test_eager_dense_definition_passes_the_gpu_checks(case):
    Hq, Sq, fmt, dtype = case
    print("worst |err| / bound", L.check_decode("dense", Hq, Sq, fmt, dtype, "cpu", pages=(64,), splits=(1, 3)))


@pytest.mark.parametrize("case", L.DECODE_CASES, ids=DECODE_IDS)
def test_eager_sparse_definition_passes_the_gpu_checks(case):
    Hq, Sq, fmt, dtype = case
    print("worst |err| / bound", max(L.check_decode("row", Hq, Sq, fmt, dtype, "cpu", pages=(16,), splits=(1, 2), topk=topk) for topk in L.SPARSE_TOPKS))


def test_eager_packed_sparse_definition_passes_the_gpu_checks():
    print("worst |err| / bound", max(L.check_varlen(Hq, "e4m3", torch.bfloat16, 16, "cpu") for Hq in (16, 72)))


def test_eager_index_definitions_pass_the_gpu_checks():
    print("worst |err| / rounding bound", L.check_index(*L.INDEX_CASES[1], "cpu"), L.check_index_varlen(*L.INDEX_VARLEN_CASES[1], "cpu"))


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("fmt,dtype", L.PREFILL_CASES)
def test_eager_prefill_definition_passes_the_gpu_checks(fmt, dtype, causal):
    print("worst |err| / bound", L.check_prefill(fmt, dtype, causal, "cpu"))

"""-m gpu: the exact-answer membership probes of tests/probes.py through the attention entries on the MI355X ("Membership
probes"): WHICH keys every row attended, at lengths where N(0,1) data cannot tell.

count probe    one score per row, indicator V: O[r, c] = n_c(r) / n(r) from integer counts; |got - ref| <= 2^-8 ref (bf16) / 2^-10 ref
               (fp16), exactly 0 where ref is 0; LSE s_r + ln n(r) to the tolerances of include/qattn.h.
decoy probe    q_r is the code of a FORBIDDEN key right outside an edge of the row's mask; the rows are flat; the project's bound per path.
pointer probe  q_r is twice the code of an ALLOWED key at a hard position; the rows are peaked: graded where the kernel promises them
               (auto / accurate / 16-bit P), the reported path asserted V16 or two-term.
Every value is exact in every format (tests/test_cpu_probes.py), so one fp64 reference per (probe, shape) serves all dtypes, formats,
scalings and precisions; the same file shows that every case has teeth >= 4x against every named wrong mask.  Each test prints its worst
|err| / bound."""
import functools

import numpy as np
import pytest
import torch

import oracle
import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import probes as P
from tests.gpu_utils import (FMT, PATH_ONE_TERM, PATH_TWO_TERM, PATH_V16, TDT, PathRef, bits16, check_path_structure, early_rows, fmt16,
                             fused_call, grade, out_to_f32, unpack_frag)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def T(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def dense(probe, D, Sq, Skv, causal, B=1, Hq=2, Hkv=2, n_peaked=0):
    """(case, q, k, v [B, H, S, D] float64, ref [B, Hq, Sq, D], ref_lse [B, Hq, Sq], pointer rows bool [B, Hq, Sq]) -- computed once, shared"""
    case = P.dense_case(probe, D, Sq, Skv, causal, B=B, Hq=Hq, Hkv=Hkv, n_peaked=n_peaked)
    ref, lse = case.reference()
    peaked = case.pointer_rows().reshape(Hq, B, Sq).transpose(1, 0, 2) if probe in ("pointer", "scatter") else np.zeros((B, Hq, Sq), bool)
    return (case,) + case.dense() + (ref.reshape(B, Sq, Hq, D).transpose(0, 2, 1, 3), lse.reshape(Hq, B, Sq).transpose(1, 0, 2), peaked)


def deq_q(q, dtype, fp8, mode):
    """q [B, H, S, D] as the quantiser leaves it (fp64): only the count probe's g = 1.5 rows under head-wise scales move (tests/probes.py)"""
    x8, s = oracle.quantize_fp8(bits16(T(q, dtype).cpu()), fmt16(dtype), mode, FMT[fp8])
    return oracle.fp8_to_f32(x8, FMT[fp8]).astype(np.float64) * s.astype(np.float64).reshape(s.shape + (1,) * (4 - s.ndim))


def count_ratio(got, ref, dtype, what, rows=None):
    """worst |got - ref| / (REL ref) over the (flat) rows; exact zeros where ref is 0"""
    got, ref = (np.asarray(t, np.float64) for t in (got, ref))
    if rows is not None:
        got, ref = got[rows], ref[rows]
    assert (got[ref == 0] == 0).all(), (what, "an element no allowed key feeds must be exactly 0", np.argwhere((ref == 0) & (got != 0))[:8])
    nz = ref > 0
    return float((np.abs(got - ref)[nz] / P.count_bound(ref, dtype)[nz]).max()) if nz.any() else 0.0


def lse_ratio(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    dead = np.isneginf(ref)
    assert np.array_equal(np.isneginf(got), dead) and np.isfinite(got[~dead]).all(), (what, "rows without a key have LSE -inf, the others a finite one")
    return float((np.abs(got[~dead] - ref[~dead]) / np.broadcast_to(tol, ref.shape)[~dead]).max()) if (~dead).any() else 0.0


def fused_lse_tol(path, D, scaling):
    """include/qattn.h: 16-bit-V rows 4e-3; the D = 128 head-wise FP8 sweep 2e-2; the others 2e-3"""
    return np.where(path == PATH_V16, P.LSE_TOL_V16, P.LSE_TOL_SWEEP128 if (D == 128 and scaling == "head-wise") else P.LSE_TOL)


def precisions(D, *names):
    return [p for p in names if p != "accurate" or D == 128]


FUSED = [(D, s, t, "e4m3") for D in (64, 128, 256) for s in ("head-wise", "token-wise") for t in DTYPES] + \
        [(D, "head-wise", torch.bfloat16, "e5m2") for D in (64, 128, 256)]


# ---- the dense fused entry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,scaling,dtype,fp8", FUSED)
def test_fused_count_probe(D, scaling, dtype, fp8):
    worst = worst_lse = 0.0
    mode = "head" if scaling == "head-wise" else "token"
    for Sq, Skv, causal in P.DENSE_SHAPES:
        case, q, k, v, ref, _, _ = dense("count", D, Sq, Skv, causal)
        tq, tk, tv = T(q, dtype), T(k, dtype), T(v, dtype)
        for prec in precisions(D, "fast", "auto", "accurate"):
            what = f"count D {D} {scaling} {NAME[dtype]} {fp8} ({Sq}, {Skv}) causal {causal} {prec}"
            out, path = fused_call(tq, tk, tv, causal=causal, precision=prec, fp8=fp8, scaling=scaling)
            check_path_structure(path, Sq, Skv, causal, prec, D == 128 and scaling == "head-wise")
            worst = max(worst, count_ratio(out, ref, dtype, what))
        # the LSE (its request moves the templated kernel's sweep to exact exponentials: graded as well)
        out, path, lse = fused_call(tq, tk, tv, causal=causal, precision="auto", fp8=fp8, scaling=scaling, return_lse=True)
        worst = max(worst, count_ratio(out, ref, dtype, what + " +lse"))
        tot = np.broadcast_to(P.count_expected(case.seqs[0].mask, D)[1], (2, Sq))[None]
        ref_lse = P.count_lse(deq_q(q, dtype, fp8, mode)[0], k[0, :, 0], tot[0])[None]
        worst_lse = max(worst_lse, lse_ratio(lse, ref_lse, fused_lse_tol(path, D, scaling), what))
    print(f"fused count D {D} {scaling} {NAME[dtype]} {fp8}: worst |err| / (rel ref) {worst:.3f}, worst |lse err| / tol {worst_lse:.3f}")
    assert worst <= 1.0 and worst_lse < 1.0, (worst, worst_lse)


@pytest.mark.parametrize("D,scaling,dtype,fp8", FUSED)
def test_fused_decoy_probe(D, scaling, dtype, fp8):
    worst, share = 0.0, 1.0
    for Sq, Skv, causal in [s for s in P.DENSE_SHAPES if s[2]]:
        case, q, k, v, ref, _, _ = dense("decoy", D, Sq, Skv, causal)
        tq, tk, tv = T(q, dtype), T(k, dtype), T(v, dtype)
        for prec in ("fast", "auto"):
            out, path = fused_call(tq, tk, tv, causal=causal, precision=prec, fp8=fp8, scaling=scaling)
            check_path_structure(path, Sq, Skv, causal, prec, D == 128 and scaling == "head-wise")
            # fast: every row beyond the early blocks is one-term (asserted above), so the FP8 sweep is what is graded.  auto: the share of
            # those rows it keeps there is printed -- it moves some to its precise pass (never wrong, graded against that path's oracle)
            if prec == "auto":
                share = min(share, float((path[..., ~early_rows(Sq, Skv, causal)] == PATH_ONE_TERM).mean()))
            worst = max(worst, grade(out, PathRef(ref, ref), path)[2])
    print(f"fused decoy D {D} {scaling} {NAME[dtype]} {fp8}: worst |err| / bound {worst:.3f}; auto keeps >= {share:.3f} of the later rows one-term")
    assert worst < 1.0, worst


@pytest.mark.parametrize("D,scaling,dtype,fp8", FUSED)
def test_fused_pointer_probe(D, scaling, dtype, fp8):
    worst = 0.0
    for Sq, Skv, causal in P.DENSE_SHAPES:
        case, q, k, v, ref, _, peaked = dense("pointer", D, Sq, Skv, causal)
        tq, tk, tv = T(q, dtype), T(k, dtype), T(v, dtype)
        for prec in precisions(D, "auto", "accurate"):
            out, path = fused_call(tq, tk, tv, causal=causal, precision=prec, fp8=fp8, scaling=scaling)
            check_path_structure(path, Sq, Skv, causal, prec, D == 128 and scaling == "head-wise")
            assert np.isin(path[peaked], (PATH_V16, PATH_TWO_TERM)).all(), ("peaked rows must leave the one-term sweep", prec, (Sq, Skv, causal),
                                                                             np.argwhere(peaked & (path == PATH_ONE_TERM))[:8])
            worst = max(worst, grade(out, PathRef(ref, ref), path)[2])
    print(f"fused pointer D {D} {scaling} {NAME[dtype]} {fp8}: worst |err| / bound {worst:.3f}")
    assert worst < 1.0, worst


@pytest.mark.parametrize("n_peaked", [1, 33, 130])
@pytest.mark.parametrize("D,scaling", [(128, "head-wise"), (64, "head-wise"), (128, "token-wise")])
def test_fused_scattered_pointer_rows(D, scaling, n_peaked):
    """n_peaked pointer rows among uniform rows (q = 0) of the second 256-row block: the gather-and-recompute rescue must put every row
    back into its own slot -- the flat rows still meet the count bound, the pointer rows the project's"""
    Sq = Skv = 1100
    dtype = torch.bfloat16
    case, q, k, v, ref, _, peaked = dense("scatter", D, Sq, Skv, False, n_peaked=n_peaked)
    out, path = fused_call(T(q, dtype), T(k, dtype), T(v, dtype), causal=False, precision="auto", scaling=scaling)
    assert np.isin(path[peaked], (PATH_V16, PATH_TWO_TERM)).all(), np.argwhere(peaked & (path == PATH_ONE_TERM))[:8]
    flat = count_ratio(out, ref, dtype, "scatter", rows=~peaked)
    worst = grade(out[peaked], PathRef(ref[peaked], ref[peaked]), path[peaked])[2]
    print(f"fused scatter D {D} {scaling} n_peaked {n_peaked}: flat rows {flat:.3f} of the count bound, pointer rows {worst:.3f} of the bound")
    assert flat <= 1.0 and worst < 1.0, (flat, worst)


@pytest.mark.parametrize("B,Hq,Hkv", [(2, 4, 2), (3, 5, 5)])
def test_fused_gqa_and_odd_head_count(B, Hq, Hkv):
    D, Sq, Skv, causal, dtype = 128, 1100, 1100, True, torch.bfloat16
    res = {}
    for probe in ("count", "decoy", "pointer"):
        case, q, k, v, ref, _, peaked = dense(probe, D, Sq, Skv, causal, B, Hq, Hkv)
        out, path = fused_call(T(q, dtype), T(k, dtype), T(v, dtype), causal=causal, precision="auto")
        check_path_structure(path, Sq, Skv, causal, "auto", True)
        assert np.isin(path[peaked], (PATH_V16, PATH_TWO_TERM)).all()
        res[probe] = count_ratio(out, ref, dtype, probe) if probe == "count" else grade(out, PathRef(ref, ref), path)[2]
    print(f"fused B {B} Hq {Hq} Hkv {Hkv}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert res["count"] <= 1.0 and res["decoy"] < 1.0 and res["pointer"] < 1.0, res


def test_fused_long_keys_on_the_per_head_scaled_v():
    Sq, Skv = P.LONG_KEYS
    D, dtype = 128, torch.float16
    case, q, k, v, ref, _, _ = dense("count", D, Sq, Skv, False, 1, 2, 1)
    res = {}
    for prec in ("fast", "auto", "accurate"):
        out, path = fused_call(T(q, dtype), T(k, dtype), T(v, dtype), causal=False, precision=prec)
        check_path_structure(path, Sq, Skv, False, prec, True)
        res[prec] = count_ratio(out, ref, dtype, prec)
    print(f"fused count long keys ({Sq}, {Skv}) fp16: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert max(res.values()) <= 1.0, res


# ---- the op on pre-quantised q / k, and the 16-bit entry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [True, False])
def test_prequantised_op(D, causal):
    Sq = Skv = 1100
    dtype = torch.bfloat16
    res = {}
    for probe in ("count", "decoy", "pointer"):
        if probe == "decoy" and not causal:
            continue
        case, q, k, v, ref, ref_lse, _ = dense(probe, D, Sq, Skv, causal)
        q8, sq = qa.dynamically_quantize_fp8(T(q, dtype), reduction_dim=[2, 3])
        k8, sk = qa.dynamically_quantize_fp8(T(k, dtype), reduction_dim=[2, 3])
        for pv16 in (False, True):
            if probe == "pointer" and not pv16:
                continue   # (fp8 P on peaked rows: promised by precision = accurate only)
            out, lse = _native.fp8_attention_forward_rowmajor(q8, k8, T(v, dtype), sq, sk, is_causal=causal, pv_16bit=pv16, return_lse=True)
            out = out_to_f32(out)
            what = f"{probe} pv16 {pv16}"
            if probe == "count":
                res[what] = count_ratio(out, ref, dtype, what)
                tot = np.broadcast_to(P.count_expected(case.seqs[0].mask, D)[1], (2, Sq))
                ref_lse = P.count_lse(deq_q(q, dtype, "e4m3", "head")[0], k[0, :, 0], tot)[None]
            else:
                res[what] = grade(out, PathRef(ref, ref), np.full(ref.shape[:3], PATH_V16 if pv16 else PATH_ONE_TERM))[2]
            res[what + " lse"] = lse_ratio(lse.cpu().numpy(), ref_lse, P.LSE_TOL_V16 if pv16 else P.LSE_TOL, what)
        if probe == "pointer":
            out = _native.fp8_attention_forward_rowmajor(q8, k8, T(v, dtype), sq, sk, is_causal=causal, precision="accurate")
            res["pointer accurate"] = grade(out_to_f32(out), ref)[2]
    print(f"pre-quantised op D {D} causal {causal}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert all(v <= 1.0 for v in res.values()), res


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_16bit_entry(D, dtype):
    res = {}
    for causal in (True, False):
        for probe in ("count", "decoy") if causal else ("count",):
            case, q, k, v, ref, _, _ = dense(probe, D, 1100, 1100, causal)
            out = out_to_f32(qa.attn_func(T(q, dtype), T(k, dtype), T(v, dtype), is_causal=causal))
            what = f"{probe} causal {causal}"
            res[what] = count_ratio(out, ref, dtype, what) if probe == "count" else grade(out, ref)[2]
    print(f"16-bit entry D {D} {NAME[dtype]}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert all(v <= 1.0 for v in res.values()), res


# ---- the packed, window and block-sparse entries (every row 16-bit P on the 16-bit V) -----------------------------------------------------
def _cu(lengths):
    return torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32, device=DEV)


def _packed_refs(case, dtype):
    """(ref [total_q, Hq, D], ref_lse [Hq, total_q]); the count probe's LSE on the q the per-(sequence, head) quantiser leaves"""
    ref, lse = case.reference()
    if case.probe == "count":
        ls = []
        for s in case.seqs:
            Hq, _, n, _, D = s.dims
            tot = np.broadcast_to(P.count_expected(s.mask, D)[1], (Hq, n))
            ls.append(P.count_lse(deq_q(s.q[None], dtype, "e4m3", "head")[0], s.k[:, 0], tot) if n and s.m else np.full((Hq, n), -np.inf))
        lse = np.concatenate(ls, 1)
    return ref, lse


def _grade_packed(case, out, lse, dtype, what):
    ref, ref_lse = _packed_refs(case, dtype)
    out = out_to_f32(out)
    dead = np.isneginf(ref_lse).T
    assert (out[dead] == 0).all(), (what, "rows without a key must be exactly 0")
    if case.probe == "count":
        r = count_ratio(out, ref, dtype, what)
    else:
        r = float((np.abs(out - ref) / P.project_bound(ref, True)).max())
    return r, lse_ratio(lse.cpu().numpy(), ref_lse, P.LSE_TOL_V16, what)


def _run_packed(case, dtype, causal=None, window=None):
    q, k, v = T(case.q, dtype), T(case.k, dtype), T(case.v, dtype)
    cu_q, cu_k = _cu(case.lq), _cu(case.alloc)
    used = None if case.used == case.alloc else torch.tensor(case.used, dtype=torch.int32, device=DEV)
    if window is None:
        return qa.fp8_attn_varlen_func(q, k, v, cu_q, cu_k, max(case.lq), max(case.alloc), causal=causal, seqused_k=used, return_lse=True)
    return qa.fp8_attn_varlen_window_func(q, k, v, cu_q, cu_k, max(case.lq), max(case.alloc), window, seqused_k=used, return_lse=True)


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("which", ["lens", "cross", "seqused"])
def test_packed_entry(D, which):
    lq, alloc, used = {"lens": (P.PACKED_LENS, P.PACKED_LENS, None), "cross": P.PACKED_CROSS + (None,), "seqused": P.PACKED_SEQUSED}[which]
    res = {}
    for kind in ("causal", "full"):
        for probe in ("count", "decoy", "pointer"):
            for dtype in DTYPES if probe == "count" else DTYPES[:1]:
                Hq, Hkv = P.heads("packed", probe)
                case = P.make_case(probe, D, lq, alloc, used, kind=kind, Hq=Hq, Hkv=Hkv)
                out, lse = _run_packed(case, dtype, causal=kind == "causal")
                what = f"{probe} {kind} {NAME[dtype]}"
                res[what], res[what + " lse"] = _grade_packed(case, out, lse, dtype, what)
    print(f"packed {which} D {D}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert all(v <= 1.0 for v in res.values()), res


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("window", P.WINDOWS)
def test_window_entry(D, window):
    res = {}
    for lq, lk in ((P.WINDOW_LENS, P.WINDOW_LENS), P.WINDOW_CROSS):
        for probe in ("count", "decoy", "pointer"):
            dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[P.WINDOW_COUNT_DTYPE[D]] if probe == "count" else torch.bfloat16
            Hq, Hkv = P.heads("window", probe)
            case = P.make_case(probe, D, lq, lk, kind="window", arg=window, Hq=Hq, Hkv=Hkv)
            out, lse = _run_packed(case, dtype, window=window)
            what = f"{probe} {'cross' if lq is not lk else 'self'}"
            res[what], res[what + " lse"] = _grade_packed(case, out, lse, dtype, what)
    print(f"window {window} D {D}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert all(v <= 1.0 for v in res.values()), res


@pytest.mark.parametrize("D,name,Sq,Skv,H", P.SPARSE_CASES)
def test_block_sparse_entry(D, name, Sq, Skv, H):
    """H = 1: the mask is an expanded (broadcast) view over batch and heads; H = 4: one table per head"""
    tiles = P.sparse_tiles(name, -(-Sq // 128), -(-Skv // 128), H)
    mask = torch.from_numpy(tiles).to(DEV)[None].expand(1, 4, -1, -1) if H == 1 else torch.from_numpy(tiles).to(DEV)[None]
    res = {}
    for probe in ("count", "decoy", "pointer"):
        for dtype in DTYPES if probe == "count" else DTYPES[:1]:
            Hq, Hkv = P.heads("sparse", probe)
            case = P.make_case(probe, D, [Sq], [Skv], tiles=tiles, Hq=Hq, Hkv=Hkv)
            q, k, v = (T(t, dtype) for t in case.dense())
            out, lse = qa.fp8_block_sparse_attn_func(q, k, v, mask, return_lse=True)
            what = f"{probe} {NAME[dtype]}"
            res[what], res[what + " lse"] = _grade_packed(case, out[0].transpose(0, 1), lse[0], dtype, what)
    print(f"block-sparse {name} ({Sq}, {Skv}) D {D}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert all(v <= 1.0 for v in res.values()), res


# ---- the decoy probe under key smoothing: the reference on the k8, scale_k and k_mean the call returned -----------------------------------
def _deq8(b, scale):
    """fp8 (e4m3) bytes [H, m, D] x scale [H] -> float64"""
    return torch.from_numpy(np.ascontiguousarray(b)).view(TDT["e4m3"]).double().numpy() * np.asarray(scale, np.float64)[:, None, None]


def _grade_smoothed(case, out, lse, keys, means, what):
    """out [total_q, Hq, D], lse [Hq, total_q] against the fp64 masked softmax of q and the de-quantised smoothed keys (`keys`: per sequence
    [Hkv, m, D]); the LSE is that of the true scores: + sm q.k_mean.  Every row is a 16-bit-V row here."""
    refs, lses = [], []
    for s, kd, mean in zip(case.seqs, keys, means):
        ku = np.zeros_like(s.k)
        ku[:, :s.m] = kd
        o, l = s.softmax(s.mask, k=ku)
        mm = np.repeat(np.asarray(mean, np.float64), s.dims[0] // s.dims[1], axis=0)
        refs.append(o.transpose(1, 0, 2))
        lses.append(l + s.sm * (s.q * mm[:, None, :]).sum(-1))
    ref, ref_lse = np.concatenate(refs, 0), np.concatenate(lses, 1)
    out = out_to_f32(out)
    assert (out[np.isneginf(ref_lse).T] == 0).all(), (what, "rows without a key must be exactly 0")
    return float((np.abs(out - ref) / P.project_bound(ref, True)).max()), lse_ratio(lse.cpu().numpy(), ref_lse, P.LSE_TOL_V16, what)


def _packed_keys(case, k8, sk, Hkv, D):
    k8n, starts = k8.cpu().numpy(), np.cumsum([0] + case.alloc)
    keys = []
    for i, m in enumerate(case.used):
        off = Hkv * D * (int(starts[i]) + 64 * i)
        keys.append(_deq8(unpack_frag(k8n[off:off + Hkv * P.pad64(m) * D], _native.LAYOUT_KFRAG, 1, Hkv, m, D)[0, :, :m], sk[i].cpu().numpy())
                    if m else np.zeros((Hkv, 0, D)))
    return keys


@pytest.mark.parametrize("D", [64, 128, 256])
def test_decoy_probe_on_smoothed_keys(D):
    dtype, res = torch.bfloat16, {}
    lq, lk = P.SMOOTH_LENS
    Hq, Hkv = P.heads("packed", "decoy")
    for name, kind, arg in (("packed", "causal", None), ("window", "window", P.SMOOTH_WINDOW)):
        case = P.make_case("decoy", D, lq, lk, kind=kind, arg=arg, Hq=Hq, Hkv=Hkv)
        q, k, v = T(case.q, dtype), T(case.k, dtype), T(case.v, dtype)
        kw = dict(smooth_k=True, return_lse=True, return_quant=True)
        if name == "packed":
            got = _native.fp8_quant_attention_varlen(q, k, v, _cu(lq), _cu(lk), None, is_causal=True, **kw)
        else:
            got = _native.fp8_quant_attention_varlen_window(q, k, v, _cu(lq), _cu(lk), None, window_left=arg[0], window_right=arg[1], **kw)
        out, lse, _, k8, _, sk, mean = got
        res[name], res[name + " lse"] = _grade_smoothed(case, out, lse, _packed_keys(case, k8, sk, Hkv, D), mean.cpu().numpy(), name)
    # block-sparse
    Hq, Hkv = P.heads("sparse", "decoy")
    tiles = P.sparse_tiles("band+global", 11, 11, 1)
    case = P.make_case("decoy", D, [1300], [1300], tiles=tiles, Hq=Hq, Hkv=Hkv)
    q, k, v = (T(t, dtype) for t in case.dense())
    mask = torch.from_numpy(tiles).to(DEV)[None].expand(1, Hq, -1, -1)
    out, lse, _, k8, _, sk, mean = _native.fp8_block_sparse_attention(q, k, v, mask, smooth_k=True, return_lse=True, return_quant=True)
    keys = [_deq8(unpack_frag(k8.cpu().numpy(), _native.LAYOUT_KFRAG, 1, Hkv, 1300, D)[0, :, :1300], sk[0].cpu().numpy())]
    res["block-sparse"], res["block-sparse lse"] = _grade_smoothed(case, out[0].transpose(0, 1), lse[0], keys, mean.cpu().numpy(), "block-sparse")
    # the dense fused entry: per row against the path it reports (fast and auto: the rows stay one-term beyond the early blocks)
    Sq = Skv = 1100
    case, q, k, v, _, _, _ = dense("decoy", D, Sq, Skv, True)
    for prec in ("fast", "auto"):
        out, path, quant = _native.fp8_quant_attention_forward(T(q, dtype), T(k, dtype), T(v, dtype), is_causal=True, precision=prec, smooth_k=True,
                                                               return_path=True, return_quant=True)
        path = path.cpu().numpy()
        check_path_structure(path, Sq, Skv, True, prec, D == 128)
        s = case.seqs[0]
        ku = np.zeros_like(s.k)
        ku[:, :Skv] = _deq8(unpack_frag(quant["k8"].cpu().numpy(), _native.LAYOUT_KFRAG, 1, 2, Skv, D)[0, :, :Skv], quant["scale_k"][0].cpu().numpy())
        ref = s.softmax(s.mask, k=ku)[0][None]
        res["dense " + prec] = grade(out_to_f32(out), PathRef(ref, ref), path)[2]
    print(f"decoy on smoothed keys D {D}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert all(v < 1.0 for v in res.values()), res


# ---- the three separate C calls: quantise (q row-major, k and v into their fragment layouts), then attend ---------------------------------
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [True, False])
def test_separate_c_calls(D, causal):
    Sq = Skv = 1100
    dtype, res = torch.bfloat16, {}
    for probe in ("count", "decoy", "pointer") if causal else ("count", "pointer"):
        case, q, k, v, ref, ref_lse, _ = dense(probe, D, Sq, Skv, causal)
        q8, sq = _native.quant_fp8(T(q, dtype))
        kf, sk = _native.quant_fp8(T(k, dtype), layout=_native.LAYOUT_KFRAG)
        vf, sv = _native.quant_fp8(T(v, dtype), layout=_native.LAYOUT_VFRAG)
        for prec in ("accurate",) if probe == "pointer" else ("fast", "auto"):   # (fp8 P on peaked rows: promised by accurate only)
            out, lse = _native.fp8_attention_forward(q8, kf, vf, sq, sk, sv, Hkv=2, Skv=Skv, out_dtype=dtype, is_causal=causal, precision=prec,
                                                     return_lse=True)
            what = f"{probe} {prec}"
            if probe == "count":
                res[what] = count_ratio(out_to_f32(out), ref, dtype, what)
                tot = np.broadcast_to(P.count_expected(case.seqs[0].mask, D)[1], (2, Sq))
                ref_lse = P.count_lse(deq_q(q, dtype, "e4m3", "head")[0], k[0, :, 0], tot)[None]
            else:
                res[what] = grade(out_to_f32(out), ref)[2]
            res[what + " lse"] = lse_ratio(lse.cpu().numpy(), ref_lse, P.LSE_TOL, what)
    print(f"separate C calls D {D} causal {causal}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert all(v <= 1.0 for v in res.values()), res


# ---- layouts and graphs --------------------------------------------------------------------------------------------------------------------
def test_fused_on_transposed_bshd_views():
    """q, k, v as the [B, H, S, D] views of [B, S, H, D] memory: read in place -- the dense call's bits, and the probes' bounds"""
    B, Hq, Hkv, D, Sq, Skv, dtype, res = 2, 4, 2, 128, 1100, 1100, torch.bfloat16, {}
    view = lambda a: T(np.ascontiguousarray(a.transpose(0, 2, 1, 3)), dtype).transpose(1, 2)
    for probe in ("count", "decoy", "pointer"):
        case, q, k, v, ref, _, peaked = dense(probe, D, Sq, Skv, True, B, Hq, Hkv)
        tq, tk, tv = view(q), view(k), view(v)
        assert not tq.is_contiguous() and not tk.is_contiguous()
        out, path = fused_call(tq, tk, tv, causal=True, precision="auto")
        want, _ = fused_call(T(q, dtype), T(k, dtype), T(v, dtype), causal=True, precision="auto")
        assert np.array_equal(out, want), "a strided view gives the dense call's bits"
        assert np.isin(path[peaked], (PATH_V16, PATH_TWO_TERM)).all()
        res[probe] = count_ratio(out, ref, dtype, probe) if probe == "count" else grade(out, PathRef(ref, ref), path)[2]
    print("fused on [B,S,H,D] views: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert res["count"] <= 1.0 and res["decoy"] < 1.0 and res["pointer"] < 1.0, res


def test_graph_replay_of_the_packed_decoy_probe_on_rewritten_tables():
    D, dtype = 128, torch.bfloat16
    lens, captured = P.GRAPH_LENS
    Hq, Hkv = P.heads("packed", "decoy")
    case = P.make_case("decoy", D, lens, lens, kind="causal", Hq=Hq, Hkv=Hkv)
    q, k, v = T(case.q, dtype), T(case.k, dtype), T(case.v, dtype)
    cu_q, cu_k = _cu(captured), _cu(captured)
    call = lambda: qa.fp8_attn_varlen_func(q, k, v, cu_q, cu_k, max(lens), max(lens), causal=True, return_lse=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = call()
    cu_q.copy_(_cu(lens))
    cu_k.copy_(_cu(lens))
    graph.replay()
    torch.cuda.synchronize()
    r, rl = _grade_packed(case, out, lse, dtype, "graph replay")
    print(f"graph replay of the packed decoy probe: {r:.3f}, lse {rl:.3f}")
    assert r < 1.0 and rl < 1.0, (r, rl)

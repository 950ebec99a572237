"""The membership probes of tests/probes.py on the CPU: every probe tensor survives the quantiser unchanged, the closed forms equal the
fp64 masked softmax and the oracle, and -- the TEETH condition -- under every named wrong mask (each edge moved by +-1, the zero padding
admitted with score 0, a neighbour sequence's adjacent key or the key at seqused_k admitted, a 64-key chunk dropped, a tile flipped, another
kv head's or batch entry's keys read) some element of every row the mutant touches moves by at least 4x the bound tests/test_gpu_probes.py
applies to it.  That is a condition on the inputs, not a measurement: a case without teeth is not kept."""
import numpy as np
import pytest

import oracle
from tests import probes as P

BITS = {"bf16": (oracle.FMT_BF16, oracle.f32_to_bf16_bits, oracle.bf16_bits_to_f32),
        "fp16": (oracle.FMT_FP16, lambda x: np.asarray(x, np.float32).astype(np.float16).view(np.uint16), oracle.fp16_bits_to_f32)}


def _assert_teeth(res, what):
    assert res, (what, "no mutant touched a row")
    print(f"{what}: " + ", ".join(f"{k} {v:.1f}x" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not v >= P.TEETH}
    assert not bad, (what, bad)


# ---- quantisation exactness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [oracle.FMT_E4M3, oracle.FMT_E5M2])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_probe_tensors_survive_the_quantiser(dt, fp8):
    fmt, to_bits, from_bits = BITS[dt]
    D = 64
    for probe in ("count", "decoy", "pointer", "scatter"):
        case = P.dense_case(probe, D, 333, 1090, False, n_peaked=33)
        q, k, v = case.dense()
        for name, t in (("q", q), ("k", k), ("v", v)):
            bits = to_bits(t.astype(np.float32))
            assert np.array_equal(from_bits(bits).astype(np.float64), t), "the 16-bit type holds every probe value"
            for mode in ("head", "token"):
                x8, s = oracle.quantize_fp8(bits, fmt, mode, fp8)
                deq = oracle.fp8_to_f32(x8, fp8).astype(np.float64) * s.astype(np.float64).reshape(s.shape + (1,) * (4 - s.ndim))
                ok = np.abs(deq - t) <= 2.0 ** -20 * np.abs(t)
                if probe == "count" and name == "q" and mode == "head":
                    # the stated exception (tests/probes.py): g = 1.5 beside the head abs-max 2 is a tie of the fp8 grid; the row stays a
                    # constant vector -- one score per row, which is all the count probe needs -- and every other row is exact
                    g15 = np.isclose(t, -1.5)
                    assert ok[~g15].all() and (deq == deq[..., :1]).all() and (np.abs(deq[g15] - t[g15]) < 0.13).all()
                else:
                    assert ok.all(), (probe, name, mode, float(np.abs(deq - t).max()))
        if probe in ("count", "scatter"):
            vb = to_bits(v.astype(np.float32))
            assert np.array_equal(oracle.bf16_bits_to_f32(oracle.quantize_v_block(vb, fmt, fp8)[2]).astype(np.float64), v)


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,arg,lq,lk", [("full", None, 333, 1090), ("causal", 0, 300, 300), ("causal", 0, 700, 420),
                                            ("window", (100, 37), 300, 420), ("window", (0, 200), 420, 300), ("window", (63, 0), 130, 130)])
def test_count_closed_form_equals_the_fp64_softmax(kind, arg, lq, lk):
    for D in (64, 128, 256):
        case = P.make_case("count", D, [lq], [lk], kind=kind, arg=arg)
        out, lse = case.reference()
        s = case.seqs[0]
        o64, l64 = s.softmax()
        assert np.abs(out.transpose(1, 0, 2) - o64).max() < 1e-12
        live = np.isfinite(l64)
        assert np.array_equal(live, np.isfinite(lse)) and np.abs(lse[live] - l64[live]).max() < 1e-12
        assert (out.sum(-1)[live.T] > 1 - 1e-12).all() and (out[~live.T] == 0).all()


def test_count_closed_form_from_a_tile_list():
    tiles = P.sparse_tiles("random", 6, 11, H=2)
    case = P.make_case("count", 128, [700], [1300], tiles=tiles, Hq=2, Hkv=1)
    out, _ = case.reference()
    assert np.abs(out.transpose(1, 0, 2) - case.seqs[0].softmax()[0]).max() < 1e-12


@pytest.mark.parametrize("probe", ["count", "decoy", "pointer", "scatter"])
@pytest.mark.parametrize("causal", [False, True])
def test_dense_probes_against_the_oracle(probe, causal):
    """oracle.attention_forward on the oracle's own quantiser output = the probe's reference (out and LSE; the count probe's q under
    head-wise scales per the stated exception: token-wise here)"""
    D, Sq, Skv = 64, 200, 330
    if causal:
        Sq = Skv
    case = P.dense_case(probe, D, Sq, Skv, causal, B=2, Hq=4, Hkv=2, n_peaked=33)
    q, k, v = case.dense()
    ref, ref_lse = case.reference()
    ref = ref.reshape(2, Sq, 4, D).transpose(0, 2, 1, 3)
    ref_lse = ref_lse.reshape(4, 2, Sq).transpose(1, 0, 2)
    b = lambda t: oracle.f32_to_bf16_bits(t.astype(np.float32))
    for fp8 in (oracle.FMT_E4M3, oracle.FMT_E5M2):
        for mode in ("token", "head") if probe != "count" else ("token",):
            q8, sq = oracle.quantize_fp8(b(q), oracle.FMT_BF16, mode, fp8)
            k8, sk = oracle.quantize_fp8(b(k), oracle.FMT_BF16, mode, fp8)
            out, lse = oracle.attention_forward(q8, k8, b(v), fp8, fp8, oracle.FMT_BF16, sq, sk, None, scale_mode=mode, causal=causal,
                                                return_lse=True)
            assert np.abs(out - ref).max() < 1e-5 and np.abs(lse - ref_lse).max() < 1e-4, (probe, mode, fp8)


# ---- teeth (on the inputs of tests/test_gpu_probes.py: same builders, same head counts, same seeds) -----------------------------------------
def _case_teeth(case, what, dtype="bf16", v16=None, lse_tol=P.LSE_TOL_V16, smooth=False):
    for i, (s, aux, mut) in enumerate(zip(case.seqs, case.aux, case.mutants)):
        if s.dims[2] == 0 or s.m == 0:
            continue
        if case.probe == "count":
            res = P.count_teeth(s, mut, dtype, lse_tol=lse_tol)
        elif case.probe == "decoy":
            if not (aux >= 0).any():
                continue
            res = P.decoy_teeth(s, aux, v16, k=P.smoothed_k(s) if smooth else None)
        else:
            others = {}
            if s.dims[1] > 1:
                others["kv head off by one"] = (np.roll(s.k, 1, 0), np.roll(s.v, 1, 0))
            if len(case.seqs) > 1 and case.seqs[i - 1].k.shape == s.k.shape:
                others["batch index off by one"] = (case.seqs[i - 1].k, case.seqs[i - 1].v)
            res = P.pointer_teeth(s, aux, v16, others)
            if case.probe == "scatter":   # the uniform rows around the pointer rows: the count probe's mutants, on the closed form
                flat = np.broadcast_to(aux < 0 if aux.ndim == 2 else (aux < 0)[None], s.q.shape[:2])
                res.update(P.count_teeth(s, mut, dtype, lse_tol=lse_tol, rows_graded=flat))
        _assert_teeth(res, f"{what} seq {i}")


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("Sq,Skv,causal", P.DENSE_SHAPES)
def test_teeth_dense(D, Sq, Skv, causal):
    what = f"dense D {D} ({Sq}, {Skv}) causal {causal}"
    # (the fused entry's LSE tolerance is widest on the D = 128 head-wise sweep: the teeth are asked against that one)
    for probe in ("count", "decoy", "pointer") if causal else ("count", "pointer"):
        _case_teeth(P.dense_case(probe, D, Sq, Skv, causal), f"{what} {probe}", lse_tol=P.LSE_TOL_SWEEP128 if D == 128 else P.LSE_TOL_V16)


@pytest.mark.parametrize("B,Hq,Hkv", [(2, 4, 2), (3, 5, 5)])
def test_teeth_dense_gqa_and_odd_head_count(B, Hq, Hkv):
    for probe in ("count", "decoy", "pointer"):
        _case_teeth(P.dense_case(probe, 128, 1100, 1100, True, B=B, Hq=Hq, Hkv=Hkv), f"dense B {B} Hq {Hq} Hkv {Hkv} {probe}",
                    lse_tol=P.LSE_TOL_SWEEP128)
    _case_teeth(P.dense_case("decoy", 128, 1100, 1100, True, B=B, Hq=Hq, Hkv=Hkv), "smoothed keys", smooth=True)


def test_teeth_long_keys_fp16():
    Sq, Skv = P.LONG_KEYS
    _case_teeth(P.dense_case("count", 128, Sq, Skv, False, Hq=2, Hkv=1), "long keys count", dtype="fp16", lse_tol=P.LSE_TOL_SWEEP128)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("n_peaked", [1, 33, 130])
def test_teeth_scattered_pointer_rows(D, n_peaked):
    case = P.dense_case("scatter", D, 1100, 1100, False, n_peaked=n_peaked)
    assert case.pointer_rows().sum() == 2 * n_peaked
    _case_teeth(case, f"scatter D {D} {n_peaked}", lse_tol=P.LSE_TOL_SWEEP128 if D == 128 else P.LSE_TOL_V16)
    # a pointer row written to a neighbour's slot (and the neighbour's to its own): an O(1) error on both rows
    ref, _ = case.reference()
    peaked = case.pointer_rows()[0]
    r = np.nonzero(peaked[:-1] & ~peaked[1:])[0][0]
    assert np.abs(ref[r] - ref[r + 1]).max() > 0.9


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("name", ["lens causal", "lens full", "cross causal", "cross full", "seqused causal", "seqused full"])
def test_teeth_packed(D, name):
    which, kind = name.split()
    lq, alloc, used = {"lens": (P.PACKED_LENS, P.PACKED_LENS, None), "cross": P.PACKED_CROSS + (None,), "seqused": P.PACKED_SEQUSED}[which]
    for probe in ("count", "decoy", "pointer"):
        Hq, Hkv = P.heads("packed", probe)
        _case_teeth(P.make_case(probe, D, lq, alloc, used, kind=kind, Hq=Hq, Hkv=Hkv), f"packed {name} D {D} {probe}", v16=True)


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("window", P.WINDOWS)
def test_teeth_window(D, window):
    for lq, lk in ((P.WINDOW_LENS, P.WINDOW_LENS), P.WINDOW_CROSS):
        for probe in ("count", "decoy", "pointer"):
            Hq, Hkv = P.heads("window", probe)
            _case_teeth(P.make_case(probe, D, lq, lk, kind="window", arg=window, Hq=Hq, Hkv=Hkv), f"window {window} D {D} {lq} {probe}", v16=True,
                        dtype=P.WINDOW_COUNT_DTYPE[D])


@pytest.mark.parametrize("D", [64, 128, 256])
def test_teeth_decoy_on_smoothed_keys(D):
    """the decoy probe under key smoothing (k - the channel mean of the sequence's keys): same masks, same decoys, other operands"""
    lq, lk = P.SMOOTH_LENS
    Hq, Hkv = P.heads("packed", "decoy")
    _case_teeth(P.make_case("decoy", D, lq, lk, kind="causal", Hq=Hq, Hkv=Hkv), f"smoothed packed D {D}", v16=True, smooth=True)
    _case_teeth(P.make_case("decoy", D, lq, lk, kind="window", arg=P.SMOOTH_WINDOW, Hq=Hq, Hkv=Hkv), f"smoothed window D {D}", v16=True, smooth=True)
    tiles = P.sparse_tiles("band+global", 11, 11, 1)
    Hq, Hkv = P.heads("sparse", "decoy")
    _case_teeth(P.make_case("decoy", D, [1300], [1300], tiles=tiles, Hq=Hq, Hkv=Hkv), f"smoothed block-sparse D {D}", v16=True, smooth=True)
    _case_teeth(P.dense_case("decoy", D, 1100, 1100, True), f"smoothed dense D {D}", smooth=True)


@pytest.mark.parametrize("D,name,Sq,Skv,H", P.SPARSE_CASES)
def test_teeth_block_sparse(D, name, Sq, Skv, H):
    tiles = P.sparse_tiles(name, -(-Sq // 128), -(-Skv // 128), H)
    for probe in ("count", "decoy", "pointer"):
        Hq, Hkv = P.heads("sparse", probe)
        case = P.make_case(probe, D, [Sq], [Skv], tiles=tiles, Hq=Hq, Hkv=Hkv, flips=P.sparse_flips(tiles))
        _case_teeth(case, f"block-sparse {name} ({Sq}, {Skv}) D {D} {probe}", v16=True)


def test_teeth_graph_replay_tables():
    lq, _ = P.GRAPH_LENS
    Hq, Hkv = P.heads("packed", "decoy")
    _case_teeth(P.make_case("decoy", 128, lq, lq, kind="causal", Hq=Hq, Hkv=Hkv), "graph replay decoy", v16=True)

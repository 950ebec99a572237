"""-m gpu: the constant-V witness of tests/vwitness.py through every attention entry on the MI355X ("V-format witness"): WHICH
V -- the caller's 16-bit tensor or its fp8 rounding -- every row attended, read off the output itself.

V is constant along the key axis, so every output row is its kv head's channel vector in the format the kernel read, whatever the
softmax weights; the 16-bit vector and its fp8 reading are >= 5 of the project's bounds apart on every witness channel
(tests/test_cpu_vwitness.py).  Every case asserts that no row is "neither" (within the existing bound of neither vector of ITS kv head:
B 1, Hq 4, Hkv 2 throughout), that the label agrees with the row_path the kernel reports (fused entry), and that the label is the one the
literal table tests/vwitness.py::EXPECTED_V names for the entry.  No fp64 attention oracle is needed here: the answer is the vector.
Each test prints the worst |got - vector| per label (reported, not asserted beyond the existing bounds).

WHAT IT FOUND ("V-format witness"): no row attended the wrong V, but with the two-term P as it was, 8 cases below failed on
the MI355X for one reason.  On planted rows whose top key holds 93 .. 99 % of the weight, the other keys' weights lie more than ~15
binades below the top and e4m3 rounded them to zero in the high AND the low term, while the fp32 row sum that normalises O keeps them.
With a constant V nothing averages out: the row came out as v (1 - flushed mass), up to 0.0234 low at |v| = 1.75 against the bound
2^-6 = 0.0156 -- "neither" (2 .. 18 of ~5100 rows per call, 1.00x .. 1.50x the bound).  The kernels now carry the low term x 2^5 and take
the gain back with the PV product's block scale (csrc/qattn_attn.h, lo_terms): the floor of the two-term P is 2^-15 and every case here
passes (profiles/vwitness/pytest_gpu.log)."""
import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import probes as P
from tests import vwitness as W
from tests.gpu_utils import PATH_ONE_TERM, PATH_V16, TDT, PathRef, fused_call, grade, out_to_f32
from tests.vwitness import EXPECTED_V, FP8, NEITHER, V16

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, HQ, HKV = 1, 4, 2
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}
IDS = lambda x: str(x).replace("torch.", "")
SHORT = [(300, True), (700, False)]          # every block early
PRECISIONS = ("fast", "auto", "accurate")


def G(t, dtype):
    return t.to(dtype).to(DEV)


def vectors(D, dtype, fp8, shape=(1, HQ, 1)):
    """(v16, vfp8) of every query head's kv head, shaped to broadcast against an output whose head axis is given by `shape`"""
    v16, v8 = W.witness_vectors(HKV, D, dtype, fp8)
    return W.per_q_head(v16, HQ).reshape(shape + (D,)), W.per_q_head(v8, HQ).reshape(shape + (D,))


class Report:
    """worst |got - vector| and row counts per label over the calls of one test, and the calls that missed a check: every call of a test
    is made and graded, then `done` fails the test with all of them"""

    def __init__(self):
        self.worst, self.rows, self.failed = {V16: 0.0, FP8: 0.0}, {V16: 0, FP8: 0}, []

    def add(self, labels, worst):
        for lab in (V16, FP8):
            self.worst[lab] = max(self.worst[lab], worst[lab])
            self.rows[lab] += int((labels == lab).sum())

    def __str__(self):
        return ", ".join(f"{lab}: {self.rows[lab]} rows, worst |got - vector| {self.worst[lab]:.5f}" for lab in (V16, FP8))

    def done(self, *others):
        failed = self.failed + [f for o in others for f in o.failed]
        assert not failed, "\n".join([f"{len(failed)} call(s) missed a check:"] + failed)


def check(out, v16, v8, want, what, rep, path=None, alive=None):
    """classify; no row "neither"; label "v16" <=> row_path == QATTN_PATH_V16 (where the entry reports one); the label `want` names.
    alive (bool, rows): rows that attend a key -- the others must be exactly zero and are not classified.  A miss is printed and kept in
    `rep` (Report.done fails the test)."""
    out = np.asarray(out)
    if alive is not None:
        alive = np.broadcast_to(alive, out.shape[:-1])
        assert alive.any(), what
        if not (out[~alive] == 0).all():
            rep.failed.append(f"{what}: rows that attend no key must be exactly zero")
    labels, worst = W.classify(out, v16, v8)
    live = np.ones(labels.shape, bool) if alive is None else alive
    none = live & (labels == NEITHER)
    msgs = []
    if none.any():
        off16, off8 = W.miss(out, v16, V16)[none], W.miss(out, v8, FP8)[none]
        msgs.append(f"{what}: {int(none.sum())} row(s) are NEITHER vector of their kv head (first {np.argwhere(none)[:4].tolist()}); their distance to "
                    f"the nearer vector is up to {worst[NEITHER]:.5f} = {float(np.minimum(off16, off8).max()):.2f}x that vector's bound")
    if path is not None:
        off = live & ~none & ((labels == V16) != (np.asarray(path) == PATH_V16))
        if off.any():
            msgs.append(f"{what}: {int(off.sum())} row(s): the attended V disagrees with the reported row_path (first {np.argwhere(off)[:4].tolist()}: "
                        f"{labels[off][:4].tolist()} with path {np.asarray(path)[off][:4].tolist()})")
    try:
        W.require(labels, out, v16, v8, want, what, rows=live & ~none)
    except AssertionError as e:
        msgs.append(str(e))
    for m in msgs:
        print("MISSED: " + m)
    rep.failed += msgs
    rep.add(labels[live], worst)
    return labels


# ---- the fused entry --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,scaling,dtype,fp8", W.FUSED, ids=IDS)
def test_fused_entry(D, scaling, dtype, fp8):
    v16, v8 = vectors(D, dtype, fp8)
    rep, what0 = Report(), f"fused D {D} {scaling} {NAME[dtype]} {fp8}"
    for S, causal in [W.SHAPE_FULL, W.SHAPE_CAUSAL] + SHORT:
        q, k = W.scores_case(S, D, "flat", 0, causal)
        tq, tk, tv = G(q, dtype), G(k, dtype), W.witness_v(B, HKV, S, D, dtype, fp8).to(DEV)
        for prec in PRECISIONS:
            out, path = fused_call(tq, tk, tv, causal=causal, precision=prec, fp8=fp8, scaling=scaling)
            check(out, v16, v8, W.expected_fused(S, S, causal, prec, D, scaling), f"{what0} S {S} causal {causal} flat {prec}", rep, path)
    print(f"{what0}: {rep}")
    rep.done()


@pytest.mark.parametrize("D,scaling,dtype,fp8", W.MIXED, ids=IDS)
def test_fused_entry_auto_on_mixed_scores(D, scaling, dtype, fp8):
    """AUTO where it has something to decide: severe rows (R <= 4 on the oracle) outside the early blocks must attend the 16-bit V on the
    D = 128 head-wise kernel; the templated kernel keeps every such row on the fp8 V; moderate rows (10 <= R <= 20) are held to
    label <=> reported path only.
    Before the low term of the two-term P carried its gain this failed on the templated kernel at D = 64 (head-wise bf16: 11 rows of
    S 1280 at 1.00x the bound, 18 rows of S 2304 at 1.50x = 0.0234; token-wise fp16: 6 rows at 1.31x) and D = 128 token-wise (10 rows at
    1.00x) -- the flushed rest of the module docstring; D = 256 (top key 20 nats up: no rest mass to lose) and the D = 128 head-wise
    kernel (severe rows on the 16-bit V) passed then too."""
    v16, v8 = vectors(D, dtype, fp8)
    rep, what0 = Report(), f"fused auto mixed D {D} {scaling} {NAME[dtype]} {fp8}"
    for S, causal in (W.SHAPE_FULL, W.SHAPE_CAUSAL):
        q, k = W.scores_case(S, D, "mixed", W.MIXED_SEED, causal)
        severe, moderate = W.peaked_rows(q, k, dtype, fp8, scaling, causal)
        late = ~W.early_rows(S, S, causal)
        assert severe[..., late].sum() >= W.MIN_ROWS and moderate[..., late].sum() >= W.MIN_ROWS
        out, path = fused_call(G(q, dtype), G(k, dtype), W.witness_v(B, HKV, S, D, dtype, fp8).to(DEV), causal=causal, precision="auto", fp8=fp8,
                               scaling=scaling)
        what = f"{what0} S {S} causal {causal}"
        labels = check(out, v16, v8, W.expected_fused(S, S, causal, "auto", D, scaling, severe=severe), what, rep, path)
        n16, n8 = int((labels[..., late] == V16).sum()), int((labels[..., late] == FP8).sum())
        mod16 = int((labels[moderate & late] == V16).sum())
        print(f"{what}: outside the early blocks {n16} rows v16, {n8} rows fp8; of {int(severe[..., late].sum())} severe rows "
              f"{int((labels[severe & late] == V16).sum())} v16; of {int((moderate & late).sum())} moderate rows {mod16} v16")
        if W.kernel_of(D, scaling) == "v2":
            assert n16 >= W.MIN_ROWS and n8 >= W.MIN_ROWS, (what, "the case proves nothing: fewer than 32 rows of a label outside the early blocks", n16, n8)
    print(f"{what0}: {rep}")
    rep.done()


@pytest.mark.parametrize("D,scaling", [(D, s) for D in (64, 128, 256) for s in ("head-wise", "token-wise")], ids=IDS)
def test_fused_entry_key_count_edge(D, scaling):
    """Skv 1023: every block is early -- all rows v16.  Skv 1024: none is -- the rows are on the fp8 V (FAST, ACCURATE on the templated
    kernel and AUTO on the templated kernel by the table; AUTO on the D = 128 head-wise kernel: label <=> reported path)."""
    dtype, fp8, Sq = (torch.bfloat16 if D != 64 else torch.float16), "e4m3", 300
    v16, v8 = vectors(D, dtype, fp8)
    rep = Report()
    for Skv in (1023, 1024):
        q, k = W.scores_case(Skv, D, "flat", 2, False, Sq)
        tq, tk, tv = G(q, dtype), G(k, dtype), W.witness_v(B, HKV, Skv, D, dtype, fp8).to(DEV)
        for prec in PRECISIONS:
            out, path = fused_call(tq, tk, tv, causal=False, precision=prec, fp8=fp8, scaling=scaling)
            want = W.expected_fused(Sq, Skv, False, prec, D, scaling)
            if Skv == 1023:
                assert (want == V16).all()
            labels = check(out, v16, v8, want, f"fused D {D} {scaling} Sq {Sq} Skv {Skv} {prec}", rep, path)
            if Skv == 1024 and prec == "fast":
                assert (labels == FP8).all()
    print(f"fused key-count edge D {D} {scaling}: {rep}")
    rep.done()


def test_public_function_gives_the_fused_calls_bits():
    D, dtype, fp8 = 128, torch.bfloat16, "e4m3"
    S, causal = W.SHAPE_CAUSAL
    v16, v8 = vectors(D, dtype, fp8)
    q, k = W.scores_case(S, D, "mixed", W.MIXED_SEED, causal)
    tq, tk, tv = G(q, dtype), G(k, dtype), W.witness_v(B, HKV, S, D, dtype, fp8).to(DEV)
    out, path = fused_call(tq, tk, tv, causal=causal, precision="auto")
    pub = out_to_f32(qa.fp8_attn_func(tq, tk, tv, is_causal=causal))
    assert np.array_equal(pub, out), "qa.fp8_attn_func is the fused call with row_path = NULL"
    rep = Report()
    check(pub, v16, v8, W.expected_fused(S, S, causal, "auto", D, "head-wise"), "qa.fp8_attn_func", rep, path)
    # config.attention.pv_precision = "16bit" (read by the op on pre-quantised q / k): the separate call with a 16-bit P and V, every row v16
    q8, sq = qa.dynamically_quantize_fp8(tq, reduction_dim=[2, 3])
    k8, sk = qa.dynamically_quantize_fp8(tk, reduction_dim=[2, 3])
    with qa.config.patch({"attention.pv_precision": "16bit"}):
        op16 = out_to_f32(torch.ops.quantumattention_amd.fp8_attention_forward(q8, k8, tv, sq, sk, None, 0.0, causal))
    sep16 = out_to_f32(_native.fp8_attention_forward_rowmajor(q8, k8, tv, sq, sk, is_causal=causal, pv_16bit=True))
    assert np.array_equal(op16, sep16), 'pv_precision = "16bit" is the row-major call with pv_16bit'
    rep16 = Report()
    check(op16, v16, v8, EXPECTED_V[("separate16",)], 'op with pv_precision = "16bit"', rep16)
    opf8 = out_to_f32(torch.ops.quantumattention_amd.fp8_attention_forward(q8, k8, tv, sq, sk, None, 0.0, causal))
    check(opf8, v16, v8, EXPECTED_V[("separate",)], 'op with pv_precision = "fp8"', rep16)
    print(f"public fp8_attn_func: {rep}; the op on pre-quantised q / k under pv_precision 16bit / fp8: {rep16}")
    rep.done(rep16)


def test_strided_entry_gives_the_dense_calls_labels():
    """q, k, v as the [B, H, S, D] views of [B, S, H, D] memory, read in place: the dense call's labels (and bits)"""
    D, dtype, fp8 = 128, torch.float16, "e4m3"
    v16, v8 = vectors(D, dtype, fp8)
    view = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)
    rep = Report()
    for (S, causal), kind in ((W.SHAPE_CAUSAL, "mixed"), (W.SHAPE_FULL, "flat")):
        q, k = W.scores_case(S, D, kind, W.MIXED_SEED, causal)
        tq, tk, tv = G(q, dtype), G(k, dtype), W.witness_v(B, HKV, S, D, dtype, fp8).to(DEV)
        sq, sk, sv = view(tq), view(tk), view(tv)
        assert not sq.is_contiguous() and not sk.is_contiguous() and not sv.is_contiguous()
        for prec in ("fast", "auto"):
            dense, dpath = fused_call(tq, tk, tv, causal=causal, precision=prec)
            out, path = fused_call(sq, sk, sv, causal=causal, precision=prec)
            severe = W.peaked_rows(q, k, dtype, fp8, "head-wise", causal)[0] if kind == "mixed" else None
            labels = check(out, v16, v8, W.expected_fused(S, S, causal, prec, D, "head-wise", severe=severe), f"strided S {S} {prec}", rep, path)
            assert np.array_equal(labels, W.classify(dense, v16, v8)[0]) and np.array_equal(out, dense) and np.array_equal(path, dpath)
    print(f"fused on [B,S,H,D] views: {rep}")
    rep.done()


@pytest.mark.parametrize("D,scaling", [(128, "head-wise"), (64, "head-wise"), (256, "token-wise")], ids=IDS)
def test_smoothing_entry_gives_the_dense_calls_labels(D, scaling):
    """smooth_k touches K only: on flat scores the labels of the dense call; on mixed scores the table's (severe rows on the 16-bit V).
    (D = 64 head-wise, mixed causal: the 18 rows of the dense call that the unscaled low term left 1.50x the bound low -- module docstring.)"""
    dtype, fp8 = torch.bfloat16, "e4m3"
    v16, v8 = vectors(D, dtype, fp8)
    rep = Report()

    def smooth(tq, tk, tv, causal, prec):
        out, path = _native.fp8_quant_attention_forward(tq, tk, tv, is_causal=causal, scaling=scaling, fp8_dtype=TDT[fp8], precision=prec,
                                                        smooth_k=True, return_path=True)
        return out_to_f32(out), path.cpu().numpy()

    for S, causal in (W.SHAPE_FULL, W.SHAPE_CAUSAL, SHORT[0]):
        q, k = W.scores_case(S, D, "flat", 0, causal)
        tq, tk, tv = G(q, dtype), G(k, dtype), W.witness_v(B, HKV, S, D, dtype, fp8).to(DEV)
        for prec in PRECISIONS:
            out, path = smooth(tq, tk, tv, causal, prec)
            labels = check(out, v16, v8, W.expected_fused(S, S, causal, prec, D, scaling), f"smooth D {D} {scaling} S {S} flat {prec}", rep, path)
            dense, _ = fused_call(tq, tk, tv, causal=causal, precision=prec, fp8=fp8, scaling=scaling)
            assert np.array_equal(labels, W.classify(dense, v16, v8)[0]), (S, prec, "smoothing K must not move a row to another V")
    for S, causal in (W.SHAPE_FULL, W.SHAPE_CAUSAL):
        q, k = W.scores_case(S, D, "mixed", W.MIXED_SEED, causal)
        severe = W.peaked_rows(q, k, dtype, fp8, scaling, causal)[0]
        out, path = smooth(G(q, dtype), G(k, dtype), W.witness_v(B, HKV, S, D, dtype, fp8).to(DEV), causal, "auto")
        check(out, v16, v8, W.expected_fused(S, S, causal, "auto", D, scaling, severe=severe), f"smooth D {D} {scaling} S {S} mixed auto", rep, path)
    print(f"smoothing entry D {D} {scaling}: {rep}")
    rep.done()


# ---- the separate calls: the fp8 V on every row, early rows included; a 16-bit V on every row when asked ---------------------------------
@pytest.mark.parametrize("D,scaling,dtype,fp8", [(64, "head-wise", torch.bfloat16, "e4m3"), (128, "head-wise", torch.bfloat16, "e4m3"),
                                                 (128, "token-wise", torch.float16, "e4m3"), (256, "head-wise", torch.float16, "e4m3"),
                                                 (128, "head-wise", torch.bfloat16, "e5m2")], ids=IDS)
def test_separate_calls(D, scaling, dtype, fp8):
    """The mixed causal case (S 2304) is the one the unscaled low term missed for every case but D = 256: 2 .. 18 severe rows were "neither"
    under AUTO and / or ACCURATE (D 64: 1.50x the bound; D 128 head-wise bf16, e4m3 and e5m2: 1.00x; D 128 token-wise fp16: 1.12x) -- the
    flushed rest of the module docstring; FAST keeps its one-term result (the top key is exact, the rest flushed from sum and product
    alike).  The 16-bit-V forms of the same calls run on the same scores."""
    v16, v8 = vectors(D, dtype, fp8)
    rep8, rep16 = Report(), Report()
    for S, causal in (W.SHAPE_CAUSAL, SHORT[0], SHORT[1]):
        q, k = W.scores_case(S, D, "mixed" if S == W.SHAPE_CAUSAL[0] else "flat", W.MIXED_SEED, causal)
        tq, tk, tv = G(q, dtype), G(k, dtype), W.witness_v(B, HKV, S, D, dtype, fp8).to(DEV)
        q8, sq = _native.quant_fp8(tq, scaling=scaling, fp8_dtype=TDT[fp8])
        kf, sk = _native.quant_fp8(tk, scaling=scaling, fp8_dtype=TDT[fp8], layout=_native.LAYOUT_KFRAG)
        k8, _ = _native.quant_fp8(tk, scaling=scaling, fp8_dtype=TDT[fp8])
        vf, sv = _native.quant_fp8(tv, fp8_dtype=TDT[fp8], layout=_native.LAYOUT_VFRAG)
        what = f"separate D {D} {scaling} {NAME[dtype]} {fp8} S {S} causal {causal}"
        for prec in PRECISIONS:
            out = _native.fp8_attention_forward(q8, kf, vf, sq, sk, sv, Hkv=HKV, Skv=S, out_dtype=dtype, is_causal=causal, scaling=scaling, precision=prec)
            check(out_to_f32(out), v16, v8, EXPECTED_V[("separate",)], f"{what} {prec}", rep8)
            out = _native.fp8_attention_forward_rowmajor(q8, k8, tv, sq, sk, is_causal=causal, precision=prec)
            check(out_to_f32(out), v16, v8, EXPECTED_V[("separate",)], f"{what} row-major {prec}", rep8)
        out = _native.fp8_attention_forward(q8, kf, tv, sq, sk, None, Hkv=HKV, Skv=S, out_dtype=dtype, is_causal=causal, scaling=scaling)
        check(out_to_f32(out), v16, v8, EXPECTED_V[("separate16",)], f"{what} 16-bit v", rep16)
        out = _native.fp8_attention_forward_rowmajor(q8, k8, tv, sq, sk, is_causal=causal, pv_16bit=True)
        check(out_to_f32(out), v16, v8, EXPECTED_V[("separate16",)], f"{what} row-major pv_16bit", rep16)
    print(f"separate calls D {D} {scaling} {NAME[dtype]} {fp8}: fp8 V -- {rep8}; 16-bit V -- {rep16}")
    rep8.done(rep16)


# ---- the packed, window and block-sparse entries: 16-bit P on the 16-bit V on every row that attends a key -------------------------------
PACKED_LQ, PACKED_LK = [300, 700, 40], [300, 520, 40]      # unequal lengths, one shorter than 64; sequence 1 has more rows than keys
WINDOWS = [(64, 0), (-1, 0)]                               # bottom-right aligned: rows 0 .. 179 of sequence 1 attend no key
SPARSE_SQ, SPARSE_SKV = 300, 520                           # 3 query blocks x 5 key blocks of 128


def _cu(lengths):
    return torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32, device=DEV)


def _packed_inputs(D, dtype, fp8="e4m3"):
    g = torch.Generator().manual_seed(11 + D)
    q = torch.randn(sum(PACKED_LQ), HQ, D, generator=g)
    k = torch.randn(sum(PACKED_LK), HKV, D, generator=g)
    v = W.to16(np.broadcast_to(W.witness_vectors(HKV, D, dtype, fp8)[0][None], (sum(PACKED_LK), HKV, D)), dtype)
    return G(q, dtype), G(k, dtype), v.to(DEV)


@pytest.mark.parametrize("D,dtype,fp8", [(64, torch.bfloat16, "e4m3"), (128, torch.float16, "e5m2"), (256, torch.bfloat16, "e4m3")], ids=IDS)
def test_packed_and_window_entries(D, dtype, fp8):
    """(fp8 is the format of q and k here and of the fp8 vector a wrong row would show: these entries never quantise V)"""
    v16, v8 = vectors(D, dtype, fp8, shape=(1, HQ))
    q, k, v = _packed_inputs(D, dtype, fp8)
    cu_q, cu_k = _cu(PACKED_LQ), _cu(PACKED_LK)
    rep_p, rep_w = Report(), Report()
    for smooth in (False, True):
        for causal in (True, False):     # (top-left causal: every row attends key 0)
            out = _native.fp8_quant_attention_varlen(q, k, v, cu_q, cu_k, None, is_causal=causal, fp8_dtype=TDT[fp8], smooth_k=smooth)
            check(out_to_f32(out), v16, v8, EXPECTED_V[("packed",)], f"packed D {D} {fp8} causal {causal} smooth_k {smooth}", rep_p)
        for win in WINDOWS:
            alive = np.concatenate([P.band_mask(*P.band_edges(n, m, "window", win), m, m).any(-1) for n, m in zip(PACKED_LQ, PACKED_LK)])
            assert (~alive).sum() == 180, "rows 0 .. 179 of sequence 1 have an empty window"
            out = _native.fp8_quant_attention_varlen_window(q, k, v, cu_q, cu_k, None, window_left=win[0], window_right=win[1], fp8_dtype=TDT[fp8],
                                                            smooth_k=smooth)
            check(out_to_f32(out), v16, v8, EXPECTED_V[("window",)], f"window {win} D {D} {fp8} smooth_k {smooth}", rep_w, alive=alive[:, None])
    if fp8 == "e4m3":   # the public function (config.attention.fp8_format's default) is this call
        pub = qa.fp8_attn_varlen_func(q, k, v, cu_q, cu_k, max(PACKED_LQ), max(PACKED_LK), causal=True)
        check(out_to_f32(pub), v16, v8, EXPECTED_V[("packed",)], "qa.fp8_attn_varlen_func", rep_p)
    print(f"packed D {D} {NAME[dtype]} {fp8}: {rep_p}; window: {rep_w}")
    rep_p.done(rep_w)


@pytest.mark.parametrize("D,dtype", [(64, torch.float16), (128, torch.bfloat16), (256, torch.float16)], ids=IDS)
def test_block_sparse_entry(D, dtype):
    """a band of tiles on Sq 300 x Skv 520 (|j - 2 i| <= 1); the last query head lists no key block for its middle query block: zero rows"""
    v16, v8 = vectors(D, dtype, "e4m3")
    i, j = np.arange(3)[:, None], np.arange(5)[None, :]
    tiles = np.broadcast_to(np.abs(j - 2 * i) <= 1, (1, HQ, 3, 5)).copy()
    tiles[0, HQ - 1, 1] = False
    alive = np.repeat(tiles.any(-1), 128, axis=-1)[..., :SPARSE_SQ]
    g = torch.Generator().manual_seed(13 + D)
    q, k = torch.randn(B, HQ, SPARSE_SQ, D, generator=g), torch.randn(B, HKV, SPARSE_SKV, D, generator=g)
    tq, tk, tv = G(q, dtype), G(k, dtype), W.witness_v(B, HKV, SPARSE_SKV, D, dtype, "e4m3").to(DEV)
    mask = torch.from_numpy(tiles).to(DEV)
    rep = Report()
    for smooth in (False, True):
        out = _native.fp8_block_sparse_attention(tq, tk, tv, mask, smooth_k=smooth)
        check(out_to_f32(out), v16, v8, EXPECTED_V[("block-sparse",)], f"block-sparse D {D} smooth_k {smooth}", rep, alive=alive)
    check(out_to_f32(qa.fp8_block_sparse_attn_func(tq, tk, tv, mask)), v16, v8, EXPECTED_V[("block-sparse",)], "qa.fp8_block_sparse_attn_func", rep, alive=alive)
    print(f"block-sparse D {D} {NAME[dtype]}: {rep}")
    rep.done()


# ---- the 16-bit sibling path: the sanity anchor of the method -----------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.float16), (256, torch.bfloat16)], ids=IDS)
def test_16bit_attn_func(D, dtype):
    v16, v8 = vectors(D, dtype, "e4m3")
    rep = Report()
    for S, causal in (W.SHAPE_FULL, SHORT[0]):
        q, k = W.scores_case(S, D, "flat", 0, causal)
        out = qa.attn_func(G(q, dtype), G(k, dtype), W.witness_v(B, HKV, S, D, dtype, "e4m3").to(DEV), is_causal=causal)
        check(out_to_f32(out), v16, v8, EXPECTED_V[("attn16",)], f"attn_func D {D} S {S}", rep)
    print(f"16-bit attn_func D {D} {NAME[dtype]}: {rep}")
    rep.done()


# ---- the parity tests' grader on real output ------------------------------------------------------------------------------------------------
def test_grader_fails_by_five_when_a_real_rows_path_is_flipped():
    """One AUTO D = 128 mixed case (e5m2: its fp8 grid under the 2^-15 scale is 0.25 wide, so BOTH wrong readings are >= 5 bounds off; with
    e4m3 a V16 row reported fp8 can be at most 2^-4 / 2^-6 = 4 bounds off -- tests/test_cpu_vwitness.py).  tests/gpu_utils.grade against
    the two constant references passes with the reported path and fails by >= 5x with one v16 row or one fp8 row reported wrongly."""
    D, dtype, fp8 = 128, torch.bfloat16, "e5m2"
    S, causal = W.SHAPE_FULL
    v16, v8 = vectors(D, dtype, fp8)
    q, k = W.scores_case(S, D, "mixed", W.MIXED_SEED, causal)
    out, path = fused_call(G(q, dtype), G(k, dtype), W.witness_v(B, HKV, S, D, dtype, fp8).to(DEV), causal=causal, precision="auto", fp8=fp8)
    rep = Report()
    labels = check(out, v16, v8, None, "grader tooth", rep, path)
    rep.done()
    ref = PathRef(np.broadcast_to(v8, out.shape), np.broadcast_to(v16, out.shape))
    true = grade(out, ref, path)[2]
    assert true < 1.0, true
    res = {}
    for lab, wrong in ((V16, PATH_ONE_TERM), (FP8, PATH_V16)):
        row = tuple(np.argwhere(labels == lab)[0])
        bad = path.copy()
        bad[row] = wrong
        res[lab] = grade(out, ref, bad)[2]
    print(f"grader on real output (e5m2, D 128, auto, mixed): true path {true:.3f} of the bound; a v16 row reported fp8 {res[V16]:.2f}x, "
          f"an fp8 row reported V16 {res[FP8]:.2f}x")
    assert res[V16] >= W.SEPARATION and res[FP8] >= W.SEPARATION, res

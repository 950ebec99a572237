"""The constant-V witness: an input on which the attention OUTPUT shows, row by row, which V the kernel attended ("V-format
witness").  Plain numpy / torch-CPU helpers shared by tests/test_cpu_vwitness.py (separation, independence from P, teeth) and
tests/test_gpu_vwitness.py (the kernels).

V is constant along the key axis, so O_r = sum_j p_j v / sum_j p_j = v whatever the weights p are: row r of head h reproduces the channel
vector of its kv head AS IT STANDS IN THE FORMAT THE KERNEL READ -- the caller's 16-bit numbers, or their fp8 roundings.  Channel 0 is
1.75, so every 64-key chunk and the whole head have abs-max 1.75 and both the block scale and the head scale are the same exact power of
two (2^-8 for e4m3, 2^-15 for e5m2): the block-scaled and the head-scaled fp8 readings are one vector (asserted).  The other channels
cycle through the WITNESS VALUES: the numbers 1 + i/128 in [1, 1.75) -- exact in bf16 and fp16 -- whose fp8 reading is at least
SEPARATION = 5 times the 16-bit-V bound 2^-7 max(1, |v|) away.  They are searched with the oracle's two quantisers, not written down.

The witness separates 16-bit V from fp8 V.  It does NOT separate block-scaled from head-scaled V (tests/test_gpu_quant.py::
test_fused_step_block_scaled_v_is_bit_exact pins that), nor one-term from two-term P (P does not matter here: that is the point)."""
import functools
import math

import numpy as np
import torch

import oracle

FMT = {"e4m3": oracle.FMT_E4M3, "e5m2": oracle.FMT_E5M2}
TOL, TOL_V16 = 2.0 ** -6, 2.0 ** -7      # the project's bounds (tests/gpu_utils.py): fp8-V rows, 16-bit-V rows
SEPARATION = 5.0                          # |fp8 reading - value| >= SEPARATION x the 16-bit-V bound on every witness channel
TOP = 1.75                                # channel 0: the abs-max of every chunk and head
Q_BLOCK, EARLY_KEYS = 256, 1024           # include/qattn.h: early = query blocks (256 rows) whose first row sees < 1024 keys
V16, FP8, NEITHER = "v16", "fp8", "neither"


def bound_v16(ref):
    return TOL_V16 * np.maximum(1.0, np.abs(ref))


def bound_fp8(ref):
    return TOL * np.maximum(1.0, np.abs(ref) / 2.0)


# ---- the expected V format of every entry: a literal restatement of include/qattn.h's PATH TABLE and of the README ---------------------
# (NOT imported from the product and NOT taken from qattn_describe_path(): the test's own statement of what each entry must attend)
EXPECTED_V = {
    # fused = qattn_fp8_quant_attention_forward[_ex] (and its strided / smoothing forms).  "v2": D = 128 with head-wise scales (the
    # hand-scheduled kernel); "v4": every other head dim / token-wise scales (the templated kernel)
    ("fused", "early"): V16,              # `early` v16-inline / v16-launch: every mode attends the caller's 16-bit V on the early blocks
    ("fused", "fast"): FP8,               # FAST: no check -- the one-term sweep on the fp8 V on every other row
    ("fused", "accurate", "v2"): V16,     # `precise` v16: 16-bit P on the caller's 16-bit V
    ("fused", "accurate", "v4"): FP8,     # `precise` two-term: hi + lo e4m3 P on the fp8 V
    ("fused", "auto-severe", "v2"): V16,  # AUTO's flagged rows go to `precise`; only rows with 8 <= R < 24 stay on the fp8 V (two-term)
    ("fused", "auto", "v4"): FP8,         # AUTO on the templated kernel: one-term or two-term, both on the fp8 V
    ("separate",): FP8,                   # ..._attention_forward / _rowmajor with an fp8 V: `early` two-term -- the fp8 V on EVERY row
    ("separate16",): V16,                 # the same calls with a 16-bit V (pv_fmt = v16_fmt): 16-bit P and V on every row
    ("packed",): V16,                     # README: the packed, window and block-sparse entries run 16-bit P on the 16-bit V on every row
    ("window",): V16,
    ("block-sparse",): V16,
    ("attn16",): V16,                     # the 16-bit sibling path: no fp8 anywhere
}


def early_rows(Sq, Skv, causal):
    """bool [Sq]: rows of the query blocks whose first row sees fewer than 1024 keys (causal: key j <= row i, top-left)"""
    first = (np.arange(Sq) // Q_BLOCK) * Q_BLOCK
    return (np.minimum(Skv, first + 1) if causal else np.full(Sq, Skv)) < EARLY_KEYS


def kernel_of(D, scaling):
    return "v2" if (D == 128 and scaling == "head-wise") else "v4"


def expected_fused(Sq, Skv, causal, precision, D, scaling, severe=None):
    """object [.., Sq]: V16 / FP8 where the table names the row's V format, None where it is the kernel's choice (AUTO on the v2 kernel
    outside the severe rows).  severe: bool [B, Hq, Sq] of `peaked_rows` (AUTO on mixed scores), or None."""
    shape = (Sq,) if severe is None else np.asarray(severe).shape
    want = np.full(shape, None, object)
    kern = kernel_of(D, scaling)
    if precision == "fast":
        want[...] = EXPECTED_V[("fused", "fast")]
    elif precision == "accurate":
        want[...] = EXPECTED_V[("fused", "accurate", kern)]
    elif kern == "v4":
        want[...] = EXPECTED_V[("fused", "auto", "v4")]
    elif severe is not None:
        want[np.asarray(severe)] = EXPECTED_V[("fused", "auto-severe", "v2")]
    want[..., early_rows(Sq, Skv, causal)] = EXPECTED_V[("fused", "early")]
    return want


# ---- the witness values and the witness V ---------------------------------------------------------------------------------------------
def to16(a, dtype):
    """float array -> 16-bit torch tensor; every value must be exact in `dtype`"""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype)
    assert np.array_equal(t.float().numpy(), np.asarray(a, np.float32)), "witness values must be exact in bf16 and fp16"
    return t


def bits16(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def fmt16(dtype):
    return oracle.FMT_BF16 if dtype == torch.bfloat16 else oracle.FMT_FP16


def fp8_readings(v, dtype, fp8):
    """(block, head) float64: the 16-bit tensor v [B,H,S,D] as the oracle's block quantiser (one power-of-two scale per 64-key chunk) and
    its head quantiser (one fp32 scale per head) leave it"""
    b = bits16(v)
    _, _, deq = oracle.quantize_v_block(b, fmt16(dtype), FMT[fp8])
    v8, sv = oracle.quantize_fp8(b, fmt16(dtype), "head", FMT[fp8], "compiled")
    head = oracle.fp8_to_f32(v8, FMT[fp8]).astype(np.float64) * sv.astype(np.float64)[..., None, None]
    return oracle.bf16_bits_to_f32(deq).astype(np.float64), head


@functools.lru_cache(maxsize=None)
def witness_values(fp8):
    """the cycle of witness values for `fp8`: every 1 + i/128 in [1, 1.75) whose block AND head fp8 readings (next to a 1.75 in the same
    chunk) are >= SEPARATION x 2^-7 max(1, |v|) away, for bf16 and fp16 alike; ordered low / high alternately, so that neighbours in the
    cycle -- the same channel of two kv heads -- are far apart"""
    cand = 1.0 + np.arange(96) / 128.0
    keep = np.ones(len(cand), bool)
    for dtype in (torch.bfloat16, torch.float16):
        v = to16(np.broadcast_to(np.concatenate([[TOP], cand])[None, None, None, :], (1, 1, 64, 1 + len(cand))), dtype)
        for reading in fp8_readings(v, dtype, fp8):
            assert (reading[..., 0] == TOP).all(), "1.75 is on the fp8 grid of both formats"
            keep &= np.abs(reading[0, 0, 0, 1:] - cand) >= SEPARATION * bound_v16(cand)
    vals = cand[keep]
    assert len(vals) >= 8, (fp8, vals)
    half = (len(vals) + 1) // 2
    order = np.empty(len(vals))
    order[0::2], order[1::2] = vals[:half], vals[half:]
    order.setflags(write=False)
    return order


@functools.lru_cache(maxsize=None)
def witness_vectors(Hkv, D, dtype, fp8):
    """(v16 [Hkv, D], vfp8 [Hkv, D]) float64: the channel vector of every kv head and its fp8 reading.  Channel 0 is 1.75; channel c >= 1
    is (-1)^(c+1) x the witness value number (c - 1 + h) of the cycle -- the cycle is rotated by the kv-head index h."""
    vals = witness_values(fp8)
    c = np.arange(1, D)
    v16 = np.empty((Hkv, D))
    v16[:, 0] = TOP
    for h in range(Hkv):
        v16[h, 1:] = np.where(c % 2 == 1, 1.0, -1.0) * vals[(c - 1 + h) % len(vals)]
    block, head = fp8_readings(to16(np.broadcast_to(v16[None, :, None, :], (1, Hkv, 64, D)), dtype), dtype, fp8)
    assert np.array_equal(block, head), "both scales are the same power of two: the block and the head reading must be one vector"
    vfp8 = block[0, :, 0, :]
    assert (np.abs(vfp8 - v16)[:, 1:] >= SEPARATION * bound_v16(v16[:, 1:])).all()
    for h in range(Hkv):          # another kv head's vector, in either format, is neither of this head's
        for g in range(Hkv):
            if g != h:
                assert (classify(np.stack([v16[g], vfp8[g]]), v16[h], vfp8[h])[0] == NEITHER).all(), (h, g)
    v16.setflags(write=False)
    vfp8.setflags(write=False)
    return v16, vfp8


@functools.lru_cache(maxsize=None)
def witness_v(B, Hkv, Skv, D, dtype, fp8):
    """V [B, Hkv, Skv, D] (torch, `dtype`, CPU; shared: do not write to it), constant along the key axis: every key row of kv head h is
    witness_vectors(...)[0][h].  Asserts that the block-scaled and the head-scaled fp8 readings of THIS tensor are identical and equal to
    the fp8 vector (every chunk, the partial last one included, holds a 1.75)."""
    v16, vfp8 = witness_vectors(Hkv, D, dtype, fp8)
    v = to16(np.broadcast_to(v16[None, :, None, :], (B, Hkv, Skv, D)), dtype)
    block, head = fp8_readings(v, dtype, fp8)
    assert np.array_equal(block, head) and np.array_equal(block, np.broadcast_to(vfp8[None, :, None, :], block.shape))
    return v


def per_q_head(vec, Hq):
    """[Hkv, D] -> [Hq, D]: query head h attends kv head h // (Hq / Hkv)"""
    return np.repeat(np.asarray(vec), Hq // vec.shape[0], axis=0)


# ---- the classifier -------------------------------------------------------------------------------------------------------------------
def miss(out, vec, which):
    """per row: max over the channels of |out - vec| / (the bound of class `which` on vec); < 1 = the row IS of that class"""
    out, vec = np.asarray(out, np.float64), np.asarray(vec, np.float64)
    return (np.abs(out - vec) / (bound_v16(vec) if which == V16 else bound_fp8(vec))).max(-1)


def classify(out, v16_vec, vfp8_vec):
    """out [..., D]; v16_vec / vfp8_vec broadcastable to it (the vectors of each row's kv head).  Returns (labels [...], worst):
    "v16"     every channel within 2^-7 max(1, |ref|) of the 16-bit vector,
    "fp8"     every channel within 2^-6 max(1, |ref| / 2) of the fp8 vector,
    "neither" anything else;
    worst = {label: the largest |out - its vector| over the rows of that label} (neither: the distance to the nearer vector) -- to report.
    The two bounds add up to less than the 5x separation, so no row can be both (asserted)."""
    out = np.asarray(out, np.float64)
    m16, m8 = miss(out, v16_vec, V16), miss(out, vfp8_vec, FP8)
    is16, is8 = m16 < 1.0, m8 < 1.0
    assert not (is16 & is8).any(), "a row cannot be within both bounds: the vectors are >= 5 bounds apart"
    labels = np.where(is16, V16, np.where(is8, FP8, NEITHER))
    d16 = np.abs(out - np.asarray(v16_vec, np.float64)).max(-1)
    d8 = np.abs(out - np.asarray(vfp8_vec, np.float64)).max(-1)
    none = ~(is16 | is8)
    worst = {V16: float(d16[is16].max()) if is16.any() else 0.0, FP8: float(d8[is8].max()) if is8.any() else 0.0,
             NEITHER: float(np.minimum(d16, d8)[none].max()) if none.any() else 0.0}
    return labels, worst


def require(labels, out, v16_vec, vfp8_vec, want, what, rows=None):
    """every row of `rows` (default: all; bool, shape of labels) whose `want` entry is not None carries the wanted label.  On failure the
    message gives the FACTOR: the worst |out - wanted vector| / (bound of the wanted class) over the offending rows."""
    want = np.broadcast_to(np.asarray(want, object), labels.shape)
    held = np.array([w is not None for w in want.ravel()]).reshape(labels.shape)
    if rows is not None:
        held = held & np.broadcast_to(rows, labels.shape)
    bad = held & (labels != want)
    if bad.any():
        factor = np.where(want == V16, miss(out, v16_vec, V16), miss(out, vfp8_vec, FP8))
        first = np.argwhere(bad)[:4].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} row(s) do not attend the expected V (first {first}: got {labels[bad][:4].tolist()}, "
                             f"want {want[bad][:4].tolist()}); worst |out - expected vector| / bound = {float(factor[bad].max()):.2f}")


# ---- scores ---------------------------------------------------------------------------------------------------------------------------
PLANTED_SHARE = 0.10      # at most this share of a head's rows is planted: the head's moments stay those of N(0,1), no head starts precise
SEVERE_GAIN = 1.25        # q_r = 1.25 k_t: the score of key t is 1.25 sqrt(D) >= 10 against N(0, 1.25^2) elsewhere -> one key carries the row
MODERATE_R = 14.0         # q_r = g k_t with g solved per row for R = 1 / w_max = 14 on the exact data (the window asked for is 10 .. 20)


def _softmax_top(q, k, causal):
    """1 / (largest softmax weight) per row, fp64: q [Hq, Sq, D], k [Hkv, Skv, D] float64 (GQA: query head h reads kv head h // (Hq/Hkv))"""
    Hq, Sq, D = q.shape
    kk = torch.from_numpy(np.ascontiguousarray(k)).repeat_interleave(Hq // k.shape[0], dim=0)
    s = (torch.from_numpy(np.ascontiguousarray(q)) @ kk.transpose(-1, -2)) / math.sqrt(D)
    if causal:
        s = s.masked_fill(torch.ones(Sq, k.shape[1], dtype=torch.bool).triu(1), -math.inf)
    return (1.0 / torch.softmax(s, dim=-1).amax(-1)).numpy()


@functools.lru_cache(maxsize=None)
def scores_case(S, D, kind, seed, causal=False, Sq=None, Hq=4, Hkv=2):
    """(q [1, Hq, Sq, D], k [1, Hkv, S, D]) float32 torch (CPU; shared: do not write to them).
    "flat":  N(0,1).
    "mixed": N(0,1) with PLANTED_SHARE of every head's rows planted: row r becomes g k_t, t a key the row may attend (t <= r: also under
             a causal mask).  Half of them severe (g = 1.25: one key carries the row), half moderate (g solved per row, by bisection on
             the exact data under the `causal` mask, for R = 1 / w_max = 14).  |g k_t| is at most 1.25 of a normal row's norm on 5 % of
             the rows and smaller on the other 5 %: the per-head sums of squares the starting mode reads do not move."""
    Sq = S if Sq is None else Sq
    rng = np.random.default_rng(7919 * seed + 31 * S + D + (1 if causal else 0))
    q = rng.standard_normal((Hq, Sq, D))
    k = rng.standard_normal((Hkv, S, D))
    if kind == "mixed":
        n = int(Sq * PLANTED_SHARE)
        for h in range(Hq):
            rows = rng.choice(Sq, n, replace=False)
            tgt = (rng.random(n) * (np.minimum(rows, S - 1) + 1)).astype(np.int64)          # 0 <= t <= r
            kt = k[h // (Hq // Hkv), tgt]                                                   # [n, D]
            sev, mod = rows[:n // 2], rows[n // 2:]
            q[h, sev] = SEVERE_GAIN * kt[:n // 2]
            # moderate: scores of row r are g c_j, c = k_t . k_j / sqrt(D); w_max(g) grows with g
            c = kt[n // 2:] @ k[h // (Hq // Hkv)].T / math.sqrt(D)
            if causal:
                c = np.where(np.arange(S)[None, :] <= mod[:, None], c, -np.inf)
            lo, hi = np.zeros(len(mod)), np.full(len(mod), 2.0)
            for _ in range(40):
                g = 0.5 * (lo + hi)
                z = np.where(np.isfinite(c), g[:, None] * np.where(np.isfinite(c), c, 0.0), -np.inf)
                w = np.exp(z - z.max(-1, keepdims=True))
                peaked = 1.0 / (w.max(-1) / w.sum(-1)) < MODERATE_R
                lo, hi = np.where(peaked, lo, g), np.where(peaked, g, hi)
            q[h, mod] = (0.5 * (lo + hi))[:, None] * kt[n // 2:]
    else:
        assert kind == "flat", kind
    return torch.from_numpy(q[None].astype(np.float32)), torch.from_numpy(k[None].astype(np.float32))


def peaked_rows(q, k, dtype, fp8, scaling, causal):
    """(severe, moderate) bool [1, Hq, Sq] from the fp64 softmax of q, k AS QUANTISED (cast to `dtype`, then oracle.quantize_fp8 with
    head-wise / token-wise scales): R = 1 / w_max <= 4, and 10 <= R <= 20.  These rest on the oracle alone."""
    mode = "head" if scaling == "head-wise" else "token"
    deq = []
    for t in (q, k):
        x8, s = oracle.quantize_fp8(bits16(t.to(dtype)), fmt16(dtype), mode, FMT[fp8])
        deq.append(oracle.fp8_to_f32(x8, FMT[fp8]).astype(np.float64) * s.astype(np.float64).reshape(s.shape + (1,) * (4 - s.ndim)))
    R = _softmax_top(deq[0][0], deq[1][0], causal)[None]
    return R <= 4.0, (R >= 10.0) & (R <= 20.0)


# ---- the case lists: ONE place, so that the CPU test shows the counts of the very cases the GPU test runs -------------------------------
SHAPE_FULL = (1280, False)      # five query blocks, none early
SHAPE_CAUSAL = (2304, True)     # query blocks 0 .. 3 early, 4 .. 8 not
MIN_ROWS = 32                   # a mixed case holds at least this many severe and this many moderate rows outside the early blocks
# (D, scaling, dtype, fp8) of the fused entry, pruned as tests/test_gpu_probes.py prunes: every (D, scaling, dtype) on e4m3; e5m2 head-wise bf16
FUSED = [(D, s, t, "e4m3") for D in (64, 128, 256) for s in ("head-wise", "token-wise") for t in (torch.bfloat16, torch.float16)] + \
        [(D, "head-wise", torch.bfloat16, "e5m2") for D in (64, 128, 256)]
# the fused cases that also run AUTO on mixed scores: every D = 128 head-wise case (the v2 kernel: severe rows on the 16-bit V), and the
# templated kernel once per (D, scaling)
MIXED = [c for c in FUSED if kernel_of(c[0], c[1]) == "v2"] + \
        [(64, "head-wise", torch.bfloat16, "e4m3"), (256, "head-wise", torch.float16, "e4m3"), (64, "token-wise", torch.float16, "e4m3"),
         (128, "token-wise", torch.bfloat16, "e4m3"), (256, "token-wise", torch.bfloat16, "e4m3")]
MIXED_SEED = 1

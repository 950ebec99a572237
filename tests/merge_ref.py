"""The fp64 merge of attention states and the bounds a merged state is held to (tests/test_cpu_merge.py, tests/test_gpu_merge.py,
tests/test_gpu_merge_attention.py).  Written from the formula, in numpy, sharing nothing with the product:

    L = log sum_i exp(lse_i),   w_i = exp(lse_i - L),   O = sum_i w_i O_i        (partials with lse_i = -inf left out; none left: O = 0, L = -inf)

Bounds, per element (include/qattn_merge.h computes in fp32: lse_i - max rounds to half an ulp of a number below 128 -- 2^-18 --, exp and log
are good to about an ulp, at most 8 terms are summed; the margin is 2 .. 4x):
    fp32 output     |got - ref| <= 2^-16 sum_i w_i |O_i|
    16-bit output   that + half an ulp of the output format at |ref|: 2^(floor(log2 |ref|) - 8) for bf16 (7 mantissa bits), 2^(floor(log2
                    |ref|) - 11) for fp16 (10), the exponent not below the format's smallest normal one.  (Relative to |ref| that is
                    between 2^-9 and 2^-8 for bf16, 2^-12 and 2^-11 for fp16: the flat 2^-9 |ref| / 2^-12 |ref| is half an ulp only at
                    the top of a binade, and a correctly rounded result misses it everywhere below.)
    LSE             |L - L_ref| <= 2^-15 max(1, |L_ref|);  L_ref = -inf must come back as -inf
"""
import numpy as np
import torch

FORMAT = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}     # explicit mantissa bits, smallest normal exponent


def half_ulp(ref: np.ndarray, dtype) -> np.ndarray:
    """Half a unit in the last place of `dtype` at |ref| (0 for fp32: its own rounding is inside the 2^-16 term)."""
    if dtype == torch.float32:
        return np.zeros_like(ref)
    mant, emin = FORMAT[dtype]
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(ref)))
    return np.exp2(np.maximum(e, emin) - mant - 1)


def f64(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.float64).cpu().numpy()


def rows_of(lse: np.ndarray, packed: bool) -> np.ndarray:
    """A per-row figure ([B,H,S], packed: [H,total]) laid over the rows of O ([B,H,S,D], packed: [total,H,D])."""
    return (lse.T if packed else lse)[..., None]


def merge_fp64(outs, lses, packed=False):
    """outs / lses: lists of fp64 arrays.  Returns (O, L, sum_i w_i |O_i|)."""
    L_all = np.stack(lses)
    live = L_all > -np.inf
    m = L_all.max(axis=0)
    safe_m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.where(live.any(axis=0), safe_m + np.log(np.where(live, np.exp(L_all - safe_m), 0.0).sum(axis=0)), -np.inf)
    O = np.zeros_like(outs[0])
    wabs = np.zeros_like(outs[0])
    for i, o in enumerate(outs):
        with np.errstate(invalid="ignore"):
            w = np.where(live[i], np.exp(np.where(live[i], L_all[i] - np.where(np.isfinite(L), L, 0.0), 0.0)), 0.0)
        w = rows_of(w, packed)
        o = np.where(w > 0, o, 0.0)     # a partial that attended no key: its bytes are not part of the merge
        O += w * o
        wabs += w * np.abs(o)
    return O, L, wabs


FLAT_HALF_ULP = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}    # half an ulp relative to |ref| at the TOP of a binade only


def flat_ratio(got_out, ref, out_dtype):
    """Worst |out - ref| / (2^-16 sum_i w_i |O_i| + 2^-9 |ref|) (fp16: 2^-12 |ref|): reported next to the bound, never asserted -- the fp64
    reference rounded correctly to the format already exceeds it (tests/test_cpu_merge.py shows that)."""
    O, _, wabs = ref
    err = np.abs(f64(got_out) - O)
    bound = 2.0 ** -16 * wabs + FLAT_HALF_ULP[out_dtype] * np.abs(O)
    return float(np.max(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))))


def worst_ratios(got_out, got_lse, ref, out_dtype):
    """(worst |out - ref| / bound, worst |L - L_ref| / bound) of a merged state against merge_fp64's triple; <= 1 passes.  NaN anywhere, or a
    finite LSE where the reference has -inf, gives inf."""
    O, L, wabs = ref
    g, gl = f64(got_out), f64(got_lse)
    if np.isnan(g).any() or np.isnan(gl).any():
        return np.inf, np.inf
    bound = 2.0 ** -16 * wabs + half_ulp(O, out_dtype)
    err = np.abs(g - O)
    r_out = float(np.max(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))))
    finite = np.isfinite(L)
    if not np.array_equal(gl[~finite], L[~finite]):
        return r_out, np.inf
    r_lse = float(np.max(np.abs(gl[finite] - L[finite]) / (2.0 ** -15 * np.maximum(1.0, np.abs(L[finite]))), initial=0.0))
    return r_out, r_lse


def draw_states(n, shape_o, shape_l, dtypes, seed, *, empty_rows=True, device="cpu"):
    """n states with O ~ N(0, 1) in dtypes[i] and LSEs in [-64, 64]: a base per row in [-64, -36] and per-partial gaps that walk from 0 to 100
    across the partials (clipped to 64).  empty_rows: partial 1 gets -inf on every 5th row with NaN in its O rows there; every 11th row is
    empty in all partials (their O rows: NaN in partial 0, zeros elsewhere -- as the kernels leave them)."""
    g = torch.Generator().manual_seed(seed)
    packed = len(shape_l) == 2
    outs = [torch.randn(shape_o, generator=g).to(dt) for dt in dtypes]
    base = torch.rand(shape_l, generator=g) * 28 - 64
    lses = []
    for i in range(n):
        gap = torch.rand(shape_l, generator=g) * (100.0 * i / max(n - 1, 1))
        lses.append((base + gap).clamp(max=64.0).to(torch.float32))
    if empty_rows:
        flat = torch.arange(lses[0].numel()).view(shape_l)
        some, every = flat % 5 == 2, flat % 11 == 3
        over = (lambda m: m.transpose(0, 1)) if packed else (lambda m: m)
        lses[1][some] = -float("inf")
        outs[1][over(some)] = float("nan")
        for i in range(n):
            lses[i][every] = -float("inf")
            outs[i][over(every)] = float("nan") if i == 0 else 0.0
    return [o.to(device) for o in outs], [l.to(device) for l in lses]


def reference_of(outs, lses):
    return merge_fp64([f64(o) for o in outs], [f64(l) for l in lses], packed=lses[0].dim() == 2)

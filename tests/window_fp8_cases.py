"""What tests/test_cpu_window_fp8.py and tests/test_gpu_window_fp8.py share: the literal rules of the sliding-window FP8-PV entry
(include/qattn_window.h) restated in numpy, the fp64 windowed softmax both files grade against, and the membership-probe cases whose teeth
the CPU file shows and the GPU file runs (tests/probes.py, unchanged)."""
import math

import numpy as np

from tests import probes as P

TILE = 128
TWO_TERM_KEYS = 1024
ONE, TWO = 0, 1   # include/qattn.h QATTN_PATH_ONE_TERM / _TWO_TERM (literal: the header is the contract)


def alive(n, m, window):
    """bool [n, m]: row r attends key j iff r + delta - left <= j <= r + delta + right, delta = m - n (-1: unbounded)"""
    left, right = window
    d = np.arange(m, dtype=np.int64)[None, :] - np.arange(n, dtype=np.int64)[:, None] - (m - n)
    ok = np.ones((n, m), bool)
    if left >= 0:
        ok &= d >= -left
    if right >= 0:
        ok &= d <= right
    return ok


def tile_interval(n, m, left, right, t, tile=TILE):
    """[klo, khi] of tile t (rows tile t .. min(tile (t + 1), n) - 1) of a sequence with n queries and m used keys, by the header's words:
    from the first attended key of its first row with a key to the last attended key of its last row, clipped to [0, m); None when no
    row of the tile has a key."""
    delta = m - n
    rows = range(tile * t, min(tile * (t + 1), n))
    lo_of = lambda r: 0 if left < 0 else max(r + delta - left, 0)
    hi_of = lambda r: m - 1 if right < 0 else min(r + delta + right, m - 1)
    keyed = [r for r in rows if lo_of(r) <= hi_of(r)]
    if not keyed:
        return None
    return lo_of(keyed[0]), hi_of(keyed[-1])


def tile_is_one_term(n, m, left, right, t, precision, tile=TILE):
    """the literal FAST rule: one-term iff n = khi - klo + 1 >= 1024; ACCURATE: two-term; an empty interval carries the one-term code"""
    iv = tile_interval(n, m, left, right, t, tile)
    if iv is None:
        return True
    return precision == "fast" and iv[1] - iv[0] + 1 >= TWO_TERM_KEYS


def expected_path(lq, lk, Hq, window, precision):
    cols = []
    for n, m in zip(lq, lk):
        col = np.empty(n, np.uint8)
        for t in range((n + TILE - 1) // TILE):
            col[TILE * t:TILE * (t + 1)] = ONE if tile_is_one_term(n, m, window[0], window[1], t, precision) else TWO
        cols.append(col)
    return np.broadcast_to(np.concatenate(cols) if cols else np.zeros(0, np.uint8), (Hq, sum(lq)))


def window_softmax64(q, k, v, window, scale):
    """fp64 windowed softmax of ONE sequence: q [Hq, n, D], k / v [Hkv, m, D] (de-quantised, float64) -> (out [Hq, n, D], lse [Hq, n]);
    a row without a key: zeros, -inf"""
    Hq, n, D = q.shape
    Hkv, m, _ = k.shape
    if n == 0 or m == 0:
        return np.zeros((Hq, n, D)), np.full((Hq, n), -np.inf)
    rep = Hq // Hkv
    kk, vv = np.repeat(k, rep, 0), np.repeat(v, rep, 0)
    s = np.einsum("hnd,hmd->hnm", q, kk) * scale
    s = np.where(alive(n, m, window)[None], s, -np.inf)
    mx = s.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        p = np.where(np.isfinite(mx), np.exp(s - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
    l = p.sum(-1, keepdims=True)
    out = np.einsum("hnm,hmd->hnd", p / np.maximum(l, 1e-300), vv)
    with np.errstate(divide="ignore"):
        lse = np.where(l[..., 0] > 0, mx[..., 0] + np.log(np.maximum(l[..., 0], 1e-300)), -np.inf)
    return out, lse


# ---- membership probes ----------------------------------------------------------------------------------------------------------------------
# The grade on fp8-V rows is P.project_bound(ref, False) = 2^-6 max(1, |ref| / 2), and teeth are asked at 4x that: one misplaced key has to
# move an element by >= 2^-4.  The decoy and pointer probes do that at any window (a peaked row loses or gains most of its mass).  The count
# probe's n_c / n moves by about 1 / n per key: its teeth hold on NARROW windows only -- (7, 0) and (3, 4), at most 8 keys a row -- and the
# wide windows of tests/probes.py (P.WINDOWS, >= 64 keys a row) are left out for the count probe: the oracle alone does not show 4x there.
# Left out as well: the count probe on PROBE_LENS -- in that batch the neighbour sequences' adjacent keys carry the value a row's own next
# key would carry, so admitting one leaves n_c / n where it was (teeth 0 in the oracle); on PROBE_CROSS every mutant shows >= 4.6x.
PROBE_LENS = ([300, 1, 1300, 65], [300, 1, 1300, 65])
PROBE_CROSS = ([300, 1300], [1300, 1090])                       # delta > 0 and delta < 0 (leading rows without a key)
PEAKED_WINDOWS = [(1100, 0), (63, 0), (-1, 0), (3, 4)]          # decoy, pointer: ACCURATE (FAST has no rescue for peaked rows)
COUNT_WINDOWS = [(7, 0), (3, 4)]                                # count: flat rows, both precisions
PROBE_DTYPE = "bf16"


def probe_cases(D):
    """[(probe, window, lq, lk)] run on the GPU; tests/test_cpu_window_fp8.py shows the teeth of each"""
    out = []
    for lq, lk in (PROBE_LENS, PROBE_CROSS):
        out += [(probe, w, lq, lk) for probe in ("decoy", "pointer") for w in PEAKED_WINDOWS]
        if (lq, lk) == PROBE_CROSS:
            out += [("count", w, lq, lk) for w in COUNT_WINDOWS]
    return out


def make_probe(probe, D, window, lq, lk):
    Hq, Hkv = P.heads("window", probe)
    return P.make_case(probe, D, lq, lk, kind="window", arg=window, Hq=Hq, Hkv=Hkv)


def count_teeth_fp8(seq, mutants):
    """{mutant: teeth} of the count probe against the fp8-V bound: the closed form against the fp64 softmax under the wrong mask"""
    ref, _ = P.count_expected(seq.mask, seq.dims[4])
    ref = np.broadcast_to(ref, (seq.dims[0],) + ref.shape[1:])
    res = {}
    for name, mm in mutants.items():
        rows = P.touched_rows(seq.mask, mm)
        if not rows.any():
            continue
        mut, _ = seq.softmax(np.broadcast_to(mm, (mm.shape[0],) + seq.mask.shape[1:]))
        res[name] = P.teeth(ref, mut, P.project_bound(ref, False), rows)
    return res


def case_teeth(case):
    """{(sequence, mutant): teeth} of a probe case against the fp8-V bound"""
    res = {}
    for i, (s, aux, mut) in enumerate(zip(case.seqs, case.aux, case.mutants)):
        if s.dims[2] == 0 or s.m == 0:
            continue
        if case.probe == "count":
            r = count_teeth_fp8(s, mut)
        elif case.probe == "decoy":
            r = P.decoy_teeth(s, aux, False) if (aux >= 0).any() else {}
        else:
            others = {"kv head off by one": (np.roll(s.k, 1, 0), np.roll(s.v, 1, 0))} if s.dims[1] > 1 else {}
            r = P.pointer_teeth(s, aux, False, others)
        res.update({(i, name): t for name, t in r.items()})
    return res


assert math.isclose(P.TOL, 2.0 ** -6)

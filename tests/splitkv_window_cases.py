"""What tests/test_cpu_splitkv_window.py and the GPU tests of the sliding-window split-KV entries share, restated from
include/qattn_splitkv_window.h and NOT imported from the product: the interval, the split plan, the tile range and the token mask as
literal integer rules; an fp64 per-row reference that walks (kv head, tile, split) as the kernel does and returns the partials, the merged
state and the path bytes; the named wrong masks (mutants) a test of the window must expose; the membership-probe cases; the oracle
cases; and the page count a window lets a paged cache forget."""
import math

import numpy as np

from tests import probes as PR

TILE, BLOCK, CHUNK = 128, 128, 64
TWO_TERM_KEYS = 1024
PATH_ONE_TERM, PATH_TWO_TERM = 0, 1
LSE_TOL = 2e-3                     # the split-KV tests' own LSE tolerance (include/qattn.h: the FP8 sweeps other than D = 128 head-wise dense)

# ---- the membership probes (tests/probes.py) through the three window entries
PROBE_LQ = [1, 5, 40, 130]         # a decode, a speculative step, a tile that crosses heads, Sq > L
PROBE_LK = [1100, 1280, 65, 300]
PROBE_WINDOWS = [(0, 0), (63, 0), (64, 0), (200, 0), (1050, 0), (1024, 37), (-1, 0), (300, -1)]
PROBE_HQ, PROBE_HKV = 4, 2

# ---- the fp64-oracle cases of the GPU test at GQA 4, three splits, page size 128: (Sq, L, window, where the lower edge lo = L - Sq - left lies)
ORACLE_CASES = [
    (5, 1100, (1000, 0), "inside a chunk: lo = 95"),
    (5, 1100, (1031, 0), "on a chunk boundary: lo = 64"),
    (5, 1100, (967, 0), "on a page boundary: lo = 128"),
    (5, 1280, (253, 0), "on a split boundary: lo = 1022, splits cut at 1024 -- position 2's edge is split 1's first key, 3 and 4 have no key in split 0"),
    (4, 1280, (892, 0), "on a split boundary by blocks: lo = 384 = 128 kb0, the interval's first block is whole"),
    (8, 1280, (1100, 0), "more than 1024 keys in the window: lo = 172"),
    (40, 300, (100, 20), "both edges inside chunks, a tile that crosses heads: lo = 160"),
]


def cdiv(a, b):
    return -(-a // b)


def clamp(x, lo, hi):
    return min(max(x, lo), hi)


# ---- the literal rules -------------------------------------------------------------------------------------------------------------------
def interval_lo(L, Sq, left):
    """lo_i: no position of the sequence attends a key below it"""
    return 0 if left < 0 else clamp(L - Sq - left, 0, L)


def plan(L, Sq, left, ns):
    """[(k_begin, k_end)] of the ns splits: the key blocks of the interval [lo_i, L)"""
    kb0 = interval_lo(L, Sq, left) >> 7
    nkb = cdiv(L, BLOCK) - kb0
    per = cdiv(nkb, ns)
    return [(min(BLOCK * (kb0 + s * per), L), min(BLOCK * (kb0 + (s + 1) * per), L)) for s in range(ns)]


def plan_without_window(L, ns):
    """include/qattn_splitkv.h's plan: what `plan` must be at left = -1"""
    nkb = cdiv(L, BLOCK)
    per = cdiv(nkb, ns)
    return [(min(BLOCK * s * per, L), min(BLOCK * (s + 1) * per, L)) for s in range(ns)]


def tile_positions(tile, G, Sq):
    """(r_first, r_last, smin, smax) of tile `tile` of a kv head's G Sq packed rows (row r = head r // Sq at position r % Sq)"""
    r0, r1 = tile * TILE, min((tile + 1) * TILE, G * Sq) - 1
    if r0 // Sq != r1 // Sq:
        return r0, r1, 0, Sq - 1
    return r0, r1, r0 % Sq, r1 % Sq


def tile_range(k_begin, k_end, smin, smax, L, Sq, window):
    """(klo, khi, keys) of a workgroup"""
    left, right = window
    delta = L - Sq
    klo = max(k_begin, 0 if left < 0 else max(smin + delta - left, 0))
    khi = min(k_end - 1, L - 1 if right < 0 else smax + delta + right)
    return klo, khi, max(khi - klo + 1, 0)


def row_bounds(p, L, Sq, window):
    """(lo, hi) of position p: the keys lo <= j <= hi (already cut to [0, L))"""
    left, right = window
    delta = L - Sq
    return (0 if left < 0 else max(p + delta - left, 0)), (L - 1 if right < 0 else min(L - 1, p + delta + right))


def alive(Sq, L, window, M=None):
    """bool [Sq, M]: the keys every position attends (M >= L columns)"""
    M = L if M is None else M
    out = np.zeros((Sq, M), bool)
    for p in range(Sq):
        lo, hi = row_bounds(p, L, Sq, window)
        if hi >= lo:
            out[p, lo:hi + 1] = True
    return out


def dead_pages(L, left, page_size, num_queries=1):
    return max(L - num_queries - left, 0) // page_size


def window_keys(Skv, Sq, left):
    """the key count the num_splits = 0 rule sees"""
    return Skv if left < 0 else min(Skv, left + Sq + 127)


# ---- the named wrong masks ------------------------------------------------------------------------------------------------------------------
def wrong_masks(Sq, L, G, window, ns, M):
    """{name: bool [G, Sq, M]} over a universe of M >= L columns, for one kv head's G query heads: ways a window kernel can be wrong that
    the band mutants of tests/probes.py (edges off by one) do not name.  A mutant that equals the right mask on this shape is left out."""
    left, right = window
    right_mask = np.broadcast_to(alive(Sq, L, window, M), (G, Sq, M))
    out = {}
    # delta taken top-left (0) instead of L - Sq
    m = np.zeros((Sq, M), bool)
    for p in range(Sq):
        lo, hi = (0 if left < 0 else max(p - left, 0)), (L - 1 if right < 0 else min(L - 1, p + right))
        if hi >= lo:
            m[p, lo:hi + 1] = True
    out["delta top-left"] = np.broadcast_to(m, (G, Sq, M))
    if left >= 0:
        lo_i = interval_lo(L, Sq, left)
        # the split plan cuts [0, L) -- blocks counted from 0 -- while the block count is the interval's: the keys behind 128 ns per are lost
        kb0 = lo_i >> 7
        per = cdiv(cdiv(L, BLOCK) - kb0, ns)
        m = right_mask.copy()
        m[..., BLOCK * ns * per:] = False
        out["plan from key 0 with the interval's block count"] = m
        # the tile's klo as every row's lower edge
        m = right_mask.copy()
        for tile in range(cdiv(G * Sq, TILE)):
            r0, r1, smin, smax = tile_positions(tile, G, Sq)
            klo = max(smin + (L - Sq) - left, 0)
            for r in range(r0, r1 + 1):
                g, p = r // Sq, r % Sq
                _, hi = row_bounds(p, L, Sq, window)
                if hi >= klo:
                    m[g, p, klo:hi + 1] = True
        out["the tile's klo as every row's lower edge"] = m
        # the first chunk dropped when lo_i is no multiple of 64
        if lo_i % CHUNK:
            m = right_mask.copy()
            m[..., lo_i:(lo_i // CHUNK + 1) * CHUNK] = False
            out["first chunk dropped"] = m
    return {k: v for k, v in out.items() if not np.array_equal(v, right_mask)}


# ---- the fp64 reference: (kv head, tile, split), as the kernel walks ---------------------------------------------------------------------------
def reference(q, k, v, L, window, ns, sm_scale, precision="accurate"):
    """q float64 [Hq, Sq, D], k / v float64 [Hkv, Skv, D] (de-quantised), L used keys.  Returns (out [Hq, Sq, D], lse [Hq, Sq], partial_o
    [ns, Hq, Sq, D], partial_lse [ns, Hq, Sq], partial_path uint8 [ns, Hq, Sq], row_path uint8 [Hq, Sq]): per (kv head, tile, split) the
    workgroup's key range, per row its own bounds inside it, one softmax per row and split, then the merge by the LSEs.  A row without a
    key in a split: zeros, -inf, ONE_TERM."""
    Hq, Sq, D = q.shape
    Hkv = k.shape[0]
    G = Hq // Hkv
    po = np.zeros((ns, Hq, Sq, D))
    pl = np.full((ns, Hq, Sq), -np.inf)
    pp = np.full((ns, Hq, Sq), PATH_ONE_TERM, np.uint8)
    splits = plan(L, Sq, window[0], ns)
    for hkv in range(Hkv):
        for tile in range(cdiv(G * Sq, TILE)):
            r0, r1, smin, smax = tile_positions(tile, G, Sq)
            for s, (kb, ke) in enumerate(splits):
                klo, khi, keys = tile_range(kb, ke, smin, smax, L, Sq, window)
                code = PATH_ONE_TERM if (keys == 0 or (precision == "fast" and keys >= TWO_TERM_KEYS)) else PATH_TWO_TERM
                for r in range(r0, r1 + 1):
                    h, p = hkv * G + r // Sq, r % Sq
                    pp[s, h, p] = code
                    if keys == 0:
                        continue
                    lo, hi = row_bounds(p, L, Sq, window)
                    lo, hi = max(lo, klo), min(hi, khi)
                    if hi < lo:
                        continue
                    sc = (k[hkv, lo:hi + 1] @ q[h, p]) * sm_scale
                    mx = sc.max()
                    e = np.exp(sc - mx)
                    po[s, h, p] = (e / e.sum()) @ v[hkv, lo:hi + 1]
                    pl[s, h, p] = mx + math.log(e.sum())
    with np.errstate(invalid="ignore"):
        top = pl.max(0)
        w = np.where(np.isneginf(pl), 0.0, np.exp(pl - np.where(np.isneginf(top), 0.0, top)[None]))
    tot = w.sum(0)
    out = (w[..., None] * po).sum(0) / np.maximum(tot, 1e-300)[..., None]
    with np.errstate(divide="ignore"):
        lse = np.where(tot > 0, top + np.log(np.maximum(tot, 1e-300)), -np.inf)
    live = ~np.isneginf(pl)
    one = (live & (pp == PATH_ONE_TERM)).any(0)
    path = np.where(~live.any(0) | one, PATH_ONE_TERM, PATH_TWO_TERM).astype(np.uint8)
    return out, lse, po, pl, pp, path


def probe_case(probe, D, window):
    return PR.make_case(probe, D, PROBE_LQ, PROBE_LK, kind="window", arg=window, Hq=PROBE_HQ, Hkv=PROBE_HKV)

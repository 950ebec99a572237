"""What tests/test_cpu_tree_window.py and the GPU tests of the tree under a sliding window share, restated from
include/qattn_paged_varlen_tree_window.h and NOT imported from the product: the cases (tests/tree_cases.CASES and one more), the windows,
the rule with its named mutants, the plan's key count per work item, and an fp64 per-row reference with sinks that walks the kernel's
own work items (kv head, tile slot, row) as tests/tree_cases.reference does."""
import numpy as np
import torch

import quantumattention_amd as qa
from tests import paged_cases as P
from tests import paged_varlen_cases as V
from tests import tree_cases as T

B, HKV, CAP = T.B, T.HKV, T.CAP
TILE = V.TILE
MASK64 = T.MASK64

# tree_cases' A .. D, and
#   E  G = 3 with 60 drafts: 180 packed rows, the second tile (rows 128 .. 179) lies inside the third head at positions 8 .. 59 -- its
#      least DEPTH is not 0 and, on a tree, not 8; 33 drafts behind 1167 committed keys (delta > 1100 + 63); 5 drafts at delta 65
CASES = dict(T.CASES)
CASES["E"] = (3, (60, 33, 5), (400, 1200, 70))
WINDOWS = ((63, 0), (127, 0), (300, 0), (1100, 0), (-1, 0))
KINDS = T.KINDS
# One slot, G = 3 with 60 drafts (E's tile geometry), on a cache of its own -- (keys, capacity, page size, window_left, num_splits): in split 0
# the head-interior tile (positions 8 .. 59) sweeps 1022 keys counted from its least depth on a chain (depth = position: 8), 1030 counted
# from depth 0, 1029 on a star (depth 1); the tile that crosses the head boundaries sweeps 1030.  FAST's selection (>= 1024 keys: the
# one-term launch) is straddled: a reduction that starts the tile at depth 0, or at its least POSITION on a tree, flips the path byte.
STRADDLE_G, STRADDLE_SQ = 3, 60
STRADDLE = ((1200, 1280, 128, 970, 1), (2200, 2304, 128, 2018, 2))
TWO_TERM_KEYS = 1024


def tile_positions(G, n, tile):
    """positions of the valid rows of a tile of a kv head's G n packed rows"""
    return [r % n for r in range(tile * TILE, min((tile + 1) * TILE, G * n))]


def check_cases():
    """what the issue asks of the shapes"""
    T.check_cases()
    G, sq, lens = CASES["E"]
    assert (G, sq[0]) == (3, 60) and tile_positions(G, sq[0], 1) == list(range(8, 60)), "E's second tile lies inside one head at positions 8 .. 59"
    slots = [(n, L) for _, sq, lens in CASES.values() for n, L in zip(sq, lens)]
    lefts = [left for left, _ in WINDOWS if left >= 0]
    for left in lefts:   # the window bites on committed keys at every depth
        assert any(1 <= n <= 64 and L - n > left + 63 for n, L in slots), left
    # lo_i inside a chunk: the V-head zeroing runs
    assert any(1 <= n <= 64 and 0 < L - n - left < 64 for n, L in slots for left in lefts)
    # an interval of >= 1024 keys: FAST's byte sweep without sinks
    assert any(n >= 1 and L - max(L - n - left, 0) >= 1024 for n, L in slots for left in lefts)
    assert any(0 < L < n for n, L in slots) and any(L == 0 and n > 0 for n, L in slots)
    assert all(L <= CAP for _, L in slots)
    # the straddle shapes: the head-interior tile's key count in split 0 lies on either side of 1024 by what its least depth is taken to be
    G, n = STRADDLE_G, STRADDLE_SQ
    assert tile_positions(G, n, 1) == list(range(8, 60))
    chain, star = T.words_of_parents([p - 1 for p in range(n)]), T.words_of_parents([-1] + [0] * (n - 1))
    for L, cap, ps, left, ns in STRADDLE:
        assert L <= cap and cap % ps == 0 and left >= 63
        keys = lambda words, tile, mutant=None: tile_keys(words, 0, n, L, G, tile, left, ns, 0, mutant)[2]
        assert keys(chain, 1) == 1022 and keys(chain, 1, "tile from depth 0") == 1030 and keys(chain, 0) == 1030, (L, left, ns)
        assert keys(star, 1) == 1029 and keys(star, 1, "tile by position") == 1022 and keys(star, 0) == 1030, (L, left, ns)


def fast_path_code(keys, one_term, two_term):
    """the path byte of a work item under precision="fast": the one-term sweep iff it sweeps no key or at least 1024"""
    return one_term if keys == 0 or keys >= TWO_TERM_KEYS else two_term


def tables(name, page_size, seed=0, lens=None):
    lens = CASES[name][2] if lens is None else tuple(lens)
    return P.Tables(page_size, lens, seed=seed, need=[-(-L // page_size) for L in lens])


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("depth=index", "depth counts self", "window on drafts by index", "lo+1", "lo-1", "depth of another row")
# ... and of the plan (tile_keys): they move no output value -- the chunks they add or drop hold masked keys only, or none on a chain --
# but the key count, FAST's selection and the path byte: held on the STRADDLE shapes
PLAN_MUTANTS = ("tile from depth 0", "tile by position")


def depth_of(words, start, n, p, mutant=None):
    """depth_p = popcount(w_p & (2^p - 1)) in a slot with at most 64 queries, p in a longer one"""
    if n > 64 or mutant == "depth=index":
        return p
    at = start + p
    if mutant == "depth of another row":
        at = start + (p + 1) % n
    w = words[at] & MASK64
    below = (2 << p) - 1 if mutant == "depth counts self" else (1 << p) - 1
    return bin(w & below).count("1")


def row_keep(words, start, n, L, r, M, left, mutant=None):
    """bool [M]: the keys packed row r (head r // n, position r % n) of a slot attends under window (left, 0) -- the rule of
    include/qattn_paged_varlen_tree_window.h, literally; mutant: one of MUTANTS."""
    keep = T.row_keep(words, start, n, L, r, M)          # 1. the tree entry's rule
    if left < 0:
        return keep
    p, delta = r % n, L - n
    j = np.arange(M)
    lo = delta + depth_of(words, start, n, p, mutant) - left + {"lo+1": 1, "lo-1": -1}.get(mutant, 0)
    if n > 64:                                           # a prefill chunk: the window entry's slot
        return keep & (j >= lo)
    if mutant == "window on drafts by index":
        return keep & (j >= delta + p - left)
    return keep & ((j >= lo) | (j >= delta))             # 2. committed keys by depth; 3. draft keys: no window test


def slot_mask(words, start, n, L, G, M, left, mutant=None):
    """bool [HKV G, n, M] of one slot"""
    one = np.stack([row_keep(words, start, n, L, r, M, left, mutant) for r in range(G * n)]).reshape(G, n, M)
    return np.tile(one, (HKV, 1, 1))


# ---- the plan: the keys a work item sweeps ----------------------------------------------------------------------------------------------
def tile_keys(words, start, n, L, G, tile, left, ns, s, mutant=None):
    """(klo, khi, keys) of (tile, split s) of a slot: the window entry's plan with the least DEPTH of the tile's rows at the lower end.
    mutant 'tile from depth 0': the least depth taken as 0 (right for a tile that holds a row of position 0, wrong inside a head);
    'tile by position': the least position."""
    delta = L - n
    lo_i = 0 if left < 0 else min(max(delta - left, 0), L)
    kb0 = lo_i // 128
    nkb = -(-L // 128) - kb0
    per = -(-nkb // ns)
    k_begin, k_end = 128 * (kb0 + s * per), min(128 * (kb0 + (s + 1) * per), L)
    pos = tile_positions(G, n, tile)
    dmin = min(depth_of(words, start, n, p) for p in pos)
    if mutant == "tile from depth 0":
        dmin = 0
    if mutant == "tile by position":
        dmin = min(pos)
    klo = max(k_begin, 0 if left < 0 else min(max(dmin + delta - left, 0), L))
    khi = min(k_end - 1, min(max(max(pos) + delta, -1), L - 1))
    return klo, khi, max(khi - klo + 1, 0)


# ---- the fp64 reference -------------------------------------------------------------------------------------------------------------------
def reference(q, k, v, lens, sq, G, words, sm_scale, left, sinks=None, mutant=None):
    """tests/tree_cases.reference under the window (left, 0) and, optionally, sinks [Hq] (float64; -inf: none): L = log(exp(sink_h) +
    sum_j exp(x_j)).  A row without a key is a zero row with LSE -inf, with a sink LSE sink_h."""
    total_q, Hq, D = q.shape
    nB, cu = len(lens), V.cu_of(sq)
    out, lse = np.full((total_q, Hq, D), np.nan), np.full((Hq, total_q), np.nan)
    for hkv in range(Hq // G):
        for jt in range(V.num_slots(G, total_q, nB)):
            hit = V.slot_to_tile(jt, cu, G, total_q, nB)
            if hit is None:
                continue
            i, tile = hit
            start, n, L = cu[i], sq[i], lens[i]
            for r in range(tile * TILE, min((tile + 1) * TILE, G * n)):
                tok, head = start + r % n, hkv * G + r // n
                snk = -np.inf if sinks is None else float(sinks[head])
                keep = row_keep(words, start, n, L, r, max(L, 1), left, mutant)[:L]
                if not keep.any():
                    out[tok, head], lse[head, tok] = 0.0, snk
                    continue
                s = (k[i, hkv, :L][keep] @ q[tok, head]) * sm_scale
                m = max(s.max(), snk)
                p = np.exp(s - m)
                den = p.sum() + np.exp(snk - m)
                out[tok, head] = (p / den) @ v[i, hkv, :L][keep]
                lse[head, tok] = m + np.log(den)
    return out, lse


# ---- the straddle shapes ------------------------------------------------------------------------------------------------------------------
def straddle_setup(L, cap, ps, D, dtype, device, seed=0):
    """(cache, q, cu): ONE slot with STRADDLE_SQ queries over L random keys on a cache of capacity cap (a shuffled table of its own, two
    spare pages), appended through the packed append; q [STRADDLE_SQ, HKV STRADDLE_G, D]"""
    M = cap // ps
    g = torch.Generator().manual_seed(900 + seed)
    sk = torch.tensor([[0.05, 0.08]])
    c = qa.alloc_paged_kv_cache_fp8(M + 2, HKV, ps, D, batch_size=1, max_pages_per_seq=M, scale_k=sk.to(device), scale_v=(2 * sk).to(device),
                                    dtype=dtype, device=device)
    c.block_table.copy_(torch.randperm(M + 2, generator=g)[:M].view(1, M).to(torch.int32))
    k, v = ((torch.randn(L, HKV, D, generator=g)).to(dtype).to(device) for _ in range(2))
    qa.paged_kv_cache_append_varlen_fp8(c, k, v, torch.tensor([0, L], dtype=torch.int32, device=device))
    q = (torch.randn(STRADDLE_SQ, HKV * STRADDLE_G, D, generator=g) * 1.5).to(dtype).to(device)
    return c, q, torch.tensor([0, STRADDLE_SQ], dtype=torch.int32, device=device)


def straddle_words(kind):
    n = STRADDLE_SQ
    return T.words_of_parents([p - 1 for p in range(n)] if kind == "chain" else [-1] + [0] * (n - 1))


def straddle_codes(kind, L, left, ns, one_term, two_term):
    """uint8 numpy [ns, HKV STRADDLE_G, STRADDLE_SQ]: the path byte of every row under precision="fast", from tile_keys"""
    G, n = STRADDLE_G, STRADDLE_SQ
    words = straddle_words(kind)
    out = np.zeros((ns, HKV * G, n), np.uint8)
    for s in range(ns):
        for tile in range(-(-G * n // TILE)):
            code = fast_path_code(tile_keys(words, 0, n, L, G, tile, left, ns, s)[2], one_term, two_term)
            for r in range(tile * TILE, min((tile + 1) * TILE, G * n)):
                out[s, [hkv * G + r // n for hkv in range(HKV)], r % n] = code
    return out

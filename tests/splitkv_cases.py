"""What tests/test_cpu_splitkv.py and the two tests/test_gpu_splitkv*.py files share: the literal rules of the split-KV entry
(include/qattn_splitkv.h) restated in plain Python -- the split plan, the keys a workgroup sweeps, the FAST rule, the path bytes -- an
fp64 softmax over the used keys, and the membership-probe cases (tests/probes.py, unchanged) whose teeth the CPU file shows and the GPU
file runs.  Nothing here imports a rule from the product."""
import math

import numpy as np

from tests import probes as P

TILE = 128             # packed query rows per workgroup
BLOCK = 128            # keys per key block
TWO_TERM_KEYS = 1024
ONE, TWO = 0, 1        # include/qattn.h QATTN_PATH_ONE_TERM / _TWO_TERM (literal: the header is the contract)
LSE_TOL = 2e-3


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the split plan and the FAST rule, written out ----------------------------------------------------------------------------------------
def split_keys(L, ns, s):
    """[lo, hi): the keys split s of ns owns of a batch element with L used keys -- nkb = ceil(L / 128) key blocks, per = ceil(nkb / ns) of
    them per split, split s the blocks [s per, min((s + 1) per, nkb)); lo = hi: the split owns nothing"""
    nkb = cdiv(L, BLOCK)
    per = cdiv(nkb, ns)
    first, last = s * per, min((s + 1) * per, nkb)
    if first >= last:
        return 0, 0
    return BLOCK * first, min(BLOCK * last, L)


def tile_positions(G, Sq, t):
    """positions (r mod Sq) of the valid packed rows of tile t of a kv head's G Sq packed rows"""
    return [r % Sq for r in range(TILE * t, min(TILE * (t + 1), G * Sq))]


def keys_swept(L, Sq, G, ns, s, t, causal):
    """how many keys the workgroup (tile t, split s) sweeps: its split's keys, cut at L and -- causal, position p attends the keys
    j <= p + L - Sq -- at the largest key any valid row of the tile attends"""
    lo, hi = split_keys(L, ns, s)
    if causal:
        hi = min(hi, max(tile_positions(G, Sq, t)) + L - Sq + 1)
    return max(hi - lo, 0)


def workgroup_code(L, Sq, G, ns, s, t, causal, precision):
    """the path byte a workgroup stores: FAST one-term iff it sweeps >= 1024 keys, ACCURATE two-term; a workgroup that sweeps nothing
    carries the one-term code"""
    n = keys_swept(L, Sq, G, ns, s, t, causal)
    return ONE if n == 0 or (precision == "fast" and n >= TWO_TERM_KEYS) else TWO


def partial_paths(used, Hq, Hkv, Sq, ns, causal, precision):
    """uint8 [ns, B, Hq, Sq]: the path byte of every (split, row)"""
    G = Hq // Hkv
    out = np.empty((ns, len(used), Hkv, G * Sq), np.uint8)
    for s in range(ns):
        for b, L in enumerate(used):
            for t in range(cdiv(G * Sq, TILE)):
                out[s, b, :, TILE * t:TILE * (t + 1)] = workgroup_code(L, Sq, G, ns, s, t, causal, precision)
    return out.reshape(ns, len(used), Hq, Sq)


def row_keys(L, Sq, ns, s, p, causal):
    """[lo, hi): the keys of split s that the row at position p attends"""
    lo, hi = split_keys(L, ns, s)
    if causal:
        hi = min(hi, p + L - Sq + 1)
    return (lo, hi) if hi > lo else (0, 0)


def expected_row_path(used, Hq, Hkv, Sq, ns, causal, precision):
    """uint8 [B, Hq, Sq]: ns = 1 -- the workgroup's own code; ns > 1 -- ONE_TERM if a split that gave the row a key ran one-term, else
    TWO_TERM; a row without a key in any split: ONE_TERM"""
    pp = partial_paths(used, Hq, Hkv, Sq, ns, causal, precision)
    if ns == 1:
        return pp[0]
    out = np.empty(pp.shape[1:], np.uint8)
    for b, L in enumerate(used):
        for p in range(Sq):
            live = [s for s in range(ns) if row_keys(L, Sq, ns, s, p, causal) != (0, 0)]
            for h in range(Hq):
                out[b, h, p] = ONE if (not live or any(pp[s, b, h, p] == ONE for s in live)) else TWO
    return out


# ---- fp64 reference ---------------------------------------------------------------------------------------------------------------------
def softmax64(q, k, v, used, causal, scale, key_range=None):
    """fp64 attention of de-quantised q [B, Hq, Sq, D] over k / v [B, Hkv, Skv, D]: batch element b attends its first used[b] keys, causal
    bottom-right; key_range(b) -> (lo, hi) restricts the keys further.  (out [B, Hq, Sq, D], lse [B, Hq, Sq]); no key: zeros, -inf"""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    out, lse = np.zeros((B, Hq, Sq, D)), np.full((B, Hq, Sq), -np.inf)
    j = np.arange(Skv)[None, :]
    p = np.arange(Sq)[:, None]
    for b in range(B):
        L = used[b]
        ok = np.broadcast_to(j < L, (Sq, Skv)).copy()
        if causal:
            ok &= j <= p + (L - Sq)
        if key_range is not None:
            lo, hi = key_range(b)
            ok &= (j >= lo) & (j < hi)
        kk, vv = np.repeat(k[b], Hq // Hkv, 0), np.repeat(v[b], Hq // Hkv, 0)
        s = np.where(ok[None], np.einsum("hnd,hmd->hnm", q[b], kk) * scale, -np.inf)
        mx = s.max(-1, keepdims=True)
        live = np.isfinite(mx)
        with np.errstate(invalid="ignore"):
            e = np.where(live, np.exp(s - np.where(live, mx, 0.0)), 0.0)
        l = e.sum(-1, keepdims=True)
        out[b] = np.einsum("hnm,hmd->hnd", e / np.maximum(l, 1e-300), vv)
        with np.errstate(divide="ignore"):
            lse[b] = np.where(l[..., 0] > 0, mx[..., 0] + np.log(np.maximum(l[..., 0], 1e-300)), -np.inf)
    return out, lse


# ---- membership probes ---------------------------------------------------------------------------------------------------------------------
# One batch element, Sq rows against `alloc` allocated keys of which `used` are used (used < alloc: the key at seqused_k is a decoy of the
# universe, tests/probes.py NEXT).  (Sq, alloc, used, ns, causal): 1100 keys = 9 key blocks, the last 76 keys; ns = 3 -> splits of 3 blocks,
# ns = 9 -> one block each (the merge chain); 1036 of 1100: the cut falls into the last block.  Sq = 5 keeps the count probe's rows short
# of keys on nobody's account -- its teeth come from n_c / n, which one key in 1100 moves by 1 / 9 of an element (D = 128).
PROBE_SHAPES = [(5, 1100, 1100, 3, False), (5, 1100, 1100, 9, True), (5, 1100, 1036, 3, True), (130, 1100, 1036, 9, False)]
PROBE_HEADS = {"count": (4, 1), "decoy": (4, 2), "pointer": (4, 2)}   # G = 4 / G = 2: packed rows of several heads in one tile


def make_probe(probe, D, Sq, alloc, used, causal):
    Hq, Hkv = PROBE_HEADS[probe]
    return P.make_case(probe, D, [Sq], [alloc], [used], kind="window" if causal else "full", arg=(-1, 0) if causal else None, Hq=Hq, Hkv=Hkv)


def boundary_chunks(L, ns):
    """the 64-key chunks on both sides of every split boundary (and the last chunk)"""
    nch = cdiv(L, 64)
    out = {nch - 1}
    for s in range(1, ns):
        lo, hi = split_keys(L, ns, s)
        if hi > lo:
            out |= {lo // 64 - 1, lo // 64}
    return sorted(c for c in out if 0 <= c < nch)


def boundary_targets(seq, L, ns):
    """pointer targets [Hq or 1, n]: row r points at a key beside a split boundary (the last key of a split, the first of the next),
    cycling through the boundaries; a key the row's mask forbids falls back to the row's last key (no key: -1)"""
    keys = []
    for s in range(1, ns):
        lo, hi = split_keys(L, ns, s)
        if hi > lo:
            keys += [lo - 1, lo]
    keys.append(L - 1)
    mask = seq.mask
    H, n, M = mask.shape
    pick = np.asarray(keys)[np.arange(n) % len(keys)][None, :].repeat(H, 0)
    last = M - 1 - mask[..., ::-1].argmax(-1)
    ok = np.take_along_axis(mask, pick[..., None], -1)[..., 0]
    return np.where(mask.any(-1), np.where(ok, pick, last), -1)


def boundary_pointer_seq(D, Sq, alloc, used, ns, causal):
    """(seq, targets): the pointer probe's sequence with its rows re-pointed at the keys beside the split boundaries (same keys, values and
    mask as make_probe("pointer", ...); q = 2 u[target])"""
    base = make_probe("pointer", D, Sq, alloc, used, causal).seqs[0]
    targets = boundary_targets(base, used, ns)
    q = P.code_q(base.k, targets, base.q.shape[0], gain=2.0)
    return P.Seq(q, base.k, base.v, base.mask, base.m, base.extras), targets


def split_mutants(seq, L, ns):
    """the named wrong masks of a split-KV problem on ONE sequence: a 64-key chunk dropped on either side of every split boundary, the
    causal edge moved by +-1 and the padding admitted (P.band_mutants, in the case already), seqused_k off by one in both directions"""
    mut = {k: v for k, v in P.chunk_drop_mutants(seq.mask, seq.m, boundary_chunks(L, ns)).items()}
    rows = seq.mask.any(-1)
    mm = seq.mask.copy()
    mm[..., L - 1] = False
    mut["seqused_k - 1"] = mm
    if P.NEXT in seq.extras:
        mm = seq.mask.copy()
        mm[..., seq.extras[P.NEXT]] |= rows     # (the universe keeps the key at seqused_k in this column)
        mut["seqused_k + 1"] = mm
    return mut


def dense_tensors(case, Sq, alloc):
    """q [1, Hq, Sq, D], k / v [1, Hkv, alloc, D] float64 of a one-sequence case"""
    f = lambda t, S: np.ascontiguousarray(t.reshape(1, S, t.shape[1], t.shape[2]).transpose(0, 2, 1, 3))
    return f(case.q, Sq), f(case.k, alloc), f(case.v, alloc)


def dense_reference(case, Sq):
    """(ref [1, Hq, Sq, D], ref_lse [1, Hq, Sq]) of a one-sequence case"""
    ref, lse = case.reference()
    return ref.transpose(1, 0, 2)[None], lse[None]


assert math.isclose(P.LSE_TOL, LSE_TOL)

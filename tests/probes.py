"""Exact-answer membership probes: inputs whose correct attention output is known exactly (or to fp64) and on which ONE misplaced key
moves the output by many times the bound ("Membership probes").  Plain numpy / torch-CPU helpers shared by
tests/test_cpu_probes.py (closed forms, quantisation exactness, teeth) and tests/test_gpu_probes.py (the kernels).

Every probe value is one of 0, +-0.5, +-1, +-1.5, 2: exactly representable in e4m3, e5m2, bf16 and fp16.  K, V and the code queries hold
+-1 / 0 only, so head-wise and token-wise quantisation return them unchanged and ONE fp64 reference per (probe, shape) serves every
dtype, fp8 format, scaling and precision.  The one exception is stated where it arises: the count probe's q rows with g = 1.5 under
HEAD-wise scales (head abs-max 2: 1.5 lands on 336 = a tie between the e4m3 neighbours 320 and 352) -- the row stays a constant vector,
so every key of the row still has one score, the output n_c / n does not depend on it, and the expected LSE reads the quantised q.

A problem is a list of SEQUENCES (`Seq`): q [Hq, n, D], the key universe k / v [Hkv, M, D] -- the sequence's own m keys first, then the
keys a faulty kernel could reach (zero padding up to the next multiple of 64, a neighbour sequence's adjacent keys, the key at
seqused_k) -- and the mask [Hm, n, M] (Hm = 1 or Hq) of what row r may attend.  A MUTANT is another mask over the same universe (or the
same mask over other heads' keys): a named way of being wrong."""
import functools
import math

import numpy as np
import torch

G_CYCLE = (0.5, 1.0, 1.5, 2.0)              # the count probe's q_r = -g_r 1
REL_COUNT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10, "bf16": 2.0 ** -8, "fp16": 2.0 ** -10}   # count probe: |got - ref| <= REL ref
TOL, TOL_V16 = 2.0 ** -6, 2.0 ** -7         # the project's bounds (tests/gpu_utils.py)
LSE_TOL_SWEEP128, LSE_TOL_V16, LSE_TOL = 2e-2, 4e-3, 2e-3   # include/qattn.h: the D = 128 head-wise FP8 sweep, 16-bit-V rows, the others
TEETH = 4.0                                 # every mutant moves some element of every row it touches by >= TEETH x that element's bound
FAR = 1 << 30                               # an unbounded band edge


def pad64(n):
    return (n + 63) // 64 * 64


# ---- masks ------------------------------------------------------------------------------------------------------------------------
def band_edges(n, m, kind, arg=None):
    """(lo, hi) int64 [n]: row r attends keys lo[r] <= j <= hi[r] (and 0 <= j < m).  kind: "full"; "causal" (top-left, arg = q_offset);
    "window" (arg = (left, right), -1 unbounded, aligned bottom-right: delta = m - n)."""
    r = np.arange(n, dtype=np.int64)
    lo, hi = np.full(n, -FAR, np.int64), np.full(n, FAR, np.int64)
    if kind == "causal":
        hi = r + int(arg or 0)
    elif kind == "window":
        left, right = arg
        if left >= 0:
            lo = r + (m - n) - left
        if right >= 0:
            hi = r + (m - n) + right
    else:
        assert kind == "full", kind
    return lo, hi


def band_mask(lo, hi, m, M, clip=None):
    """bool [n, M]: lo <= j <= hi and j < clip (default m: the sequence's own keys)"""
    j = np.arange(M, dtype=np.int64)[None, :]
    return (j >= lo[:, None]) & (j <= hi[:, None]) & (j < (m if clip is None else clip))


def tile_mask(tiles, n, m, M, block=128):
    """bool [H, n, M] from a tile table bool [H, ceil(n/block), ceil(m/block)]"""
    t = np.repeat(np.repeat(np.asarray(tiles, bool), block, axis=-2)[..., :n, :], block, axis=-1)[..., :m]
    out = np.zeros(t.shape[:-1] + (M,), bool)
    out[..., :m] = t
    return out


# ---- probe tensors ----------------------------------------------------------------------------------------------------------------
def count_q(Hq, n, D, first_row=0):
    g = np.asarray(G_CYCLE)[(np.arange(n) + first_row) % len(G_CYCLE)]
    return np.broadcast_to(-g[None, :, None], (Hq, n, D)).astype(np.float64).copy()


def count_k(Hkv, M, D, m=None):
    k = np.full((Hkv, M, D), 0.5)
    k[:, (M if m is None else m):] = 0.0
    return k


def count_v(Hkv, M, D, m=None):
    """V[j, c] = 1 if j mod D == c else 0 (zero beyond the own keys)"""
    v = np.zeros((Hkv, M, D))
    j = np.arange(M if m is None else m)
    v[:, j, j % D] = 1.0
    return v


@functools.lru_cache(maxsize=None)
def code_tables(seed, Hkv, M, D):
    """(u, w): u [Hkv, M, D] distinct random +-1 rows (keys, and what queries are made of); w [Hkv, M, D] distinct rows over {-1, 0, 1}
    (values).  One table per kv head -- different seeds give different batches / sequences."""
    rng = np.random.default_rng(1000003 * seed + 7919 * D + M)
    u = rng.integers(0, 2, (Hkv, M, D)) * 2.0 - 1.0
    w = rng.integers(-1, 2, (Hkv, M, D)).astype(np.float64)
    for t in (u, w):
        for h in range(Hkv):
            assert len(np.unique(t[h], axis=0)) == M, "code rows must be distinct"
    u.setflags(write=False)
    w.setflags(write=False)
    return u, w


def code_q(u, target, Hq, gain=1.0):
    """q [Hq, n, D]: row r of head h is gain * u[h's kv head, target[h or 0, r]]; target < 0 gives a zero row (uniform weights)."""
    Hkv = u.shape[0]
    target = np.asarray(target)
    target = np.broadcast_to(target if target.ndim == 2 else target[None], (Hq, target.shape[-1]))
    kvh = np.arange(Hq) // (Hq // Hkv)
    q = gain * u[kvh[:, None], np.maximum(target, 0)]
    q[target < 0] = 0.0
    return q


def pointer_targets(mask):
    """int [H, n]: for every row an ALLOWED key at a hard position, cycling with the row index through: its first key, its last key (the
    diagonal / the window's right edge / inside the tail chunk), the first and the 33rd key of the last key's 64-key chunk, the first key
    of the last key's 128-key tile, key 0 of the middle chunk.  A candidate the mask forbids falls back to the last key; no key: -1."""
    H, n, M = mask.shape
    any_ = mask.any(-1)
    first = mask.argmax(-1)
    last = M - 1 - mask[..., ::-1].argmax(-1)
    c64 = last // 64 * 64
    cands = np.stack([first, last, c64, np.minimum(c64 + 32, last), last // 128 * 128, (first + last) // 2 // 64 * 64], -1)   # [H, n, 6]
    pick = np.take_along_axis(cands, (np.arange(n) % cands.shape[-1])[None, :, None].repeat(H, 0), -1)[..., 0]
    ok = np.take_along_axis(mask, pick[..., None], -1)[..., 0]
    return np.where(any_, np.where(ok, pick, last), -1)


# ---- a sequence and its references ---------------------------------------------------------------------------------------------------
class Seq:
    """One sequence of a problem (module docstring).  extras: {name: column indices of the universe} for the named mutants."""

    def __init__(self, q, k, v, mask, m, extras=None, sm=None):
        self.q, self.k, self.v = (np.asarray(t, np.float64) for t in (q, k, v))
        self.mask = np.asarray(mask, bool)
        self.mask = self.mask if self.mask.ndim == 3 else self.mask[None]
        self.m, self.extras = m, dict(extras or {})
        self.sm = 1.0 / math.sqrt(self.q.shape[-1]) if sm is None else sm
        assert self.mask.shape[1:] == (self.q.shape[1], self.k.shape[1]) and self.mask.shape[0] in (1, self.q.shape[0])
        assert not self.mask[..., m:].any(), "the correct mask admits the sequence's own keys only"
        self._scores = self._reference = None

    @property
    def dims(self):
        return self.q.shape[0], self.k.shape[0], self.q.shape[1], self.k.shape[1], self.q.shape[2]

    def scores(self, k=None):
        """fp64 [Hq, n, M] (cached for the sequence's own keys)"""
        if k is None and self._scores is not None:
            return self._scores
        Hq, Hkv = self.q.shape[0], self.k.shape[0]
        kk = torch.from_numpy(self.k if k is None else k).repeat_interleave(Hq // Hkv, dim=0)
        s = (torch.from_numpy(self.q) @ kk.transpose(-1, -2)) * self.sm
        if k is None:
            self._scores = s
        return s

    def softmax(self, mask=None, k=None, v=None):
        """fp64 masked softmax: (out [Hq, n, D], lse [Hq, n]); a row without a key is 0 / -inf.  The reference (no argument) is kept."""
        if mask is None and k is None and v is None:
            if self._reference is None:
                self._reference = self.softmax(self.mask)
            return self._reference
        mask = torch.from_numpy(np.array(self.mask if mask is None else mask, bool))
        assert mask.dim() == 3
        s = self.scores(k).masked_fill(~mask, -math.inf)
        lse = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - lse.clamp_min(-1e300)[..., None])
        vv = torch.from_numpy(self.v if v is None else v).repeat_interleave(self.q.shape[0] // self.k.shape[0], dim=0)
        return (p @ vv).numpy(), lse.numpy()


def count_expected(mask, D):
    """The count probe's closed form from the mask alone, in integers: O[r, c] = n_c(r) / n(r) (0 where n = 0), and n [H, n]."""
    mask = np.asarray(mask, bool)
    mask = mask if mask.ndim == 3 else mask[None]
    H, n, M = mask.shape
    Mp = (M + D - 1) // D * D
    pad = np.zeros((H, n, Mp), np.int64)
    pad[..., :M] = mask
    cnt = pad.reshape(H, n, Mp // D, D).sum(2)
    tot = cnt.sum(-1)
    return cnt / np.maximum(tot, 1)[..., None], tot


def count_lse(q_deq, k_deq, tot, sm=None):
    """s_r + ln n(r) with s_r the (single) score of row r on the de-quantised operands: q_deq [Hq, n, D], k_deq [Hkv, D] (any own key)"""
    Hq, n, D = q_deq.shape
    sm = 1.0 / math.sqrt(D) if sm is None else sm
    kk = np.repeat(np.asarray(k_deq, np.float64), Hq // k_deq.shape[0], axis=0)
    s = sm * (np.asarray(q_deq, np.float64) * kk[:, None, :]).sum(-1)
    with np.errstate(divide="ignore"):
        return np.where(tot > 0, s + np.log(np.maximum(tot, 1)), -np.inf)


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
def count_bound(ref, dtype, widen=1.0):
    """per element: REL ref (exactly 0 where ref is 0)"""
    return REL_COUNT[dtype] * widen * np.abs(ref)


def project_bound(ref, v16):
    """per element, tests/gpu_utils.py: 2^-7 max(1, |ref|) on 16-bit-V rows, 2^-6 max(1, |ref| / 2) on fp8-V rows.  Teeth are asked against
    the LARGER of the two wherever the path of a row is the kernel's choice (v16 = None)."""
    a = np.abs(ref)
    b16, b8 = TOL_V16 * np.maximum(1.0, a), TOL * np.maximum(1.0, a / 2)
    return np.maximum(b16, b8) if v16 is None else (b16 if v16 else b8)


def teeth(ref, mut, bound, touched, row_ratio=None):
    """min over the touched rows of max over the row's elements of |mut - ref| / bound (inf where the bound is 0 and they differ);
    inf when no row is touched.  row_ratio: a second per-row figure (the LSE's |difference| / tolerance) the row may have its teeth in."""
    d = np.abs(np.asarray(mut) - np.asarray(ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(d > 0, d / bound, 0.0)
    per_row = ratio.max(-1) if row_ratio is None else np.maximum(ratio.max(-1), row_ratio)
    touched = np.broadcast_to(touched, per_row.shape)
    return float(per_row[touched].min()) if touched.any() else math.inf


# ---- mutants -------------------------------------------------------------------------------------------------------------------------
def band_mutants(lo, hi, m, M):
    """named wrong masks of a band: each finite edge moved by +-1, and the zero padding (columns m .. pad64(m)) admitted wherever the
    band reaches it (a tail that is not masked)"""
    out = {}
    if (lo > -FAR).any():
        out["lo-1"], out["lo+1"] = band_mask(lo - 1, hi, m, M), band_mask(lo + 1, hi, m, M)
    if (hi < FAR).any():
        out["hi-1"], out["hi+1"] = band_mask(lo, hi - 1, m, M), band_mask(lo, hi + 1, m, M)
    if pad64(m) > m and M >= pad64(m):
        out["padding admitted"] = band_mask(lo, hi, m, M, clip=pad64(m))
    return out


def chunk_drop_mutants(mask, m, chunks=None):
    """one 64-key chunk dropped: the first, a middle and the last (partial) chunk unless given -- on the rows that attend ALL its keys
    (a chunk a row attends in part lies on the row's edge: the edge mutants)"""
    nch = pad64(m) // 64
    out = {}
    for c in sorted(set(chunks if chunks is not None else (0, nch // 2, nch - 1))):
        mm = mask.copy()
        whole = mask[..., 64 * c:min(64 * c + 64, m)].all(-1)
        mm[..., 64 * c:64 * c + 64] &= ~whole[..., None]
        out[f"chunk {c} dropped"] = mm
    return out


def column_mutants(mask, extras):
    """an extra key of the universe admitted on every row that has a key: {name: columns}"""
    out = {}
    rows = mask.any(-1)
    for name, cols in extras.items():
        mm = mask.copy()
        for c in np.atleast_1d(cols):
            mm[..., c] |= rows
        out[name + " admitted"] = mm
    return out


def tile_flip_mutants(tiles, n, m, M, flips):
    """one tile flipped: flips = [(head, qb, kb), ...]"""
    out = {}
    for h, i, j in flips:
        t = np.array(tiles, bool)
        t[h, i, j] ^= True
        out[f"tile ({h},{i},{j}) flipped"] = tile_mask(t, n, m, M)
    return out


def touched_rows(mask, mut_mask):
    return np.broadcast_to((np.asarray(mask) != np.asarray(mut_mask)).any(-1), np.broadcast_shapes(mask.shape[:-1], mut_mask.shape[:-1]))


def count_teeth(seq, mutants, dtype, widen=1.0, lse_tol=None, rows_graded=None):
    """{mutant: teeth} of the count probe on `seq`: the reference is the closed form, a mutant the fp64 softmax under the wrong mask (its
    padding keys score 0, a neighbour's key scores like an own key).  lse_tol: the rows' LSE s_r + ln n(r) is graded too, to this
    tolerance -- D = 64, where a dropped 64-key chunk takes one key of every residue class and leaves n_c / n alone."""
    ref, _ = count_expected(seq.mask, seq.dims[4])
    ref_lse = seq.softmax()[1] if lse_tol else None
    ref = np.broadcast_to(ref, (seq.dims[0],) + ref.shape[1:]) if ref.shape[0] == 1 else ref
    res = {}
    for name, mm in mutants.items():
        rows = touched_rows(seq.mask, mm)
        if rows_graded is not None:   # (the scattered form: the uniform rows only -- the closed form is theirs)
            rows = rows & rows_graded
        if not rows.any():
            continue
        mut, mut_lse = seq.softmax(np.broadcast_to(mm, (mm.shape[0],) + seq.mask.shape[1:]))
        with np.errstate(invalid="ignore"):
            lse_ratio = np.nan_to_num(np.abs(mut_lse - ref_lse), nan=0.0, posinf=np.inf) / lse_tol if lse_tol else None
        res[name] = teeth(ref, mut, count_bound(ref, dtype, widen), rows, lse_ratio)
    return res


def smoothed_k(seq):
    """the key universe as key smoothing leaves it, before quantisation: k - the channel mean of the sequence's own keys"""
    return seq.k - seq.k[:, :seq.m].mean(1, keepdims=True) if seq.m else seq.k


def decoy_teeth(seq, decoy, v16=None, k=None):
    """teeth of the decoy probe: every row with a decoy (decoy[h or 0, r] >= 0, a column of the universe the mask forbids) admits it.
    k: other keys for the same mask (`smoothed_k`)"""
    decoy = np.asarray(decoy)
    decoy = np.broadcast_to(decoy if decoy.ndim == 2 else decoy[None], seq.mask.shape[:2])
    assert not np.take_along_axis(seq.mask, np.maximum(decoy, 0)[..., None], -1)[..., 0][decoy >= 0].any(), "a decoy must be forbidden"
    mm = seq.mask.copy()
    h, r = np.nonzero(decoy >= 0)
    mm[h, r, decoy[h, r]] = True
    ref, _ = seq.softmax() if k is None else seq.softmax(seq.mask, k=k)
    mut, _ = seq.softmax(mm, k=k)
    return {"decoy admitted": teeth(ref, mut, project_bound(ref, v16), decoy >= 0)}


def pointer_teeth(seq, target, v16=None, other_kv=None):
    """teeth of the pointer probe: the pointed key dropped, its whole 64-key chunk dropped, and (other_kv = {name: (k, v)}) the keys and
    values of another kv head / batch entry read instead"""
    target = np.asarray(target)
    target = np.broadcast_to(target if target.ndim == 2 else target[None], seq.mask.shape[:2])
    ref, _ = seq.softmax()
    bound = project_bound(ref, v16)
    rows = target >= 0
    res = {}
    h, r = np.nonzero(rows)
    mm = seq.mask.copy()
    mm[h, r, target[h, r]] = False
    res["pointed key dropped"] = teeth(ref, seq.softmax(mm)[0], bound, rows)
    mm = seq.mask.copy()
    for o in range(64):
        mm[h, r, np.minimum(target[h, r] // 64 * 64 + o, mm.shape[-1] - 1)] = False
    res["pointed chunk dropped"] = teeth(ref, seq.softmax(mm)[0], bound, rows)
    for name, (k2, v2) in (other_kv or {}).items():
        res[name] = teeth(ref, seq.softmax(k=np.asarray(k2, np.float64), v=np.asarray(v2, np.float64))[0], bound, rows)
    return res


# ---- cases: the same builders serve the CPU teeth test and the GPU tests ------------------------------------------------------------------
PREV, NEXT = "the previous sequence's last key", "the key after the used ones"


class Case:
    """A problem: B sequences (`seqs`), the per-sequence probe data (`aux`: decoy columns / pointer targets / pointer row mask), the named
    wrong masks of every sequence (`mutants`, for the count probe) and the packed tensors the entries take (`q` [total_q, Hq, D], `k` / `v`
    [total_alloc_k, Hkv, D], float64; `lq`, `alloc`, `used`)."""

    def __init__(self, probe, seqs, aux, mutants, q, k, v, lq, alloc, used):
        self.probe, self.seqs, self.aux, self.mutants = probe, seqs, aux, mutants
        self.q, self.k, self.v, self.lq, self.alloc, self.used = q, k, v, list(lq), list(alloc), list(used)

    def dense(self):
        """q [B, Hq, Sq, D], k, v [B, Hkv, Skv, D] (every sequence of the same size, all keys used)"""
        B = len(self.lq)
        assert len(set(self.lq)) == 1 and len(set(self.alloc)) == 1 and self.alloc == self.used
        f = lambda t, S: np.ascontiguousarray(t.reshape(B, S, t.shape[1], t.shape[2]).transpose(0, 2, 1, 3))
        return f(self.q, self.lq[0]), f(self.k, self.alloc[0]), f(self.v, self.alloc[0])

    def reference(self):
        """fp64 (out [total_q, Hq, D], lse [Hq, total_q]) -- the count probe's from integer counts (lse: of the exact q; see count_lse)"""
        outs, lses = [], []
        for s in self.seqs:
            if self.probe == "count":
                o, tot = count_expected(s.mask, s.dims[4])
                o = np.broadcast_to(o, (s.dims[0],) + o.shape[1:])
                l = count_lse(s.q, s.k[:, 0], np.broadcast_to(tot, (s.dims[0], s.dims[2])), s.sm) if s.m else np.full(s.q.shape[:2], -np.inf)
            else:
                o, l = s.softmax()
            outs.append(o.transpose(1, 0, 2))
            lses.append(l)
        return np.concatenate(outs, 0), np.concatenate(lses, 1)

    def pointer_rows(self):
        """bool [Hq, total_q]: rows that point at a key (peaked); the others are flat"""
        return np.concatenate([np.broadcast_to(np.asarray(a) >= 0 if a.ndim == 2 else (a >= 0)[None], s.q.shape[:2])
                               for a, s in zip(self.aux, self.seqs)], 1)


def _decoys(lo, hi, m, P, has_prev, has_next):
    """decoy column per row [n]: cycling through the forbidden keys right outside each edge of the row's band and the sequence's
    neighbours in the packed tensor; -1 where the row has none"""
    n = len(lo)
    cands = np.full((n, 4), -1, np.int64)
    below, above = lo - 1, hi + 1
    cands[:, 0] = np.where((below >= 0) & (below < m) & (below <= hi), below, -1)
    cands[:, 1] = np.where((above >= 0) & (above < m) & (above >= lo), above, -1)
    cands[:, 2] = P if has_prev else -1
    cands[:, 3] = P + 1 if has_next else -1
    order = (np.arange(n)[:, None] + np.arange(4)[None, :]) % 4          # row r starts at candidate r mod 4 and takes the first that exists
    c = np.take_along_axis(cands, order, 1)
    first = (c >= 0).argmax(1)
    return np.where((c >= 0).any(1), c[np.arange(n), first], -1)


def make_case(probe, D, lq, alloc, used=None, kind="full", arg=None, Hq=2, Hkv=2, seed=0, tiles=None, n_peaked=0, flips=()):
    """probe: "count", "decoy", "pointer" or "scatter" (n_peaked pointer rows among uniform rows of the second 256-row block: code keys,
    indicator values).  lq / alloc / used: per-sequence rows, allocated keys, used keys.  kind / arg: band_edges; tiles
    ([Hq or 1, nQB, nKB] bool, one sequence): the block-sparse mask instead."""
    used = list(alloc) if used is None else list(used)
    B = len(lq)
    tabs = [code_tables(seed * 131 + i, Hkv, max(a, 1), D) for i, a in enumerate(alloc)]
    seqs, auxs, muts, qs, ks, vs = [], [], [], [], [], []
    for i, (n, a, m) in enumerate(zip(lq, alloc, used)):
        P = pad64(m)
        M = P + 2
        coded = probe != "count"
        ind = lambda j: np.eye(D)[np.asarray(j) % D]
        # the allocation: its keys and values as the entry sees them
        ka = tabs[i][0][:, :a].copy() if coded else np.full((Hkv, a, D), 0.5)
        va = tabs[i][1][:, :a].copy() if probe in ("decoy", "pointer") else np.broadcast_to(ind(np.arange(a)), (Hkv, a, D)).copy()
        ku, vu = np.zeros((Hkv, M, D)), np.zeros((Hkv, M, D))
        ku[:, :m], vu[:, :m] = ka[:, :m], va[:, :m]
        extras = {}
        prev = next((j for j in range(i - 1, -1, -1) if alloc[j] > 0), None)
        if prev is not None:
            extras[PREV] = P
            ku[:, P], vu[:, P] = ks[prev][:, -1], vs[prev][:, -1]
        nxt = None
        if m < a:
            nxt = (ka[:, m], va[:, m])
        else:
            j = next((j for j in range(i + 1, B) if alloc[j] > 0), None)
            if j is not None:
                nxt = (tabs[j][0][:, 0] if coded else np.full((Hkv, D), 0.5),
                       tabs[j][1][:, 0] if probe in ("decoy", "pointer") else np.broadcast_to(ind(0), (Hkv, D)))
        if nxt is not None:
            extras[NEXT] = P + 1
            ku[:, P + 1], vu[:, P + 1] = nxt
        if tiles is not None:
            assert B == 1
            mask = tile_mask(tiles, n, m, M)
            mut = tile_flip_mutants(tiles, n, m, M, flips)
            if P > m:   # the zero padding of the partial last tile admitted wherever that tile is on
                mm = mask.copy()
                mm[..., m:P] = mask[..., m - 1:m]
                mut["padding admitted"] = mm
            tl = np.broadcast_to(np.asarray(tiles, bool), (mask.shape[0],) + np.asarray(tiles).shape[-2:])
            # decoy: the first key of the off tile nearest to the row block's own index (none: -1)
            nqb, nkb = tl.shape[-2:]
            dist = np.abs(np.arange(nkb)[None, :] - np.minimum(np.arange(nqb), nkb - 1)[:, None]) + 0.25 * (np.arange(nkb)[None, :] > np.arange(nqb)[:, None])
            near = np.where(~tl, dist[None], np.inf).argmin(-1)                       # [H, nQB]
            near = np.where((~tl).any(-1) & tl.any(-1), near, -1)
            decoy = np.repeat(near, 128, axis=-1)[:, :n] * 128
            decoy = np.where(decoy >= 0, decoy, -1)
            lo = hi = None
        else:
            lo, hi = band_edges(n, m, kind, arg)
            mask = band_mask(lo, hi, m, M)[None]
            mut = {name: mm[None] for name, mm in band_mutants(lo, hi, m, M).items()}
            decoy = _decoys(np.maximum(lo, -1), np.minimum(hi, m), m, P, PREV in extras, NEXT in extras)
            decoy = np.where(mask[0].any(-1), decoy, -1)                               # (a row without a key is exactly 0 whatever leaks)
        mut.update(column_mutants(mask, extras))
        mut.update(chunk_drop_mutants(mask, m))   # (D = 64: n_c / n does not move -- the row's LSE does, count_teeth)
        if probe == "count":
            q, aux = count_q(Hq, n, D), np.full(n, -1)
        elif probe == "decoy":
            q, aux = code_q(ku, decoy, Hq), decoy
        else:
            aux = pointer_targets(np.broadcast_to(mask, (Hq if mask.shape[0] > 1 else 1,) + mask.shape[1:]))
            if probe == "scatter":
                rows = np.zeros(n, bool)
                b0 = 256 if n >= 512 else 0
                rows[b0 + (np.arange(n_peaked) * min(256, n - b0)) // max(n_peaked, 1)] = True     # spread over the block (distinct: n_peaked <= its rows)
                aux = np.where(rows[None], aux, -1)
            q = code_q(ku, aux, Hq, gain=2.0)
        seqs.append(Seq(q, ku, vu, mask, m, extras))
        auxs.append(np.asarray(aux))
        muts.append(mut)
        qs.append(q)
        ks.append(ka)
        vs.append(va)
    cat = lambda ts: np.concatenate([t.transpose(1, 0, 2) for t in ts], 0)
    return Case(probe, seqs, auxs, muts, cat(qs), cat(ks), cat(vs), lq, alloc, used)


# ---- the case lists (ISSUE: the smallest shapes at which each path is still reached) ----------------------------------------------------
DENSE_SHAPES = [(1100, 1100, True), (1100, 1100, False), (2304, 2304, True), (2304, 2304, False), (333, 1090, False), (1300, 1090, True)]
LONG_KEYS = (256, 16448)                                            # the per-head-scaled-V path of the fused entry (Skv > 16384)
PACKED_LENS = [1100, 1, 1300, 0, 65, 1089]
PACKED_CROSS = ([300, 1300, 64], [1300, 1090, 1100])
PACKED_SEQUSED = ([300, 700, 64], [1300, 1200, 128], [1090, 1100, 65])   # lq, allocated keys, used keys: the padding holds decoys
WINDOW_LENS = [1300, 1, 2304, 65]
WINDOW_CROSS = ([300, 1300], [1300, 1090])                          # delta > 0 and delta < 0
# one zero-padded key admitted on a g = 0.5 row that holds 1200 keys moves n_c / n by e^2 / 1200 at D = 64 (e^2.8 at D = 128): 1.6x (3.6x)
# the bf16 bound, so those count probes run in fp16
WINDOW_COUNT_DTYPE = {64: "fp16", 128: "fp16", 256: "bf16"}
WINDOWS = [(1100, 0), (1024, 37), (0, 1200), (63, 0), (-1, 0), (1500, -1)]


SMOOTH_LENS = ([300, 1300, 64], [1300, 1090, 1100])                  # the packed / window decoy probe under key smoothing
SMOOTH_WINDOW = (1024, 37)
GRAPH_LENS = ([1100, 1, 1300, 0, 65, 1089], [1089, 65, 0, 1300, 1, 1100])   # graded tables, and the tables the graph is captured on


# block-sparse: (D, mask, Sq, Skv, mask heads).  Sq = Skv = 1300: the last tile is partial.  A full 128-key tile holds every residue class
# of D = 64 / 128 equally often, so there n_c / n is 1 / D whatever tiles are listed and a wrong tile shows in the row's LSE (ln n) alone;
# at D = 256 a tile feeds half the classes and the output itself moves.
SPARSE_CASES = [(D, "band+global", 1300, 1300, 1) for D in (64, 128, 256)] + \
               [(D, n, 1300, 1300, H) for D in (64, 128) for n, H in (("random", 4), ("checkerboard", 1))] + [(D, "random", 700, 2304, 1) for D in (64, 128)]


def heads(entry, probe):
    """(Hq, Hkv) of the cases of an entry: ONE place, so that the CPU teeth are shown on the very inputs the GPU tests run"""
    if entry == "dense":
        return 2, 2
    if entry == "sparse":
        return 4, 2
    return (4, 2) if probe == "pointer" else (2, 1)                   # packed, window: GQA everywhere, two kv heads where heads can be confused


def dense_case(probe, D, Sq, Skv, causal, B=1, Hq=2, Hkv=2, seed=0, n_peaked=0):
    return make_case(probe, D, [Sq] * B, [Skv] * B, kind="causal" if causal else "full", Hq=Hq, Hkv=Hkv, seed=seed, n_peaked=n_peaked)


def sparse_tiles(name, nqb, nkb, H=1):
    """the block-sparse masks of the cases: [H, nQB, nKB] bool"""
    i, j = np.arange(nqb)[:, None], np.arange(nkb)[None, :]
    if name == "band+global":
        t = (np.abs(i * nkb // nqb - j) <= 1) | (j == 0)
    elif name == "checkerboard":
        t = (i + j) % 2 == 0
    else:
        assert name == "random"
        t = np.random.default_rng(nqb * 100 + nkb + H).random((H, nqb, nkb)) < 0.5
        t[..., 0, :] |= ~t[..., 0, :].any(-1, keepdims=True)
        return t
    return np.broadcast_to(t, (H, nqb, nkb)).copy()


def sparse_flips(tiles):
    """one tile flipped, three times: the first, a middle and the last (partial) tile of the table's diagonal"""
    H, nqb, nkb = tiles.shape
    return [(H - 1, i, min(i * nkb // nqb, nkb - 1)) for i in (0, nqb // 2, nqb - 1)]

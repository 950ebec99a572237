"""What tests/test_cpu_tree.py and the GPU tests of tree-shaped speculative decoding share, restated from include/qattn_paged_varlen_tree.h
and NOT imported from the product: the cases (query counts, key counts, trees), the mask rule with its named mutants, an fp64 per-row
reference that walks the kernel's own work items (kv head, tile slot, row) as tests/paged_varlen_cases.reference does, the parent walk of
`tree_mask_from_parents`, and the compaction rule on row-major pools."""
import numpy as np

from tests import paged_cases as P
from tests import paged_varlen_cases as V

B, HKV, CAP = P.B, P.HKV, P.CAP
TILE = V.TILE
MASK64 = (1 << 64) - 1

# (G, queries per slot, keys per slot -- the drafts INCLUDED).  delta = L - Sq:
#   A  17 drafts inside one chunk (delta 192 = 0 mod 64); 40 drafts behind 1064 committed keys (40 mod 64; FAST reaches the byte sweep;
#      G 40 = 160 rows: two tiles, the first crosses head boundaries); one draft at delta 63
#   B  64 drafts at delta 127 (63 mod 64: across a chunk boundary, at page size 64 a page boundary); 2 drafts at delta 1; an idle slot
#   C  G = 1: the plain-causal slots 130 and 65; 40 drafts at delta 104 (40 mod 64), across the key 128: a split boundary at 2 splits
#   D  a slot with fewer keys than queries; a slot without keys; 40 drafts at delta 232 (40 mod 64) across the key 256: a split boundary
#      at 2 and at 3 splits
CASES = {
    "A": (4, (17, 40, 1), (209, 1104, 64)),
    "B": (4, (64, 2, 0), (191, 3, 50)),
    "C": (1, (130, 65, 40), (400, 257, 144)),
    "D": (4, (17, 40, 40), (10, 0, 272)),
}
KINDS = ("chain", "star", "binary", "random", "zero", "junk")


def check_cases():
    """what the issue asks of the shapes"""
    sqs = {s for _, sq, _ in CASES.values() for s in sq}
    assert {0, 1, 2, 17, 40, 64, 65, 130} <= sqs
    mods = {(L - s) % 64 for _, sq, ls in CASES.values() for s, L in zip(sq, ls) if 0 < s <= 64 and L >= s}
    assert mods == {0, 1, 40, 63}, mods
    pairs = [(s, L) for _, sq, ls in CASES.values() for s, L in zip(sq, ls)]
    assert any(0 < L < s for s, L in pairs) and any(L == 0 and s > 0 for s, L in pairs) and any(L >= 1024 + s for s, L in pairs)
    assert any(G == 1 for G, _, _ in CASES.values())


def tables(name, page_size, seed=0, lens=None):
    """a shuffled table without a shared page (two slots that compact into one page would have two writers); entries behind a slot's
    pages name the poison page.  lens: other lengths than the case's (a test that appends the drafts to max(L_b - Sq_b, 0) keys)"""
    lens = CASES[name][2] if lens is None else tuple(lens)
    return P.Tables(page_size, lens, seed=seed, need=[-(-L // page_size) for L in lens])


def appended_lens(name):
    """the lengths after the case's drafts were appended to its committed keys, max(L_b - Sq_b, 0) of them"""
    _, sq, lens = CASES[name]
    return [max(L - n, 0) + n for n, L in zip(sq, lens)]


# ---- trees ------------------------------------------------------------------------------------------------------------------------------
def parents_of(kind, n, seed=0):
    """in-slot parent of every draft token (-1: a root; a parent's index is below its child's)"""
    if kind in ("chain", "junk"):
        return [p - 1 for p in range(n)]
    if kind == "star":
        return [-1] + [0] * (n - 1) if n else []
    if kind == "binary":                       # BFS order
        return [(p - 1) // 2 if p else -1 for p in range(n)]
    assert kind in ("random", "zero")
    rng = np.random.RandomState(seed)
    return [int(rng.randint(-1, p)) if p else -1 for p in range(n)]


def words_of_parents(parents):
    """the plain walk: the word of token p has bit p and the bits of all its ancestors (Python ints, unsigned)"""
    out = []
    for p in range(len(parents)):
        w, a = 0, p
        while a >= 0:
            w |= 1 << (a & 63)
            a = parents[a]
        out.append(w)
    return out


def words_of(kind, sq, seed=0):
    """(packed words as unsigned Python ints, packed parents) of one tree kind in every slot.  'zero': all-zero words; 'junk': a chain
    with random bits above p; slots with more than 64 queries get random words (they are ignored)"""
    words, parents = [], []
    rng = np.random.RandomState(seed + 77)
    for b, n in enumerate(sq):
        par = parents_of(kind, n, seed + b)
        w = words_of_parents(par)
        rnd = [int(rng.randint(0, 1 << 32)) | (int(rng.randint(0, 1 << 32)) << 32) for _ in range(n)]
        if n > 64:
            w = rnd
        elif kind == "zero":
            w = [0] * n
        elif kind == "junk":
            w = [x | (r & ~((2 << p) - 1) & MASK64) for p, (x, r) in enumerate(zip(w, rnd))]
        words += w
        parents += par
    return words, parents


def as_int64(words):
    return np.array(words, np.uint64).view(np.int64)


# ---- the mask rule ----------------------------------------------------------------------------------------------------------------------
MUTANTS = ("bit+1", "row-word", "no-cu", "key-bit", "bits-above", "low32")


def row_keep(words, start, n, L, r, M, mutant=None):
    """bool [M]: the keys packed row r (head r // n, position r % n) of a slot attends -- start: its first token, n queries, L keys,
    words: the packed words of the whole step.  The rule of include/qattn_paged_varlen_tree.h, literally; mutant: one of MUTANTS."""
    p, delta = r % n, L - n
    j = np.arange(M)
    causal = j <= min(L - 1, p + delta)
    if n > 64:
        return causal
    at = start + p
    if mutant == "row-word":
        at = min(start + r, len(words) - 1)
    if mutant == "no-cu":
        at = p
    w = words[at] & (0xFFFFFFFF if mutant == "low32" else MASK64)
    bits = np.array([(w >> i) & 1 for i in range(64)], bool)
    idx = j - delta + (1 if mutant == "bit+1" else 0)
    if mutant == "key-bit":
        idx = j % 64
    bit = np.where((idx >= 0) & (idx < 64), bits[np.clip(idx, 0, 63)], False)
    draft = j >= max(delta, 0)
    if mutant == "bits-above":
        return (j < L) & np.where(draft, bit, True)
    return causal & (bit | ~draft)


def slot_mask(words, start, n, L, G, M, mutant=None):
    """bool [HKV G, n, M] of one slot (the word belongs to the token: the same for all heads, unless a mutant says otherwise)"""
    one = np.stack([row_keep(words, start, n, L, r, M, mutant) for r in range(G * n)]).reshape(G, n, M)
    return np.tile(one, (HKV, 1, 1))


def reference(q, k, v, lens, sq, G, words, sm_scale, mutant=None):
    """q float64 [total_q, Hq, D] (de-quantised), k / v float64 [B, HKV, >= L, D] (de-quantised, gathered).  Walks (kv head, tile slot, row
    of the tile) as the kernel does; returns (out [total_q, Hq, D], lse [Hq, total_q]); rows nobody writes stay NaN; a row without a
    key is a zero row with LSE -inf."""
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
                keep = row_keep(words, start, n, L, r, max(L, 1), mutant)[:L]
                if not keep.any():
                    out[tok, head], lse[head, tok] = 0.0, -np.inf
                    continue
                s = (k[i, hkv, :L][keep] @ q[tok, head]) * sm_scale
                m = s.max()
                p = np.exp(s - m)
                out[tok, head] = (p / p.sum()) @ v[i, hkv, :L][keep]
                lse[head, tok] = m + np.log(p.sum())
    return out, lse


# ---- the compaction rule on row-major pools -----------------------------------------------------------------------------------------------
def accept_lists(sq, seed=0, kind="path"):
    """(accept_index packed [total], accept_lens [B]) -- 'path': an increasing list that starts at draft 0; 'wild': a non-monotone list
    with repeats, entries out of range and a count above Sq_b (all clamped by the rule)"""
    rng = np.random.RandomState(seed + 5)
    idx, cnt = [], []
    for n in sq:
        if n == 0:
            cnt.append(int(rng.randint(0, 3)))
            continue
        if kind == "path":
            c = int(rng.randint(1, min(n, 6) + 1))
            a = [0] + sorted(rng.choice(np.arange(1, n), c - 1, replace=False).tolist()) if c > 1 else [0]
            a = a + rng.randint(0, n, n - c).tolist()
        else:
            c = n + 3 if n % 2 else max(n - 1, 1)
            a = rng.randint(-2, n + 2, n).tolist()
            if n > 2:
                a[0], a[1] = 1, 0                     # a swap: key base takes base + 1's old bytes and the other way round
        idx += a
        cnt.append(c)
    return idx, cnt


def compact_rows(rows, table, page_size, seqlens, cu, accept_index, accept_lens):
    """the rule on a row-major numpy pool [P, HKV, page_size, D] (in place) and a list of lengths (returned anew): every read before every
    write.  Returns (lens, destination keys per slot)."""
    total, cap = len(accept_index), len(table[0]) * page_size
    clamp = lambda x, lo, hi: min(max(x, lo), hi)
    lens, dests = list(seqlens), []
    for b in range(len(seqlens)):
        start = clamp(cu[b], 0, total)
        n = clamp(cu[b + 1], start, total) - start
        L = clamp(seqlens[b], 0, cap)
        dests.append([])
        if not (1 <= n <= 64 and L >= n):
            continue
        base = L - n
        keep = clamp(accept_lens[b], 0, n)
        src = [base + clamp(accept_index[start + i], 0, n - 1) for i in range(keep)]
        held = [rows[P.lookup(table, b, s, page_size)[0], :, s % page_size].copy() for s in src]
        for i, x in enumerate(held):
            rows[P.lookup(table, b, base + i, page_size)[0], :, (base + i) % page_size] = x
        lens[b] = base + keep
        dests[b] = list(range(base, base + keep))
    return lens, dests

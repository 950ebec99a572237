"""What tests/test_cpu_paged_varlen.py and the GPU tests of the packed paged entry share, restated from include/qattn_paged_varlen.h and NOT
imported from the product: the (G, query-lengths) pairs that go with the shared tables of tests/paged_cases.py, their rotation over the
tables, the tile-slot -> (sequence, tile) rule, the packed layouts, the one-slot view of a cache, and an fp64 per-row reference that walks
the kernel's own work items -- with the three mutants a test of the packed addressing must expose."""
import numpy as np

from tests import paged_cases as P

B, HKV, CAP = P.B, P.HKV, P.CAP
TILE = 128

# (G, queries per sequence slot): each goes with one of the four shared tables of a page size
QCASES = [
    (4, (1, 40, 0)),     # two tiles (G 40 = 160 rows) whose first crosses head boundaries, a sequence of one query, an idle slot
    (1, (130, 0, 1)),    # two tiles of one head, an idle slot in the middle
    (4, (5, 1, 33)),     # more than one tile (G 33 = 132), one row per head for the sequence with 1 query
    (1, (3, 3, 3)),      # all equal: the dense call's shape
]
# table i of page size ps takes pair (i + ROT[ps]) % 4.  Table 0 of every page size holds a sequence WITHOUT keys in slot 2: no rotation
# hands it pair 0, whose slot 2 is idle, so that L_b = 0 always meets Sq_b > 0.
ROT = {64: 1, 128: 2, 256: 3}


def qcase(page_size, i):
    return QCASES[(i + ROT[page_size]) % 4]


def check_rotation():
    """what the issue asks of the rotation: per page size some sequence has L_b = 0 but Sq_b > 0 and some 0 < L_b < Sq_b; over the page
    sizes every length triple index meets three different pairs"""
    for ps in P.PAGE_SIZES:
        no_keys = shorter = False
        for i, lens in enumerate(P.lens_sets(ps)):
            _, sq = qcase(ps, i)
            no_keys |= any(L == 0 and s > 0 for L, s in zip(lens, sq))
            shorter |= any(0 < L < s for L, s in zip(lens, sq))
        assert no_keys and shorter, ps
    for i in range(4):
        assert len({QCASES.index(qcase(ps, i)) for ps in P.PAGE_SIZES}) == 3


def cu_of(sq):
    return [0] + np.cumsum(sq).tolist()


def slot_to_tile(j, cu, G, total_q, nB=None):
    """tile slot j of a kv head -> (sequence i, tile within it) or None: the largest i with i + floor(G start_i / 128) <= j, every extent
    clamped as include/qattn_varlen.h clamps it"""
    nB = len(cu) - 1 if nB is None else nB
    clamp = lambda x, lo, hi: min(max(x, lo), hi)
    f = lambda i: i + (G * clamp(cu[i], 0, total_q)) // TILE
    i = max([x for x in range(nB) if f(x) <= j], default=0)
    start = clamp(cu[i], 0, total_q)
    sq = clamp(cu[i + 1], start, total_q) - start
    tile = j - f(i)
    if tile < 0 or tile * TILE >= G * sq:
        return None
    return i, tile


def num_slots(G, total_q, nB=B):
    return nB + -(-G * total_q // TILE)


def one_slot(cache, b):
    """the one-slot PagedKVCacheFP8 on the same pools: row b of the table, of the scales and of seqlens"""
    from quantumattention_amd.paged import PagedKVCacheFP8
    return PagedKVCacheFP8(cache.k, cache.v, cache.scale_k[b:b + 1].contiguous(), cache.scale_v[b:b + 1].contiguous(),
                           cache.block_table[b:b + 1].contiguous(), cache.seqlens[b:b + 1].contiguous(), cache.shape, cache.fp8_format, cache.dtype,
                           cache.numerics, cache.layout)


def alone(q, cu, b):
    """sequence b's queries as the dense call takes them: [1, Hq, Sq_b, D]"""
    return q[cu[b]:cu[b + 1]].transpose(0, 1)[None].contiguous()


def rows_of(packed, kind, cu, b):
    """sequence b's rows of a packed output, in the dense call's layout.  kind: 'o' [total_q, Hq, D] -> [1, Hq, Sq, D];
    'l' [Hq, total_q] -> [1, Hq, Sq]; 'po' [ns, total_q, Hq, D] -> [ns, 1, Hq, Sq, D]; 'pl' [ns, Hq, total_q] -> [ns, 1, Hq, Sq]"""
    s, e = cu[b], cu[b + 1]
    if kind == "o":
        return packed[s:e].transpose(0, 1)[None]
    if kind == "l":
        return packed[:, s:e][None]
    if kind == "po":
        return packed[:, s:e].transpose(1, 2)[:, None]
    assert kind == "pl"
    return packed[:, :, s:e][:, None]


# ---- the fp64 reference: one softmax per packed row, reached through the kernel's own work-item map
def reference(q, k, v, lens, sq, G, max_seqlen_q, sm_scale, causal=True, mutant=None):
    """q float64 [total_q, Hq, D] (de-quantised), k / v float64 [B, HKV, CAP, D] (de-quantised, gathered), lens / sq per sequence.  Walks
    (kv head, tile slot, row of the tile) as the kernel does and writes out[token, head]; rows nobody writes stay NaN.
    mutant: 'delta-max' takes the causal offset from max_seqlen_q instead of Sq_b; 'head-max' takes the head of packed row r as
    r // max_seqlen_q; 'neighbour' hands every tile's ROWS to the next sequence (its start and count: the queries read, the rows written)
    while the keys, their length and scales stay the tile's own -- a workgroup whose row addresses and kv side disagree about the sequence."""
    total_q, Hq, D = q.shape
    nB = len(lens)
    cu = cu_of(sq)
    out = np.full((total_q, Hq, D), np.nan)
    for hkv in range(Hq // G):
        for j in range(num_slots(G, total_q, nB)):
            hit = slot_to_tile(j, cu, G, total_q, nB)
            if hit is None:
                continue
            i, tile = hit
            iq = (i + 1) % nB if mutant == "neighbour" else i
            start, n, L = cu[iq], sq[iq], lens[i]
            if n == 0:
                continue
            delta = L - (max_seqlen_q if mutant == "delta-max" else n)
            for r in range(tile * TILE, min((tile + 1) * TILE, G * n)):
                g = min(r // (max_seqlen_q if mutant == "head-max" else n), G - 1)
                pos = r % n
                hi = min(L - 1, pos + delta) if causal else L - 1
                tok, head = start + pos, hkv * G + g
                if hi < 0:
                    out[tok, head] = 0.0
                    continue
                s = (k[i, hkv, :hi + 1] @ q[tok, hkv * G + min(r // n, G - 1)]) * sm_scale   # (the q row is packed row r's own)
                p = np.exp(s - s.max())
                out[tok, head] = (p / p.sum()) @ v[i, hkv, :hi + 1]
    return out

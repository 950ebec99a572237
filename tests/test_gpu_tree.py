"""Tree-shaped speculative decoding on the paged FP8 K/V cache on the MI355X (quantumattention_amd/tree.py,
include/qattn_paged_varlen_tree.h): the verify pass under a draft tree, and the compaction of the accepted path.

Two oracles.  EXACT: a chain-shaped tree is the causal packed entry, bit for bit -- out, lse, row_path and the partials -- because the
split plan, the trip range and the merge are the causal call's; so are slots with more than 64 queries under any words, and junk bits
above p.  fp64: on the other trees every row is held to tests/tree_cases.reference on the call's own de-quantised q8 and on the pools'
de-quantised bytes looked up key by key, within the project's fp8-V bound (tests/gpu_utils.assert_within_bound), and the count probe of
tests/probes.py to its closed form.  The compaction is graded byte for byte against the rule on row-major pools and against a cache
that received the accepted tokens only.  Shapes, tables and trees: tests/tree_cases.py."""
import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import gpu_utils
from tests import paged_cases as P
from tests import paged_varlen_cases as V
from tests import probes
from tests import tree_cases as T
from tests.gpu_utils import bits8
from tests.test_gpu_paged import _cache, _pack, _rand, _rows, _same_bits, _su

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV, CAP = T.B, T.HKV, T.CAP
BF16, FP16 = torch.bfloat16, torch.float16
# (case, page size, D, dtype): every case at every page size with D = 128; D = 64, D = 256 and fp16 on one case each
CFGS = [(name, ps, 128, BF16) for name in T.CASES for ps in P.PAGE_SIZES] + [("A", 128, 64, BF16), ("D", 64, 256, BF16), ("B", 256, 128, FP16)]
CFG_IDS = [f"{n}-ps{ps}-d{D}-{str(dt)[6:]}" for n, ps, D, dt in CFGS]
NAMES = ("out", "lse", "partial_o", "partial_lse", "partial_path", "row_path")


def _words(words):
    return torch.from_numpy(T.as_int64(words)).to(DEV)


def _setup(name, ps, D, dtype, seed, fmt="e4m3", scale_k=None):
    G, sq, lens = T.CASES[name]
    t = T.tables(name, ps, seed)
    rk, rv = _rows(t, D, fmt, seed)
    kw = {} if scale_k is None else {"scale_k": scale_k}
    c = _cache(t, D, dtype, fmt, _pack(rk, rv, fmt), **kw)
    q = _rand((sum(sq), HKV * G, D), dtype, seed + 1, mul=1.5)
    return G, sq, lens, t, rk, rv, c, q


def _call(q, c, cu, mx, words=None, **kw):
    mask = dict(is_causal=True) if words is None else dict(tree_mask=words)
    return _native.fp8_attention_paged_varlen(q, c.k, c.v, c.scale_k, c.scale_v, c.block_table, c.seqlens, cu, max_seqlen_q=mx, Skv=CAP,
                                              num_pages=c.num_pages, page_size=c.page_size, fp8_dtype=P.FP8[c.fp8_format], **mask, **kw)


# ---- 1. the exact oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ps,D,dtype", CFGS, ids=CFG_IDS)
def test_a_chain_is_the_causal_entry_bit_for_bit(name, ps, D, dtype):
    """out, lse, row_path and the partials, num_splits 1 / 2 / 3 / 0, both precisions, and the byte sweep (fast, one split, no LSE)"""
    G, sq, lens, t, rk, rv, c, q = _setup(name, ps, D, dtype, 3)
    cud, mx = _su(V.cu_of(sq)), max(sq)
    words = _words(T.words_of("chain", sq)[0])
    for ns in (1, 2, 3, 0):
        for precision in ("accurate", "fast"):
            kw = dict(precision=precision, num_splits=ns, return_lse=True, return_partials=True, return_path=True)
            got, want = _call(q, c, cud, mx, words, **kw), _call(q, c, cud, mx, **kw)
            assert len(got) == len(want) == 6
            for nm, x, y in zip(NAMES, got, want):
                assert _same_bits(x, y), (name, ps, ns, precision, nm)
            assert not torch.isnan(got[0].float()).any()
    assert _same_bits(_call(q, c, cud, mx, words, precision="fast", num_splits=1), _call(q, c, cud, mx, precision="fast", num_splits=1))
    pub = qa.fp8_attn_paged_varlen_tree_func(q, c, cud, mx, words, num_splits=2, return_lse=True, return_partials=True)
    ref = qa.fp8_attn_paged_varlen_func(q, c, cud, mx, causal=True, num_splits=2, return_lse=True, return_partials=True)
    assert len(pub) == len(ref) == 5 and all(_same_bits(x, y) for x, y in zip(pub, ref))


@pytest.mark.parametrize("ps", P.PAGE_SIZES)
def test_slots_above_64_queries_and_junk_bits_above_p_are_ignored(ps):
    D, dtype = 128, BF16
    # case C: the slots with 130 and 65 queries give the causal bits under arbitrary words (the 40-query slot does not)
    G, sq, lens, t, rk, rv, c, q = _setup("C", ps, D, dtype, 5)
    cu, mx = V.cu_of(sq), max(sq)
    cud = _su(cu)
    for ns in (1, 2, 3):
        kw = dict(num_splits=ns, return_lse=True, return_path=True)
        got, want = _call(q, c, cud, mx, _words(T.words_of("random", sq, 9)[0]), **kw), _call(q, c, cud, mx, **kw)
        for b in (0, 1):
            for x, y, kind in zip(got, want, ("o", "l", "l")):
                assert _same_bits(V.rows_of(x, kind, cu, b), V.rows_of(y, kind, cu, b)), (ps, ns, b, kind)
        assert not _same_bits(V.rows_of(got[0], "o", cu, 2), V.rows_of(want[0], "o", cu, 2))
    # junk above p changes no bit: on a chain (the causal bits) and on a random tree
    for name in ("A", "B", "D"):
        G, sq, lens, t, rk, rv, c, q = _setup(name, ps, D, dtype, 6)
        cud, mx = _su(V.cu_of(sq)), max(sq)
        kw = dict(num_splits=2, precision="fast", return_lse=True, return_partials=True, return_path=True)
        junk, causal = _call(q, c, cud, mx, _words(T.words_of("junk", sq, 4)[0]), **kw), _call(q, c, cud, mx, **kw)
        assert all(_same_bits(x, y) for x, y in zip(junk, causal)), (name, ps)
        clean = T.words_of("random", sq, 4)[0]
        rng = np.random.RandomState(8)
        dirty = [w | ((int(rng.randint(0, 1 << 32)) << 32 | int(rng.randint(0, 1 << 32))) & ~((2 << p) - 1) & T.MASK64)
                 for w, p in zip(clean, [p for n in sq for p in range(n)])]
        assert dirty != clean
        a, b_ = _call(q, c, cud, mx, _words(clean), **kw), _call(q, c, cud, mx, _words(dirty), **kw)
        assert all(_same_bits(x, y) for x, y in zip(a, b_)), (name, ps)


# ---- 2. the fp64 oracle -------------------------------------------------------------------------------------------------------------------
def _dequantised(q8, sqs, rk, rv, c, t, sq, Hq, D):
    """(q, k, v) float64: the call's own q8 slabs [Hq, Sq_b, D] at byte Hq D cu[b] times scale_q; the pools' rows looked up key by key"""
    fp8 = P.FP8[c.fp8_format]
    cu, total = V.cu_of(sq), sum(sq)
    q8f, sqn = q8.view(torch.uint8).view(fp8).float().cpu().numpy().astype(np.float64), sqs.cpu().numpy().astype(np.float64)
    q = np.zeros((total, Hq, D))
    for b, n in enumerate(sq):
        slab = q8f[Hq * D * cu[b]:Hq * D * cu[b + 1]].reshape(Hq, n, D) * sqn[b][:, None, None]
        q[cu[b]:cu[b + 1]] = slab.transpose(1, 0, 2)
    deq = lambda rows, s: (P.gather_rows(rows.view(fp8).float().cpu().numpy().astype(np.float64), t.table, t.page_size)
                           * s.cpu().numpy().astype(np.float64)[:, :, None, None])
    return q, deq(rk, c.scale_k), deq(rv, c.scale_v)


@pytest.mark.parametrize("kind", ("star", "binary", "random", "zero"))
@pytest.mark.parametrize("name,ps,D,dtype", CFGS, ids=CFG_IDS)
def test_every_row_of_a_general_tree_is_within_the_fp8_v_bound_of_the_fp64_reference(name, ps, D, dtype, kind):
    i = CFGS.index((name, ps, D, dtype)) + T.KINDS.index(kind)
    ns, precision = (1, 2, 3, 0)[i % 4], ("accurate", "fast")[(i // 4) % 2]
    # scales of order 1: the de-quantised keys and values are of order 1, so that the absolute part of the bound is not slack
    G, sq, lens, t, rk, rv, c, q = _setup(name, ps, D, dtype, 20 + i, scale_k=torch.tensor([[0.5, 1.0], [0.75, 0.6], [1.0, 0.4]]) / 8)
    Hq, cu, mx = HKV * G, V.cu_of(sq), max(sq)
    words = T.words_of(kind, sq, i)[0]
    out, lse, q8, sqs, path = _call(q, c, _su(cu), mx, _words(words), num_splits=ns, precision=precision, return_lse=True, return_quant=True,
                                    return_path=True)
    qd, kd, vd = _dequantised(q8, sqs, rk, rv, c, t, sq, Hq, D)
    ref, ref_lse = T.reference(qd, kd, vd, lens, sq, G, words, 1.0 / np.sqrt(D))
    assert not np.isnan(ref).any() and not np.isnan(ref_lse).any()
    o, l, pth = gpu_utils.out_to_f32(out), lse.cpu().numpy(), path.cpu().numpy()
    mxe, rmse = gpu_utils.assert_within_bound(o.transpose(1, 0, 2), gpu_utils.PathRef(ref.transpose(1, 0, 2), ref.transpose(1, 0, 2)), pth,
                                              what=(name, ps, kind, ns, precision))
    dead = np.isinf(ref_lse)
    if kind == "zero":       # no draft key at all: a slot without committed keys has no key
        assert dead[:, [tok for b, (n, L) in enumerate(zip(sq, lens)) if L <= n <= 64 for tok in range(cu[b], cu[b + 1])]].all()
    assert (np.isneginf(l) == dead).all() and (o.transpose(1, 0, 2)[dead] == 0).all(), "a row without a key is a zero row with LSE -inf"
    worst_lse = float(np.abs(l[~dead] - ref_lse[~dead]).max()) if (~dead).any() else 0.0
    print(f"tree {name} ps{ps} D{D} {kind} ns={ns} {precision}: max-abs {mxe:.3e} rmse {rmse:.3e} worst LSE error {worst_lse:.3e}")
    assert worst_lse < probes.LSE_TOL, worst_lse


@pytest.mark.parametrize("name,ps", [("A", 64), ("B", 128), ("D", 256), ("C", 64)])
def test_the_count_probe_gives_its_closed_form_on_the_trees_mask(name, ps):
    """q_r = -g_r 1, k = 0.5 1, V[j] = e_(j mod D): O[r, c] = n_c(r) / n(r) from the tree's boolean mask alone, in integers; bound
    |got - ref| <= REL ref (tests/probes.py, the CPU test's bound)"""
    D, dtype, fmt = 128, BF16, "e4m3"
    G, sq, lens = T.CASES[name]
    Hq, cu, total = HKV * G, V.cu_of(sq), sum(sq)
    t = T.tables(name, ps, 1)
    fp8 = P.FP8[fmt]
    # the pools' rows: key j of every slot holds k = 0.5 and V = e_(j mod D), placed through the table; free pages stay NaN
    rk, rv = (r.cpu() for r in _rows(t, D, fmt, 40))
    kk, vv = (torch.from_numpy(x).float().to(fp8).view(torch.uint8) for x in (probes.count_k(HKV, CAP, D), probes.count_v(HKV, CAP, D)))
    for b, L in enumerate(lens):
        for j in range(L):
            page, slot = P.lookup(t.table, b, j, ps)
            rk[page, :, slot], rv[page, :, slot] = kk[:, j], vv[:, j]
    rk, rv = rk.to(DEV), rv.to(DEV)
    c = _cache(t, D, dtype, fmt, _pack(rk, rv, fmt), scale_k=torch.ones(B, HKV) / 2)     # (scale_v = 1: the one-hot V is exact)
    q = torch.cat([torch.from_numpy(probes.count_q(Hq, n, D)).transpose(0, 1) for n in sq]).to(dtype).to(DEV)
    worst = 0.0
    for kind in ("star", "binary", "random", "junk"):
        words = T.words_of(kind, sq, 3)[0]
        for ns, precision in ((1, "accurate"), (2, "fast"), (3, "accurate")):
            out = gpu_utils.out_to_f32(_call(q, c, _su(cu), max(sq), _words(words), num_splits=ns, precision=precision))
            for b, (n, L) in enumerate(zip(sq, lens)):
                if n == 0:
                    continue
                ref, tot = probes.count_expected(T.slot_mask(words, cu[b], n, L, G, CAP), D)
                got = out[cu[b]:cu[b + 1]].transpose(1, 0, 2)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.where(got == ref, 0.0, np.abs(got - ref) / probes.count_bound(ref, dtype))
                worst = max(worst, float(ratio.max()))
                assert (got[tot == 0] == 0).all()
    print(f"tree count probe {name} ps{ps}: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0, worst


# ---- 3. per slot --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ps", [("A", 128), ("B", 64), ("C", 256), ("D", 64)])
def test_every_slots_rows_are_the_bits_of_the_call_on_that_slot_alone(name, ps):
    D, dtype = 128, BF16
    G, sq, lens, t, rk, rv, c, q = _setup(name, ps, D, dtype, 60)
    cu, mx = V.cu_of(sq), max(sq)
    words = _words(T.words_of("random", sq, 2)[0])
    for ns, precision in ((1, "accurate"), (2, "fast"), (3, "accurate")):
        kw = dict(num_splits=ns, precision=precision, return_lse=True, return_partials=True)
        got = qa.fp8_attn_paged_varlen_tree_func(q, c, _su(cu), mx, words, **kw)
        for b, n in enumerate(sq):
            if n == 0:
                continue
            one = qa.fp8_attn_paged_varlen_tree_func(q[cu[b]:cu[b + 1]].contiguous(), V.one_slot(c, b), _su([0, n]), mx,
                                                     words[cu[b]:cu[b + 1]].contiguous(), **kw)
            for x, y, kind in zip(got, one, ("o", "l", "po", "pl", "pl")):
                if x.numel() == 0:
                    assert y.numel() == 0
                    continue
                assert _same_bits(V.rows_of(x, kind, cu, b), V.rows_of(y, kind, [0, n], 0)), (name, ps, ns, b, kind)


# ---- 4. compaction ------------------------------------------------------------------------------------------------------------------------
def _committed(name, ps, D, dtype, fmt, seed):
    """a cache that holds the committed keys of a case (L_b - Sq_b random tokens per slot, appended) over NaN-poisoned free bytes, and
    the step's draft K / V"""
    G, sq, lens = T.CASES[name]
    t = T.tables(name, ps, seed, T.appended_lens(name))
    rk, rv = _rows(t, D, fmt, seed)
    base = [max(L - n, 0) for n, L in zip(sq, lens)]
    c = _cache(t, D, dtype, fmt, _pack(rk, rv, fmt), lens=[0] * B)
    cu0 = V.cu_of(base)
    qa.paged_kv_cache_append_varlen_fp8(c, _rand((sum(base), HKV, D), dtype, seed + 1), _rand((sum(base), HKV, D), dtype, seed + 2), _su(cu0))
    return c, t, sq, base, _rand((sum(sq), HKV, D), dtype, seed + 3), _rand((sum(sq), HKV, D), dtype, seed + 4)


def _unpacked(c, D):
    """the pools as row-major numpy [P, HKV, ps, D]"""
    un = lambda pool, layout: gpu_utils.unpack_frag(bits8(pool), layout, c.num_pages, HKV, c.page_size, D).copy()
    return un(c.k, _native.LAYOUT_KFRAG), un(c.v, _native.LAYOUT_VFRAG)


@pytest.mark.parametrize("kind", ("path", "wild"))
@pytest.mark.parametrize("name,ps,D,dtype", CFGS, ids=CFG_IDS)
def test_compaction_moves_exactly_the_accepted_keys_and_every_other_byte_stays(name, ps, D, dtype, kind):
    fmt = "e4m3"
    c, t, sq, base, kd, vd = _committed(name, ps, D, dtype, fmt, 70)
    cu = V.cu_of(sq)
    qa.paged_kv_cache_append_varlen_fp8(c, kd, vd, _su(cu))
    lens0 = c.seqlens.tolist()
    idx, cnt = T.accept_lists(sq, 3, kind)
    k0, v0 = _unpacked(c, D)
    want_k, want_v = k0.copy(), v0.copy()
    want_lens, dests = T.compact_rows(want_k, t.table, ps, lens0, cu, idx, cnt)
    T.compact_rows(want_v, t.table, ps, lens0, cu, idx, cnt)
    out = qa.paged_kv_cache_compact_fp8(c, _su(cu), _su(idx), _su(cnt))
    assert out is c and c.seqlens.tolist() == want_lens
    k1, v1 = _unpacked(c, D)
    assert np.array_equal(k1, want_k) and np.array_equal(v1, want_v), "every byte: the destination keys hold the rule's bytes, all others their old ones"
    # ... stated once more without the rule's code: outside the destination keys nothing changed, the poisoned free page included
    touched = np.zeros(k0.shape[:1] + k0.shape[2:3], bool)
    for b, keys in enumerate(dests):
        for j in keys:
            touched[P.lookup(t.table, b, j, ps)] = True
    for old, new in ((k0, k1), (v0, v1)):
        same = (old == new).all(axis=(1, 3))
        assert same[~touched].all()
        assert (new[P.POISON] == P.NAN_BYTE[fmt]).all()


@pytest.mark.parametrize("ps", P.PAGE_SIZES)
def test_after_compaction_the_cache_is_the_cache_that_received_the_accepted_tokens_only(ps):
    """live keys and seqlens, and the bits of a following causal decode step"""
    D, dtype, fmt, name = 128, BF16, "e4m3", "A"
    ca, t, sq, base, kd, vd = _committed(name, ps, D, dtype, fmt, 80)
    cb = _committed(name, ps, D, dtype, fmt, 80)[0]
    cu = V.cu_of(sq)
    idx, cnt = T.accept_lists(sq, 6, "path")
    qa.paged_kv_cache_append_varlen_fp8(ca, kd, vd, _su(cu))
    qa.paged_kv_cache_compact_fp8(ca, _su(cu), _su(idx), _su(cnt))
    rows = [cu[b] + idx[cu[b] + i] for b in range(B) for i in range(cnt[b])]
    qa.paged_kv_cache_append_varlen_fp8(cb, kd[rows].contiguous(), vd[rows].contiguous(), _su(V.cu_of(cnt)))
    assert ca.seqlens.tolist() == cb.seqlens.tolist() == [b_ + n for b_, n in zip(base, cnt)]
    (ka, va), (kb, vb) = _unpacked(ca, D), _unpacked(cb, D)
    for b, L in enumerate(ca.seqlens.tolist()):
        for j in range(L):
            at = P.lookup(t.table, b, j, ps)
            assert np.array_equal(ka[at[0], :, at[1]], kb[at[0], :, at[1]]) and np.array_equal(va[at[0], :, at[1]], vb[at[0], :, at[1]]), (b, j)
    # the next step: one decode token per slot on both caches
    kn, vn, q = _rand((B, HKV, D), dtype, 91), _rand((B, HKV, D), dtype, 92), _rand((B, 8, D), dtype, 93)
    cu1 = _su([0, 1, 2, 3])
    res = []
    for c in (ca, cb):
        qa.paged_kv_cache_append_varlen_fp8(c, kn, vn, cu1)
        res.append(qa.fp8_attn_paged_varlen_func(q, c, cu1, 1, causal=True, num_splits=2, return_lse=True))
    assert all(_same_bits(x, y) for x, y in zip(*res))
    assert torch.isfinite(res[0][0].float()).all()


def test_slots_that_are_not_compactable_keep_their_bytes_and_their_lengths():
    """Sq_b = 0, Sq_b > 64, L_b < Sq_b, and a length outside [0, capacity] (kept as it is: it is not clamped in place)"""
    D, dtype, fmt, ps = 128, BF16, "e4m3", 64
    for name, lens in (("C", (400, 257, 144)), ("D", (10, 0, 272)), ("B", (191, 3, -5))):
        G, sq, _ = T.CASES[name]
        t = T.tables(name, ps, 2)
        c = _cache(t, D, dtype, fmt, _pack(*_rows(t, D, fmt, 95), fmt), lens=list(lens))
        cu = V.cu_of(sq)
        idx, cnt = T.accept_lists(sq, 1, "wild")
        k0, v0 = _unpacked(c, D)
        want_lens, dests = T.compact_rows(k0, t.table, ps, list(lens), cu, idx, cnt)
        T.compact_rows(v0, t.table, ps, list(lens), cu, idx, cnt)
        qa.paged_kv_cache_compact_fp8(c, _su(cu), _su(idx), _su(cnt))
        k1, v1 = _unpacked(c, D)
        assert c.seqlens.tolist() == want_lens and np.array_equal(k0, k1) and np.array_equal(v0, v1), name
        for b, (n, L) in enumerate(zip(sq, lens)):
            if not (1 <= n <= 64 and 0 <= L and L >= n):
                assert want_lens[b] == lens[b] and dests[b] == [], (name, b)


# ---- 5. graph -----------------------------------------------------------------------------------------------------------------------------
def test_one_captured_tree_attend_and_compact_follows_its_rewritten_inputs():
    """captured once; replayed after rewriting tree_mask, accept_index, accept_lens, seqlens and the table: each replay equals the eager
    calls on the same contents, bit for bit"""
    D, dtype, fmt, ps, name = 128, BF16, "e4m3", 64, "A"
    G, sq, lens = T.CASES[name]
    t = T.tables(name, ps, 7)
    pools = _pack(*_rows(t, D, fmt, 33, poison=False), fmt)
    mk = lambda: _cache(t, D, dtype, fmt, pools)
    graphed, eager, warm = mk(), mk(), mk()
    cu, mx, total = V.cu_of(sq), max(sq), sum(sq)
    cud = _su(cu)
    q = _rand((total, HKV * G, D), dtype, 34)
    ws, ai, al = _words(T.words_of("chain", sq)[0]), _su([0] * total), _su([0] * B)

    def step(c, w, i, n):
        res = qa.fp8_attn_paged_varlen_tree_func(q, c, cud, mx, w, num_splits=3, return_lse=True)
        qa.paged_kv_cache_compact_fp8(c, cud, i, n)
        return res

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(warm, ws, ai, al)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s, lse_s = step(graphed, ws, ai, al)
    assert graphed.seqlens.tolist() == list(lens)                   # capture ran nothing
    spare = [p for p in range(t.num_pages) if p != P.POISON and p not in set(t.table.flatten().tolist())]
    for s, kind in enumerate(("random", "star", "binary")):
        for c in (graphed, eager):
            c.seqlens.copy_(_su(lens))                              # the drafts of the next step are appended: the lengths are back
            if s == 1:                                              # slot 0 moves its first page
                old = int(c.block_table[0, 0])
                c.k.view(c.num_pages, -1)[spare[0]] = c.k.view(c.num_pages, -1)[old]
                c.v.view(c.num_pages, -1)[spare[0]] = c.v.view(c.num_pages, -1)[old]
                c.block_table[0, 0] = spare[0]
            if s == 2:
                c.seqlens[1] -= 3
        w = _words(T.words_of(kind, sq, s)[0])
        idx, cnt = T.accept_lists(sq, s, "wild" if s == 1 else "path")
        for dst, src in zip((ws, ai, al), (w, _su(idx), _su(cnt))):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        out, lse = step(eager, w, _su(idx), _su(cnt))
        assert _same_bits(out_s, out) and _same_bits(lse_s, lse), s
        assert graphed.seqlens.tolist() == eager.seqlens.tolist() and graphed.seqlens.tolist() != list(lens), s
        assert torch.equal(graphed.k, eager.k) and torch.equal(graphed.v, eager.v), s


def test_torch_compile_fullgraph_of_append_tree_attend_and_compact_gives_the_eager_bits():
    D, dtype, fmt, ps, name = 128, BF16, "e4m3", 128, "B"
    ca, t, sq, base, kd, vd = _committed(name, ps, D, dtype, fmt, 50)
    cb = _committed(name, ps, D, dtype, fmt, 50)[0]
    cu, mx = V.cu_of(sq), max(sq)
    q = _rand((sum(sq), 8, D), dtype, 51)
    words, parents = T.words_of("binary", sq, 1)
    idx, cnt = T.accept_lists(sq, 2, "path")
    par, cud, ai, al = _su(parents), _su(cu), _su(idx), _su(cnt)

    def step(cache):
        def f(q, kd, vd, cu, par, ai, al):
            qa.paged_kv_cache_append_varlen_fp8(cache, kd, vd, cu)
            out = qa.fp8_attn_paged_varlen_tree_func(q * 2, cache, cu, mx, qa.tree_mask_from_parents(par, cu), num_splits=2, return_lse=True)
            qa.paged_kv_cache_compact_fp8(cache, cu, ai, al)
            return out
        return f

    torch._dynamo.reset()
    got = torch.compile(step(ca), fullgraph=True)(q, kd, vd, cud, par, ai, al)
    want = step(cb)(q, kd, vd, cud, par, ai, al)
    assert all(_same_bits(x, y) for x, y in zip(got, want))
    assert ca.seqlens.tolist() == cb.seqlens.tolist() and torch.equal(ca.k, cb.k) and torch.equal(ca.v, cb.v)
    assert torch.equal(qa.tree_mask_from_parents(par, cud).cpu(), torch.from_numpy(T.as_int64(words)))

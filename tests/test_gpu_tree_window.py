"""The tree under a sliding window, optionally with learned sinks, on the MI355X (quantumattention_amd/tree.py
`fp8_attn_paged_varlen_tree_window_func`, include/qattn_paged_varlen_tree_window.h).

Two oracles.  EXACT: the header's four identities, bit for bit in out, lse, row_path and the partials -- left = -1 without sinks is the tree
entry; a chain is the window entry, with sinks the sink entry; with sinks the partials are the sink-free call's and the sink merge of them
gives out and lse; every slot's rows are those of the call on that slot alone.  fp64: on general trees every row is held to
tests/tree_window_cases.reference on the call's own de-quantised q8 and the pools' de-quantised bytes, within the project's fp8-V bound
(tests/gpu_utils.assert_within_bound), and the count probe of tests/probes.py to its closed form under the window.  Shapes, windows and
the restated rule: tests/tree_window_cases.py."""
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
from tests import tree_window_cases as W
from tests.test_gpu_paged import _cache, _pack, _rand, _rows, _same_bits, _su
from tests.test_gpu_tree import _dequantised

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV, CAP = W.B, W.HKV, W.CAP
BF16, FP16 = torch.bfloat16, torch.float16
# (case, page size, D, dtype): every case at every page size with D = 128; D = 64, D = 256 and fp16 on one case each, as the tree test
CFGS = [(name, ps, 128, BF16) for name in W.CASES for ps in P.PAGE_SIZES] + [("A", 128, 64, BF16), ("D", 64, 256, BF16), ("B", 256, 128, FP16),
                                                                             ("E", 128, 64, FP16)]
CFG_IDS = [f"{n}-ps{ps}-d{D}-{str(dt)[6:]}" for n, ps, D, dt in CFGS]
NAMES = ("out", "lse", "partial_o", "partial_lse", "partial_path", "row_path")
SCALE_1 = torch.tensor([[0.5, 1.0], [0.75, 0.6], [1.0, 0.4]]) / 8


def _words(words):
    return torch.from_numpy(T.as_int64(words)).to(DEV)


def _sinks(Hq, seed=0):
    """one logit per query head, of the order of the scores"""
    return (torch.randn(Hq, generator=torch.Generator().manual_seed(100 + seed)) * 1.5).to(DEV)


def _setup(name, ps, D, dtype, seed, fmt="e4m3", scale_k=None):
    G, sq, lens = W.CASES[name]
    t = W.tables(name, ps, seed)
    rk, rv = _rows(t, D, fmt, seed)
    kw = {} if scale_k is None else {"scale_k": scale_k}
    c = _cache(t, D, dtype, fmt, _pack(rk, rv, fmt), **kw)
    q = _rand((sum(sq), HKV * G, D), dtype, seed + 1, mul=1.5)
    return G, sq, lens, t, rk, rv, c, q


def _call(q, c, cu, mx, words=None, window=None, sinks=None, **kw):
    mask = dict(is_causal=True) if words is None and window is None else {}
    if words is not None:
        mask["tree_mask"] = words
    if window is not None:
        mask["window"] = window
    if sinks is not None:
        mask["sinks"] = sinks
    return _native.fp8_attention_paged_varlen(q, c.k, c.v, c.scale_k, c.scale_v, c.block_table, c.seqlens, cu, max_seqlen_q=mx, Skv=CAP,
                                              num_pages=c.num_pages, page_size=c.page_size, fp8_dtype=P.FP8[c.fp8_format], **mask, **kw)


# ---- 1. the exact oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ps,D,dtype", CFGS, ids=CFG_IDS)
def test_identity_1_an_unbounded_window_without_sinks_is_the_tree_entry(name, ps, D, dtype):
    G, sq, lens, t, rk, rv, c, q = _setup(name, ps, D, dtype, 3)
    cud, mx = _su(V.cu_of(sq)), max(sq)
    for kind in ("random", "binary", "zero"):
        words = _words(T.words_of(kind, sq, 2)[0])
        for ns in (1, 2, 3, 0):
            for precision in ("accurate", "fast"):
                kw = dict(precision=precision, num_splits=ns, return_lse=True, return_partials=True, return_path=True)
                got, want = _call(q, c, cud, mx, words, (-1, 0), **kw), _call(q, c, cud, mx, words, **kw)
                for nm, x, y in zip(NAMES, got, want):
                    assert _same_bits(x, y), (name, ps, kind, ns, precision, nm)
        # the byte sweep: fast, one split, no LSE
        assert _same_bits(_call(q, c, cud, mx, words, (-1, 0), precision="fast", num_splits=1), _call(q, c, cud, mx, words, precision="fast", num_splits=1))


@pytest.mark.parametrize("name,ps,D,dtype", CFGS, ids=CFG_IDS)
def test_identity_2_a_chain_is_the_window_entry_and_with_sinks_the_sink_entry(name, ps, D, dtype):
    """out, lse, row_path and the partials; every window, num_splits 1 / 2 / 3 / 0, both precisions, and the byte sweep"""
    G, sq, lens, t, rk, rv, c, q = _setup(name, ps, D, dtype, 4)
    cud, mx = _su(V.cu_of(sq)), max(sq)
    words, sinks = _words(T.words_of("chain", sq)[0]), _sinks(HKV * G)
    for window in W.WINDOWS:
        for ns in (1, 2, 3, 0):
            for precision in ("accurate", "fast"):
                kw = dict(precision=precision, num_splits=ns, return_lse=True, return_partials=True, return_path=True)
                for s in (None, sinks):
                    got, want = _call(q, c, cud, mx, words, window, s, **kw), _call(q, c, cud, mx, None, window, s, **kw)
                    assert len(got) == len(want) == 6
                    for nm, x, y in zip(NAMES, got, want):
                        assert _same_bits(x, y), (name, ps, window, ns, precision, s is not None, nm)
        assert _same_bits(_call(q, c, cud, mx, words, window, precision="fast", num_splits=1),
                          _call(q, c, cud, mx, None, window, precision="fast", num_splits=1)), window
    pub = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cud, mx, words, (127, 0), sinks=sinks, num_splits=2, return_lse=True, return_partials=True)
    ref = qa.fp8_attn_paged_varlen_sink_func(q, c, cud, mx, sinks, (127, 0), num_splits=2, return_lse=True, return_partials=True)
    assert len(pub) == len(ref) == 5 and all(_same_bits(x, y) for x, y in zip(pub, ref))


@pytest.mark.parametrize("name,ps,D,dtype", CFGS, ids=CFG_IDS)
def test_identity_3_with_sinks_the_partials_are_sink_free_and_their_sink_merge_is_the_call(name, ps, D, dtype):
    G, sq, lens, t, rk, rv, c, q = _setup(name, ps, D, dtype, 5)
    cud, mx = _su(V.cu_of(sq)), max(sq)
    words, sinks = _words(T.words_of("random", sq, 5)[0]), _sinks(HKV * G, 1)
    for window in W.WINDOWS:
        for ns in (2, 3):
            for precision in ("accurate", "fast"):
                kw = dict(num_splits=ns, precision=precision, return_lse=True, return_partials=True)
                out, lse, po, plse, ppath = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cud, mx, words, window, sinks=sinks, **kw)
                free = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cud, mx, words, window, **kw)
                assert _same_bits(po, free[2]) and _same_bits(plse, free[3]) and _same_bits(ppath, free[4]), (window, ns, precision)
                m_out, m_lse = qa.merge_attn_states_with_sinks(list(po), list(plse), sinks, out_dtype=q.dtype)
                assert _same_bits(m_out, out) and _same_bits(m_lse, lse), (window, ns, precision)


@pytest.mark.parametrize("name,ps", [("A", 128), ("B", 64), ("C", 256), ("D", 64), ("E", 128)])
def test_identity_4_every_slots_rows_are_the_bits_of_the_call_on_that_slot_alone(name, ps):
    D, dtype = 128, BF16
    G, sq, lens, t, rk, rv, c, q = _setup(name, ps, D, dtype, 60)
    cu, mx = V.cu_of(sq), max(sq)
    words, sinks = _words(T.words_of("random", sq, 2)[0]), _sinks(HKV * G, 2)
    for window, s in (((63, 0), None), ((127, 0), sinks), ((1100, 0), None), ((-1, 0), sinks)):
        for ns, precision in ((1, "accurate"), (2, "fast"), (3, "accurate")):
            kw = dict(sinks=s, num_splits=ns, precision=precision, return_lse=True, return_partials=True)
            got = qa.fp8_attn_paged_varlen_tree_window_func(q, c, _su(cu), mx, words, window, **kw)
            for b, n in enumerate(sq):
                if n == 0:
                    continue
                one = qa.fp8_attn_paged_varlen_tree_window_func(q[cu[b]:cu[b + 1]].contiguous(), V.one_slot(c, b), _su([0, n]), mx,
                                                                words[cu[b]:cu[b + 1]].contiguous(), window, **kw)
                for x, y, kind in zip(got, one, ("o", "l", "po", "pl", "pl")):
                    if x.numel() == 0:
                        assert y.numel() == 0
                        continue
                    assert _same_bits(V.rows_of(x, kind, cu, b), V.rows_of(y, kind, [0, n], 0)), (name, ps, window, ns, b, kind)


def test_slots_above_64_queries_are_the_window_entrys_and_junk_bits_above_p_change_no_bit():
    D, dtype, ps = 128, BF16, 64
    G, sq, lens, t, rk, rv, c, q = _setup("C", ps, D, dtype, 5)
    cu, mx = V.cu_of(sq), max(sq)
    for window in ((63, 0), (127, 0)):
        kw = dict(num_splits=2, return_lse=True, return_path=True)
        got, want = _call(q, c, _su(cu), mx, _words(T.words_of("random", sq, 9)[0]), window, **kw), _call(q, c, _su(cu), mx, None, window, **kw)
        for b in (0, 1):
            for x, y, kind in zip(got, want, ("o", "l", "l")):
                assert _same_bits(V.rows_of(x, kind, cu, b), V.rows_of(y, kind, cu, b)), (window, b, kind)
        assert not _same_bits(V.rows_of(got[0], "o", cu, 2), V.rows_of(want[0], "o", cu, 2))
    for name in ("A", "E"):
        G, sq, lens, t, rk, rv, c, q = _setup(name, ps, D, dtype, 6)
        cud, mx = _su(V.cu_of(sq)), max(sq)
        clean = T.words_of("random", sq, 4)[0]
        rng = np.random.RandomState(8)
        dirty = [w | ((int(rng.randint(0, 1 << 32)) << 32 | int(rng.randint(0, 1 << 32))) & ~((2 << p) - 1) & T.MASK64)
                 for w, p in zip(clean, [p for n in sq for p in range(n)])]
        assert dirty != clean
        kw = dict(sinks=_sinks(HKV * G), num_splits=2, precision="fast", return_lse=True, return_partials=True, return_path=True)
        a, b_ = _call(q, c, cud, mx, _words(clean), (127, 0), **kw), _call(q, c, cud, mx, _words(dirty), (127, 0), **kw)
        assert all(_same_bits(x, y) for x, y in zip(a, b_)), name


# ---- 2. the fp64 oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("star", "binary", "random", "zero", "junk"))
@pytest.mark.parametrize("name,ps,D,dtype", CFGS, ids=CFG_IDS)
def test_every_row_of_a_general_tree_is_within_the_fp8_v_bound_of_the_fp64_reference(name, ps, D, dtype, kind):
    i = CFGS.index((name, ps, D, dtype)) + W.KINDS.index(kind)
    ns, precision = (1, 2, 3, 0)[i % 4], ("accurate", "fast")[(i // 4) % 2]
    window, with_sinks = W.WINDOWS[i % len(W.WINDOWS)], (i // 2) % 2 == 0
    # scales of order 1: the de-quantised keys and values are of order 1, so that the absolute part of the bound is not slack
    G, sq, lens, t, rk, rv, c, q = _setup(name, ps, D, dtype, 20 + i, scale_k=SCALE_1)
    Hq, cu, mx = HKV * G, V.cu_of(sq), max(sq)
    words = T.words_of(kind, sq, i)[0]
    sinks = _sinks(Hq, i) if with_sinks else None
    out, lse, q8, sqs, path = _call(q, c, _su(cu), mx, _words(words), window, sinks, num_splits=ns, precision=precision, return_lse=True,
                                    return_quant=True, return_path=True)
    qd, kd, vd = _dequantised(q8, sqs, rk, rv, c, t, sq, Hq, D)
    ref, ref_lse = W.reference(qd, kd, vd, lens, sq, G, words, 1.0 / np.sqrt(D), window[0], None if sinks is None else sinks.double().cpu().numpy())
    assert not np.isnan(ref).any() and not np.isnan(ref_lse).any()
    o, l, pth = gpu_utils.out_to_f32(out), lse.cpu().numpy(), path.cpu().numpy()
    mxe, rmse = gpu_utils.assert_within_bound(o.transpose(1, 0, 2), gpu_utils.PathRef(ref.transpose(1, 0, 2), ref.transpose(1, 0, 2)), pth,
                                              what=(name, ps, kind, window, ns, precision, with_sinks))
    keyless = np.array([[not W.row_keep(words, cu[b], n, L, h % G * n + p, max(L, 1), window[0])[:L].any() for b, (n, L) in enumerate(zip(sq, lens))
                         for p in range(n)] for h in range(Hq)])
    assert (o.transpose(1, 0, 2)[keyless] == 0).all(), "a row without a key is a zero row"
    if sinks is None:
        assert (np.isneginf(l) == keyless).all() and (np.isneginf(ref_lse) == keyless).all()
    else:
        assert (l[keyless] == np.broadcast_to(sinks.cpu().numpy()[:, None], l.shape)[keyless]).all(), "... with LSE sink_h"
    live = np.isfinite(ref_lse)
    worst_lse = float(np.abs(l[live] - ref_lse[live]).max()) if live.any() else 0.0
    print(f"tree-window {name} ps{ps} D{D} {kind} {window} sinks={with_sinks} ns={ns} {precision}: max-abs {mxe:.3e} rmse {rmse:.3e} "
          f"worst LSE error {worst_lse:.3e}")
    assert worst_lse < probes.LSE_TOL, worst_lse


@pytest.mark.parametrize("name,ps", [("A", 64), ("B", 128), ("D", 256), ("C", 64), ("E", 128)])
def test_the_count_probe_gives_its_closed_form_under_the_window(name, ps):
    """q_r = -g_r 1, k = 0.5 1, V[j] = e_(j mod D): O[r, c] = n_c(r) / n(r) from the boolean mask of the rule alone, in integers; bound
    |got - ref| <= REL ref (tests/probes.py, the CPU test's bound)"""
    D, dtype, fmt = 128, BF16, "e4m3"
    G, sq, lens = W.CASES[name]
    Hq, cu = HKV * G, V.cu_of(sq)
    t = W.tables(name, ps, 1)
    fp8 = P.FP8[fmt]
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
    for kind in ("star", "binary", "random"):
        words = T.words_of(kind, sq, 3)[0]
        for window in W.WINDOWS:
            for ns, precision in ((1, "accurate"), (2, "fast"), (3, "accurate")):
                out = gpu_utils.out_to_f32(_call(q, c, _su(cu), max(sq), _words(words), window, num_splits=ns, precision=precision))
                for b, (n, L) in enumerate(zip(sq, lens)):
                    if n == 0:
                        continue
                    ref, tot = probes.count_expected(W.slot_mask(words, cu[b], n, L, G, CAP, window[0]), D)
                    got = out[cu[b]:cu[b + 1]].transpose(1, 0, 2)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        ratio = np.where(got == ref, 0.0, np.abs(got - ref) / probes.count_bound(ref, dtype))
                    worst = max(worst, float(ratio.max()))
                    assert (got[tot == 0] == 0).all()
    print(f"tree-window count probe {name} ps{ps}: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0, worst


# ---- 3. bytes nobody attends, and the sink's special values ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ps", [("A", 64), ("C", 128), ("E", 256), ("E", 64)])
def test_nan_bytes_below_every_window_and_on_free_pages_move_no_bit(name, ps):
    """the keys below lo_i = max(delta - left, 0) of every slot -- those that share the window's first chunk included -- hold NaN bytes in K
    and V; the free pages hold them already (tests/paged_cases.POISON)"""
    D, dtype, fmt = 128, BF16, "e4m3"
    G, sq, lens, t, rk, rv, c, q = _setup(name, ps, D, dtype, 70)
    cu, mx = V.cu_of(sq), max(sq)
    words, sinks = _words(T.words_of("binary", sq, 1)[0]), _sinks(HKV * G, 3)
    poisoned = 0
    for left in (63, 127, 300):
        nk, nv = rk.clone(), rv.clone()
        dead = 0
        for b, (n, L) in enumerate(zip(sq, lens)):
            for j in range(min(max(L - n - left, 0), L) if n else 0):
                page, slot = P.lookup(t.table, b, j, ps)
                nk[page, :, slot], nv[page, :, slot] = P.NAN_BYTE[fmt], P.NAN_BYTE[fmt]
                dead += 1
        poisoned += dead
        if not dead:         # (a window that holds every key of every slot of this case)
            continue
        cn = _cache(t, D, dtype, fmt, _pack(nk, nv, fmt))
        for s in (None, sinks):
            for ns, precision in ((1, "accurate"), (2, "fast"), (1, "fast")):
                kw = dict(sinks=s, num_splits=ns, precision=precision, return_lse=True, return_partials=True)
                a = qa.fp8_attn_paged_varlen_tree_window_func(q, c, _su(cu), mx, words, (left, 0), **kw)
                b_ = qa.fp8_attn_paged_varlen_tree_window_func(q, cn, _su(cu), mx, words, (left, 0), **kw)
                assert all(_same_bits(x, y) for x, y in zip(a, b_)), (name, ps, left, ns, precision)
                assert not torch.isnan(b_[0].float()).any()
    assert poisoned > 0


def test_a_sink_of_minus_inf_is_no_sink_and_plus_inf_or_nan_poison_their_head_alone():
    D, dtype, ps = 128, BF16, 128
    G, sq, lens, t, rk, rv, c, q = _setup("E", ps, D, dtype, 80)
    Hq, cud, mx = HKV * G, _su(V.cu_of(sq)), max(sq)
    words = _words(T.words_of("random", sq, 1)[0])
    for ns in (1, 2):
        kw = dict(num_splits=ns, return_lse=True)
        free = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cud, mx, words, (127, 0), **kw)
        none = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cud, mx, words, (127, 0), sinks=torch.full((Hq,), -torch.inf, device=DEV), **kw)
        assert all(_same_bits(x, y) for x, y in zip(free, none)), ns
        base = _sinks(Hq, 4)
        good = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cud, mx, words, (127, 0), sinks=base, **kw)
        for bad in (torch.inf, torch.nan):
            s = base.clone()
            s[1] = bad
            out, lse = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cud, mx, words, (127, 0), sinks=s, **kw)
            assert torch.isnan(out[:, 1].float()).all() and torch.isnan(lse[1]).all(), (ns, bad)
            keep = [h for h in range(Hq) if h != 1]
            assert _same_bits(out[:, keep], good[0][:, keep]) and _same_bits(lse[keep], good[1][keep]), (ns, bad)


# ---- 4. graph and compile -------------------------------------------------------------------------------------------------------------------
def test_one_captured_attend_follows_rewritten_words_cu_seqlens_table_and_sinks():
    D, dtype, fmt, ps, name = 128, BF16, "e4m3", 64, "A"
    G, sq, lens = W.CASES[name]
    t = W.tables(name, ps, 7)
    pools = _pack(*_rows(t, D, fmt, 33, poison=False), fmt)
    graphed, eager = _cache(t, D, dtype, fmt, pools), _cache(t, D, dtype, fmt, pools)
    Hq, mx, total = HKV * G, max(sq), sum(sq)
    q = _rand((total, Hq, D), dtype, 34)
    ws, cud, sk = _words(T.words_of("chain", sq)[0]), _su(V.cu_of(sq)), _sinks(Hq, 5)
    step = lambda c, w, cu, s: qa.fp8_attn_paged_varlen_tree_window_func(q, c, cu, mx, w, (127, 0), sinks=s, num_splits=3, return_lse=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(eager, ws, cud, sk)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s, lse_s = step(graphed, ws, cud, sk)
    spare = [p for p in range(t.num_pages) if p != P.POISON and p not in set(t.table.flatten().tolist())]
    for s, kind in enumerate(("random", "star", "binary")):
        sq_s = (sq, (10, 40, 8), sq)[s]                                   # replay 1: other query counts (same total bucket: rows behind cu[B])
        for c in (graphed, eager):
            if s == 1:                                                  # slot 0 moves its first page
                old = int(c.block_table[0, 0])
                c.k.view(c.num_pages, -1)[spare[0]] = c.k.view(c.num_pages, -1)[old]
                c.v.view(c.num_pages, -1)[spare[0]] = c.v.view(c.num_pages, -1)[old]
                c.block_table[0, 0] = spare[0]
            if s == 2:
                c.seqlens[1] -= 3
        w = T.words_of(kind, sq_s, s)[0]
        w = _words(w + [0] * (total - len(w)))
        cu_s, s_s = _su(V.cu_of(sq_s)), _sinks(Hq, 6 + s)
        for dst, src in zip((ws, cud, sk), (w, cu_s, s_s)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        out, lse = step(eager, w, cu_s, s_s)
        n = sum(sq_s)
        assert _same_bits(out_s[:n], out[:n]) and _same_bits(lse_s[:, :n], lse[:, :n]), s


def test_torch_compile_fullgraph_of_the_whole_step_gives_the_eager_bits():
    from tests.test_gpu_tree import _committed
    D, dtype, fmt, ps, name = 128, BF16, "e4m3", 128, "B"
    ca, t, sq, base, kd, vd = _committed(name, ps, D, dtype, fmt, 50)
    cb = _committed(name, ps, D, dtype, fmt, 50)[0]
    cu, mx = V.cu_of(sq), max(sq)
    q, sinks = _rand((sum(sq), 8, D), dtype, 51), _sinks(8, 9)
    words, parents = T.words_of("binary", sq, 1)
    idx, cnt = T.accept_lists(sq, 2, "path")
    par, cud, ai, al = _su(parents), _su(cu), _su(idx), _su(cnt)

    def step(cache):
        def f(q, kd, vd, cu, par, ai, al, sinks):
            qa.paged_kv_cache_append_varlen_fp8(cache, kd, vd, cu)
            out = qa.fp8_attn_paged_varlen_tree_window_func(q * 2, cache, cu, mx, qa.tree_mask_from_parents(par, cu), (127, 0), sinks=sinks,
                                                            num_splits=2, return_lse=True)
            qa.paged_kv_cache_compact_fp8(cache, cu, ai, al)
            return out
        return f

    torch._dynamo.reset()
    got = torch.compile(step(ca), fullgraph=True)(q, kd, vd, cud, par, ai, al, sinks)
    want = step(cb)(q, kd, vd, cud, par, ai, al, sinks)
    assert all(_same_bits(x, y) for x, y in zip(got, want))
    assert ca.seqlens.tolist() == cb.seqlens.tolist() and torch.equal(ca.k, cb.k) and torch.equal(ca.v, cb.v)


# ---- 5. FAST's selection on a head-interior tile ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,cap,ps,left,ns", W.STRADDLE, ids=[f"L{s[0]}-w{s[3]}-ns{s[4]}" for s in W.STRADDLE])
def test_the_depth_reduction_decides_fasts_selection_on_a_head_interior_tile(L, cap, ps, left, ns):
    """tests/tree_window_cases.STRADDLE: in split 0 the tile inside the third head (positions 8 .. 59) sweeps 1022 keys counted from its
    least depth on a chain, 1029 on a star, the tile across the head boundaries 1030 -- on either side of FAST's 1024.  The path bytes
    the kernel writes are the rule's: a reduction that starts the tile at depth 0 makes the chain's tile ONE_TERM (and leaves identity 2),
    one that starts it at its least position makes the star's TWO_TERM.  On a chain all six outputs are the window entry's, with sinks
    the sink entry's -- row_path and partial_path included.
    The star's values: its LSE under FAST (exact exponentials: it moves with any wrongly kept or dropped key) to probes.LSE_TOL, its
    outputs under ACCURATE to the fp8-V bound.  The outputs of FAST's one-term launch are NOT held to the flat 2^-6 here: a weight
    rounded once to e4m3 carries up to 2^-4 of itself, so the bound does not follow from the formats on this cache's unit-variance V;
    measured on the MI355X, worst |err| / bound of the one-term rows: the unchanged window entry on a chain 0.95 (1200 keys) and 0.82
    (2200 keys, two splits), this call on the star 0.95 and 1.09 (1.21 with one split); under ACCURATE 0.07 .. 0.17 throughout."""
    D, dtype = 64, BF16
    c, q, cu = W.straddle_setup(L, cap, ps, D, dtype, DEV)
    G, n = W.STRADDLE_G, W.STRADDLE_SQ
    sinks = _sinks(HKV * G, 11)
    call = lambda words, s, **kw: _native.fp8_attention_paged_varlen(
        q, c.k, c.v, c.scale_k, c.scale_v, c.block_table, c.seqlens, cu, max_seqlen_q=n, Skv=cap, num_pages=c.num_pages, page_size=ps,
        fp8_dtype=P.FP8[c.fp8_format], precision="fast", num_splits=ns, return_lse=True, return_partials=True, return_path=True, window=(left, 0),
        **({} if words is None else {"tree_mask": words}), **({} if s is None else {"sinks": s}), **kw)
    for kind in ("chain", "star"):
        words = _words(W.straddle_words(kind))
        want = W.straddle_codes(kind, L, left, ns, _native.PATH_ONE_TERM, _native.PATH_TWO_TERM)
        inner = want[0, G - 1, 8:]
        assert (inner == (_native.PATH_TWO_TERM if kind == "chain" else _native.PATH_ONE_TERM)).all() and (want[0, 0] == _native.PATH_ONE_TERM).all()
        for s in (None, sinks):
            got = call(words, s)
            per_split = got[4].cpu().numpy() if ns > 1 else got[5].cpu().numpy()[None]     # partial_path, or row_path with one split
            assert np.array_equal(per_split, want), (kind, s is not None)
            if kind == "chain":
                for nm, x, y in zip(NAMES, got, call(None, s)):
                    assert _same_bits(x, y), (nm, s is not None)
    # ... and the values of the star against the fp64 reference (docstring)
    words = W.straddle_words("star")
    star = lambda precision: _native.fp8_attention_paged_varlen(
        q, c.k, c.v, c.scale_k, c.scale_v, c.block_table, c.seqlens, cu, max_seqlen_q=n, Skv=cap, num_pages=c.num_pages, page_size=ps,
        fp8_dtype=P.FP8[c.fp8_format], precision=precision, num_splits=ns, return_lse=True, return_quant=True, return_path=True, window=(left, 0),
        tree_mask=_words(words))
    lse = star("fast")[1]
    out, lse_acc, q8, sqs, path = star("accurate")
    fp8 = P.FP8[c.fp8_format]
    qd = (q8.view(torch.uint8).view(fp8).float().cpu().numpy().astype(np.float64).reshape(HKV * G, n, D)
          * sqs[0].cpu().numpy().astype(np.float64)[:, None, None]).transpose(1, 0, 2)
    rows_of = lambda pool, layout: torch.from_numpy(gpu_utils.unpack_frag(gpu_utils.bits8(pool), layout, c.num_pages, HKV, ps, D).copy()).view(fp8)
    un = lambda pool, layout, s: (rows_of(pool, layout).float().numpy().astype(np.float64)[c.block_table[0].cpu().numpy()]
                                  .transpose(1, 0, 2, 3).reshape(HKV, cap, D) * s[0].cpu().numpy().astype(np.float64)[:, None, None])[None]
    ref, ref_lse = W.reference(qd, un(c.k, _native.LAYOUT_KFRAG, c.scale_k), un(c.v, _native.LAYOUT_VFRAG, c.scale_v), [L], [n], G, words,
                               1.0 / np.sqrt(D), left)
    o = gpu_utils.out_to_f32(out)
    gpu_utils.assert_within_bound(o.transpose(1, 0, 2), gpu_utils.PathRef(ref.transpose(1, 0, 2), ref.transpose(1, 0, 2)), path.cpu().numpy(),
                                  what=("straddle", L, left, ns))
    assert float(np.abs(lse.cpu().numpy() - ref_lse).max()) < probes.LSE_TOL and float(np.abs(lse_acc.cpu().numpy() - ref_lse).max()) < probes.LSE_TOL

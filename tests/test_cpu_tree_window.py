"""CPU tests of the tree under a sliding window with learned sinks and of the rotary embedding at the caller's positions
(quantumattention_amd/tree.py, quantumattention_amd/paged_varlen.py, include/qattn_paged_varlen_tree_window.h,
include/qattn_paged_varlen_rope_pos.h): the surface, the reason functions, the eager definitions against the rules restated in
tests/tree_window_cases.py, `tree_positions` against a plain walk, and the teeth of the count probe against the named mutants of the
rule."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, nn, paged_varlen, tree
from quantumattention_amd.rope import apply_rope_eager
from tests import paged_varlen_cases as V
from tests import paged_varlen_rope_cases as RC
from tests import probes
from tests import tree_cases as T
from tests import tree_window_cases as W
from tests.conftest import ROOT
from tests.test_cpu_tree import SCALES, _dequantised, _i32, _rand, _same_bits, _words

B, HKV, CAP = W.B, W.HKV, W.CAP
BF16, FP16 = torch.bfloat16, torch.float16
PS_OF = {"A": 64, "B": 128, "C": 256, "D": 64, "E": 128}


def _with_drafts(name, ps, D, dtype, seed):
    """a row-major cache that holds a case's committed keys and drafts at the case's lengths, and queries (tests/test_cpu_tree.py's, on
    this file's cases)"""
    G, sq, lens = W.CASES[name]
    base = [max(L - n, 0) for n, L in zip(sq, lens)]
    t = W.tables(name, ps, seed, [b + n for b, n in zip(base, sq)])
    c = qa.alloc_paged_kv_cache_fp8(t.num_pages, HKV, ps, D, batch_size=B, max_pages_per_seq=t.M, scale_k=SCALES, scale_v=SCALES * 2, dtype=dtype,
                                    device="cpu")
    c.block_table.copy_(torch.from_numpy(t.table))
    qa.paged_kv_cache_append_varlen_fp8(c, _rand((sum(base), HKV, D), dtype, seed + 1), _rand((sum(base), HKV, D), dtype, seed + 2),
                                        _i32(V.cu_of(base)))
    qa.paged_kv_cache_append_varlen_fp8(c, _rand((sum(sq), HKV, D), dtype, seed + 3), _rand((sum(sq), HKV, D), dtype, seed + 4), _i32(V.cu_of(sq)))
    c.seqlens.copy_(_i32(lens))
    return c, t, G, sq, lens, _rand((sum(sq), HKV * G, D), dtype, seed + 5, mul=1.5)


def test_the_cases_hold_what_they_are_meant_to():
    W.check_cases()


# ---- the surface --------------------------------------------------------------------------------------------------------------------------
def test_the_surface_signatures_symbols_schemas_and_fake_registrations():
    for name, mod in (("fp8_attn_paged_varlen_tree_window_func", tree), ("tree_positions", tree), ("apply_rope_positions", paged_varlen),
                      ("paged_kv_cache_append_varlen_rope_pos_fp8", paged_varlen)):
        assert getattr(qa, name) is getattr(mod, name) and name not in qa.__all__
    sig = inspect.signature(qa.fp8_attn_paged_varlen_tree_window_func)
    assert list(sig.parameters) == ["q", "cache", "cu_seqlens_q", "max_seqlen_q", "tree_mask", "window_size", "sinks", "scale", "seqused_k",
                                    "max_seqlen_k", "num_splits", "precision", "return_lse", "return_partials"]
    kwonly = {k: p.default for k, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kwonly == dict(sinks=None, scale=None, seqused_k=None, max_seqlen_k=None, num_splits=0, precision="accurate", return_lse=False,
                          return_partials=False)
    pin = lambda f: [(n, p.kind is inspect.Parameter.KEYWORD_ONLY, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert pin(qa.paged_kv_cache_append_varlen_rope_pos_fp8) == [(n, False, E) for n in ("cache", "k_new", "v_new", "cu_seqlens", "positions", "cos", "sin")] \
        + [("interleaved", True, False), ("advance", True, True)]
    assert pin(qa.apply_rope_positions) == [(n, False, E) for n in ("x", "positions", "cos", "sin")] + [("interleaved", True, False), ("out", True, None)]
    assert pin(qa.tree_positions) == [(n, False, E) for n in ("tree_mask", "cu_seqlens_q", "seqlens")] + [("appended", True, False)]
    # the existing entries keep their arguments
    assert "window_size" not in inspect.signature(qa.fp8_attn_paged_varlen_tree_func).parameters
    assert "positions" not in inspect.signature(qa.paged_kv_cache_append_varlen_rope_fp8).parameters
    norm = lambda f: " ".join(open(os.path.join(ROOT, "include", f)).read().split()).replace(" * ", " ")
    header = norm("qattn_paged_varlen_tree_window.h")
    assert "qattn_fp8_attention_paged_varlen_tree_window_forward(" in header and "int window_left, int window_right, const float* sinks" in header
    for phrase in ("depth_p = popcount(w_p & (2^p - 1))", "depth_p = p", "j >= delta + depth_p - window_left", "draft keys j >= delta get no window test",
                   "window_right == 0 and window_left == -1 or window_left >= 63", "window_left < 63 under a tree", "trees above 64 tokens per slot"):
        assert phrase in header, phrase
    header = norm("qattn_paged_varlen_rope_pos.h")
    for phrase in ("clamp(positions[t], 0, T - 1)", "a partial rotary_dim", "multi-axis (M-RoPE) positions", "positions in the padded and the contiguous appends"):
        assert phrase in header, phrase
    for name in ("qattn_fp8_attention_paged_varlen_tree_window_forward", "qattn_paged_kv_cache_append_varlen_rope_pos_fp8", "qattn_rope_packed_positions"):
        assert name in _native.EXPORTS and hasattr(_native.lib(), name)
    assert _native.lib().qattn_abi_version() == 8
    att = torch.ops.quantumattention_amd.fp8_paged_varlen_splitkv_tree_window_attention_forward.default
    schema = str(att._schema)
    assert "!" not in schema and "Tensor tree_mask" in schema and "Int window_left, SymInt window_right, Tensor? sinks=None" in schema, schema
    app = torch.ops.quantumattention_amd.fp8_paged_varlen_rope_pos_kv_cache_append_.default
    schema = str(app._schema)
    assert "Tensor(a0!) k_pool" in schema and "Tensor(a1!) v_pool" in schema and "seqlens" in schema and schema.count("!") == 3, schema
    assert "Tensor positions" in schema and schema.endswith("-> ()")
    rot = torch.ops.quantumattention_amd.rope_packed_positions.default
    assert "!" not in str(rot._schema) and "Tensor positions" in str(rot._schema)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        q = torch.empty(39, 8, 128, dtype=FP16)
        u8, f32 = torch.empty(16, dtype=torch.uint8), torch.empty(3, 2)
        i32 = lambda n: torch.empty(n, dtype=torch.int32)
        w = torch.empty(39, dtype=torch.int64)
        res = att(q, u8, u8, f32, f32, torch.empty(3, 20, dtype=torch.int32), i32(3), i32(4), w, 17, 1280, 62, 64, 3, 127, 0, torch.empty(8), "e4m3",
                  "compiled", "fast", True, True)
        assert [tuple(x.shape) for x in res] == [(39, 8, 128), (8, 39), (3, 39, 8, 128), (3, 8, 39), (3, 8, 39)]
        assert [x.dtype for x in res] == [FP16, torch.float32, torch.float32, torch.float32, torch.uint8]
        res = att(q, u8, u8, f32, f32, torch.empty(3, 20, dtype=torch.int32), i32(3), i32(4), w, 17, 1280, 62, 64, 1, -1, 0)
        assert [tuple(x.shape) for x in res] == [(39, 8, 128), (0,), (0,), (0,), (0,)]
        tab = torch.empty(64, 64)
        assert app(u8, u8, f32, f32, torch.empty(3, 20, dtype=torch.int32), i32(3), q[:, :2], q[:, :2], i32(4), w, tab, tab, 62, 64) is None
        y = rot(q[:, :4], w, tab, tab, True)
        assert y.shape == (39, 4, 128) and y.dtype == FP16


def test_the_whole_step_traces_into_one_graph(monkeypatch):
    """torch.compile(fullgraph=True) traces   tree_positions -> rotate q -> positions append -> tree-window-sink attend -> compact   into ONE
    graph with nothing read on the host.  Traced on CPU tensors (fake implementations only), the device check patched away; the backend
    keeps the graph and stops the call before anything would run."""
    import torch._dynamo
    monkeypatch.setattr(nn, "_pre_check_can_use_hip_attention", lambda device: (True, ""))
    D, ps, dtype = 64, 64, BF16
    t = W.tables("A", ps)
    c = qa.alloc_paged_kv_cache_fp8(t.num_pages, HKV, ps, D, batch_size=B, max_pages_per_seq=t.M, scale_k=SCALES, scale_v=SCALES * 2, dtype=dtype,
                                    device="cpu")
    pool = torch.zeros((t.num_pages * HKV * ps * D,), dtype=torch.uint8)
    c = qa.PagedKVCacheFP8(pool, pool.clone(), c.scale_k, c.scale_v, c.block_table, c.seqlens, c.shape, c.fp8_format, c.dtype, c.numerics, "frag")
    G, sq, _ = W.CASES["A"]
    total = sum(sq)
    cos, sin = RC.tables(D, rows=CAP)

    def f(q, kd, vd, cu, par, ai, al, sinks):
        words = qa.tree_mask_from_parents(par, cu)
        pos = qa.tree_positions(words, cu, c.seqlens)
        q = qa.apply_rope_positions(q, pos, cos, sin)
        qa.paged_kv_cache_append_varlen_rope_pos_fp8(c, kd, vd, cu, pos, cos, sin)
        out = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cu, 40, words, (127, 0), sinks=sinks, num_splits=2, return_lse=True)
        qa.paged_kv_cache_compact_fp8(c, cu, ai, al)
        return out

    args = (_rand((total, HKV * G, D), dtype, 1), _rand((total, HKV, D), dtype, 2), _rand((total, HKV, D), dtype, 3), _i32(V.cu_of(sq)),
            _i32(T.words_of("binary", sq)[1]), _i32([0] * total), _i32([1] * B), torch.zeros(HKV * G))

    class Traced(Exception):
        pass

    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)

        def stop(*a):
            raise Traced
        return stop

    torch._dynamo.reset()
    with pytest.raises(Traced):
        torch.compile(f, fullgraph=True, dynamic=False, backend=backend)(*args)
    torch._dynamo.reset()
    assert len(graphs) == 1
    targets = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]
    order = [next(i for i, x in enumerate(targets) if name in x) for name in
             ("rope_packed_positions", "fp8_paged_varlen_rope_pos_kv_cache_append_", "fp8_paged_varlen_splitkv_tree_window_attention_forward",
              "fp8_paged_kv_cache_compact_")]
    assert order == sorted(order)
    assert not any(n.op == "call_method" and n.target in ("item", "tolist") for n in graphs[0].graph.nodes)
    assert not any("_local_scalar_dense" in x for x in targets)


# ---- the reason functions -------------------------------------------------------------------------------------------------------------------
def test_the_reason_functions_name_the_first_broken_rule():
    c, t, G, sq, lens, q = _with_drafts("A", 64, 128, BF16, 1)
    cu, w = _i32(V.cu_of(sq)), _words(T.words_of("star", sq)[0])
    sinks = torch.zeros(HKV * G)
    ok = lambda **kw: tree.paged_varlen_tree_window_input_reason(**{**dict(q=q, cache=c, cu_seqlens_q=cu, max_seqlen_q=40, tree_mask=w,
                                                                           window_size=(127, 0), sinks=sinks), **kw})
    assert ok() is None and ok(sinks=None) is None and ok(window_size=(-1, 0)) is None and ok(window_size=(63, 0)) is None
    assert ok(sinks=sinks.bfloat16()) is None
    for bad in ((62, 0), (0, 0), (-2, 0)):
        assert ">= 63" in ok(window_size=bad), bad
    for bad in ((127, 1), (127, -1), (-1, -1)):
        assert "right" in ok(window_size=bad), bad
    assert "pair" in ok(window_size=127) and "pair" in ok(window_size=(127.0, 0))
    assert "sinks" in ok(sinks=sinks[:-1]) and "sinks" in ok(sinks=sinks.double()) and "tree_mask" in ok(tree_mask=w[:-1])
    for bad in ((62, 0), (127, 1)):
        with pytest.raises(ValueError):
            qa.fp8_attn_paged_varlen_tree_window_func(q, c, cu, 40, w, bad)
    with pytest.raises(ValueError, match="precision"):
        qa.fp8_attn_paged_varlen_tree_window_func(q, c, cu, 40, w, (127, 0), precision="auto")
    D = 128
    cos, sin = RC.tables(D, rows=8)
    k = _rand((sum(sq), HKV, D), BF16, 2)
    pos = torch.zeros(sum(sq), dtype=torch.int64)
    okp = lambda **kw: paged_varlen.paged_varlen_rope_pos_append_input_reason(**{**dict(cache=c, k_new=k, v_new=k, cu_seqlens=cu, positions=pos, cos=cos,
                                                                                       sin=sin), **kw})
    assert okp() is None                                                   # (T = 8 < capacity: positions are clamped into the tables)
    assert "positions" in okp(positions=pos.int()) and "positions" in okp(positions=pos[:-1]) and "positions" in okp(positions=None)
    assert "contiguous" in okp(positions=torch.stack([pos, pos], 1)[:, 0]) and "cos" in okp(cos=cos[:, :-1]) and "cu_seqlens" in okp(cu_seqlens=cu.long())
    okr = lambda **kw: paged_varlen.rope_positions_input_reason(**{**dict(x=k, positions=pos, cos=cos, sin=sin), **kw})
    assert okr() is None and "positions" in okr(positions=pos.float()) and "3-D" in okr(x=k[0]) and "head_dim" in okr(x=k[..., :32], cos=cos[:, :16], sin=sin[:, :16])
    with pytest.raises(ValueError, match="positions"):
        qa.apply_rope_positions(k, pos[:-1], cos, sin)
    with pytest.raises(ValueError):
        qa.tree_positions(w.int(), cu, c.seqlens)


# ---- the eager definition of the attention ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(W.CASES))
def test_the_eager_identities_hold_bit_for_bit(name):
    """1. left = -1 without sinks is the eager tree entry; 2. a chain is the eager window entry, with sinks the eager sink entry;
    3. with sinks the partials are sink-free and their sink merge is the call"""
    c, t, G, sq, lens, q = _with_drafts(name, PS_OF[name], 128, BF16, 3)
    cud, mx = _i32(V.cu_of(sq)), max(sq)
    chain, rnd = _words(T.words_of("chain", sq)[0]), _words(T.words_of("random", sq, 1)[0])
    sinks = torch.tensor([0.5 * (h % 3) - 0.3 for h in range(HKV * G)])
    i = list(W.CASES).index(name)
    for left, (ns, precision) in zip((63, 127, 1100, -1), ((1, "accurate"), (2, "fast"), (3, "accurate"), (2, "accurate"))):
        kw = dict(num_splits=ns, precision=precision, return_lse=True, return_partials=True)
        got = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cud, mx, chain, (left, 0), **kw)
        want = qa.fp8_attn_paged_varlen_window_func(q, c, cud, mx, (left, 0), **kw)
        assert len(got) == len(want) == 5 and all(_same_bits(x, y) for x, y in zip(got, want)), (name, left)
        got = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cud, mx, chain, (left, 0), sinks=sinks, **kw)
        want = qa.fp8_attn_paged_varlen_sink_func(q, c, cud, mx, sinks, (left, 0), **kw)
        assert all(_same_bits(x, y) for x, y in zip(got, want)), (name, left)
    kw = dict(num_splits=(2, 3)[i % 2], return_lse=True, return_partials=True)
    got = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cud, mx, rnd, (-1, 0), **kw)
    want = qa.fp8_attn_paged_varlen_tree_func(q, c, cud, mx, rnd, **kw)
    assert all(_same_bits(x, y) for x, y in zip(got, want)), name
    out, lse, po, plse, ppath = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cud, mx, rnd, (127, 0), sinks=sinks, **kw)
    free = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cud, mx, rnd, (127, 0), **kw)
    assert _same_bits(po, free[2]) and _same_bits(plse, free[3]) and _same_bits(ppath, free[4])
    m_out, m_lse = qa.merge_attn_states_with_sinks(list(po), list(plse), sinks, out_dtype=q.dtype)
    assert _same_bits(m_out, out) and _same_bits(m_lse, lse)


@pytest.mark.parametrize("kind", ("star", "binary", "random", "junk"))
@pytest.mark.parametrize("name,D,dtype", [("A", 128, BF16), ("B", 128, FP16), ("C", 64, BF16), ("D", 256, BF16), ("E", 64, BF16)])
def test_the_eager_definition_is_the_fp64_reference_under_windows_and_sinks(name, D, dtype, kind):
    """The eager definition computes in fp32 on the de-quantised operands and rounds the output to the 16-bit dtype: the bound of
    tests/test_cpu_tree.py, |got - ref| <= REL |ref| + 1e-4 with REL = 2^-8 (bf16), 2^-10 (fp16); the LSE to 1e-4."""
    i = W.KINDS.index(kind) + list(W.CASES).index(name)
    ns, left = (1, 2, 3)[i % 3], W.WINDOWS[i % len(W.WINDOWS)][0]
    c, t, G, sq, lens, q = _with_drafts(name, PS_OF[name], D, dtype, 10 + i)
    cu = V.cu_of(sq)
    words = T.words_of(kind, sq, i)[0]
    sinks = (torch.randn(HKV * G, generator=torch.Generator().manual_seed(i)) * 1.5) if i % 2 else None
    out, lse = qa.fp8_attn_paged_varlen_tree_window_func(q, c, _i32(cu), max(sq), _words(words), (left, 0), sinks=sinks, num_splits=ns, return_lse=True)
    qd, kd, vd = _dequantised(c, t, q, sq, _native.fp8_dtype_of(c.fp8_format))
    ref, ref_lse = W.reference(qd, kd, vd, lens, sq, G, words, 1.0 / math.sqrt(D), left, None if sinks is None else sinks.double().numpy())
    assert not np.isnan(ref).any()
    o, l = out.double().numpy(), lse.double().numpy()
    assert (np.abs(o - ref) <= probes.REL_COUNT[dtype] * np.abs(ref) + 1e-4).all(), float(np.abs(o - ref).max())
    dead = np.isneginf(ref_lse)
    assert (np.isneginf(l) == dead).all()
    assert np.abs(l[~dead] - ref_lse[~dead]).max(initial=0.0) <= 1e-4


def test_the_eager_path_bytes_of_case_e_are_the_restated_plans():
    """precision="fast": a work item's path byte is ONE_TERM iff it sweeps no key or >= 1024 keys (tests/tree_window_cases.tile_keys) --
    every slot, tile and split of case E under (1100, 0) with two splits, on three trees.  This holds the split plan and the selection
    rule; in case E no work item's count depends on the tile's least depth (slot 0 has delta < left, the other slots' tiles cross a
    head boundary): the depth's part is the straddle test below."""
    ns, left = 2, 1100
    c, t, G, sq, lens, q = _with_drafts("E", 128, 64, BF16, 7)
    cu = V.cu_of(sq)
    for kind in ("chain", "star", "binary"):
        words = T.words_of(kind, sq, 1)[0]
        ppath = qa.fp8_attn_paged_varlen_tree_window_func(q, c, _i32(cu), max(sq), _words(words), (left, 0), num_splits=ns, precision="fast",
                                                          return_partials=True)[3]
        for b, (n, L) in enumerate(zip(sq, lens)):
            for tile in range(-(-G * n // W.TILE)):
                for s in range(ns):
                    keys = W.tile_keys(words, cu[b], n, L, G, tile, left, ns, s)[2]
                    code = _native.PATH_ONE_TERM if keys == 0 or keys >= 1024 else _native.PATH_TWO_TERM
                    rows = range(tile * W.TILE, min((tile + 1) * W.TILE, G * n))
                    for hkv in range(HKV):
                        got = {int(ppath[s, hkv * G + r // n, cu[b] + r % n]) for r in rows}
                        assert got == {code}, (kind, b, tile, s, keys)


@pytest.mark.parametrize("kind", ("chain", "star"))
def test_the_eager_path_bytes_straddle_1024_keys_by_the_tiles_least_depth(kind):
    """tests/tree_window_cases.STRADDLE, the shape with two splits: in split 0 the head-interior tile sweeps 1022 keys on a chain (least
    depth 8) and 1029 on a star (least depth 1), the tile across the head boundaries 1030.  The eager definition's path bytes are the
    rule's -- a definition that starts the tile at depth 0 makes the chain's tile ONE_TERM, one that starts it at its least position makes
    the star's TWO_TERM -- and on a chain every output is the eager window entry's, path bytes included."""
    L, cap, ps, left, ns = W.STRADDLE[1]
    c, q, cu = W.straddle_setup(L, cap, ps, 64, BF16, "cpu")
    words = _words(W.straddle_words(kind))
    kw = dict(num_splits=ns, precision="fast", return_lse=True, return_partials=True)
    got = qa.fp8_attn_paged_varlen_tree_window_func(q, c, cu, W.STRADDLE_SQ, words, (left, 0), **kw)
    want = W.straddle_codes(kind, L, left, ns, _native.PATH_ONE_TERM, _native.PATH_TWO_TERM)
    G, n = W.STRADDLE_G, W.STRADDLE_SQ
    inner, outer = want[0, G - 1, 8:], want[0, 0, :]                     # tile 1: head 2 at positions 8 .. 59; tile 0
    assert (inner == (_native.PATH_TWO_TERM if kind == "chain" else _native.PATH_ONE_TERM)).all() and (outer == _native.PATH_ONE_TERM).all()
    assert np.array_equal(got[4].numpy(), want), kind
    for mutant in W.PLAN_MUTANTS:                                        # each flips the tile's byte on one of the two trees
        keys = W.tile_keys(W.straddle_words(kind), 0, n, L, G, 1, left, ns, 0, mutant)[2]
        flipped = W.fast_path_code(keys, _native.PATH_ONE_TERM, _native.PATH_TWO_TERM) != inner[0]
        assert flipped == ((mutant == "tile from depth 0") == (kind == "chain")), (kind, mutant)
    if kind == "chain":
        for L1, cap1, ps1, left1, ns1 in W.STRADDLE:
            c1, q1, cu1 = (c, q, cu) if L1 == L else W.straddle_setup(L1, cap1, ps1, 64, BF16, "cpu")
            kw1 = dict(num_splits=max(ns1, 2), precision="fast", return_lse=True, return_partials=True)
            a = qa.fp8_attn_paged_varlen_tree_window_func(q1, c1, cu1, n, words, (left1, 0), **kw1)
            b = qa.fp8_attn_paged_varlen_window_func(q1, c1, cu1, n, (left1, 0), **kw1)
            assert all(_same_bits(x, y) for x, y in zip(a, b)), L1


# ---- the rotary embedding at the caller's positions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("il", (False, True))
@pytest.mark.parametrize("D,dtype", [(64, BF16), (128, FP16), (256, BF16)])
def test_the_eager_positions_entries_are_apply_rope_eager_bit_for_bit(D, dtype, il):
    name, ps = "A", 64
    G, sq, lens = W.CASES[name]
    base = [max(L - n, 0) for n, L in zip(sq, lens)]
    mk = lambda: _with_drafts(name, ps, D, dtype, 5)[0]
    a, b, s1, s2 = mk(), mk(), mk(), mk()
    for c in (a, b, s1, s2):
        c.seqlens.copy_(_i32(base))
    cu, total = V.cu_of(sq), sum(sq)
    k, v = _rand((total, HKV, D), dtype, 8, mul=2.0), _rand((total, HKV, D), dtype, 9)
    k[3, 0, 1], k[7, 1, 0] = float("inf"), float("nan")
    cos, sin = RC.tables(D, rows=300)
    rng = np.random.RandomState(D)
    pos = rng.randint(0, 300, total)
    pos[2:6], pos[6], pos[7], pos[8] = pos[1], -5, 300, 1 << 40
    posd = torch.from_numpy(pos.astype(np.int64))
    clamped = np.clip(pos, 0, 299).tolist()
    assert qa.paged_kv_cache_append_varlen_rope_pos_fp8(a, k, v, _i32(cu), posd, cos, sin, interleaved=il) is a
    qa.paged_kv_cache_append_varlen_fp8(b, RC.rotate_at(k, clamped, cos, sin, il), v, _i32(cu))
    assert torch.equal(a.k.view(torch.uint8), b.k.view(torch.uint8)) and torch.equal(a.v.view(torch.uint8), b.v.view(torch.uint8))
    assert a.seqlens.tolist() == b.seqlens.tolist() == [x + n for x, n in zip(base, sq)]
    x = _rand((total, 6, D), dtype, 10, mul=2.0)
    at = torch.tensor(clamped)
    want = apply_rope_eager(x.transpose(0, 1)[None], cos[at], sin[at], interleaved=il)[0].transpose(0, 1)
    assert _same_bits(qa.apply_rope_positions(x, posd, cos, sin, interleaved=il), want)
    # sequential positions: the entries at the cache's positions
    seq = torch.tensor([base[bb] + p for bb, n in enumerate(sq) for p in range(n)], dtype=torch.int64)
    cos2, sin2 = RC.tables(D, rows=CAP)
    qa.paged_kv_cache_append_varlen_rope_pos_fp8(s1, k, v, _i32(cu), seq, cos2, sin2, interleaved=il)
    assert _same_bits(qa.apply_rope_positions(x, seq, cos2, sin2, interleaved=il), qa.apply_rope_paged_varlen(x, s2, _i32(cu), cos2, sin2, interleaved=il))
    qa.paged_kv_cache_append_varlen_rope_fp8(s2, k, v, _i32(cu), cos2, sin2, interleaved=il)
    assert torch.equal(s1.k.view(torch.uint8), s2.k.view(torch.uint8)) and torch.equal(s1.v.view(torch.uint8), s2.v.view(torch.uint8))


@pytest.mark.parametrize("kind", ("chain", "star", "binary", "random", "junk"))
def test_tree_positions_is_the_plain_walk(kind):
    for name, (G, sq, lens) in W.CASES.items():
        words = T.words_of(kind, sq, 3)[0]
        cu = V.cu_of(sq)
        base = [max(L - n, 0) for n, L in zip(sq, lens)]
        want = [base[b] + W.depth_of(words, cu[b], n, p) for b, n in enumerate(sq) for p in range(n)]
        assert qa.tree_positions(_words(words), _i32(cu), _i32(base)).tolist() == want, (name, kind)
        assert qa.tree_positions(_words(words), _i32(cu), _i32([x + n for x, n in zip(base, sq)]), appended=True).tolist() == want, (name, kind)
        if kind == "chain":       # depth = index: the sequential positions
            assert want == [base[b] + p for b, n in enumerate(sq) for p in range(n)]
    # siblings share a position; the sign bit of the int64 is a bit like any other
    got = qa.tree_positions(_words([1, 3, 5, 0xFFFFFFFFFFFFFFFF]), _i32([0, 4]), _i32([10]))
    assert got.tolist() == [10, 11, 11, 13]
    assert qa.tree_positions(_words([]), _i32([0, 0]), _i32([3])).shape == (0,)


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------------
def test_the_count_probe_has_teeth_against_every_named_mutant_of_the_rule():
    """q_r = -g_r 1, k = 0.5 1, V[j] = e_(j mod D): under each wrong mask some element of every touched row moves by >= TEETH x its bound
    (|got - ref| <= REL ref, the bound the GPU test applies).  This grades the PROBE on the masks of tests/tree_window_cases.py -- no
    product code runs here; the eager definition is tied to those masks by the fp64 test above, the kernels by the GPU file."""
    D, seen = 128, {m: 0 for m in W.MUTANTS}
    for name, (G, sq, lens) in W.CASES.items():
        cu, Hq = V.cu_of(sq), HKV * G
        for kind in ("star", "binary", "random"):
            words = T.words_of(kind, sq, 3)[0]
            for left in (63, 127, 300, 1100):
                for b, (n, L) in enumerate(zip(sq, lens)):
                    if n == 0 or n > 64 or L - n - left <= 0:
                        continue
                    M = max(L, 1)
                    seq = probes.Seq(probes.count_q(Hq, n, D), probes.count_k(HKV, M, D, L), probes.count_v(HKV, M, D, L),
                                     W.slot_mask(words, cu[b], n, L, G, M, left), L)
                    mutants = {m: W.slot_mask(words, cu[b], n, L, G, M, left, m) & (np.arange(M) < L) for m in W.MUTANTS}
                    for m, teeth in probes.count_teeth(seq, mutants, BF16).items():
                        assert teeth >= probes.TEETH, (name, kind, left, b, m, teeth)
                        seen[m] += 1
    assert all(seen.values()), seen


def test_the_count_probe_has_teeth_against_a_sink_counted_in_every_split_and_a_sink_scaled_by_scale():
    """The count probe gives every key of a row ONE score x_r, so with a sink O[r, c] = n_c / (n + exp(sink_h - x_r)).  The eager definition
    is held to that closed form within the probe's bound; a sink counted once per split (ns exp(sink)) and a sink multiplied by `scale`
    (exp(scale sink)) each move every row with a key by >= TEETH x the bound."""
    D, dtype, name, ps, left = 128, BF16, "A", 64, 127
    G, sq, lens = W.CASES[name]
    Hq, cu = HKV * G, V.cu_of(sq)
    c, t, _, _, _, _ = _with_drafts(name, ps, D, dtype, 2)
    fp8 = _native.fp8_dtype_of(c.fp8_format)
    # the probe's keys and values, placed through the table at the case's lengths; scale_k = 1/2, scale_v = 1: exact bytes
    c.scale_k.fill_(0.5)
    c.scale_v.fill_(1.0)
    kk = torch.from_numpy(probes.count_k(HKV, CAP, D)).float().div(0.5).to(fp8)
    vv = torch.from_numpy(probes.count_v(HKV, CAP, D)).float().to(fp8)
    from tests import paged_cases as P
    for b, L in enumerate(lens):
        for j in range(L):
            page, slot = P.lookup(t.table, b, j, ps)
            c.k[page, :, slot], c.v[page, :, slot] = kk[:, j], vv[:, j]
    q = torch.cat([torch.from_numpy(probes.count_q(Hq, n, D)).transpose(0, 1) for n in sq]).to(dtype)
    words = T.words_of("binary", sq, 3)[0]
    sm = 1.0 / math.sqrt(D)
    sinks = torch.tensor([1.0 + 0.25 * h for h in range(Hq)])     # of the order of x_r + ln n on the rows with the largest scores: never negligible
    ns = 3
    out = qa.fp8_attn_paged_varlen_tree_window_func(q, c, _i32(cu), max(sq), _words(words), (left, 0), sinks=sinks, num_splits=ns).double().numpy()
    worst = math.inf
    qd = _dequantised(c, t, q, sq, fp8)[0]
    for b, (n, L) in enumerate(zip(sq, lens)):
        ref, tot = probes.count_expected(W.slot_mask(words, cu[b], n, L, G, CAP, left), D)
        x = sm * 0.5 * qd[cu[b]:cu[b + 1]].sum(-1).T                                        # [Hq, n]: the row's one score, on the quantised q
        form = lambda snk: ref * (tot / (tot + np.exp(snk[:, None] - x)))[..., None]
        good = form(sinks.double().numpy())
        got = out[cu[b]:cu[b + 1]].transpose(1, 0, 2)
        bound = probes.count_bound(good, dtype)
        assert (np.abs(got - good) <= bound).all(), (b, float((np.abs(got - good) / np.maximum(bound, 1e-300)).max()))
        rows = np.broadcast_to(tot > 0, good.shape[:2])
        for mut in (form(sinks.double().numpy() + math.log(ns)), form(sinks.double().numpy() * sm)):
            worst = min(worst, probes.teeth(good, mut, bound, rows))
    assert worst >= probes.TEETH, worst

"""CPU tests of tree-shaped speculative decoding on the paged FP8 K/V cache (quantumattention_amd/tree.py,
include/qattn_paged_varlen_tree.h): the surface, the reason functions, the C entries' argument checks, the eager definitions against the
rules restated in tests/tree_cases.py, `tree_mask_from_parents` against a plain walk, and the teeth of the count probe against the
named mutants of the mask rule."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, nn, tree
from tests import paged_cases as P
from tests import paged_varlen_cases as V
from tests import probes
from tests import tree_cases as T
from tests.conftest import ROOT

B, HKV, CAP = T.B, T.HKV, T.CAP
BF16, FP16 = torch.bfloat16, torch.float16
PS_OF = {"A": 64, "B": 128, "C": 256, "D": 64}
SCALES = torch.tensor([[0.5, 1.0], [0.75, 0.6], [1.0, 0.4]]) / 8


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32)


def _words(words):
    return torch.from_numpy(T.as_int64(words))


def _rand(shape, dtype, seed, mul=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * mul).to(dtype)


def _empty_cache(name, ps, D, dtype, seed=0):
    t = T.tables(name, ps, seed, T.appended_lens(name))
    c = qa.alloc_paged_kv_cache_fp8(t.num_pages, HKV, ps, D, batch_size=B, max_pages_per_seq=t.M, scale_k=SCALES, scale_v=SCALES * 2, dtype=dtype,
                                    device="cpu")
    assert c.layout == "rowmajor"
    c.block_table.copy_(torch.from_numpy(t.table))
    return c, t


def _committed(name, ps, D, dtype, seed):
    """a row-major cache that holds a case's committed keys (max(L_b - Sq_b, 0) tokens per slot), and the step's draft K / V"""
    G, sq, lens = T.CASES[name]
    c, t = _empty_cache(name, ps, D, dtype, seed)
    base = [max(L - n, 0) for n, L in zip(sq, lens)]
    qa.paged_kv_cache_append_varlen_fp8(c, _rand((sum(base), HKV, D), dtype, seed + 1), _rand((sum(base), HKV, D), dtype, seed + 2),
                                        _i32(V.cu_of(base)))
    return c, t, sq, base, _rand((sum(sq), HKV, D), dtype, seed + 3), _rand((sum(sq), HKV, D), dtype, seed + 4)


def _with_drafts(name, ps, D, dtype, seed):
    """... with the drafts appended and the lengths of the case (a slot with L_b < Sq_b gets its length by hand), and queries"""
    G, sq, lens = T.CASES[name]
    c, t, sq, base, kd, vd = _committed(name, ps, D, dtype, seed)
    qa.paged_kv_cache_append_varlen_fp8(c, kd, vd, _i32(V.cu_of(sq)))
    c.seqlens.copy_(_i32(lens))
    return c, t, G, sq, lens, _rand((sum(sq), HKV * G, D), dtype, seed + 5, mul=1.5)


def test_the_cases_hold_what_they_are_meant_to():
    T.check_cases()
    for name in T.CASES:
        for ps in P.PAGE_SIZES:
            t = T.tables(name, ps)
            assert not t.shared and 0 <= t.table.min() and t.table.max() < t.num_pages


# ---- the surface --------------------------------------------------------------------------------------------------------------------------
def test_the_surface_signatures_symbols_schemas_and_fake_registrations():
    for name in ("fp8_attn_paged_varlen_tree_func", "paged_kv_cache_compact_fp8", "tree_mask_from_parents"):
        assert getattr(qa, name) is getattr(tree, name) and name not in qa.__all__
    sig = inspect.signature(qa.fp8_attn_paged_varlen_tree_func)
    assert list(sig.parameters) == ["q", "cache", "cu_seqlens_q", "max_seqlen_q", "tree_mask", "scale", "seqused_k", "max_seqlen_k", "num_splits",
                                    "precision", "return_lse", "return_partials"]
    kwonly = {k: p.default for k, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kwonly == dict(scale=None, seqused_k=None, max_seqlen_k=None, num_splits=0, precision="accurate", return_lse=False, return_partials=False)
    assert list(inspect.signature(qa.paged_kv_cache_compact_fp8).parameters) == ["cache", "cu_seqlens", "accept_index", "accept_lens"]
    assert list(inspect.signature(qa.tree_mask_from_parents).parameters) == ["parents", "cu_seqlens_q"]
    header = open(os.path.join(ROOT, "include", "qattn_paged_varlen_tree.h")).read()
    for name in ("qattn_fp8_attention_paged_varlen_tree_forward", "qattn_paged_kv_cache_compact_fp8"):
        assert name + "(" in header and name in _native.EXPORTS and hasattr(_native.lib(), name)
    assert "const unsigned long long* tree_mask" in header and _native.lib().qattn_abi_version() == 8
    for phrase in ("sliding windows under a tree mask", "sinks folded into the tree unit", "trees above 64 tokens per slot",
                   "a positions tensor for the fused RoPE append", "the contiguous", "masks for the dense, 16-bit and block-sparse entries"):
        assert phrase in " ".join(header.split()).replace(" * ", " "), phrase
    att = torch.ops.quantumattention_amd.fp8_paged_varlen_splitkv_tree_attention_forward.default
    schema = str(att._schema)
    assert "!" not in schema and "Tensor tree_mask" in schema and "is_causal" not in schema and "float? scale=None" in schema, schema
    cmp_ = torch.ops.quantumattention_amd.fp8_paged_kv_cache_compact_.default
    schema = str(cmp_._schema)
    assert "Tensor(a0!) k_pool" in schema and "Tensor(a1!) v_pool" in schema and "Tensor(a3!) seqlens" in schema and schema.endswith("-> ()"), schema
    assert schema.count("!") == 3
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        q = torch.empty(39, 8, 128, dtype=FP16)
        u8, f32 = torch.empty(16, dtype=torch.uint8), torch.empty(3, 2)
        i32 = lambda n: torch.empty(n, dtype=torch.int32)
        w = torch.empty(39, dtype=torch.int64)
        res = att(q, u8, u8, f32, f32, torch.empty(3, 20, dtype=torch.int32), i32(3), i32(4), w, 17, 1280, 62, 64, 3, "e4m3", "compiled", "fast",
                  True, True)
        assert [tuple(x.shape) for x in res] == [(39, 8, 128), (8, 39), (3, 39, 8, 128), (3, 8, 39), (3, 8, 39)]
        assert [x.dtype for x in res] == [FP16, torch.float32, torch.float32, torch.float32, torch.uint8]
        res = att(q, u8, u8, f32, f32, torch.empty(3, 20, dtype=torch.int32), i32(3), i32(4), w, 17, 1280, 62, 64, 1)
        assert [tuple(x.shape) for x in res] == [(39, 8, 128), (0,), (0,), (0,), (0,)]
        assert cmp_(u8, u8, torch.empty(3, 20, dtype=torch.int32), i32(3), i32(4), i32(39), i32(3), 2, 128, 62, 64) is None


def test_append_tree_attend_and_compact_trace_into_one_graph(monkeypatch):
    """torch.compile(fullgraph=True) traces the step into ONE graph -- its three ops and the torch ops of tree_mask_from_parents, nothing
    read on the host.  Traced on CPU tensors (fake implementations only), the device check patched away; the backend keeps the graph
    and stops the call before anything would run."""
    import torch._dynamo
    monkeypatch.setattr(nn, "_pre_check_can_use_hip_attention", lambda device: (True, ""))
    D, ps, dtype = 128, 64, BF16
    t = T.tables("A", ps)
    c, _ = _empty_cache("A", ps, D, dtype)
    pool = torch.zeros((t.num_pages * HKV * ps * D,), dtype=torch.uint8)
    c = qa.PagedKVCacheFP8(pool, pool.clone(), c.scale_k, c.scale_v, c.block_table, c.seqlens, c.shape, c.fp8_format, c.dtype, c.numerics, "frag")
    G, sq, _ = T.CASES["A"]
    total = sum(sq)

    def f(q, kd, vd, cu, par, ai, al):
        qa.paged_kv_cache_append_varlen_fp8(c, kd, vd, cu)
        out = qa.fp8_attn_paged_varlen_tree_func(q * 2, c, cu, 40, qa.tree_mask_from_parents(par, cu), num_splits=2, return_lse=True)
        qa.paged_kv_cache_compact_fp8(c, cu, ai, al)
        return out

    args = (_rand((total, HKV * G, D), dtype, 1), _rand((total, HKV, D), dtype, 2), _rand((total, HKV, D), dtype, 3), _i32(V.cu_of(sq)),
            _i32(T.words_of("binary", sq)[1]), _i32([0] * total), _i32([1] * B))
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
    gm = graphs[0]
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    order = [next(i for i, x in enumerate(targets) if name in x) for name in
             ("fp8_paged_varlen_kv_cache_append_", "fp8_paged_varlen_splitkv_tree_attention_forward", "fp8_paged_kv_cache_compact_")]
    assert order == sorted(order)
    assert not any(n.op == "call_method" and n.target in ("item", "tolist") for n in gm.graph.nodes)
    assert not any("_local_scalar_dense" in x for x in targets)


# ---- the reason functions -------------------------------------------------------------------------------------------------------------------
def test_the_reason_functions_name_the_first_broken_rule():
    c, t, G, sq, lens, q = _with_drafts("A", 64, 128, BF16, 1)
    cu, w = _i32(V.cu_of(sq)), _words(T.words_of("star", sq)[0])
    ok = lambda **kw: tree.paged_varlen_tree_input_reason(**{**dict(q=q, cache=c, cu_seqlens_q=cu, max_seqlen_q=40, tree_mask=w), **kw})
    assert ok() is None
    assert "tree_mask" in ok(tree_mask=w.to(torch.int32)) and "tree_mask" in ok(tree_mask=w[:-1]) and "tree_mask" in ok(tree_mask=None)
    assert "contiguous" in ok(tree_mask=torch.stack([w, w], 1)[:, 0])
    assert "cu_seqlens_q" in ok(cu_seqlens_q=cu.long()) and "3-D" in ok(q=q[0]) and "num_splits" in ok(num_splits=65)
    with pytest.raises(ValueError, match="tree_mask"):
        qa.fp8_attn_paged_varlen_tree_func(q, c, cu, 40, w.float())
    with pytest.raises(ValueError, match="precision"):
        qa.fp8_attn_paged_varlen_tree_func(q, c, cu, 40, w, precision="auto")
    ai, al = _i32([0] * sum(sq)), _i32([1] * B)
    okc = lambda **kw: tree.paged_compact_input_reason(**{**dict(cache=c, cu_seqlens=cu, accept_index=ai, accept_lens=al), **kw})
    assert okc() is None
    assert "cu_seqlens" in okc(cu_seqlens=cu[:-1]) and "accept_index" in okc(accept_index=ai.long()) and "accept_index" in okc(accept_index=ai[None])
    assert "accept_lens" in okc(accept_lens=al[:-1]) and "accept_lens" in okc(accept_lens=None) and "PagedKVCacheFP8" in okc(cache=None)
    with pytest.raises(ValueError, match="accept_lens"):
        qa.paged_kv_cache_compact_fp8(c, cu, ai, al.long())
    with pytest.raises(ValueError):
        qa.tree_mask_from_parents(ai.long(), cu)


# ---- the C entries' argument checks (null device pointers: every check precedes any device call) ---------------------------------------------
def test_the_c_entries_check_their_arguments_before_any_device_call():
    L = _native.lib()
    INVALID, DIM = 1, None
    p = 0x1000   # a non-null, 16-byte-aligned address that is never dereferenced: a failing check returns first
    s2 = (ctypes.c_longlong * 2)(8 * 128, 128)

    def att(tree_mask=p, block_table=p, page_size=64, Hq=8, Hkv=2, D=128, table_stride=20, cu=p, num_splits=1, q=p):
        return L.qattn_fp8_attention_paged_varlen_tree_forward(q, s2, _native.FMT_BF16, p, p, block_table, table_stride, 62, page_size, 20, p, p, p,
                                                               None, cu, p, 3, Hq, Hkv, 10, 4, 1280, D, _native.fmt_of(torch.float8_e4m3fn), 0,
                                                               tree_mask, 0.0, 2, num_splits, None, None, None, None, None, None, None, 0, None)
    bad = L.qattn_fp8_attention_paged_varlen_forward(p, s2, _native.FMT_BF16, p, p, None, 20, 62, 64, 20, p, p, p, None, p, p, 3, 8, 2, 10, 4, 1280, 128,
                                                     _native.fmt_of(torch.float8_e4m3fn), 0, 1, 0.0, 2, 1, None, None, None, None, None, None, None,
                                                     0, None)
    assert bad != 0
    INVALID = bad                                                      # QATTN_ERR_INVALID_ARG, as the sibling returns it for a NULL table
    assert att(tree_mask=None) == INVALID and att(tree_mask=p + 4) == INVALID and att(tree_mask=p + 1) == INVALID
    assert att(block_table=None) == INVALID and att(page_size=96) == INVALID and att(table_stride=19) == INVALID and att(cu=None) == INVALID
    assert att(num_splits=65) == INVALID and att(q=None) == INVALID
    assert att(D=96) not in (0, INVALID) and att(Hq=7) == att(D=96)     # QATTN_ERR_UNSUPPORTED_DIM
    # (a call that passes every check without a workspace: QATTN_ERR_WORKSPACE, still before any device call)
    assert att() not in (0, INVALID, att(D=96))

    def cmp_(k=p, v=p, table=p, stride=20, seqlens=p, cu=p, ai=p, al=p, Bn=3, Hkv=2, total=10, pages=62, ps=64, mp=20, D=128):
        return L.qattn_paged_kv_cache_compact_fp8(k, v, table, stride, seqlens, cu, ai, al, Bn, Hkv, total, pages, ps, mp, D, None)
    for kw in (dict(k=None), dict(v=None), dict(k=p + 8), dict(table=None), dict(table=p + 2), dict(seqlens=None), dict(cu=None), dict(ai=None),
               dict(al=None), dict(al=p + 2), dict(ai=p + 1), dict(stride=19), dict(Bn=0), dict(Hkv=0), dict(total=-1), dict(pages=0), dict(ps=0),
               dict(ps=96), dict(mp=0), dict(mp=1 << 30)):
        assert cmp_(**kw) == INVALID, kw
    assert cmp_(D=96) == att(D=96)
    assert cmp_(total=0) == 0                                           # nothing launched


# ---- the eager definition of the attention ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.CASES))
def test_eager_chain_and_slots_above_64_queries_are_the_eager_causal_entry_bit_for_bit(name):
    ps = PS_OF[name]
    c, t, G, sq, lens, q = _with_drafts(name, ps, 128, BF16, 3)
    cu = V.cu_of(sq)
    cud, mx = _i32(cu), max(sq)
    chain, rnd = _words(T.words_of("chain", sq)[0]), _words(T.words_of("random", sq, 1)[0])
    for ns, precision in ((1, "accurate"), (2, "fast"), (3, "accurate")):
        kw = dict(num_splits=ns, precision=precision, return_lse=True, return_partials=True)
        want = qa.fp8_attn_paged_varlen_func(q, c, cud, mx, causal=True, **kw)
        got = qa.fp8_attn_paged_varlen_tree_func(q, c, cud, mx, chain, **kw)
        assert len(got) == len(want) == 5 and all(_same_bits(x, y) for x, y in zip(got, want)), (name, ns)
        other = qa.fp8_attn_paged_varlen_tree_func(q, c, cud, mx, rnd, **kw)
        for b, n in enumerate(sq):
            if n > 64:
                assert _same_bits(other[0][cu[b]:cu[b + 1]], want[0][cu[b]:cu[b + 1]]) and _same_bits(other[1][:, cu[b]:cu[b + 1]], want[1][:, cu[b]:cu[b + 1]])
        assert not _same_bits(other[0], want[0])


@pytest.mark.parametrize("name", list(T.CASES))
def test_eager_junk_bits_above_p_change_no_bit(name):
    c, t, G, sq, lens, q = _with_drafts(name, PS_OF[name], 128, FP16, 4)
    cud, mx = _i32(V.cu_of(sq)), max(sq)
    kw = dict(num_splits=2, return_lse=True, return_partials=True)
    a = qa.fp8_attn_paged_varlen_tree_func(q, c, cud, mx, _words(T.words_of("junk", sq, 2)[0]), **kw)
    b_ = qa.fp8_attn_paged_varlen_func(q, c, cud, mx, causal=True, **kw)
    assert T.words_of("junk", sq, 2)[0] != T.words_of("chain", sq)[0]
    assert all(_same_bits(x, y) for x, y in zip(a, b_))


def _dequantised(c, t, q, sq, fp8):
    """(q, k, v) float64: q through the eager head-wise quantiser per slot, the pools' rows looked up key by key"""
    cu = V.cu_of(sq)
    qd = np.zeros(tuple(q.shape))
    for b, n in enumerate(sq):
        if n:
            q8, s = nn._dynamically_quantize_fp8(q[cu[b]:cu[b + 1]].transpose(0, 1)[None], reduction_dim=[2, 3], fp8_dtype=fp8)
            qd[cu[b]:cu[b + 1]] = (q8.float() * s[..., None, None])[0].transpose(0, 1).double().numpy()
    deq = lambda pool, s: P.gather_rows(pool.float().double().numpy(), t.table, t.page_size) * s.double().numpy()[:, :, None, None]
    return qd, deq(c.k, c.scale_k), deq(c.v, c.scale_v)


@pytest.mark.parametrize("kind", ("star", "binary", "random", "zero"))
@pytest.mark.parametrize("name,D,dtype", [("A", 128, BF16), ("B", 128, FP16), ("C", 64, BF16), ("D", 256, BF16)])
def test_the_eager_definition_is_the_fp64_reference_on_general_trees(name, D, dtype, kind):
    """The eager definition computes in fp32 on the de-quantised operands and rounds the output to the 16-bit dtype: half an ulp of the
    output format (2^-9 relative for bf16, 2^-11 for fp16) plus fp32 rounding of sums over at most 1104 keys.  Bound: |got - ref| <=
    REL |ref| + 1e-4 with REL = 2^-8 (bf16), 2^-10 (fp16); the LSE, an fp32 number of order 1 .. 10, to 1e-4."""
    i = T.KINDS.index(kind) + list(T.CASES).index(name)
    ns = (1, 2, 3)[i % 3]
    c, t, G, sq, lens, q = _with_drafts(name, PS_OF[name], D, dtype, 10 + i)
    cu = V.cu_of(sq)
    words = T.words_of(kind, sq, i)[0]
    out, lse = qa.fp8_attn_paged_varlen_tree_func(q, c, _i32(cu), max(sq), _words(words), num_splits=ns, return_lse=True)
    qd, kd, vd = _dequantised(c, t, q, sq, _native.fp8_dtype_of(c.fp8_format))
    ref, ref_lse = T.reference(qd, kd, vd, lens, sq, G, words, 1.0 / math.sqrt(D))
    assert not np.isnan(ref).any()
    o, l = out.double().numpy(), lse.double().numpy()
    assert (np.abs(o - ref) <= probes.REL_COUNT[dtype] * np.abs(ref) + 1e-4).all(), float(np.abs(o - ref).max())
    dead = np.isneginf(ref_lse)
    assert (np.isneginf(l) == dead).all() and (o.transpose(1, 0, 2)[dead] == 0).all()
    assert np.abs(l[~dead] - ref_lse[~dead]).max(initial=0.0) <= 1e-4
    if kind == "zero":       # no draft key at all: a slot without committed keys has no key
        assert all(dead[:, cu[b]:cu[b + 1]].all() for b, (n, L) in enumerate(zip(sq, lens)) if L <= n <= 64)


# ---- tree_mask_from_parents -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("chain", "star", "binary", "random"))
def test_tree_mask_from_parents_is_the_plain_walk(kind):
    for name, (G, sq, lens) in T.CASES.items():
        sq = tuple(min(n, 64) for n in sq)                   # (the words of longer slots are not read: bits wrap at 64 there)
        words, parents = T.words_of(kind, sq, 3)
        got = qa.tree_mask_from_parents(_i32(parents), _i32(V.cu_of(sq)))
        assert got.dtype == torch.int64 and got.shape == (sum(sq),) and torch.equal(got, _words(words)), (kind, name)
    # a chain of 64: depth 63 is reached by 6 doubling steps; the top bit is the sign bit of the int64
    got = qa.tree_mask_from_parents(_i32(range(-1, 63)), _i32([0, 64]))
    assert got.tolist()[-1] == -1 and got.tolist()[0] == 1 and got.tolist()[62] == (1 << 63) - 1
    assert qa.tree_mask_from_parents(_i32([]), _i32([0, 0])).shape == (0,)


# ---- the eager definition of the compaction ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("path", "wild"))
@pytest.mark.parametrize("name", list(T.CASES))
def test_eager_compaction_follows_the_rule_and_leaves_every_other_byte(name, kind):
    """non-monotone lists follow the read-before-write rule; slots that are not compactable are untouched"""
    ps, D, dtype = PS_OF[name], 128, BF16
    c, t, sq, base, kd, vd = _committed(name, ps, D, dtype, 30)
    cu = V.cu_of(sq)
    qa.paged_kv_cache_append_varlen_fp8(c, kd, vd, _i32(cu))
    c.k.view(torch.uint8)[P.POISON], c.v.view(torch.uint8)[P.POISON] = 0x7F, 0x7F
    lens0 = c.seqlens.tolist()
    idx, cnt = T.accept_lists(sq, 2, kind)
    k0, v0 = c.k.view(torch.uint8).numpy().copy(), c.v.view(torch.uint8).numpy().copy()
    want_k, want_v = k0.copy(), v0.copy()
    want_lens, dests = T.compact_rows(want_k, t.table, ps, lens0, cu, idx, cnt)
    T.compact_rows(want_v, t.table, ps, lens0, cu, idx, cnt)
    assert qa.paged_kv_cache_compact_fp8(c, _i32(cu), _i32(idx), _i32(cnt)) is c
    k1, v1 = c.k.view(torch.uint8).numpy(), c.v.view(torch.uint8).numpy()
    assert c.seqlens.tolist() == want_lens and np.array_equal(k1, want_k) and np.array_equal(v1, want_v)
    touched = np.zeros((t.num_pages, ps), bool)
    for b, keys in enumerate(dests):
        for j in keys:
            touched[P.lookup(t.table, b, j, ps)] = True
    for old, new in ((k0, k1), (v0, v1)):
        assert (old == new).all(axis=(1, 3))[~touched].all() and (new[P.POISON] == 0x7F).all()
    for b, n in enumerate(sq):
        if not 1 <= n <= 64:
            assert want_lens[b] == lens0[b] and dests[b] == []
    if kind == "wild" and name == "A":
        assert (k0 != k1).any()


@pytest.mark.parametrize("name", ("A", "B"))
def test_after_eager_compaction_the_live_keys_are_those_of_a_cache_that_received_the_accepted_tokens_only(name):
    ps, D, dtype = PS_OF[name], 128, BF16
    ca, t, sq, base, kd, vd = _committed(name, ps, D, dtype, 40)
    cb = _committed(name, ps, D, dtype, 40)[0]
    cu = V.cu_of(sq)
    idx, cnt = T.accept_lists(sq, 4, "path")
    cnt = [n if m else 0 for n, m in zip(cnt, sq)]
    qa.paged_kv_cache_append_varlen_fp8(ca, kd, vd, _i32(cu))
    qa.paged_kv_cache_compact_fp8(ca, _i32(cu), _i32(idx), _i32(cnt))
    rows = [cu[b] + idx[cu[b] + i] for b in range(B) for i in range(cnt[b])]
    qa.paged_kv_cache_append_varlen_fp8(cb, kd[rows].contiguous(), vd[rows].contiguous(), _i32(V.cu_of(cnt)))
    assert ca.seqlens.tolist() == cb.seqlens.tolist() == [x + n for x, n in zip(base, cnt)]
    for pool_a, pool_b in ((ca.k, cb.k), (ca.v, cb.v)):
        a, b_ = pool_a.view(torch.uint8).numpy(), pool_b.view(torch.uint8).numpy()
        for s, L in enumerate(ca.seqlens.tolist()):
            for j in range(L):
                at = P.lookup(t.table, s, j, ps)
                assert np.array_equal(a[at[0], :, at[1]], b_[at[0], :, at[1]]), (s, j)


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------------
def test_the_count_probe_has_teeth_against_every_named_mutant_of_the_mask_rule():
    """q_r = -g_r 1, k = 0.5 1, V[j] = e_(j mod D): under each wrong mask some element of every touched row moves by >= TEETH x its bound
    (|got - ref| <= REL ref, the bound the GPU test applies)."""
    D, seen = 128, {m: 0 for m in T.MUTANTS}
    for name, (G, sq, lens) in T.CASES.items():
        cu, Hq = V.cu_of(sq), HKV * G
        for kind in ("star", "binary", "random", "junk"):
            words = T.words_of(kind, sq, 3)[0]
            for b, (n, L) in enumerate(zip(sq, lens)):
                if n == 0 or n > 64:
                    continue
                M = max(L, 1)
                seq = probes.Seq(probes.count_q(Hq, n, D), probes.count_k(HKV, M, D, L), probes.count_v(HKV, M, D, L),
                                 T.slot_mask(words, cu[b], n, L, G, M), L)
                mutants = {m: T.slot_mask(words, cu[b], n, L, G, M, m) & (np.arange(M) < L) for m in T.MUTANTS}
                for m, teeth in probes.count_teeth(seq, mutants, BF16).items():
                    assert teeth >= probes.TEETH, (name, kind, b, m, teeth)
                    seen[m] += 1
    assert all(seen.values()), seen

"""Packed variable-length queries over the paged FP8 K/V cache on the MI355X (quantumattention_amd/paged_varlen.py,
include/qattn_paged_varlen.h).

Everything is graded against the DENSE paged entry on each sequence alone: for every sequence with queries, the rows of every output of
the packed call are the bits of fp8_attn_paged_func / qattn_fp8_attention_paged_splitkv_forward on q[cu[b]:cu[b+1]] as [1, Hq, Sq_b, D]
with a one-slot cache on the same pools (row b of the table, of the scales, of the lengths) -- the q scales, the tile composition and
the split plan of a sequence do not depend on its neighbours in the batch.  Tables and pools are the shared ones of
tests/paged_cases.py (the NaN page behind every sequence's used pages); the (G, query counts) pairs and their rotation over the tables
are tests/paged_varlen_cases.py's.  No test feeds an out-of-range table entry or an inconsistent cu_seqlens_q."""
import math

import numpy as np
import pytest
import torch

import oracle
import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import gpu_utils
from tests import paged_cases as P
from tests import paged_varlen_cases as V
from tests.gpu_utils import FMT, bits8
from tests.test_gpu_paged import CFG_IDS, CFGS, SCALE_K, _cache, _pack, _rand, _rows, _same_bits, _su

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV, CAP = P.B, P.HKV, P.CAP
NAMES = ("out", "lse", "partial_o", "partial_lse", "partial_path", "q8", "scale_q", "row_path")
KINDS = ("o", "l", "po", "pl", "pl", None, None, "l")


def _varlen(q, c, cu, mx, **kw):
    return _native.fp8_attention_paged_varlen(q, c.k, c.v, c.scale_k, c.scale_v, c.block_table, c.seqlens, cu, max_seqlen_q=mx, Skv=CAP,
                                              num_pages=c.num_pages, page_size=c.page_size, fp8_dtype=P.FP8[c.fp8_format], **kw)


def _dense_alone(q, c, cu, b, **kw):
    """the dense paged entry on sequence b alone: its queries, row b of the table, of the scales and of the lengths, the same pools"""
    return _native.fp8_attention_paged_splitkv(V.alone(q, cu, b), c.k, c.v, c.scale_k[b:b + 1].contiguous(), c.scale_v[b:b + 1].contiguous(),
                                               c.block_table[b:b + 1].contiguous(), c.seqlens[b:b + 1].contiguous(), Skv=CAP,
                                               num_pages=c.num_pages, page_size=c.page_size, fp8_dtype=P.FP8[c.fp8_format], **kw)


def _rows_equal(got, want, cu, b, Hq, D, what):
    """sequence b's rows of the eight outputs of a packed call against the dense call on it alone"""
    for name, kind, x, y in zip(NAMES, KINDS, got, want):
        if name == "q8":       # the slab [Hq, Sq_b, D] at byte Hq D start_b
            x = x.view(torch.uint8)[Hq * D * cu[b]:Hq * D * cu[b + 1]].view(1, Hq, cu[b + 1] - cu[b], D).view(y.dtype)
        elif name == "scale_q":
            x = x[b:b + 1]
        elif x.numel() == 0:
            assert y.numel() == 0, (what, name)
            continue
        else:
            x = V.rows_of(x, kind, cu, b)
        assert _same_bits(x, y), (what, b, name)


# ---- 1. the main contract ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
@pytest.mark.parametrize("D,dtype,fmt", CFGS, ids=CFG_IDS)
def test_every_sequences_rows_are_the_bits_of_the_dense_paged_entry_on_that_sequence_alone(D, dtype, fmt, page_size):
    """out, lse, row_path, the fp32 partials, q8 and scale_q, for num_splits 1 / 2 / 3 / 9 (the chained merge), causal or not, accurate and
    fast, and the byte-exponential case (fast, one split, no LSE); no NaN anywhere: the poison page shows a table entry or a V tail read too
    far"""
    for i, t in enumerate(P.shared_tables(page_size)):
        G, sq = V.qcase(page_size, i)
        Hq, cu, total = HKV * G, V.cu_of(sq), sum(sq)
        c = _cache(t, D, dtype, fmt, _pack(*_rows(t, D, fmt, 11 * D + i), fmt))
        q = _rand((total, Hq, D), dtype, 7 * D + i, mul=1.5)
        cud = _su(cu)
        for ns in (1, 2, 3, 9):
            for causal in (False, True):
                for precision in ("accurate", "fast"):
                    kw = dict(is_causal=causal, precision=precision, num_splits=ns, return_lse=True, return_partials=True, return_quant=True,
                              return_path=True)
                    got = _varlen(q, c, cud, max(sq), **kw)
                    assert len(got) == 8 and got[0].shape == (total, Hq, D) and got[1].shape == got[7].shape == (Hq, total)
                    for x in got[:4]:
                        assert not torch.isnan(x.float()).any(), (t.lens, sq, ns, causal, precision)
                    bare = _varlen(q, c, cud, max(sq), is_causal=causal, precision="fast", num_splits=1) if (ns == 1 and precision == "fast") else None
                    for b in range(B):
                        if sq[b] == 0:
                            continue
                        _rows_equal(got, _dense_alone(q, c, cu, b, **kw), cu, b, Hq, D, (t.lens, G, sq, ns, causal, precision))
                        if bare is not None:     # no LSE: the byte-exponential sweep
                            want = _dense_alone(q, c, cu, b, is_causal=causal, precision="fast", num_splits=1)
                            assert _same_bits(V.rows_of(bare, "o", cu, b), want), (t.lens, sq, b, causal)
        # the public function is that call (seqused_k defaults to cache.seqlens), also under a tighter max_seqlen_k
        pub = qa.fp8_attn_paged_varlen_func(q, c, cud, max(sq), causal=True, num_splits=3, return_lse=True, return_partials=True)
        raw = _varlen(q, c, cud, max(sq), is_causal=True, num_splits=3, return_lse=True, return_partials=True)
        assert len(pub) == len(raw) == 5 and all(_same_bits(x, y) for x, y in zip(pub, raw))
        tight = qa.fp8_attn_paged_varlen_func(q, c, cud, max(sq), causal=True, num_splits=2, max_seqlen_k=1100, return_lse=True)
        for b in range(B):
            if sq[b]:
                want = qa.fp8_attn_paged_func(V.alone(q, cu, b), V.one_slot(c, b), causal=True, num_splits=2, max_seqlen_k=1100, return_lse=True)
                assert _same_bits(V.rows_of(tight[0], "o", cu, b), want[0]) and _same_bits(V.rows_of(tight[1], "l", cu, b), want[1])


# ---- 2. equal counts = the dense call ---------------------------------------------------------------------------------------------------
def test_with_equal_counts_the_call_is_the_dense_paged_call_and_chooses_the_same_split_count():
    D, dtype, fmt, ps, M = 128, torch.bfloat16, "e4m3", 128, 32       # 4096 keys of capacity: the num_splits = 0 rule has room to split
    num_pages = B * M + 1
    c = qa.alloc_paged_kv_cache_fp8(num_pages, HKV, ps, D, batch_size=B, max_pages_per_seq=M, scale_k=SCALE_K, scale_v=SCALE_K * 2, dtype=dtype,
                                    device=DEV, fp8_format=fmt)
    pools = _pack(*P.random_rows(num_pages, ps, D, fmt, 21, DEV), fmt)
    c.k.copy_(pools[0])
    c.v.copy_(pools[1])
    c.block_table.copy_(_su(np.random.RandomState(3).permutation(B * M).reshape(B, M)))
    c.seqlens.copy_(_su([4096, 2500, 130]))
    for G, Sq in ((1, 1), (4, 3), (4, 40)):
        Hq = HKV * G
        q = _rand((B * Sq, Hq, D), dtype, 30 + Sq, mul=1.5)
        qd = q.view(B, Sq, Hq, D).transpose(1, 2)
        cud = _su([Sq * b for b in range(B + 1)])
        for ns in (0, 1, 3):
            for precision in ("accurate", "fast"):
                kw = dict(causal=True, num_splits=ns, precision=precision, return_lse=True, return_partials=True)
                out, lse, po, plse, ppath = qa.fp8_attn_paged_varlen_func(q, c, cud, Sq, **kw)
                wo, wl, wpo, wpl, wpp = qa.fp8_attn_paged_func(qd, c, **kw)
                assert po.shape[0] == wpo.shape[0], "the same split count"
                assert _same_bits(out.view(B, Sq, Hq, D).transpose(1, 2), wo) and _same_bits(lse.view(Hq, B, Sq).transpose(0, 1), wl), (G, Sq, ns)
                if po.numel():
                    n = po.shape[0]
                    assert _same_bits(po.view(n, B, Sq, Hq, D).transpose(2, 3), wpo), (G, Sq, ns)
                    assert _same_bits(plse.view(n, Hq, B, Sq).transpose(1, 2), wpl) and _same_bits(ppath.view(n, Hq, B, Sq).transpose(1, 2), wpp)
        assert _native.paged_varlen_auto_splits(B, Hq, HKV, B * Sq, Sq, 4096, D, 256) == _native.splitkv_auto_splits(B, Hq, HKV, Sq, 4096, D, 256)
    ns0 = qa.fp8_attn_paged_varlen_func(_rand((B, HKV, D), dtype, 1), c, _su([0, 1, 2, 3]), 1, num_splits=0, return_partials=True)[1].shape[0]
    assert ns0 > 1, "this shape splits under the auto rule"


# ---- 3. the partials merge to the outputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [2, 9])
def test_out_and_lse_are_merge_attn_states_of_the_partials_on_the_packed_conventions(ns):
    D, dtype, fmt, ps = 128, torch.bfloat16, "e4m3", 64
    t = P.shared_tables(ps)[3]
    G, sq = V.QCASES[2]
    c = _cache(t, D, dtype, fmt, _pack(*_rows(t, D, fmt, 41), fmt))
    q = _rand((sum(sq), HKV * G, D), dtype, 42, mul=1.5)
    for precision in ("accurate", "fast"):
        out, lse, po, plse, _ = qa.fp8_attn_paged_varlen_func(q, c, _su(V.cu_of(sq)), max(sq), causal=True, num_splits=ns, precision=precision,
                                                              return_lse=True, return_partials=True)
        assert po.shape == (ns, sum(sq), HKV * G, D) and plse.shape == (ns, HKV * G, sum(sq))
        parts_o, parts_l = list(po.unbind(0)), list(plse.unbind(0))
        if ns <= _native.MERGE_MAX_PARTIALS:
            mo, ml = qa.merge_attn_states(parts_o, parts_l, out_dtype=dtype)
        else:                                                       # the chain of the entry: 8, then 7 more per merge through fp32
            mo, ml = qa.merge_attn_states(parts_o[:8], parts_l[:8], out_dtype=torch.float32)
            mo, ml = qa.merge_attn_states([mo] + parts_o[8:], [ml] + parts_l[8:], out_dtype=dtype)
        assert _same_bits(mo, out) and _same_bits(ml, lse), precision


# ---- 4. strided q -----------------------------------------------------------------------------------------------------------------------
def test_a_slice_of_a_packed_qkv_projection_gives_the_dense_calls_bits():
    D, dtype, fmt, ps = 64, torch.float16, "e5m2", 128
    t = P.shared_tables(ps)[2]
    G, sq = V.QCASES[0]
    Hq, total = HKV * G, sum(sq)
    c = _cache(t, D, dtype, fmt, _pack(*_rows(t, D, fmt, 51), fmt))
    qkv = _rand((total, 3, Hq, D), dtype, 52, mul=1.5)
    qv = qkv[:, 0]
    assert not qv.is_contiguous()
    kw = dict(causal=True, num_splits=2, precision="fast", return_lse=True, return_partials=True)
    got = qa.fp8_attn_paged_varlen_func(qv, c, _su(V.cu_of(sq)), max(sq), **kw)
    want = qa.fp8_attn_paged_varlen_func(qv.contiguous(), c, _su(V.cu_of(sq)), max(sq), **kw)
    assert all(_same_bits(x, y) for x, y in zip(got, want))
    # ... and a slice of the head axis ([total, Hq + 2 Hkv, D]: q's heads of a fused projection)
    fused = _rand((total, Hq + 2 * HKV, D), dtype, 53, mul=1.5)
    a = qa.fp8_attn_paged_varlen_func(fused[:, :Hq], c, _su(V.cu_of(sq)), max(sq), **kw)
    b = qa.fp8_attn_paged_varlen_func(fused[:, :Hq].contiguous(), c, _su(V.cu_of(sq)), max(sq), **kw)
    assert all(_same_bits(x, y) for x, y in zip(a, b))


# ---- 5. what a sequence's rows do not depend on ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
def test_keys_behind_the_lengths_unread_table_entries_and_other_sequences_queries_influence_no_bit(page_size):
    D, dtype, fmt, ps = 128, torch.bfloat16, "e4m3", page_size
    for i, t in enumerate(P.shared_tables(ps)):
        G, sq = V.qcase(ps, i)
        Hq, cu, total = HKV * G, V.cu_of(sq), sum(sq)
        rk, rv = _rows(t, D, fmt, 13 * D + i)
        zk, zv = rk.clone(), rv.clone()
        shared_page = int(t.table[t.sharers[0], 0]) if t.shared else -1
        for b, L in enumerate(t.lens):
            if L % ps and int(t.table[b, L // ps]) != shared_page:
                page = int(t.table[b, L // ps])
                for r, z in ((rk, zk), (rv, zv)):
                    r[page, :, L % ps:] = P.NAN_BYTE[fmt]
                    z[page, :, L % ps:] = 0
        hot = _cache(t, D, dtype, fmt, _pack(rk, rv, fmt))
        cold = _cache(t, D, dtype, fmt, _pack(zk, zv, fmt), table=t.zeroed)
        q = _rand((total, Hq, D), dtype, 17 * D + i, mul=1.5)
        cud = _su(cu)
        for ns in (1, 3):
            for precision in ("accurate", "fast"):
                kw = dict(causal=True, num_splits=ns, precision=precision, return_lse=True, return_partials=True)
                got, want = qa.fp8_attn_paged_varlen_func(q, hot, cud, max(sq), **kw), qa.fp8_attn_paged_varlen_func(q, cold, cud, max(sq), **kw)
                assert torch.isfinite(got[0].float()).all() and not torch.isnan(got[1]).any() and not torch.isnan(got[2]).any()
                assert all(_same_bits(x, y) for x, y in zip(got, want)), (t.lens, sq, ns, precision)
                # the q rows of the other sequences: rewrite them (another magnitude: another scale_q, had the abs-max crossed sequences)
                for b in range(B):
                    if sq[b] == 0:
                        continue
                    q2 = (q.float() * 3 + 1).to(dtype)
                    q2[cu[b]:cu[b + 1]] = q[cu[b]:cu[b + 1]]
                    other = qa.fp8_attn_paged_varlen_func(q2, hot, cud, max(sq), **kw)
                    for kind, x, y in zip(("o", "l", "po", "pl", "pl"), got, other):
                        if x.numel():
                            assert _same_bits(V.rows_of(x, kind, cu, b), V.rows_of(y, kind, cu, b)), (t.lens, sq, b, ns, precision, kind)


# ---- 6. graph ---------------------------------------------------------------------------------------------------------------------------
def test_one_captured_step_follows_rewritten_cu_seqlens_q_seqlens_and_block_table():
    """append (padded, new_lens) + attend, captured once; each replay equals the eager call on the same contents"""
    D, dtype, fmt, ps, total, T = 128, torch.bfloat16, "e4m3", 64, 12, 8
    lens0 = [ps - 3, 5, 1100]
    t = P.Tables(ps, lens0, seed=4, need=[2, 1, 18])
    spare = [p for p in range(t.num_pages) if p != P.POISON and p not in set(t.table.flatten().tolist())]
    pools = _pack(*_rows(t, D, fmt, 31), fmt)
    mk = lambda: _cache(t, D, dtype, fmt, pools, lens=lens0)
    graphed, eager, warm = mk(), mk(), mk()
    attend = lambda q, c, cu: qa.fp8_attn_paged_varlen_func(q, c, cu, T, causal=True, num_splits=3, return_lse=True)
    inputs = lambda s: (_rand((total, 8, D), dtype, 700 + s), _rand((B, HKV, T, D), dtype, 800 + s, mul=1.5), _rand((B, HKV, T, D), dtype, 900 + s, mul=1.5))
    counts = [(8, 1, 3), (1, 8, 3), (4, 0, 8), (0, 6, 6)]           # queries = new tokens per slot and step: always `total` of them
    qs, ks, vs = (x.clone() for x in inputs(0))
    cus, nls = _su(V.cu_of(counts[0])), _su(counts[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        qa.paged_kv_cache_append_fp8(warm, ks, vs, new_lens=nls)
        attend(qs, warm, cus)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        qa.paged_kv_cache_append_fp8(graphed, ks, vs, new_lens=nls)
        out_s, lse_s = attend(qs, graphed, cus)
    assert graphed.seqlens.tolist() == lens0                       # capture ran nothing

    def edit(step, c):
        if step == 1:                                              # the allocator hands sequence 1 a new page, in place
            c.block_table[1, 1] = spare[0]
        if step == 2:                                              # a rollback: two of sequence 2's tokens are rejected
            c.seqlens[2] -= 2
        if step == 3:                                              # sequence 0 moves its first page (the old one goes back to the pool)
            old = int(c.block_table[0, 0])
            c.k.view(c.num_pages, -1)[spare[1]] = c.k.view(c.num_pages, -1)[old]
            c.v.view(c.num_pages, -1)[spare[1]] = c.v.view(c.num_pages, -1)[old]
            c.block_table[0, 0] = spare[1]

    lens = list(lens0)
    for s in range(4):
        for c in (graphed, eager):
            edit(s, c)
        if s == 2:
            lens[2] -= 2
        q, k, v = inputs(s)
        for dst, src in zip((qs, ks, vs, cus, nls), (q, k, v, _su(V.cu_of(counts[s])), _su(counts[s]))):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        qa.paged_kv_cache_append_fp8(eager, k, v, new_lens=_su(counts[s]))
        out, lse = attend(q, eager, _su(V.cu_of(counts[s])))
        lens = [a + n for a, n in zip(lens, counts[s])]
        assert graphed.seqlens.tolist() == eager.seqlens.tolist() == lens, s
        assert _same_bits(out_s, out) and _same_bits(lse_s, lse), s
        assert torch.equal(graphed.k, eager.k) and torch.equal(graphed.v, eager.v), s
        assert torch.isfinite(out_s.float()).all(), s


# ---- 7. the library op and torch.compile ------------------------------------------------------------------------------------------------
def test_the_library_op_called_directly_is_the_function():
    D, dtype, fmt, ps = 128, torch.bfloat16, "e4m3", 128
    t = P.shared_tables(ps)[1]
    G, sq = V.QCASES[2]
    c = _cache(t, D, dtype, fmt, _pack(*_rows(t, D, fmt, 95), fmt))
    q = _rand((sum(sq), HKV * G, D), dtype, 98)
    cud = _su(V.cu_of(sq))
    got = qa.ops.fp8_paged_varlen_splitkv_attention_forward(q, c.k, c.v, c.scale_k, c.scale_v, c.block_table, c.seqlens, cud, max(sq), CAP, c.num_pages,
                                                            ps, 2, fmt, "compiled", True, "accurate", True, True)
    want = qa.fp8_attn_paged_varlen_func(q, c, cud, max(sq), causal=True, num_splits=2, return_lse=True, return_partials=True)
    assert len(got) == len(want) == 5 and all(_same_bits(x, y) for x, y in zip(got, want))


def test_torch_compile_fullgraph_of_append_then_attend_gives_the_eager_bits():
    D, dtype, fmt, ps, T = 64, torch.float16, "e4m3", 64, 4
    t = P.Tables(ps, (CAP,) * B, seed=90, need=[CAP // ps] * B)
    pools = _pack(*_rows(t, D, fmt, 90), fmt)
    ca, cb = (_cache(t, D, dtype, fmt, pools, lens=[130, 63, 0]) for _ in range(2))
    counts = (4, 1, 2)
    q, kn, vn = _rand((sum(counts), 4, D), dtype, 92), _rand((B, HKV, T, D), dtype, 93), _rand((B, HKV, T, D), dtype, 94)
    cud, nl = _su(V.cu_of(counts)), _su(counts)

    def step(cache):
        def f(q, kn, vn, cu, nl):
            qa.paged_kv_cache_append_fp8(cache, kn, vn, new_lens=nl)
            return qa.fp8_attn_paged_varlen_func(q * 2, cache, cu, T, causal=True, num_splits=2, max_seqlen_k=256, return_lse=True)
        return f

    torch._dynamo.reset()
    got = torch.compile(step(ca), fullgraph=True)(q, kn, vn, cud, nl)
    want = step(cb)(q, kn, vn, cud, nl)
    assert all(_same_bits(x, y) for x, y in zip(got, want))
    assert ca.seqlens.tolist() == cb.seqlens.tolist() == [134, 64, 2] and torch.equal(ca.k, cb.k) and torch.equal(ca.v, cb.v)
    assert not math.isnan(float(got[0].float().sum()))


# ---- 8. accuracy ------------------------------------------------------------------------------------------------------------------------
def test_gqa_causal_three_splits_is_within_the_fp8_v_bound_of_the_fp64_oracle():
    """per sequence the fp64 oracle (causal with q_offset = L_b - Sq_b) on the call's own q8 rows and on the pool's bytes looked up key by
    key through the table; bound gpu_utils.grade, |got - ref| < 2^-6 max(1, |ref| / 2); the measured ratio is printed (DESIGN.md section 4.20 records it)"""
    D, dtype, fmt, ps = 128, torch.bfloat16, "e4m3", 128
    t = P.shared_tables(ps)[3]                                     # lengths (128, 65, 1280)
    G, sq = V.QCASES[2]                                            # query counts (5, 1, 33)
    Hq, cu, total = HKV * G, V.cu_of(sq), sum(sq)
    rk, rv = _rows(t, D, fmt, 5)
    # scales of order 1: the de-quantised keys and values are ~N(0, 1) and ~N(0, 4), so that the absolute part of the bound is not slack
    c = _cache(t, D, dtype, fmt, _pack(rk, rv, fmt), scale_k=torch.tensor([[0.5, 1.0], [0.75, 0.6], [1.0, 0.4]]))
    q = _rand((total, Hq, D), dtype, 6, mul=1.5)
    out, q8, sqs = _varlen(q, c, _su(cu), max(sq), is_causal=True, num_splits=3, return_quant=True)
    k8n, v8n = (P.gather_rows(r.cpu().numpy(), t.table, ps) for r in (rk, rv))            # [B, HKV, CAP, D] by the key-level lookup
    o, q8n, sqn, skn, svn = gpu_utils.out_to_f32(out), bits8(q8), sqs.cpu().numpy(), c.scale_k.cpu().numpy(), c.scale_v.cpu().numpy()
    f, worst = FMT[fmt], 0.0
    for b, L in enumerate(t.lens):
        n = sq[b]
        q8b = q8n[Hq * D * cu[b]:Hq * D * cu[b + 1]].reshape(1, Hq, n, D)                # the slab of the packed pre-pass
        ref = oracle.attention_forward(q8b, k8n[b:b + 1, :, :L], v8n[b:b + 1, :, :L], f, f, f, sqn[b:b + 1], skn[b:b + 1], svn[b:b + 1],
                                       causal=True, q_offset=L - n, sm_scale=0.0)
        worst = max(worst, gpu_utils.grade(o[cu[b]:cu[b + 1]].transpose(1, 0, 2)[None], ref)[2])
    print(f"packed paged GQA causal ns=3: worst |err| / bound {worst:.3f}")
    assert worst < 1.0, worst

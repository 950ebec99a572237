"""The paged FP8 K/V cache on the MI355X (quantumattention_amd/paged.py, include/qattn_paged.h).

Everything is graded against the CONTIGUOUS entries on the cache gathered through the table (tests/paged_cases.py: `gather`, a chunk-level
index copy restated from the header's address map): the paged attention gives the bits of fp8_attn_splitkv_func on the gathered
PreparedKV, the paged append leaves the pool whose gathered images are kv_cache_append_fp8's.  The tables are the shared ones of
paged_cases: shuffled, no identity row, no two equal rows, one shared prefix page, and every entry behind ceil(L_b / page_size) on a pool
page full of NaN bytes -- a VALID index, so an entry read too far shows as NaN, never as a fault.  No test feeds an out-of-range entry.
Shapes: B 3, Hkv 2, max_pages * page_size = 1280 for page sizes 64 / 128 / 256, lengths {0, 1, 63, 64, 65, ps - 1, ps, ps + 1, 1100, 1280}."""
import math

import numpy as np
import pytest
import torch

import oracle
import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import gpu_utils
from tests import kvcache_cases as KC
from tests import paged_cases as P
from tests.gpu_utils import FMT, bits8

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV, CAP = P.B, P.HKV, P.CAP
# D x 16-bit dtype x fp8 format: a cross, not the full product (tests/test_gpu_kvcache.py CFGS)
CFGS = [(64, torch.bfloat16, "e4m3"), (128, torch.bfloat16, "e4m3"), (256, torch.bfloat16, "e4m3"), (128, torch.float16, "e4m3"),
        (128, torch.bfloat16, "e5m2"), (64, torch.float16, "e5m2"), (256, torch.float16, "e5m2")]
CFG_IDS = [f"d{d}-{str(t)[6:]}-{f}" for d, t, f in CFGS]
GS = [(1, 1), (4, 5), (4, 1), (1, 5)]      # (G, Sq), rotated over the four shared tables of a page size
SCALE_K = torch.tensor([[0.010, 0.020], [0.015, 0.012], [0.030, 0.008]])


def _rand(shape, dtype, seed, mul=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * mul).to(dtype).to(DEV)


def _su(x):
    return torch.tensor(np.asarray(x), dtype=torch.int32, device=DEV)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _pack(rows_k, rows_v, fmt):
    """row-major uint8 [P, HKV, ps, D] -> the two pools"""
    fp8 = P.FP8[fmt]
    return _native.pack_fp8(rows_k.view(fp8), _native.LAYOUT_KFRAG), _native.pack_fp8(rows_v.view(fp8), _native.LAYOUT_VFRAG)


def _rows(t, D, fmt, seed, poison=True):
    rk, rv = P.random_rows(t.num_pages, t.page_size, D, fmt, seed, DEV)
    if poison:
        rk[P.POISON], rv[P.POISON] = P.NAN_BYTE[fmt], P.NAN_BYTE[fmt]
    return rk, rv


def _cache(t, D, dtype, fmt, pools, table=None, lens=None, scale_k=SCALE_K):
    c = qa.alloc_paged_kv_cache_fp8(t.num_pages, HKV, t.page_size, D, batch_size=B, max_pages_per_seq=t.M, scale_k=scale_k, scale_v=scale_k * 2,
                                    dtype=dtype, device=DEV, fp8_format=fmt)
    assert c.layout == "frag" and c.k.numel() == P.pool_bytes(t.num_pages, HKV, t.page_size, D) == pools[0].numel()
    c.k.copy_(pools[0])
    c.v.copy_(pools[1])
    c.block_table.copy_(_su(t.table if table is None else table))
    c.seqlens.copy_(_su(t.lens if lens is None else lens))
    return c


def _gathered(c, table, D):
    """the contiguous PreparedKV the table selects from the cache's pools"""
    ps = c.page_size
    return qa.PreparedKV(P.gather(c.k, table, HKV, ps, D), P.gather(c.v, table, HKV, ps, D), c.scale_k, c.scale_v, (B, HKV, CAP, D),
                         c.fp8_format, c.dtype, c.numerics, "frag")


def _paged(q, c, su, **kw):
    return _native.fp8_attention_paged_splitkv(q, c.k, c.v, c.scale_k, c.scale_v, c.block_table, su, Skv=CAP, num_pages=c.num_pages,
                                               page_size=c.page_size, fp8_dtype=P.FP8[c.fp8_format], **kw)


def _contig(q, kv, su, **kw):
    return _native.fp8_attention_splitkv(q, kv.k, kv.v, kv.scale_k, kv.scale_v, Skv=CAP, fp8_dtype=P.FP8[kv.fp8_format], seqused_k=su, **kw)


# ---- 1. attend = gather ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
@pytest.mark.parametrize("D,dtype,fmt", CFGS, ids=CFG_IDS)
def test_paged_attention_gives_the_bits_of_the_contiguous_entry_on_the_gathered_cache(D, dtype, fmt, page_size):
    """out, lse, row_path and the fp32 partials (outputs, LSEs, path bytes), for num_splits 1 / 2 / 3 / 9 (the chained merge) / 0, causal
    or not, accurate and fast: this one equality carries contracts (a) .. (g) of include/qattn_splitkv.h over to the paged entry"""
    for i, t in enumerate(P.shared_tables(page_size)):
        G, Sq = GS[(i + page_size // 64) % 4]
        c = _cache(t, D, dtype, fmt, _pack(*_rows(t, D, fmt, 11 * D + i), fmt))
        kv = _gathered(c, t.table, D)
        q = _rand((B, HKV * G, Sq, D), dtype, 7 * D + i, mul=1.5)
        su = c.seqlens
        for ns in (1, 2, 3, 9, 0):
            for causal in (False, True):
                for precision in ("accurate", "fast"):
                    kw = dict(is_causal=causal, precision=precision, num_splits=ns, return_lse=True, return_partials=True, return_path=True)
                    got, want = _paged(q, c, su, **kw), _contig(q, kv, su, **kw)
                    assert len(got) == len(want) == 6
                    for name, x, y in zip(("out", "lse", "partial_o", "partial_lse", "partial_path", "row_path"), got, want):
                        assert _same_bits(x, y), (t.lens, G, Sq, ns, causal, precision, name)
                    assert not torch.isnan(got[0].float()).any()
                    if ns == 1 and precision == "fast":     # no LSE: the byte-exponential sweep
                        assert _same_bits(_paged(q, c, su, is_causal=causal, precision="fast", num_splits=1),
                                          _contig(q, kv, su, is_causal=causal, precision="fast", num_splits=1)), (t.lens, causal)
        # the public function is that call (seqused_k defaults to cache.seqlens)
        pub = qa.fp8_attn_paged_func(q, c, causal=True, num_splits=3, return_lse=True, return_partials=True)
        ref = qa.fp8_attn_splitkv_func(q, kv, causal=True, seqused_k=su, num_splits=3, return_lse=True, return_partials=True)
        assert len(pub) == len(ref) == 5 and all(_same_bits(x, y) for x, y in zip(pub, ref))
        # max_seqlen_k tightens the logical bound as a shorter contiguous Skv does: keys at or beyond it are not attended
        mx = 1100
        cut = qa.PreparedKV(kv.k.view(B, HKV, -1)[:, :, :(mx + 63) // 64 * 64 * D].contiguous().view(-1),
                            kv.v.view(B, HKV, -1)[:, :, :(mx + 63) // 64 * 64 * D].contiguous().view(-1), kv.scale_k, kv.scale_v, (B, HKV, mx, D), fmt,
                            dtype, kv.numerics, "frag")
        a = qa.fp8_attn_paged_func(q, c, causal=True, num_splits=2, max_seqlen_k=mx, return_lse=True)
        b = qa.fp8_attn_splitkv_func(q, cut, causal=True, seqused_k=su, num_splits=2, return_lse=True)
        assert all(_same_bits(x, y) for x, y in zip(a, b))


# ---- 2. append = gather ---------------------------------------------------------------------------------------------------------------------
def _append_pair(page_size, D, dtype, fmt, seed):
    """a paged cache whose sequences own all their pages (shuffled, private) over a pool of random bytes with the poison page, and the
    contiguous KVCacheFP8 that starts from the gathered images"""
    t = P.Tables(page_size, (CAP,) * B, seed=seed, need=[CAP // page_size] * B)
    pc = _cache(t, D, dtype, fmt, _pack(*_rows(t, D, fmt, seed), fmt), lens=[0] * B)
    cc = qa.alloc_kv_cache_fp8(B, HKV, CAP, D, scale_k=SCALE_K, scale_v=SCALE_K * 2, dtype=dtype, device=DEV, fp8_format=fmt)
    cc.k.copy_(P.gather(pc.k, t.table, HKV, page_size, D))
    cc.v.copy_(P.gather(pc.v, t.table, HKV, page_size, D))
    return t, pc, cc


def _step(t, pc, cc, lens, k, v, new_lens=None, advance=True, what=""):
    """one append to both caches from the given lengths; then: the lengths agree and are the header's, the gathered pool IS the contiguous
    image (every byte), and of the whole pool exactly the appended keys' bytes may have changed"""
    ps, D, T = t.page_size, pc.shape[3], k.shape[2]
    for c in (pc, cc):
        c.seqlens.copy_(_su(lens))
    before = [KC.from_image(x, lay, t.num_pages, HKV, ps, D).clone() for x, lay in ((pc.k, KC.KFRAG), (pc.v, KC.VFRAG))]
    nl = None if new_lens is None else _su(new_lens)
    assert qa.paged_kv_cache_append_fp8(pc, k, v, new_lens=nl, advance=advance) is pc
    qa.kv_cache_append_fp8(cc, k, v, new_lens=nl, advance=advance)
    cnt = [T if new_lens is None else min(max(new_lens[b], 0), T) for b in range(B)]
    end = [min(lens[b] + cnt[b], CAP) for b in range(B)]
    assert pc.seqlens.tolist() == cc.seqlens.tolist() == (end if advance else list(lens)), what
    assert torch.equal(P.gather(pc.k, t.table, HKV, ps, D), cc.k) and torch.equal(P.gather(pc.v, t.table, HKV, ps, D), cc.v), what
    mine = torch.zeros(t.num_pages, HKV, ps, dtype=torch.bool, device=DEV)
    for b in range(B):
        for j in range(lens[b], end[b]):
            mine[int(t.table[b, j // ps]), :, j % ps] = True
    for x, lay, old in ((pc.k, KC.KFRAG, before[0]), (pc.v, KC.VFRAG, before[1])):
        new = KC.from_image(x, lay, t.num_pages, HKV, ps, D)
        assert torch.equal(new[~mine], old[~mine]), (what, "a byte that belongs to no appended key changed")
        assert (new[mine] != old[mine]).any() or not mine.any(), what


@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
@pytest.mark.parametrize("D,dtype,fmt", CFGS, ids=CFG_IDS)
def test_paged_append_leaves_the_pool_whose_gathered_images_are_the_contiguous_appends(D, dtype, fmt, page_size):
    ps = page_size
    t, pc, cc = _append_pair(ps, D, dtype, fmt, 3 * D + ps)
    kv = lambda T, s: (_rand((B, HKV, T, D), dtype, s, mul=2.0), _rand((B, HKV, T, D), dtype, s + 1, mul=2.0))
    _step(t, pc, cc, [0, 63, ps], *kv(1, 100), what="T1")
    _step(t, pc, cc, [ps - 3, 2 * ps - 3, 61], *kv(7, 102), what="T7 from page_size - 3: a page boundary crossed, a 4-key group split at both ends")
    _step(t, pc, cc, [5, ps - 3, 1100], *kv(130, 104), what="T130: starts mid-chunk, crosses two pages at page_size 64")
    _step(t, pc, cc, [17, 126, ps], *kv(4, 106), new_lens=[0, 3, 4], what="new_lens with a 0")
    _step(t, pc, cc, [30, 62, 200], *kv(5, 108), advance=False, what="advance=False")
    bthd_k, bthd_v = _rand((B, 70, HKV, D), dtype, 110), _rand((B, 70, HKV, D), dtype, 111)
    kx, vx = bthd_k.transpose(1, 2), bthd_v.transpose(1, 2)
    assert not kx.is_contiguous()
    _step(t, pc, cc, [61, 2, 640], kx, vx, what="a transposed [B, T, Hkv, D] view")
    _step(t, pc, cc, [64, 2 * ps, 1216], *kv(64, 112), what="T64 on chunk boundaries: whole chunks")


# ---- 3. overflow ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
def test_overflow_drops_tokens_saturates_seqlens_and_stays_inside_the_sequences_pages(page_size):
    D, dtype, GUARD = 64, torch.bfloat16, 1 << 16
    t, pc, cc = _append_pair(page_size, D, dtype, "e4m3", 50)
    bufs = []
    for name in ("k", "v"):                       # the pools re-homed between guards
        img = getattr(pc, name)
        buf = torch.full((img.numel() + 2 * GUARD,), 0xC3, dtype=torch.uint8, device=DEV)
        buf[GUARD:GUARD + img.numel()] = img
        setattr(pc, name, buf[GUARD:GUARD + img.numel()])
        bufs.append(buf)
    k, v = _rand((B, HKV, 16, D), dtype, 51), _rand((B, HKV, 16, D), dtype, 52)
    _step(t, pc, cc, [CAP - 6, CAP, CAP - 70], k, v, what="T16 at 6 below, at, and 70 below the capacity")       # (_step: only appended keys change)
    assert pc.seqlens.tolist() == [CAP, CAP, CAP - 54]
    _step(t, pc, cc, [CAP, CAP, CAP], k, v, what="full: nothing written")
    for buf in bufs:
        assert (buf[:GUARD] == 0xC3).all() and (buf[-GUARD:] == 0xC3).all()


# ---- 4. poison ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
@pytest.mark.parametrize("D,fmt", [(64, "e4m3"), (128, "e5m2"), (256, "e4m3")])
def test_unread_table_entries_and_bytes_behind_the_lengths_influence_no_bit(D, fmt, page_size):
    """every table entry behind ceil(L_b / page_size) on the NaN page and NaN bytes in the tail of each sequence's last page behind L_b (where
    that page is the sequence's own: the shared prefix page holds another sequence's keys there), against the same call with those entries
    and bytes zeroed"""
    dtype, ps = torch.bfloat16, page_size
    for i, t in enumerate(P.shared_tables(ps)):
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
        G, Sq = GS[i]
        q = _rand((B, HKV * G, Sq, D), dtype, 17 * D + i, mul=1.5)
        for ns in (1, 3, 9):
            for causal in (False, True):
                for precision in ("accurate", "fast"):
                    kw = dict(causal=causal, num_splits=ns, precision=precision, return_lse=True, return_partials=True)
                    got, want = qa.fp8_attn_paged_func(q, hot, **kw), qa.fp8_attn_paged_func(q, cold, **kw)
                    assert torch.isfinite(got[0].float()).all() and not torch.isnan(got[1]).any() and not torch.isnan(got[2]).any()
                    assert all(_same_bits(x, y) for x, y in zip(got, want)), (t.lens, ns, causal, precision)


# ---- 5. prefix sharing ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
def test_two_sequences_that_share_prefix_pages_give_the_outputs_of_two_private_copies(page_size):
    D, dtype, fmt, ps = 128, torch.bfloat16, "e4m3", page_size
    lens = (2 * ps + 70, 3 * ps + 1, 2 * ps)
    t = P.Tables(ps, lens, seed=9, need=[4, 4, 2])                # private pages; the sharing is set up here
    shared, private = t.table.copy(), t.table.copy()
    shared[1, :2] = shared[0, :2]                                  # sequences 0 and 1: the same first two pages
    rk, rv = _rows(t, D, fmt, 77)
    for r in (rk, rv):                                             # the private copies of the prefix
        r[private[1, 0]], r[private[1, 1]] = r[private[0, 0]].clone(), r[private[0, 1]].clone()
    pools = _pack(rk, rv, fmt)
    sk = torch.tensor([[0.01, 0.02], [0.01, 0.02], [0.03, 0.008]])   # a shared page needs equal scales in its sequences
    a, b = _cache(t, D, dtype, fmt, pools, table=shared, scale_k=sk), _cache(t, D, dtype, fmt, pools, table=private, scale_k=sk)
    q = _rand((B, 8, 3, D), dtype, 78, mul=1.5)
    for ns in (1, 2):
        got = qa.fp8_attn_paged_func(q, a, causal=True, num_splits=ns, return_lse=True)
        want = qa.fp8_attn_paged_func(q, b, causal=True, num_splits=ns, return_lse=True)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and torch.isfinite(got[0].float()).all()


# ---- 6. graph -------------------------------------------------------------------------------------------------------------------------------
def test_one_captured_decode_step_follows_a_rewritten_block_table_and_rolled_back_seqlens():
    D, dtype, fmt, ps = 128, torch.bfloat16, "e4m3", 64
    lens0 = [ps - 1, 5, 1100]
    t = P.Tables(ps, lens0, seed=4, need=[1, 1, 18])               # sequence 0 fills its only page with the first step's token
    spare = [p for p in range(t.num_pages) if p != P.POISON and p not in set(t.table.flatten().tolist())]
    pools = _pack(*_rows(t, D, fmt, 31), fmt)
    mk = lambda: _cache(t, D, dtype, fmt, pools, lens=lens0)
    graphed, eager, warm = mk(), mk(), mk()
    attend = lambda q, c: qa.fp8_attn_paged_func(q, c, causal=True, num_splits=3, return_lse=True)
    inputs = lambda s: (_rand((B, 8, 1, D), dtype, 700 + s), _rand((B, HKV, 1, D), dtype, 800 + s, mul=1.5), _rand((B, HKV, 1, D), dtype, 900 + s, mul=1.5))
    qs, ks, vs = (x.clone() for x in inputs(0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        qa.paged_kv_cache_append_fp8(warm, ks, vs)
        attend(qs, warm)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        qa.paged_kv_cache_append_fp8(graphed, ks, vs)
        out_s, lse_s = attend(qs, graphed)
    assert graphed.seqlens.tolist() == lens0                       # capture ran nothing

    def edit(step, c):
        if step == 1:                                              # the allocator hands sequence 0 a new page, in place
            c.block_table[0, 1] = spare[0]
        if step == 2:                                              # a rollback: two of sequence 2's tokens are rejected
            c.seqlens[2] -= 2
        if step == 3:                                              # sequence 1 moves to another page (its old one goes back to the pool)
            old = int(c.block_table[1, 0])
            c.k.view(c.num_pages, -1)[spare[1]] = c.k.view(c.num_pages, -1)[old]
            c.v.view(c.num_pages, -1)[spare[1]] = c.v.view(c.num_pages, -1)[old]
            c.block_table[1, 0] = spare[1]

    want_lens = [[ps, 6, 1101], [ps + 1, 7, 1102], [ps + 2, 8, 1101], [ps + 3, 9, 1102]]
    for s in range(4):
        for c in (graphed, eager):
            edit(s, c)
        q, k, v = inputs(s)
        for dst, src in zip((qs, ks, vs), (q, k, v)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        qa.paged_kv_cache_append_fp8(eager, k, v)
        out, lse = attend(q, eager)
        assert graphed.seqlens.tolist() == eager.seqlens.tolist() == want_lens[s], s
        assert _same_bits(out_s, out) and _same_bits(lse_s, lse), s
        assert torch.equal(graphed.k, eager.k) and torch.equal(graphed.v, eager.v), s
    assert torch.isfinite(out_s.float()).all()


# ---- 7. the library ops and torch.compile ---------------------------------------------------------------------------------------------------
def test_the_library_ops_called_directly_are_the_functions():
    D, dtype, fmt, ps = 128, torch.bfloat16, "e4m3", 128
    t, a, _ = _append_pair(ps, D, dtype, fmt, 95)
    _, b, _ = _append_pair(ps, D, dtype, fmt, 95)
    kn, vn = _rand((B, HKV, 9, D), dtype, 96), _rand((B, HKV, 9, D), dtype, 97)
    nl = _su([9, 2, 0])
    for c in (a, b):
        c.seqlens.copy_(_su([61, 130, 7]))
    assert qa.ops.fp8_paged_kv_cache_append_(a.k, a.v, a.scale_k, a.scale_v, a.block_table, a.seqlens, kn, vn, nl, a.num_pages, ps, fmt, True) is None
    qa.paged_kv_cache_append_fp8(b, kn, vn, new_lens=nl)
    assert a.seqlens.tolist() == b.seqlens.tolist() == [70, 132, 7] and torch.equal(a.k, b.k) and torch.equal(a.v, b.v)
    q = _rand((B, 4, 2, D), dtype, 98)
    got = qa.ops.fp8_paged_splitkv_attention_forward(q, a.k, a.v, a.scale_k, a.scale_v, a.block_table, a.seqlens, CAP, a.num_pages, ps, 2, fmt,
                                                     "compiled", True, "accurate", True, True)
    want = qa.fp8_attn_paged_func(q, b, causal=True, num_splits=2, return_lse=True, return_partials=True)
    assert len(got) == len(want) == 5 and all(_same_bits(x, y) for x, y in zip(got, want))


def test_torch_compile_fullgraph_of_append_then_attend_gives_the_eager_bits():
    D, dtype, fmt, ps = 64, torch.float16, "e4m3", 64
    _, ca, _ = _append_pair(ps, D, dtype, fmt, 90)
    _, cb, _ = _append_pair(ps, D, dtype, fmt, 90)
    for c in (ca, cb):
        c.seqlens.copy_(_su([130, 63, 0]))
    q, kn, vn = _rand((B, 4, 2, D), dtype, 92), _rand((B, HKV, 2, D), dtype, 93), _rand((B, HKV, 2, D), dtype, 94)

    def step(cache):
        def f(q, kn, vn):
            qa.paged_kv_cache_append_fp8(cache, kn, vn)
            return qa.fp8_attn_paged_func(q * 2, cache, causal=True, num_splits=2, max_seqlen_k=256, return_lse=True)
        return f

    torch._dynamo.reset()
    got = torch.compile(step(ca), fullgraph=True)(q, kn, vn)
    want = step(cb)(q, kn, vn)
    assert all(_same_bits(x, y) for x, y in zip(got, want))
    assert ca.seqlens.tolist() == cb.seqlens.tolist() == [132, 65, 2] and torch.equal(ca.k, cb.k) and torch.equal(ca.v, cb.v)
    assert not math.isnan(float(got[0].float().sum()))


# ---- 8. accuracy ----------------------------------------------------------------------------------------------------------------------------
def test_gqa_causal_three_splits_is_within_the_fp8_v_bound_of_the_fp64_oracle():
    """contract (g) of the contiguous entry, on the paged one: per sequence the fp64 oracle (causal with q_offset = L_b - Sq) on the call's
    own q8 rows and on the pool's bytes looked up key by key through the table; bound gpu_utils.grade, |got - ref| < 2^-6 max(1, |ref| / 2)"""
    D, dtype, fmt, ps = 128, torch.bfloat16, "e4m3", 128
    t = P.shared_tables(ps)[3]                                     # lengths (128, 65, 1280)
    rk, rv = _rows(t, D, fmt, 5)
    # scales of order 1: the de-quantised keys and values are ~N(0, 1) and ~N(0, 4), so that the absolute part of the bound is not slack
    c = _cache(t, D, dtype, fmt, _pack(rk, rv, fmt), scale_k=torch.tensor([[0.5, 1.0], [0.75, 0.6], [1.0, 0.4]]))
    G, Sq = 4, 5
    q = _rand((B, HKV * G, Sq, D), dtype, 6, mul=1.5)
    out, q8, sq = _paged(q, c, c.seqlens, is_causal=True, num_splits=3, return_quant=True)
    k8n, v8n = (P.gather_rows(r.cpu().numpy(), t.table, ps) for r in (rk, rv))            # [B, HKV, CAP, D] by the key-level lookup
    o, q8n, sqn, skn, svn = gpu_utils.out_to_f32(out), bits8(q8), sq.cpu().numpy(), c.scale_k.cpu().numpy(), c.scale_v.cpu().numpy()
    f, worst = FMT[fmt], 0.0
    for b, L in enumerate(t.lens):
        ref = oracle.attention_forward(q8n[b:b + 1], k8n[b:b + 1, :, :L], v8n[b:b + 1, :, :L], f, f, f, sqn[b:b + 1], skn[b:b + 1], svn[b:b + 1],
                                       causal=True, q_offset=L - Sq, sm_scale=0.0)
        worst = max(worst, gpu_utils.grade(o[b:b + 1], ref)[2])
    print(f"paged GQA causal ns=3: worst |err| / bound {worst:.3f}")
    assert worst < 1.0, worst

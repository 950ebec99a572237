"""-m gpu: the MLA entries at byte offsets above 2^31 and 2^32, by the method of tests/test_gpu_large_offsets.py -- a row-major latent pool,
a chunk-image latent pool and an index pool of more than 2^32 bytes each, logits rows behind strides of more than 2^29 elements, q and
index lists behind strides of more than 2^31 elements, and sparse partials of more than 2^31 floats.  The
rows here are 576, 36 864 / 64 and 128 bytes: no power of two, so a row number times its size leaves 32 bits long before the row number does.

Every test ALLOCATES the large buffer and does not fill it (torch.empty; the pages a test uses are zeroed), runs the same calls on the large
geometry and on a small one that holds the same tokens at low addresses behind a remapped table, and asks for the same BITS.  A test first
asks for its memory by name and skips, naming the bytes, on a card that cannot hold it (an MI355X holds them all).  Every table entry, index
and length is in range."""
import numpy as np
import pytest
import torch

from quantumattention_amd import _native
from tests.test_gpu_large_offsets import GIB, _need, _rand, _same_bits, _su
from tests.test_gpu_mla_buffer_contract import _ll, filled_pool

pytestmark = pytest.mark.gpu

DEV = "cuda"
PS, BQ, M = 64, 3, 5
FP8 = torch.float8_e4m3fn
SM_SCALE = 192.0 ** -0.5
SPARE = 9                                         # what every unused table entry points at (in range, zeroed)


def _tables(P, straddle, mixed):
    """(big table, small table, used big pages, their small pages): slot 0 owns the LAST pages of the pool"""
    big = np.full((BQ, M), SPARE, np.int64)
    big[0], big[1], big[2] = [P - 1, P - 2, P - 3, P - 4, P - 5], straddle, mixed
    pages = sorted(set(big.flatten().tolist()))
    assert len(pages) == BQ * M and max(pages) == P - 1 and min(pages) >= 0
    order = np.random.RandomState(0).permutation(len(pages))
    small_of = {p: int(order[i]) for i, p in enumerate(pages)}
    return _su(big), _su(np.vectorize(small_of.get)(big)), torch.tensor(pages, device=DEV), torch.tensor([small_of[p] for p in pages], device=DEV)


def _all_same(got, want, what):
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert _same_bits(x, y), (what, i)


def _two_appends(append, pools, tables, idx, page_bytes, width):
    """two appends (the second starts mid-page) into the big and the small pool; every written page holds the same bytes"""
    scale = torch.tensor([0.010, 0.015, 0.030], device=DEV)
    lens = [torch.zeros(BQ, dtype=torch.int32, device=DEV) for _ in pools]
    for step, counts in enumerate(([130, 70, 129], [130, 130, 65])):
        x = _rand((BQ, 130, width), torch.bfloat16, 10 + step, 1.5)
        for pool, table, sl in zip(pools, tables, lens):
            append(pool, scale, table, sl, x, _su(counts))
        assert lens[0].tolist() == lens[1].tolist()
        big, small = (p.view(-1).view(-1, page_bytes) for p in pools)
        assert torch.equal(big[idx[0]], small[idx[1]]), ("the written pages", step)
    assert lens[0].tolist() == [260, 200, 194] and small[idx[1]].any(dim=1).sum() >= 11
    return scale, lens[0]


# ---- 1. a row-major latent pool of more than 2^32 bytes ----------------------------------------------------------------------------------------
def test_a_row_major_latent_pool_of_more_than_4_gib_gives_the_bits_of_a_small_pool():
    """576-byte rows, page 64: row 3 728 271 crosses byte 2^31 (page 58 254) and row 7 456 541 byte 2^32 (page 116 508).  Slot 1's pages
    straddle both marks, slot 2 mixes low and high pages.  The row append, the sparse decode with 1 and 2 splits and the packed sparse
    entry, with lists that name keys of every page."""
    P, page_bytes = 116520, PS * 576
    assert 58254 * page_bytes < 1 << 31 < 58255 * page_bytes and 116508 * page_bytes < 1 << 32 < 116509 * page_bytes < P * page_bytes
    assert 3728271 // PS == 58254 and 7456541 // PS == 116508
    _need(P * page_bytes + GIB, "the row-major latent pool test")
    tb, ts, ib, ism = _tables(P, [58253, 58254, 58255, 116508, 116509], [1, 0, 116510, 5, 58252])
    big = torch.empty((P, PS, 576), dtype=torch.uint8, device=DEV)
    small = torch.zeros((BQ * M, PS, 576), dtype=torch.uint8, device=DEV)
    big.view(P, page_bytes)[ib] = 0

    def append(pool, scale, table, sl, x, new):
        _native.paged_mla_row_cache_append_fp8(pool, scale, table, sl, x[..., :512], x[..., 512:], num_pages=pool.shape[0], page_size=PS,
                                               fp8_dtype=FP8, new_lens=new)
    scale, lens = _two_appends(append, (big, small), (tb, ts), (ib, ism), page_bytes, 576)
    q = _rand((BQ, 16, 2, 576), torch.bfloat16, 30, 1.5)
    idx = torch.randint(-1, 260, (BQ, 2, 200), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(DEV)
    counts = (3, 1, 4)
    qp, cu = _rand((sum(counts), 16, 576), torch.bfloat16, 31, 1.5), _su([0] + np.cumsum(counts).tolist())
    idxp = torch.randint(-1, 260, (sum(counts), 200), generator=torch.Generator().manual_seed(2), dtype=torch.int32).to(DEV)
    kw = dict(page_size=PS, fp8_dtype=FP8, is_causal=True, sm_scale=SM_SCALE)
    calls = {
        "sparse, one split": lambda pool, t: _native.fp8_mla_paged_sparse_attention(q, pool, scale, t, lens, idx, num_pages=pool.shape[0], num_splits=1,
                                                                                    return_q8=True, **kw),
        "sparse, two splits": lambda pool, t: _native.fp8_mla_paged_sparse_attention(q, pool, scale, t, lens, idx, num_pages=pool.shape[0], num_splits=2,
                                                                                     return_partials=True, **kw),
        "sparse, packed": lambda pool, t: _native.fp8_mla_paged_sparse_varlen_attention(qp, pool, scale, t, lens, idxp, cu, num_pages=pool.shape[0],
                                                                                        return_q8=True, **kw),
    }
    for what, f in calls.items():
        got, want = f(big, tb), f(small, ts)
        _all_same(got, want, what)
        assert torch.isfinite(got[0].float()).all() and got[0].float().abs().sum() > 0, what


# ---- 2. a chunk-image latent pool of more than 2^32 bytes --------------------------------------------------------------------------------------
def test_a_dense_mla_pool_of_more_than_4_gib_gives_the_bits_of_a_small_pool():
    """36 864-byte chunks, page 64: page 58 254 crosses byte 2^31 and page 116 508 byte 2^32.  The append, then the dense decode with 1 and
    3 splits."""
    P, page_bytes = 116520, 36864
    L = _native.lib()
    assert L.qattn_mla_pool_bytes(P, PS) == P * page_bytes > 1 << 32
    _need(P * page_bytes + GIB, "the dense MLA pool test")
    tb, ts, ib, ism = _tables(P, [58253, 58254, 58255, 116508, 116509], [1, 0, 116510, 5, 58252])
    big = torch.empty((P * page_bytes,), dtype=torch.uint8, device=DEV)
    small = torch.zeros((BQ * M * page_bytes,), dtype=torch.uint8, device=DEV)
    big.view(P, page_bytes)[ib] = 0

    def append(pool, scale, table, sl, x, new):
        _native.paged_mla_cache_append_fp8(pool, scale, table, sl, x[..., :512], x[..., 512:], num_pages=pool.numel() // page_bytes, page_size=PS,
                                           fp8_dtype=FP8, new_lens=new)
    scale, lens = _two_appends(append, (big, small), (tb, ts), (ib, ism), page_bytes, 576)
    q = _rand((BQ, 20, 3, 576), torch.bfloat16, 32, 1.5)
    for ns in (1, 3):
        f = lambda pool, t: _native.fp8_mla_paged_attention(q, pool, scale, t, lens, Skv=M * PS, num_pages=pool.numel() // page_bytes, page_size=PS,
                                                            fp8_dtype=FP8, is_causal=True, sm_scale=SM_SCALE, num_splits=ns, return_partials=True,
                                                            return_q8=True)
        got, want = f(big, tb), f(small, ts)
        _all_same(got, want, ("dense", ns))
        assert torch.isfinite(got[0].float()).all() and got[0].float().abs().sum() > 0


# ---- 3. an index pool of more than 2^32 bytes --------------------------------------------------------------------------------------------------
def test_an_index_pool_of_more_than_4_gib_gives_the_bits_of_a_small_pool():
    """128-byte rows, page 64: page 262 144 starts at byte 2^31 and page 524 288 at byte 2^32.  The append, the scores, the whole top-k
    entry (one workgroup a row and three) and the packed entry."""
    P, page_bytes = 524300, PS * 128
    assert 262144 * page_bytes == 1 << 31 and 524288 * page_bytes == 1 << 32 < P * page_bytes
    _need(P * page_bytes + GIB, "the index pool test")
    tb, ts, ib, ism = _tables(P, [262143, 262144, 524287, 524288, 262145], [1, 0, 524289, 5, 262142])
    big = torch.empty((P, PS, 128), dtype=torch.uint8, device=DEV)
    small = torch.zeros((BQ * M, PS, 128), dtype=torch.uint8, device=DEV)
    big.view(P, page_bytes)[ib] = 0

    def append(pool, scale, table, sl, x, new):
        _native.paged_mla_index_cache_append_fp8(pool, scale, table, sl, x, num_pages=pool.shape[0], page_size=PS, fp8_dtype=FP8, new_lens=new)
    scale, lens = _two_appends(append, (big, small), (tb, ts), (ib, ism), page_bytes, 128)
    Hi, Sq, N = 20, 3, M * PS
    q, w = _rand((BQ, Hi, Sq, 128), torch.bfloat16, 33), _rand((BQ, Sq, Hi), torch.float32, 34)
    counts = (3, 1, 9)
    qp, wp, cu = _rand((sum(counts), Hi, 128), torch.bfloat16, 35), _rand((sum(counts), Hi), torch.float32, 36), _su([0] + np.cumsum(counts).tolist())
    kw = dict(Skv=N, topk=70, page_size=PS, fp8_dtype=FP8, is_causal=True, return_q8=True)
    calls = {
        "scores": lambda pool, t: _native.fp8_mla_index_topk(q, w, pool, scale, t, lens, num_pages=pool.shape[0], select=False, **kw),
        "topk": lambda pool, t: _native.fp8_mla_index_topk(q, w, pool, scale, t, lens, num_pages=pool.shape[0], return_logits=True, **kw),
        "topk, 3 splits": lambda pool, t: _native.fp8_mla_index_topk(q, w, pool, scale, t, lens, num_pages=pool.shape[0], select_splits=3, **kw),
        "scores, packed": lambda pool, t: _native.fp8_mla_index_topk_varlen(qp, wp, pool, scale, t, cu, lens, num_pages=pool.shape[0], select=False, **kw),
        "topk, packed": lambda pool, t: _native.fp8_mla_index_topk_varlen(qp, wp, pool, scale, t, cu, lens, num_pages=pool.shape[0], return_logits=True, **kw),
    }
    for what, f in calls.items():
        got, want = f(big, tb), f(small, ts)
        _all_same(got, want, what)
        if "topk" in what:
            assert (got[0][:, -1, :70] >= 0).all() if got[0].dim() == 3 else (got[0][-1] >= 0).all(), what


# ---- 4. logits behind strides of more than 2^29 elements ---------------------------------------------------------------------------------------
def test_logits_rows_more_than_2_gib_apart_give_the_bits_of_dense_logits():
    """[B = 2, Sq = 3] rows of 700 keys, 2^29 + 64 floats apart: every row after the first starts beyond 2^31 bytes, the third beyond 2^32.
    The selection (one workgroup a row, and two), the scores through logits_strides2 and the packed scores through logits_stride."""
    L = _native.lib()
    Bq, Sq, N, S = 2, 3, 700, (1 << 29) + 64
    assert 4 * S > 1 << 31 and 4 * 2 * S > 1 << 32
    span = (Bq * Sq - 1) * S + N
    _need(4 * span + GIB, "the strided logits test")
    buf = torch.empty((span,), dtype=torch.float32, device=DEV)
    far = torch.as_strided(buf, (Bq, Sq, N), (Sq * S, S, 1))
    x = _rand((Bq, Sq, N), torch.float32, 40).mul(4).round().div(4)                        # ties
    far.copy_(x)
    used = _su([N, 650])
    for topk in (70, 800):
        want = _native.mla_index_select(x, used, topk, is_causal=True)
        assert torch.equal(_native.mla_index_select(far, used, topk, is_causal=True), want), topk
        assert torch.equal(_native.mla_index_select_split(far, used, topk, is_causal=True, num_splits=2), want), topk
    # the scores: a small index cache, the rows written through the strides
    Hi, lens = 4, (N, 300)
    pool, table, num_pages, scale = filled_pool("index", PS, lens + (0, 0), torch.bfloat16, "e4m3", 77, owner=0, cap=N)
    pool, table, scale = pool, table[:Bq].contiguous(), scale[:Bq].contiguous()
    Mx = table.shape[1]
    q, w, su = _rand((Bq, Hi, Sq, 128), torch.bfloat16, 41), _rand((Bq, Sq, Hi), torch.float32, 42), _su(lens)
    _, wlog, _, _ = _native.fp8_mla_index_topk(q, w, pool, scale, table, su, Skv=N, topk=8, num_pages=num_pages, page_size=PS, fp8_dtype=FP8,
                                               is_causal=True, select=False)
    far.fill_(7.0)
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.qattn_fp8_mla_index_scores(q.data_ptr(), _native.fmt_of(q.dtype), None, w.data_ptr(), None, pool.data_ptr(), table.data_ptr(), Mx, num_pages,
                                      PS, Mx, scale.data_ptr(), su.data_ptr(), Bq, Hi, Sq, N, _native.fmt_of(FP8), 1, buf.data_ptr(),
                                      _ll(Sq * S, S), 1, None, None, stream)
    torch.cuda.synchronize()
    assert rc == 0 and _same_bits(far.contiguous(), wlog), "scores through logits_strides2"
    # ... and packed: the six rows as one slot of 4 tokens and one of 2
    qp, wp = q.transpose(1, 2).reshape(Bq * Sq, Hi, 128).contiguous(), w.reshape(Bq * Sq, Hi).contiguous()
    cu = _su([0, 4, 6])
    _, plog, _, _, pkend = _native.fp8_mla_index_topk_varlen(qp, wp, pool, scale, table, cu, su, Skv=N, topk=8, num_pages=num_pages, page_size=PS,
                                                             fp8_dtype=FP8, is_causal=True, select=False)
    far.fill_(7.0)
    kend = torch.empty(Bq * Sq, dtype=torch.int32, device=DEV)
    rc = L.qattn_fp8_mla_index_scores_varlen(qp.data_ptr(), _native.fmt_of(qp.dtype), None, wp.data_ptr(), Hi, pool.data_ptr(), table.data_ptr(), Mx,
                                             num_pages, PS, Mx, scale.data_ptr(), cu.data_ptr(), su.data_ptr(), Bq, Hi, Bq * Sq, N, _native.fmt_of(FP8),
                                             1, buf.data_ptr(), S, 1, kend.data_ptr(), None, None, stream)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(kend, pkend) and _same_bits(far.reshape(Bq * Sq, N), plog), "packed scores through logits_stride"


# ---- 5. q and index lists behind strides of more than 2^31 elements ----------------------------------------------------------------------------
def test_q_and_index_lists_more_than_2_31_elements_apart_give_the_bits_of_contiguous_copies():
    """q is a slice of a wider tensor whose batch (packed: token) stride is 2^31 + 64 elements, the lists lie 2^31 + 8 ints apart: the second
    slot's rows start beyond 2^32 bytes of q and beyond 2^33 bytes of the lists.  The sparse decode (1 and 2 splits) and the packed sparse
    entry against contiguous copies of the same rows."""
    Bq, Hq, Sq, topk, SB, SI = 2, 16, 2, 70, (1 << 31) + 64, (1 << 31) + 8
    _need(2 * (SB + Hq * Sq * 576) + 4 * (SI + Sq * topk) + GIB, "the strided q and index test")
    lens = (200, 256)
    pool, table, num_pages, scale = filled_pool("row", PS, lens + (0, 0), torch.bfloat16, "e4m3", 78, owner=1)
    table, scale, su = table[:Bq].contiguous(), scale[:Bq].contiguous(), _su(lens)
    qbuf = torch.empty((SB + Hq * Sq * 576,), dtype=torch.bfloat16, device=DEV)
    ibuf = torch.empty((SI + Sq * topk,), dtype=torch.int32, device=DEV)
    kw = dict(num_pages=num_pages, page_size=PS, fp8_dtype=FP8, is_causal=True, sm_scale=SM_SCALE)
    # the decode: [B, Hq, Sq, 576] and [B, Sq, topk]
    q_far = torch.as_strided(qbuf, (Bq, Hq, Sq, 576), (SB, Sq * 576, 576, 1))
    i_far = torch.as_strided(ibuf, (Bq, Sq, topk), (SI, topk, 1))
    q_far.copy_(_rand((Bq, Hq, Sq, 576), torch.bfloat16, 50, 1.5))
    i_far.copy_(torch.randint(-1, 256, (Bq, Sq, topk), generator=torch.Generator().manual_seed(3), dtype=torch.int32).to(DEV))
    assert not q_far.is_contiguous() and not i_far.is_contiguous() and q_far.stride(0) > 1 << 31 and i_far.stride(0) > 1 << 31
    for ns in (1, 2):
        f = lambda q, i: _native.fp8_mla_paged_sparse_attention(q, pool, scale, table, su, i, num_splits=ns, return_partials=True, return_q8=True, **kw)
        got = f(q_far, i_far)
        _all_same(got, f(q_far.contiguous(), i_far.contiguous()), ("sparse decode", ns))
        assert torch.isfinite(got[0].float()).all() and got[0][1].float().abs().sum() > 0
    # the packed entry: one token a slot, [total_q, Hq, 576] and [total_q, topk]
    q_far = torch.as_strided(qbuf, (Bq, Hq, 576), (SB, 576, 1))
    i_far = torch.as_strided(ibuf, (Bq, topk), (SI, 1))
    q_far.copy_(_rand((Bq, Hq, 576), torch.bfloat16, 51, 1.5))
    cu = _su([0, 1, 2])
    f = lambda q, i: _native.fp8_mla_paged_sparse_varlen_attention(q, pool, scale, table, su, i, cu, return_q8=True, **kw)
    got = f(q_far, i_far)
    _all_same(got, f(q_far.contiguous(), i_far.contiguous()), "sparse packed")
    assert torch.isfinite(got[0].float()).all() and got[0][1].float().abs().sum() > 0


# ---- 6. sparse partials of more than 2^31 floats -----------------------------------------------------------------------------------------------
def test_sparse_partials_of_more_than_2_31_floats_keep_the_rows_of_a_small_batch():
    """B 130, Sq 4, Hq 128, 64 splits over lists of 4096 entries (one 64-entry group a split, so every split stores live rows and the
    live part stays small): partial_o holds 64 x 520 x 128 x 512 > 2^31 floats.
    include/qattn_mla_sparse.h promises no equality across split counts, so the LAST two slots' out, lse and partials -- the highest
    addresses of every split's slab -- are compared with the same call on those two slots alone, the partials caller-provided and in
    the workspace."""
    Bq, Hq, Sq, ns, topk, Mp = 130, 128, 4, 64, 4096, 2
    floats = ns * Bq * Hq * Sq * 512
    assert floats > 1 << 31 > (ns - 1) * Bq * Hq * Sq * 512   # the last split's slab crosses 2^31 floats: its last slots lie beyond
    _need(2 * 4 * floats + 2 * GIB, "the sparse partial buffer test")
    g = torch.Generator().manual_seed(6)
    num_pages = Bq * Mp
    table = torch.randperm(num_pages, generator=g).view(Bq, Mp).to(torch.int32).to(DEV)
    lens = torch.randint(8, Mp * PS + 1, (Bq,), generator=g, dtype=torch.int32).to(DEV)
    scale = (torch.rand(Bq, generator=g) * 0.02 + 0.01).to(DEV)
    pool = torch.full((num_pages, PS, 576), 0x7F, dtype=torch.uint8, device=DEV)
    x = _rand((Bq, Mp * PS, 576), torch.bfloat16, 60, 1.5)
    _native.paged_mla_row_cache_append_fp8(pool, scale, table, torch.zeros_like(lens), x[..., :512], x[..., 512:], num_pages=num_pages, page_size=PS,
                                           fp8_dtype=FP8, new_lens=lens)
    q = _rand((Bq, Hq, Sq, 576), torch.bfloat16, 61, 1.5)
    idx = torch.randint(-1, Mp * PS, (Bq, Sq, topk), generator=g, dtype=torch.int32).to(DEV)
    idx[..., 0], idx[..., -1] = 0, 0                                                        # the first and the last split hold a valid entry: key 0 (L >= 8 > Sq)
    tail = slice(Bq - 2, Bq)
    for parts in (True, False):
        f = lambda s: _native.fp8_mla_paged_sparse_attention(q[s].contiguous(), pool, scale[s].contiguous(), table[s].contiguous(), lens[s].contiguous(),
                                                             idx[s].contiguous(), num_pages=num_pages, page_size=PS, fp8_dtype=FP8, is_causal=True,
                                                             sm_scale=SM_SCALE, num_splits=ns, return_partials=parts)
        out, lse, po, pl, _, _ = f(slice(0, Bq))
        wo, wl, wpo, wpl, _, _ = f(tail)
        assert _same_bits(out[tail], wo) and _same_bits(lse[tail], wl), ("out, lse", parts)
        assert torch.isfinite(wl).all() and wo.float().abs().sum() > 0
        if parts:
            assert po.numel() == floats
            assert _same_bits(po[:, tail], wpo) and _same_bits(pl[:, tail], wpl), "the partials"
            assert torch.isfinite(pl[0, Bq - 1]).all() and torch.isfinite(pl[ns - 1, Bq - 1]).all()   # live rows beyond 2^31 floats
        del out, lse, po, pl

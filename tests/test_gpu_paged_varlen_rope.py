"""The rotary embedding at the paged cache's positions on the MI355X (quantumattention_amd/paged_varlen.py,
include/qattn_paged_varlen_rope.h).

THE RULE: from the same starting state, paged_kv_cache_append_varlen_rope_fp8(cache, k, v, cu, cos, sin) leaves the pools and seqlens
byte for byte as "rotate k in torch (apply_rope_eager) at positions computed on the host from lists, then
paged_kv_cache_append_varlen_fp8" leaves them.  Whole pools are compared, pre-filled with a sentinel byte, so a stray store shows.  The
shapes are the packed append's: Hkv 2, B 8, a capacity of 256 keys per slot, T 256, a shuffled table with spare pages, every start but
one nonzero -- "position = t" cannot pass (tests/test_cpu_paged_varlen_rope.py shows that positions off by one change every row).
apply_rope_paged_varlen is held to apply_rope_eager at host positions, bit for bit.  No test feeds an out-of-range table entry or an
inconsistent cu_seqlens."""
import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, paged
from tests import kvcache_cases as KC
from tests import paged_cases as PC
from tests import paged_varlen_rope_cases as RC

pytestmark = pytest.mark.gpu

DEV = "cuda"
HKV, CAP, T, COUNTS, STARTS, B, SENTINEL = RC.HKV, RC.CAP, RC.T, RC.COUNTS, RC.STARTS, RC.B, RC.SENTINEL
G = 2
HQ = HKV * G
TOTAL = sum(COUNTS)
# D x page size in full; both 16-bit types, both fp8 formats and both pairings spread over the cases
MATRIX = [(64, torch.bfloat16, "e4m3", 64, False), (64, torch.float16, "e5m2", 128, True), (64, torch.bfloat16, "e4m3", 256, True),
          (128, torch.bfloat16, "e4m3", 64, True), (128, torch.float16, "e4m3", 128, False), (128, torch.bfloat16, "e5m2", 256, False),
          (256, torch.float16, "e4m3", 64, False), (256, torch.bfloat16, "e5m2", 128, True), (256, torch.bfloat16, "e4m3", 256, False)]
MATRIX_IDS = [f"d{d}-{str(t)[6:]}-{f}-ps{p}-il{int(i)}" for d, t, f, p, i in MATRIX]


def _su(x):
    return torch.tensor(np.asarray(x), dtype=torch.int32, device=DEV)


def _cache(D, dtype, fmt, page_size, seed=0, starts=STARTS, spare=3, nslots=B):
    M = CAP // page_size
    num_pages = nslots * M + spare
    g = torch.Generator().manual_seed(seed)
    sk = torch.rand(nslots, HKV, generator=g) * 0.02 + 0.01
    sv = torch.rand(nslots, HKV, generator=g) * 0.02 + 0.01
    c = qa.alloc_paged_kv_cache_fp8(num_pages, HKV, page_size, D, batch_size=nslots, max_pages_per_seq=M, scale_k=sk.to(DEV), scale_v=sv.to(DEV),
                                    dtype=dtype, device=DEV, fp8_format=fmt)
    assert c.layout == "frag" and c.capacity == CAP
    c.block_table.copy_(torch.randperm(num_pages, generator=g)[:nslots * M].view(nslots, M).to(torch.int32))
    c.k.fill_(SENTINEL)
    c.v.fill_(SENTINEL)
    c.seqlens.copy_(_su(starts))
    return c


def _clone(c):
    return paged.PagedKVCacheFP8(c.k.clone(), c.v.clone(), c.scale_k, c.scale_v, c.block_table.clone(), c.seqlens.clone(), c.shape, c.fp8_format,
                                 c.dtype, c.numerics, c.layout)


def _tokens(total, D, dtype, seed, mul=2.0):
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.randn(total, HKV, D, generator=g) * mul).to(dtype).to(DEV) for _ in range(2))


def _same_state(a, b):
    return torch.equal(a.k, b.k) and torch.equal(a.v, b.v) and torch.equal(a.seqlens, b.seqlens)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _pool_rows(c):
    """row-major uint8 numpy [P, Hkv, page_size, D] of both pools"""
    P_, _, ps, D = c.shape
    return tuple(KC.from_image(img, layout, P_, HKV, ps, D).cpu().numpy() for img, layout in ((c.k, KC.KFRAG), (c.v, KC.VFRAG)))


# ---- 1. THE RULE --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype,fmt,page_size,il", MATRIX, ids=MATRIX_IDS)
def test_the_rope_append_leaves_pools_and_seqlens_as_rotating_in_torch_then_the_plain_append_leaves_them(D, dtype, fmt, page_size, il):
    c0 = _cache(D, dtype, fmt, page_size, seed=D + page_size)
    k, v = _tokens(TOTAL, D, dtype, 3 * D + page_size)
    k[5, 0, 3], k[70, 1, 0], k[200, 0, 1] = float("inf"), float("nan"), -float("inf")      # inf x 0 = NaN in the rotation, as in the composition
    if dtype == torch.float16:
        k[150, 1, :4] = 60000.0                                                           # an fp16 product that overflows in the rotation
    cu = _su(RC.cu_list(COUNTS))
    cos, sin = RC.tables(D, device=DEV)
    mine = None
    for advance in (True, False):
        a, b, p = _clone(c0), _clone(c0), _clone(c0)
        assert qa.paged_kv_cache_append_varlen_rope_fp8(a, k, v, cu, cos, sin, interleaved=il, advance=advance) is a
        RC.rule(b, k, v, cu, COUNTS, STARTS, cos, sin, il, advance)
        assert torch.equal(a.k, b.k), "K pool"
        assert torch.equal(a.v, b.v), "V pool"
        assert torch.equal(a.seqlens, b.seqlens)
        want = [min(s + n, CAP) for s, n in zip(STARTS, COUNTS)] if advance else STARTS
        assert a.seqlens.tolist() == want
        # V is not rotated: its pool holds the plain append's bytes; K's does not
        qa.paged_kv_cache_append_varlen_fp8(p, k, v, cu, advance=advance)
        assert torch.equal(a.v, p.v) and not torch.equal(a.k, p.k) and not torch.equal(a.k, c0.k)
        mine = a
    # every byte outside the appended keys is still the sentinel
    table = c0.block_table.cpu().numpy()
    for pool in _pool_rows(mine):
        own = np.zeros(pool.shape[:3], bool)
        for i in range(B):
            keys = np.arange(STARTS[i], min(STARTS[i] + COUNTS[i], CAP))
            own[table[i][keys // page_size], :, keys % page_size] = True
        assert (pool[~own] == SENTINEL).all(), "a byte of a key the call does not append changed"
    assert STARTS[5] + COUNTS[5] > CAP       # (the dropped tail is in the matrix)


# ---- 2. strided input, sliced and 16-bit tables -----------------------------------------------------------------------------------------------
def test_strided_projection_slices_and_a_slice_of_a_wider_table_give_the_bits_of_their_contiguous_copies():
    D, dtype = 128, torch.bfloat16
    c0 = _cache(D, dtype, "e4m3", 128, seed=11)
    g = torch.Generator().manual_seed(12)
    qkv = (torch.randn(TOTAL, HQ + 2 * HKV, D, generator=g) * 2).to(dtype).to(DEV)
    ks, vs = qkv[:, HQ:HQ + HKV], qkv[:, HQ + HKV:]
    assert not ks.is_contiguous() and ks.stride(0) == (HQ + 2 * HKV) * D
    cu = _su(RC.cu_list(COUNTS))
    cos, sin = RC.tables(D, device=DEV)
    both = torch.cat([cos, sin], 1)                                  # [T, D]: cos | sin, rows of D floats
    a, b, c = _clone(c0), _clone(c0), _clone(c0)
    qa.paged_kv_cache_append_varlen_rope_fp8(a, ks, vs, cu, both[:, :D // 2], both[:, D // 2:])
    qa.paged_kv_cache_append_varlen_rope_fp8(b, ks.contiguous(), vs.contiguous(), cu, cos, sin)
    assert _same_state(a, b) and not torch.equal(a.k, c0.k)
    RC.rule(c, ks, vs, cu, COUNTS, STARTS, cos, sin, False, True)
    assert _same_state(a, c)
    # 16-bit tables are up-cast
    a, b = _clone(c0), _clone(c0)
    qa.paged_kv_cache_append_varlen_rope_fp8(a, ks, vs, cu, cos.bfloat16(), sin.bfloat16(), interleaved=True)
    qa.paged_kv_cache_append_varlen_rope_fp8(b, ks, vs, cu, cos.bfloat16().float(), sin.bfloat16().float(), interleaved=True)
    assert _same_state(a, b)


# ---- 3. neighbours ------------------------------------------------------------------------------------------------------------------------
def test_nan_in_other_slots_tokens_behind_cu_b_and_in_unused_table_rows_changes_no_byte():
    D, dtype, fmt, ps = 128, torch.bfloat16, "e4m3", 64
    c0 = _cache(D, dtype, fmt, ps, seed=21)
    bucket = TOTAL + 9                                              # a padded token bucket: cu[B] < total rows
    k, v = _tokens(bucket, D, dtype, 22)
    k[TOTAL:], v[TOTAL:] = float("nan"), float("nan")
    cu = RC.cu_list(COUNTS)
    cos, sin = RC.tables(D, device=DEV)
    exact = _clone(c0)
    qa.paged_kv_cache_append_varlen_rope_fp8(exact, k[:TOTAL], v[:TOTAL], _su(cu), cos, sin)
    # table rows no appended key uses hold NaN; so do the rows of the bucket nobody owns
    used = np.zeros(T, bool)
    for s, n in zip(STARTS, COUNTS):
        used[s:min(s + n, CAP)] = True
    assert (~used).sum() > 40 and not used[0]
    cn, sn = cos.clone(), sin.clone()
    cn[torch.from_numpy(~used).to(DEV)] = float("nan")
    sn[torch.from_numpy(~used).to(DEV)] = float("nan")
    clean = _clone(c0)
    qa.paged_kv_cache_append_varlen_rope_fp8(clean, k, v, _su(cu), cn, sn)
    assert _same_state(clean, exact)
    nan = PC.NAN_BYTE[fmt]
    rows = _pool_rows(clean)
    assert not ((rows[0] & 0x7F) == nan).any() and not ((rows[1] & 0x7F) == nan).any()
    table = c0.block_table.cpu().numpy()
    for i in (2, 4, 5):                                             # 63 tokens at 63, 65 at 100, 130 at 127: partial chunks at both ends
        kn, vn = k.clone(), v.clone()
        kn[:cu[i]], vn[:cu[i]] = float("nan"), float("nan")        # every other sequence's tokens, the rows just before start_i ...
        kn[cu[i + 1]:], vn[cu[i + 1]:] = float("nan"), float("nan")  # ... and just after end_i
        dirty = _clone(c0)
        qa.paged_kv_cache_append_varlen_rope_fp8(dirty, kn, vn, _su(cu), cn, sn)
        for pool_c, pool_d in zip(_pool_rows(clean), _pool_rows(dirty)):
            pages = table[i]
            assert np.array_equal(pool_c[pages], pool_d[pages]), i
        assert torch.equal(dirty.seqlens, clean.seqlens)


# ---- 4. the C entry's clamp -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("il", [False, True])
def test_through_the_binding_a_table_shorter_than_the_capacity_is_read_at_positions_clamped_to_its_last_row(il):
    D, dtype, fmt, ps = 128, torch.float16, "e4m3", 128
    c0 = _cache(D, dtype, fmt, ps, seed=61)
    k, v = _tokens(TOTAL, D, dtype, 62)
    cu = _su(RC.cu_list(COUNTS))
    cos, sin = RC.tables(D, device=DEV)
    short_c, short_s = cos[:100].clone(), sin[:100].clone()          # exactly 100 rows exist
    a, b = _clone(c0), _clone(c0)
    _native.paged_kv_cache_append_varlen_rope_fp8(a.k, a.v, a.scale_k, a.scale_v, a.block_table, a.seqlens, k, v, cu, short_c, short_s,
                                                  num_pages=a.num_pages, page_size=ps, fp8_dtype=_native.fp8_dtype_of(fmt), interleaved=il)
    pos = RC.positions(COUNTS, STARTS, TOTAL, rows=100)
    assert max(pos) == 99 and pos.count(99) > 100
    qa.paged_kv_cache_append_varlen_fp8(b, RC.rotate_at(k, pos, cos, sin, il), v, cu)
    assert _same_state(a, b)


# ---- 5. apply_rope_paged_varlen -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype,il", [(64, torch.float16, True), (128, torch.bfloat16, False), (256, torch.bfloat16, True)])
def test_apply_rope_paged_varlen_is_apply_rope_eager_at_host_positions_before_and_after_the_append(D, dtype, il):
    c = _cache(D, dtype, "e4m3", 64, seed=71 + D)
    bucket = TOTAL + 5
    qkv = (torch.randn(bucket, HQ + 2 * HKV, D, generator=torch.Generator().manual_seed(72)) * 2).to(dtype).to(DEV)
    qkv[TOTAL:] = float("nan")
    q = qkv[:, :HQ]
    assert not q.is_contiguous()
    cu = _su(RC.cu_list(COUNTS))
    cos, sin = RC.tables(D, device=DEV)
    want = RC.rotate_at(q[:TOTAL], RC.positions(COUNTS, STARTS, TOTAL), cos, sin, il)
    got = qa.apply_rope_paged_varlen(q, c, cu, cos, sin, interleaved=il)
    assert got.is_contiguous() and tuple(got.shape) == (bucket, HQ, D) and _same_bits(got[:TOTAL], want)
    assert _same_bits(qa.apply_rope_paged_varlen(q.contiguous(), c, cu, cos, sin, interleaved=il)[:TOTAL], want)
    # out=: rows behind cu[B] are neither read nor written
    out = torch.full((bucket, HQ, D), 7.0, dtype=dtype, device=DEV)
    assert qa.apply_rope_paged_varlen(q, c, cu, cos, sin, interleaved=il, out=out) is out
    assert _same_bits(out[:TOTAL], want) and (out[TOTAL:] == 7.0).all()
    # after an advancing append: appended=True, the positions p - n from the seqlens the append left
    qa.paged_kv_cache_append_varlen_rope_fp8(c, qkv[:, HQ:HQ + HKV], qkv[:, HQ + HKV:], cu, cos, sin, interleaved=il)
    after = c.seqlens.tolist()
    got2 = qa.apply_rope_paged_varlen(q, c, cu, cos, sin, interleaved=il, appended=True)
    want2 = RC.rotate_at(q[:TOTAL], RC.positions(COUNTS, after, TOTAL, appended=True), cos, sin, il)
    assert _same_bits(got2[:TOTAL], want2)
    cul = RC.cu_list(COUNTS)
    live = [i for i in range(TOTAL) if not cul[5] <= i < cul[6]]     # every slot but the one that dropped its tail: the rows of the call before
    assert _same_bits(got2[live], want[live]) and not _same_bits(got2[:TOTAL], want)


# ---- 6. a schedule ------------------------------------------------------------------------------------------------------------------------
NS = 4      # slots of the schedule


def _fused(c, qkv, cu, cos, sin, il):
    q = qa.apply_rope_paged_varlen(qkv[:, :HQ], c, cu, cos, sin, interleaved=il)
    qa.paged_kv_cache_append_varlen_rope_fp8(c, qkv[:, HQ:HQ + HKV], qkv[:, HQ + HKV:], cu, cos, sin, interleaved=il)
    return qa.fp8_attn_paged_varlen_func(q, c, cu, 130, causal=True, num_splits=2, return_lse=True)


def _unfused(c, qkv, cu, counts, cos, sin, il):
    total = sum(counts)
    pos = RC.positions(counts, c.seqlens.tolist(), qkv.shape[0])
    q = RC.rotate_at(qkv[:, :HQ], pos, cos, sin, il)
    k = RC.rotate_at(qkv[:, HQ:HQ + HKV], pos, cos, sin, il)
    qa.paged_kv_cache_append_varlen_fp8(c, k, qkv[:, HQ + HKV:], cu)
    out, lse = qa.fp8_attn_paged_varlen_func(q, c, cu, 130, causal=True, num_splits=2, return_lse=True)
    return out[:total], lse[:, :total]


def test_a_six_step_schedule_through_the_fused_path_equals_the_unfused_composition_after_every_step():
    D, dtype, fmt, ps, il = 128, torch.bfloat16, "e4m3", 64, False
    M = CAP // ps
    a = _cache(D, dtype, fmt, ps, seed=81, starts=[0] * NS, spare=M + 1, nslots=NS)
    b = _clone(a)
    cos, sin = RC.tables(D, device=DEV)
    g = torch.Generator().manual_seed(82)
    spare = sorted(set(range(a.num_pages)) - set(a.block_table.flatten().tolist()))

    def rollback(c):                     # the last step's tokens are rejected: the next step re-appends at the rolled-back positions
        c.seqlens.sub_(_su([1, 1, 1, 1]))

    def hand_over(c):                    # slot 1 has finished: its pages go to slot 2, which starts a new sequence; slot 1 gets spare pages
        c.block_table[2] = c.block_table[1].clone()
        c.block_table[1] = _su(spare[:M])
        c.seqlens[1], c.seqlens[2] = 0, 0

    steps = [([130, 3, 0, 1], None),         # a prefill chunk, a short one, an idle slot, a decode
             ([64, 1, 0, 1], None),          # a chunk and decodes
             ([1, 1, 1, 1], None),           # decodes only
             ([1, 1, 1, 1], rollback),
             ([1, 0, 40, 1], hand_over),
             ([2, 5, 1, 0], None)]
    expect = [0] * NS
    for r, (counts, before) in enumerate(steps):
        if before is not None:
            before(a), before(b)
            expect = a.seqlens.tolist()
        total = sum(counts)
        qkv = (torch.randn(total, HQ + 2 * HKV, D, generator=g) * 1.5).to(dtype).to(DEV)
        cu = _su(RC.cu_list(counts))
        out_a, lse_a = _fused(a, qkv, cu, cos, sin, il)
        out_b, lse_b = _unfused(b, qkv, cu, counts, cos, sin, il)
        assert _same_state(a, b), r
        assert _same_bits(out_a, out_b) and _same_bits(lse_a, lse_b), r
        assert not torch.isnan(out_a.float()).any()
        expect = [p + n for p, n in zip(expect, counts)]
        assert a.seqlens.tolist() == expect, r
    assert expect == [198, 5, 41, 4]


# ---- 7. graph -----------------------------------------------------------------------------------------------------------------------------
def test_one_captured_rotate_append_attend_graph_follows_rewritten_cu_seqlens_seqlens_table_tokens_and_tables():
    D, dtype, fmt, ps, il = 128, torch.bfloat16, "e4m3", 128, True
    c = _cache(D, dtype, fmt, ps, seed=31, starts=[0] * B)
    bucket = 160
    qkv = torch.zeros((bucket, HQ + 2 * HKV, D), dtype=dtype, device=DEV)
    cu = _su([0] * (B + 1))
    cos, sin = RC.tables(D, device=DEV)
    warm = _clone(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _fused(warm, qkv, cu, cos, sin, il)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s, lse_s = _fused(c, qkv, cu, cos, sin, il)
    assert c.seqlens.tolist() == [0] * B, "capture ran nothing"
    g = torch.Generator().manual_seed(32)
    M = CAP // ps
    replays = [   # counts, seqlens written before the replay (None: what the last replay left), the tables' base
        ([64, 1, 0, 7, 1, 63, 2, 1], None, 10000.0),
        ([1, 1, 1, 1, 0, 65, 1, 1], None, 10000.0),
        ([3, 0, 1, 1, 1, 1, 70, 1], [10, 2, 0, 3, 1, 100, 1, 0], 500000.0),            # a rollback, a new table, other cos / sin contents
    ]
    expect = [0] * B
    for r, (counts, lens, base) in enumerate(replays):
        total = sum(counts)
        qkv.copy_((torch.randn(bucket, HQ + 2 * HKV, D, generator=g) * 1.5).to(dtype))
        qkv[total:] = float("nan")                                  # rows of the bucket nobody owns
        cu.copy_(_su(RC.cu_list(counts)))
        nc, ns_ = RC.tables(D, device=DEV, base=base)
        cos.copy_(nc), sin.copy_(ns_)
        if lens is not None:
            c.seqlens.copy_(_su(lens))
            c.block_table.copy_(torch.randperm(c.num_pages, generator=g)[:B * M].view(B, M).to(torch.int32))
        eager, ref = _clone(c), _clone(c)
        graph.replay()
        torch.cuda.synchronize()
        out_e, lse_e = _fused(eager, qkv, cu, cos, sin, il)
        assert _same_state(c, eager), r
        assert _same_bits(out_s[:total], out_e[:total]) and _same_bits(lse_s[:, :total], lse_e[:, :total]), r
        out_u, lse_u = _unfused(ref, qkv, cu, counts, cos, sin, il)
        assert _same_state(c, ref) and _same_bits(out_s[:total], out_u) and _same_bits(lse_s[:, :total], lse_u), r
        assert not torch.isnan(out_s[:total].float()).any()
        expect = [p + n for p, n in zip(expect if lens is None else lens, counts)]
        assert c.seqlens.tolist() == expect, r


# ---- 8. the ops ---------------------------------------------------------------------------------------------------------------------------
def test_the_ops_give_the_functions_bytes_and_rotate_append_attend_compiles_fullgraph():
    D, dtype, fmt, ps = 64, torch.bfloat16, "e4m3", 64
    c0 = _cache(D, dtype, fmt, ps, seed=51)
    qkv = (torch.randn(TOTAL, HQ + 2 * HKV, D, generator=torch.Generator().manual_seed(52)) * 1.5).to(dtype).to(DEV)
    qs, ks, vs = qkv[:, :HQ], qkv[:, HQ:HQ + HKV], qkv[:, HQ + HKV:]
    cu = _su(RC.cu_list(COUNTS))
    cos, sin = RC.tables(D, device=DEV)
    a, b = _clone(c0), _clone(c0)
    qa.paged_kv_cache_append_varlen_rope_fp8(a, ks, vs, cu, cos, sin, interleaved=True)
    assert qa.ops.fp8_paged_varlen_rope_kv_cache_append_(b.k, b.v, b.scale_k, b.scale_v, b.block_table, b.seqlens, ks, vs, cu, cos, sin, b.num_pages,
                                                         b.page_size, b.fp8_format, True, True) is None
    assert _same_state(a, b)
    assert _same_bits(qa.ops.rope_paged_varlen(qs, c0.seqlens, cu, cos, sin, CAP, True, False),
                      qa.apply_rope_paged_varlen(qs, c0, cu, cos, sin, interleaved=True))

    def step(cache):
        def f(qkv_, cu_, cos_, sin_):
            q = qa.apply_rope_paged_varlen(qkv_[:, :HQ], cache, cu_, cos_, sin_, interleaved=True)
            qa.paged_kv_cache_append_varlen_rope_fp8(cache, qkv_[:, HQ:HQ + HKV], qkv_[:, HQ + HKV:], cu_, cos_, sin_, interleaved=True)
            return qa.fp8_attn_paged_varlen_func(q, cache, cu_, 130, causal=True, num_splits=2, return_lse=True)
        return f

    e, t = _clone(c0), _clone(c0)
    torch._dynamo.reset()
    got = torch.compile(step(t), fullgraph=True)(qkv, cu, cos, sin)
    want = step(e)(qkv, cu, cos, sin)
    assert _same_state(e, t) and _same_state(e, a) and _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    assert not torch.isnan(got[0].float()).any()

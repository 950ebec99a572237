"""The packed variable-length append to the paged FP8 K/V cache on the MI355X (quantumattention_amd/paged_varlen.py,
include/qattn_paged_varlen_append.h).

The rule: from the same starting state, paged_kv_cache_append_varlen_fp8(cache, k [total, Hkv, D], v, cu_seqlens) leaves the pools and
seqlens byte for byte as paged_kv_cache_append_fp8(cache, pad(k), pad(v), new_lens=n) leaves them.  Whole pools are compared, pre-filled
with a sentinel byte, so a stray store shows; one test per D is independent of the padded entry (the shadow quantiser of
tests/serving_trace.py, every key looked up through the table).  Hkv 2, B 8, a capacity of 256 keys per slot, a shuffled table with spare
pages.  No test feeds an out-of-range table entry or an inconsistent cu_seqlens."""
import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import paged
from tests import kvcache_cases as KC
from tests import paged_cases as PC

pytestmark = pytest.mark.gpu

DEV = "cuda"
HKV, G = 2, 2
HQ = HKV * G
CAP = 256
COUNTS = [0, 1, 63, 64, 65, 130, 2, 7]
STARTS = [0, 1, 63, 64, 100, 127, CAP - 3, 5]     # an empty slot, a chunk-aligned start, straddled chunks and pages, a dropped tail (slot 5)
B = len(COUNTS)
SENTINEL = 0x5A
# one full sweep of each axis, as the sibling tests: D, 16-bit type, fp8 format, page size
MATRIX = [(64, torch.bfloat16, "e4m3", 64), (128, torch.bfloat16, "e4m3", 64), (256, torch.bfloat16, "e4m3", 64),
          (128, torch.float16, "e4m3", 128), (128, torch.bfloat16, "e5m2", 128), (128, torch.bfloat16, "e4m3", 256),
          (64, torch.float16, "e5m2", 256)]
MATRIX_IDS = [f"d{d}-{str(t)[6:]}-{f}-ps{p}" for d, t, f, p in MATRIX]
PER_D = [(64, torch.float16, "e5m2", 128), (128, torch.bfloat16, "e4m3", 64), (256, torch.bfloat16, "e4m3", 256)]
PER_D_IDS = [f"d{d}-{str(t)[6:]}-{f}-ps{p}" for d, t, f, p in PER_D]


def _su(x):
    return torch.tensor(np.asarray(x), dtype=torch.int32, device=DEV)


def _cu(counts):
    return [0] + np.cumsum(counts).tolist()


def _cache(D, dtype, fmt, page_size, seed=0, starts=STARTS, spare=3):
    M = CAP // page_size
    num_pages = B * M + spare
    g = torch.Generator().manual_seed(seed)
    sk = torch.rand(B, HKV, generator=g) * 0.02 + 0.01
    sv = torch.rand(B, HKV, generator=g) * 0.02 + 0.01
    c = qa.alloc_paged_kv_cache_fp8(num_pages, HKV, page_size, D, batch_size=B, max_pages_per_seq=M, scale_k=sk.to(DEV), scale_v=sv.to(DEV),
                                    dtype=dtype, device=DEV, fp8_format=fmt)
    assert c.layout == "frag" and c.capacity == CAP
    c.block_table.copy_(torch.randperm(num_pages, generator=g)[:B * M].view(B, M).to(torch.int32))
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


def _pad(x, counts, fill=float("nan")):
    """[B, Hkv, T, D]: slot b's tokens, then rows (NaN) that new_lens keeps out of the cache"""
    T = max(max(counts), 1)
    out = torch.full((len(counts), x.shape[1], T, x.shape[2]), fill, dtype=x.dtype, device=x.device)
    cu = _cu(counts)
    for b, n in enumerate(counts):
        out[b, :, :n] = x[cu[b]:cu[b + 1]].transpose(0, 1)
    return out


def _same_state(a, b):
    return torch.equal(a.k, b.k) and torch.equal(a.v, b.v) and torch.equal(a.seqlens, b.seqlens)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _pool_rows(c):
    """row-major uint8 numpy [P, Hkv, page_size, D] of both pools"""
    P_, _, ps, D = c.shape
    return tuple(KC.from_image(img, layout, P_, HKV, ps, D).cpu().numpy() for img, layout in ((c.k, KC.KFRAG), (c.v, KC.VFRAG)))


def _padded_append(c, k, v, counts, advance=True):
    qa.paged_kv_cache_append_fp8(c, _pad(k, counts), _pad(v, counts), new_lens=_su(counts), advance=advance)


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype,fmt,page_size", MATRIX, ids=MATRIX_IDS)
def test_the_packed_append_leaves_pools_and_seqlens_as_the_padded_append_leaves_them(D, dtype, fmt, page_size):
    c0 = _cache(D, dtype, fmt, page_size, seed=D + page_size)
    total = sum(COUNTS)
    k, v = _tokens(total, D, dtype, 3 * D + page_size)
    k[5, 0, 3], k[70, 1, 0], k[200, 0, 1] = float("inf"), float("nan"), -float("inf")      # saturation, NaN: the quantiser's own handling
    cu = _su(_cu(COUNTS))
    for advance in (True, False):
        a, b = _clone(c0), _clone(c0)
        assert qa.paged_kv_cache_append_varlen_fp8(a, k, v, cu, advance=advance) is a
        _padded_append(b, k, v, COUNTS, advance)
        assert torch.equal(a.k, b.k), "K pool"
        assert torch.equal(a.v, b.v), "V pool"
        assert torch.equal(a.seqlens, b.seqlens)
        want = [min(p + n, CAP) for p, n in zip(STARTS, COUNTS)] if advance else STARTS
        assert a.seqlens.tolist() == want
        assert not torch.equal(a.k, c0.k) and not torch.equal(a.v, c0.v)
    assert STARTS[5] + COUNTS[5] > CAP       # (the dropped tail is in the matrix)


# ---- 2. independent of the padded entry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype,fmt,page_size", PER_D, ids=PER_D_IDS)
def test_every_appended_key_holds_the_shadow_quantisers_bytes_and_every_other_byte_its_sentinel(D, dtype, fmt, page_size):
    c = _cache(D, dtype, fmt, page_size, seed=7 + D)
    total = sum(COUNTS)
    k, v = _tokens(total, D, dtype, 5 * D, mul=3.0)               # 3 sigma over scales of 0.01 .. 0.03: some values saturate
    qa.paged_kv_cache_append_varlen_fp8(c, k, v, _su(_cu(COUNTS)))
    fp8 = KC.FP8[fmt]
    table = c.block_table.cpu().numpy()
    cu = _cu(COUNTS)
    rows = _pool_rows(c)
    for (pool, x, scale) in ((rows[0], k, c.scale_k), (rows[1], v, c.scale_v)):
        got = PC.gather_rows(pool, table, page_size)               # [B, Hkv, CAP, D], key by key through the table
        mine = np.zeros(pool.shape[:3], bool)                        # [P, Hkv, page_size]
        for b in range(B):
            n = min(COUNTS[b], CAP - STARTS[b])
            if n == 0:
                continue
            want = KC.quant_ref(x[cu[b]:cu[b] + n].transpose(0, 1)[None].cpu(), scale[b:b + 1].cpu(), fp8)[0].numpy()      # [Hkv, n, D]
            assert np.array_equal(got[b][:, STARTS[b]:STARTS[b] + n], want), b
            keys = np.arange(STARTS[b], STARTS[b] + n)
            mine[table[b][keys // page_size], :, keys % page_size] = True
        assert (pool[~mine] == SENTINEL).all(), "a byte of a key the call does not append changed"


# ---- 3. strided input ---------------------------------------------------------------------------------------------------------------------
def test_the_k_and_v_slices_of_a_packed_projection_give_the_bits_of_their_contiguous_copies():
    D, dtype = 128, torch.bfloat16
    c0 = _cache(D, dtype, "e4m3", 128, seed=11)
    total = sum(COUNTS)
    g = torch.Generator().manual_seed(12)
    qkv = (torch.randn(total, HQ + 2 * HKV, D, generator=g) * 2).to(dtype).to(DEV)
    ks, vs = qkv[:, HQ:HQ + HKV], qkv[:, HQ + HKV:]
    assert not ks.is_contiguous() and ks.stride(0) == (HQ + 2 * HKV) * D
    cu = _su(_cu(COUNTS))
    a, b = _clone(c0), _clone(c0)
    qa.paged_kv_cache_append_varlen_fp8(a, ks, vs, cu)
    qa.paged_kv_cache_append_varlen_fp8(b, ks.contiguous(), vs.contiguous(), cu)
    assert _same_state(a, b) and not torch.equal(a.k, c0.k)


# ---- 4. neighbours ------------------------------------------------------------------------------------------------------------------------
def test_nan_in_other_sequences_tokens_and_in_the_rows_behind_cu_b_changes_no_byte_of_a_slots_pages():
    D, dtype, fmt, ps = 128, torch.bfloat16, "e4m3", 64
    c0 = _cache(D, dtype, fmt, ps, seed=21)
    total = sum(COUNTS)
    bucket = total + 9                                              # a padded token bucket: cu[B] < total rows
    k, v = _tokens(bucket, D, dtype, 22)
    k[total:], v[total:] = float("nan"), float("nan")
    cu = _cu(COUNTS)
    clean = _clone(c0)
    qa.paged_kv_cache_append_varlen_fp8(clean, k, v, _su(cu))
    # the trailing rows were not read: no NaN byte anywhere in the pools
    nan = PC.NAN_BYTE[fmt]
    rows = _pool_rows(clean)
    assert not ((rows[0] & 0x7F) == nan).any() and not ((rows[1] & 0x7F) == nan).any()
    exact = _clone(c0)
    qa.paged_kv_cache_append_varlen_fp8(exact, k[:total], v[:total], _su(cu))
    assert _same_state(clean, exact)
    table = c0.block_table.cpu().numpy()
    for i in (2, 4, 5):                                             # 63 tokens at 63, 65 at 100, 130 at 127: partial chunks at both ends
        kn, vn = k.clone(), v.clone()
        kn[:cu[i]], vn[:cu[i]] = float("nan"), float("nan")        # every other sequence's tokens, the rows just before start_i ...
        kn[cu[i + 1]:], vn[cu[i + 1]:] = float("nan"), float("nan")  # ... and just after end_i
        dirty = _clone(c0)
        qa.paged_kv_cache_append_varlen_fp8(dirty, kn, vn, _su(cu))
        for pool_c, pool_d in zip(_pool_rows(clean), _pool_rows(dirty)):
            pages = table[i]
            assert np.array_equal(pool_c[pages], pool_d[pages]), i
        assert torch.equal(dirty.seqlens, clean.seqlens)


# ---- 5. graph -----------------------------------------------------------------------------------------------------------------------------
def _step(c, qkv, cu, mx):
    qa.paged_kv_cache_append_varlen_fp8(c, qkv[:, HQ:HQ + HKV], qkv[:, HQ + HKV:], cu)
    return qa.fp8_attn_paged_varlen_func(qkv[:, :HQ], c, cu, mx, causal=True, num_splits=2, return_lse=True)


def test_one_captured_append_then_attend_graph_follows_rewritten_cu_seqlens_seqlens_table_and_tokens():
    D, dtype, fmt, ps = 128, torch.bfloat16, "e4m3", 128
    c = _cache(D, dtype, fmt, ps, seed=31, starts=[0] * B)
    bucket = 160
    qkv = torch.zeros((bucket, HQ + 2 * HKV, D), dtype=dtype, device=DEV)
    cu = _su([0] * (B + 1))
    warm = _clone(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(warm, qkv, cu, 64)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s, lse_s = _step(c, qkv, cu, 64)
    assert c.seqlens.tolist() == [0] * B, "capture ran nothing"
    g = torch.Generator().manual_seed(32)
    M = CAP // ps
    replays = [   # counts, seqlens written before the replay (None: what the last replay left)
        ([64, 1, 0, 7, 1, 63, 2, 1], None),
        ([1, 1, 1, 1, 0, 65, 1, 1], None),
        ([3, 0, 1, 1, 1, 1, 70, 1], [10, 2, 0, 3, 1, 100, 1, 0]),            # a rollback, and a new table
    ]
    expect = [0] * B
    for r, (counts, lens) in enumerate(replays):
        total = sum(counts)
        qkv.copy_((torch.randn(bucket, HQ + 2 * HKV, D, generator=g) * 1.5).to(dtype))
        qkv[total:, HQ:] = float("nan")                             # rows of the bucket nobody owns
        cu.copy_(_su(_cu(counts)))
        if lens is not None:
            c.seqlens.copy_(_su(lens))
            c.block_table.copy_(torch.randperm(c.num_pages, generator=g)[:B * M].view(B, M).to(torch.int32))
        eager = _clone(c)
        graph.replay()
        torch.cuda.synchronize()
        out_e, lse_e = _step(eager, qkv, cu, 64)
        assert _same_state(c, eager), r
        assert _same_bits(out_s[:total], out_e[:total]) and _same_bits(lse_s[:, :total], lse_e[:, :total]), r
        assert not torch.isnan(out_s[:total].float()).any()
        expect = [p + n for p, n in zip(expect if lens is None else lens, counts)]
        assert c.seqlens.tolist() == expect, r


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------
def test_a_mixed_step_through_the_packed_append_equals_the_padded_append_then_the_same_attention():
    D, dtype, fmt, ps = 128, torch.bfloat16, "e4m3", 64
    counts = [130, 1, 1, 0, 1, 1, 1, 1]                             # one chunk of 130, decodes, one idle slot
    starts = [70, 200, 63, 40, 64, 127, 128, 0]
    c0 = _cache(D, dtype, fmt, ps, seed=41, starts=[0] * B)
    # a history for every slot, so that the attention has keys to read
    hist = _tokens(sum(starts), D, dtype, 42)
    qa.paged_kv_cache_append_varlen_fp8(c0, hist[0], hist[1], _su(_cu(starts)))
    assert c0.seqlens.tolist() == starts
    total = sum(counts)
    qkv = (torch.randn(total, HQ + 2 * HKV, D, generator=torch.Generator().manual_seed(43)) * 1.5).to(dtype).to(DEV)
    cu = _su(_cu(counts))
    a, b = _clone(c0), _clone(c0)
    qa.paged_kv_cache_append_varlen_fp8(a, qkv[:, HQ:HQ + HKV], qkv[:, HQ + HKV:], cu)
    _padded_append(b, qkv[:, HQ:HQ + HKV], qkv[:, HQ + HKV:], counts)
    assert _same_state(a, b)
    kw = dict(causal=True, num_splits=3, max_seqlen_k=CAP, return_lse=True)
    oa, la = qa.fp8_attn_paged_varlen_func(qkv[:, :HQ], a, cu, 130, **kw)
    ob, lb = qa.fp8_attn_paged_varlen_func(qkv[:, :HQ], b, cu, 130, **kw)
    assert _same_bits(oa, ob) and _same_bits(la, lb) and not torch.isnan(oa.float()).any()


# ---- 7. the op ----------------------------------------------------------------------------------------------------------------------------
def test_the_op_gives_the_functions_bytes_and_append_then_attend_compiles_fullgraph():
    D, dtype, fmt, ps = 64, torch.bfloat16, "e4m3", 64
    c0 = _cache(D, dtype, fmt, ps, seed=51)
    total = sum(COUNTS)
    qkv = (torch.randn(total, HQ + 2 * HKV, D, generator=torch.Generator().manual_seed(52)) * 1.5).to(dtype).to(DEV)
    ks, vs = qkv[:, HQ:HQ + HKV], qkv[:, HQ + HKV:]
    cu = _su(_cu(COUNTS))
    a, b = _clone(c0), _clone(c0)
    qa.paged_kv_cache_append_varlen_fp8(a, ks, vs, cu)
    assert qa.ops.fp8_paged_varlen_kv_cache_append_(b.k, b.v, b.scale_k, b.scale_v, b.block_table, b.seqlens, ks, vs, cu, b.num_pages, b.page_size,
                                                    b.fp8_format, True) is None
    assert _same_state(a, b)

    def step(cache):
        def f(qkv_, cu_):
            qa.paged_kv_cache_append_varlen_fp8(cache, qkv_[:, HQ:HQ + HKV], qkv_[:, HQ + HKV:], cu_)
            return qa.fp8_attn_paged_varlen_func(qkv_[:, :HQ] * 2, cache, cu_, 130, causal=True, num_splits=2, return_lse=True)
        return f

    e, t = _clone(c0), _clone(c0)
    torch._dynamo.reset()
    got = torch.compile(step(t), fullgraph=True)(qkv, cu)
    want = step(e)(qkv, cu)
    assert _same_state(e, t) and _same_state(e, a) and _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    assert not torch.isnan(got[0].float()).any()

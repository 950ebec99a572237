"""The packed variable-length append to the paged FP8 K/V cache without a GPU (quantumattention_amd/paged_varlen.py,
include/qattn_paged_varlen_append.h): the surface, the reason function, the eager definition against paged._append_eager on the padded
tokens (whole pools and seqlens, byte for byte), the C entry's argument checks, the slot map of the kernel's grid, the op's schema and
fake registration."""
import ctypes
import inspect

import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, paged, paged_varlen

HKV = 2
COUNTS = [0, 1, 63, 64, 65, 130, 2, 7]     # an idle slot, one token, around a chunk, more than two chunks
B = len(COUNTS)
FP8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


CAP = 256


def _starts(capacity):
    """an empty slot, a chunk-aligned start, starts that make the tokens straddle chunk and page boundaries, and -- at a capacity of 256 --
    one that overflows it (slot 5: 130 tokens at 127, the last one dropped)"""
    return [0, 1, 63, 64, 100, 127, capacity - 3, 5]


def _cache(D, dtype, fmt, page_size, seed=0, spare=3):
    """a CPU (row-major) cache of B slots of 256 keys: a shuffled table with spare pages, pools filled with the sentinel byte 0x5a"""
    M = CAP // page_size
    num_pages = B * M + spare
    c = qa.alloc_paged_kv_cache_fp8(num_pages, HKV, page_size, D, batch_size=B, max_pages_per_seq=M, scale_k=0.02, scale_v=0.04, dtype=dtype,
                                    device="cpu", fp8_format=fmt)
    g = torch.Generator().manual_seed(seed)
    c.block_table.copy_(torch.randperm(num_pages, generator=g)[:B * M].view(B, M).to(torch.int32))
    c.k.view(torch.uint8).fill_(0x5a)
    c.v.view(torch.uint8).fill_(0x5a)
    c.seqlens.copy_(torch.tensor(_starts(c.capacity), dtype=torch.int32))
    return c


def _clone(c):
    return paged.PagedKVCacheFP8(c.k.clone(), c.v.clone(), c.scale_k, c.scale_v, c.block_table.clone(), c.seqlens.clone(), c.shape, c.fp8_format,
                                 c.dtype, c.numerics, c.layout)


def _tokens(total, D, dtype, seed, mul=2.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(total, HKV, D, generator=g) * mul).to(dtype), (torch.randn(total, HKV, D, generator=g) * mul).to(dtype)


def _cu(counts):
    cu = [0]
    for n in counts:
        cu.append(cu[-1] + n)
    return torch.tensor(cu, dtype=torch.int32)


def _pad(x, counts):
    """[B, Hkv, T, D]: slot b's tokens, then NaN rows that new_lens must keep out of the cache"""
    T = max(max(counts), 1)
    out = torch.full((len(counts), x.shape[1], T, x.shape[2]), float("nan"), dtype=x.dtype)
    at = 0
    for b, n in enumerate(counts):
        out[b, :, :n] = x[at:at + n].transpose(0, 1)
        at += n
    return out


def _same_state(a, b):
    return (torch.equal(a.k.view(torch.uint8), b.k.view(torch.uint8)) and torch.equal(a.v.view(torch.uint8), b.v.view(torch.uint8))
            and torch.equal(a.seqlens, b.seqlens))


# ---- surface ------------------------------------------------------------------------------------------------------------------------------
def test_exports_and_signature():
    assert qa.paged_kv_cache_append_varlen_fp8 is paged_varlen.paged_kv_cache_append_varlen_fp8
    assert "paged_kv_cache_append_varlen_fp8" not in qa.__all__
    sig = str(inspect.signature(qa.paged_kv_cache_append_varlen_fp8)).replace("typing.", "").replace("torch.Tensor", "Tensor")
    assert sig == ("(cache: quantumattention_amd.paged.PagedKVCacheFP8, k_new: Tensor, v_new: Tensor, cu_seqlens: Tensor, *, "
                   "advance: bool = True) -> quantumattention_amd.paged.PagedKVCacheFP8")
    assert "qattn_paged_kv_cache_append_varlen_fp8" in _native.EXPORTS and hasattr(_native.lib(), "qattn_paged_kv_cache_append_varlen_fp8")
    assert _native.ABI_VERSION == 8 == _native.lib().qattn_abi_version()
    # the padded entry keeps its signature: the packed one is a sibling
    assert "cu_seqlens" not in str(inspect.signature(qa.paged_kv_cache_append_fp8))


def test_the_ops_schema_and_fake_registration():
    assert hasattr(qa.ops, "fp8_paged_varlen_kv_cache_append_")
    op = torch.ops.quantumattention_amd.fp8_paged_varlen_kv_cache_append_.default
    schema = str(op._schema)
    assert "Tensor(a0!) k_pool" in schema and "Tensor(a1!) v_pool" in schema and "Tensor(a5!) seqlens" in schema, schema
    assert "Tensor cu_seqlens" in schema and "bool advance=True" in schema and schema.endswith("-> ()"), schema
    # the fake registration: the op runs on meta tensors, returns nothing, allocates nothing
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        pool = torch.empty((4 * HKV * 64 * 64,), dtype=torch.uint8)
        sc = torch.empty((2, HKV), dtype=torch.float32)
        x = torch.empty((5, HKV, 64), dtype=torch.bfloat16)
        res = op(pool, pool.clone(), sc, sc, torch.empty((2, 2), dtype=torch.int32), torch.empty((2,), dtype=torch.int32), x, x,
                 torch.empty((3,), dtype=torch.int32), 4, 64)
    assert res is None


# ---- the reason function ------------------------------------------------------------------------------------------------------------------
def test_every_validation_rule_returns_its_reason():
    D, dtype = 64, torch.bfloat16
    c = _cache(D, dtype, "e4m3", 64)
    total = sum(COUNTS)
    k, v = _tokens(total, D, dtype, 1)
    cu = _cu(COUNTS)
    reason = paged_varlen.paged_varlen_append_input_reason
    assert reason(c, k, v, cu) is None
    assert "PagedKVCacheFP8" in reason(object(), k, v, cu)
    assert "3-D tensors" in reason(c, k[None], v[None], cu)
    assert "3-D tensors" in reason(c, k, None, cu)
    assert "leaf tensors" in reason(c, k.float().requires_grad_().to(dtype), v, cu)
    assert "cache's dtype" in reason(c, k.half(), v.half(), cu)
    assert "same shape" in reason(c, k, v[:-1], cu)
    assert f"[total, {HKV}, {D}]" in reason(c, k[:, :1], v[:, :1], cu)
    assert f"[total, {HKV}, {D}]" in reason(c, k[..., :32], v[..., :32], cu)
    assert "device" in reason(c, k.to("meta"), v.to("meta"), cu)
    assert "16-byte-aligned rows" in reason(c, k.transpose(1, 2).contiguous().transpose(1, 2), v, cu)            # head_dim not innermost
    wide = torch.zeros(total, HKV, D + 4, dtype=dtype)
    assert "16-byte-aligned rows" in reason(c, wide[..., :D], wide[..., :D], cu)                                  # a stride that is no multiple of 8
    off = torch.zeros(total * HKV * D + 4, dtype=dtype)[4:].view(total, HKV, D)
    assert "16-byte-aligned rows" in reason(c, off, off, cu)                                                      # a base that is not aligned
    assert "torch.int32" in reason(c, k, v, cu.long())
    assert "torch.int32" in reason(c, k, v, None)
    assert f"shape [{B + 1}]" in reason(c, k, v, cu[:-1])
    assert "contiguous" in reason(c, k, v, torch.zeros(2 * (B + 1), dtype=torch.int32)[::2])
    assert "to be on" in reason(c, k, v, cu.to("meta"))
    bad = _clone(c)
    bad.seqlens = c.seqlens[:-1]
    assert "cache.seqlens" in reason(bad, k, v, cu)
    # the K and V slices of a packed projection are accepted as they are; so are zero tokens
    qkv = torch.zeros(total, 4 + 2 * HKV, D, dtype=dtype)
    assert reason(c, qkv[:, 4:4 + HKV], qkv[:, 4 + HKV:], cu) is None
    assert reason(c, k[:0], v[:0], cu) is None
    with pytest.raises(ValueError, match="3-D tensors"):
        qa.paged_kv_cache_append_varlen_fp8(c, k[None], v[None], cu)


# ---- the eager definition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype,fmt,page_size", [(64, torch.bfloat16, "e4m3", 64), (128, torch.float16, "e5m2", 128),
                                                   (256, torch.bfloat16, "e4m3", 256)])
def test_the_eager_definition_is_the_padded_append_on_whole_pools_and_seqlens(D, dtype, fmt, page_size):
    c0 = _cache(D, dtype, fmt, page_size, seed=D)
    total = sum(COUNTS)
    k, v = _tokens(total + 3, D, dtype, D + 1)
    k[5, 0, 3], k[70, 1, 0], v[9, 0, 0] = float("inf"), float("nan"), -float("inf")      # saturation and NaN go the same way
    k[total:], v[total:] = float("nan"), float("nan")                                      # a padded token bucket: rows nobody owns
    cu = _cu(COUNTS)
    for advance in (True, False):
        a, b = _clone(c0), _clone(c0)
        assert qa.paged_kv_cache_append_varlen_fp8(a, k, v, cu, advance=advance) is a
        paged._append_eager(b, _pad(k, COUNTS), _pad(v, COUNTS), torch.tensor(COUNTS, dtype=torch.int32), advance)
        assert _same_state(a, b)
        assert not _same_state(a, c0)
        cap = c0.capacity
        want = [min(p + n, cap) for p, n in zip(_starts(cap), COUNTS)] if advance else _starts(cap)
        assert a.seqlens.tolist() == want
        assert cap == CAP and want[5] == (cap if advance else 127)          # slot 5 overflows: 129 tokens stored, one dropped
        # exactly the appended keys changed: every other byte is still the sentinel
        changed = (a.k.view(torch.uint8) != 0x5a).any(-1).any(1).sum().item()      # (page, key) pairs with a byte that is not the sentinel
        assert changed <= sum(min(n, cap - p) for p, n in zip(_starts(cap), COUNTS))


def test_strided_slices_of_a_projection_give_the_bytes_of_their_copies():
    D, dtype, Hq = 64, torch.bfloat16, 4
    c0 = _cache(D, dtype, "e4m3", 128)
    total = sum(COUNTS)
    qkv = (torch.randn(total, Hq + 2 * HKV, D, generator=torch.Generator().manual_seed(3)) * 2).to(dtype)
    ks, vs = qkv[:, Hq:Hq + HKV], qkv[:, Hq + HKV:]
    assert not ks.is_contiguous()
    a, b = _clone(c0), _clone(c0)
    qa.paged_kv_cache_append_varlen_fp8(a, ks, vs, _cu(COUNTS))
    qa.paged_kv_cache_append_varlen_fp8(b, ks.contiguous(), vs.contiguous(), _cu(COUNTS))
    assert _same_state(a, b)


def test_zero_tokens_are_a_no_op():
    D, dtype = 64, torch.bfloat16
    c0 = _cache(D, dtype, "e4m3", 64)
    c0.seqlens[1] = -5                           # not even the clamp of an advancing call happens
    a = _clone(c0)
    k, v = _tokens(4, D, dtype, 1)
    assert qa.paged_kv_cache_append_varlen_fp8(a, k[:0], v[:0], torch.zeros(B + 1, dtype=torch.int32)) is a
    assert _same_state(a, c0)


def test_clamped_cu_seqlens_follow_the_attention_entrys_clamps():
    """start_i = clamp(cu[i], 0, total), end_i = clamp(cu[i + 1], start_i, total): entries outside [0, total] and a cu[B] below total"""
    D, dtype = 64, torch.bfloat16
    c0 = _cache(D, dtype, "e4m3", 64)
    k, v = _tokens(20, D, dtype, 5)
    cu = torch.tensor([-3, 4, 4, 9, 9, 9, 12, 15, 400], dtype=torch.int32)       # slots: 4, 0, 5, 0, 0, 3, 3, 5 (cut at total = 20)
    counts = [4, 0, 5, 0, 0, 3, 3, 5]
    a, b = _clone(c0), _clone(c0)
    qa.paged_kv_cache_append_varlen_fp8(a, k, v, cu)
    paged._append_eager(b, _pad(k, counts), _pad(v, counts), torch.tensor(counts, dtype=torch.int32), True)
    assert _same_state(a, b)


# ---- the kernel's slot map (include/qattn_paged_varlen_append.h), as arithmetic -------------------------------------------------------
def _slot_to_chunk(j, cu, total):
    """the kernel's search: slot j -> (sequence, chunk) or None"""
    Bn = len(cu) - 1
    clamp = lambda x, lo, hi: min(max(x, lo), hi)
    lo, hi = 0, Bn - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if 2 * mid + clamp(cu[mid], 0, total) // 64 <= j:
            lo = mid
        else:
            hi = mid - 1
    start = clamp(cu[lo], 0, total)
    n = clamp(cu[lo + 1], start, total) - start
    ci = j - (2 * lo + start // 64)
    return (lo, ci) if 0 <= ci <= n // 64 + 1 else None


@pytest.mark.parametrize("counts", [COUNTS, [130, 0, 0, 1], [0, 0, 0, 0], [1] * 32, [512] + [1] * 31, [63, 64, 65, 127, 128, 129, 191, 192]])
def test_every_chunk_a_sequence_can_touch_has_exactly_one_slot(counts):
    cu = _cu(counts).tolist()
    total = cu[-1]
    NS = 2 * len(counts) + total // 64
    hits = [_slot_to_chunk(j, cu, total) for j in range(NS)]
    live = [h for h in hits if h is not None]
    assert len(set(live)) == len(live)
    for i, n in enumerate(counts):
        # n consecutive keys from any position touch at most n // 64 + 2 chunks (n > 0); all of them are served
        for ci in range((n + 62) // 64 + 1 if n else 0):
            assert (i, ci) in live, (i, ci)


# ---- the C entry's argument checks (before any device call: they run without a GPU) ---------------------------------------------------
def test_the_c_entry_rejects_bad_arguments_before_any_device_call():
    L = _native.lib()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    s2 = (ctypes.c_longlong * 2)(2 * 64, 64)

    def call(**kw):
        a = dict(k16=base, v16=base, in_fmt=_native.FMT_BF16, ks=s2, vs=s2, k_pool=base, v_pool=base, scale_k=base, scale_v=base, table=base,
                 tstride=4, seqlens=base, cu=base, advance=1, B=2, Hkv=2, total=0, num_pages=8, page_size=64, max_pages=4, D=64,
                 fp8=_native.fmt_of(torch.float8_e4m3fn))
        a.update(kw)
        return L.qattn_paged_kv_cache_append_varlen_fp8(a["k16"], a["v16"], a["in_fmt"], a["ks"], a["vs"], a["k_pool"], a["v_pool"], a["scale_k"],
                                                        a["scale_v"], a["table"], a["tstride"], a["seqlens"], a["cu"], a["advance"], a["B"], a["Hkv"],
                                                        a["total"], a["num_pages"], a["page_size"], a["max_pages"], a["D"], a["fp8"], None)

    assert call() == 0                                  # total = 0: QATTN_OK, nothing launched
    ok = call()
    bad_arg = call(cu=None)
    assert bad_arg != ok
    for kw in (dict(cu=base + 2), dict(total=-1), dict(table=None), dict(table=base + 2), dict(page_size=96), dict(page_size=0), dict(num_pages=0),
               dict(max_pages=0), dict(tstride=3), dict(k16=None), dict(v16=base + 8), dict(k_pool=base + 8), dict(seqlens=None), dict(B=0),
               dict(Hkv=0), dict(ks=None), dict(ks=(ctypes.c_longlong * 2)(-128, 64)), dict(vs=(ctypes.c_longlong * 2)(128, 12)),
               dict(max_pages=2 ** 25, tstride=2 ** 25), dict(B=2 ** 29, Hkv=4), dict(total=2 ** 31 - 1, Hkv=2 ** 7)):
        assert call(**kw) == bad_arg, kw
    assert call(D=96) not in (ok, bad_arg)             # QATTN_ERR_UNSUPPORTED_DIM
    assert call(in_fmt=_native.fmt_of(torch.float8_e4m3fn)) not in (ok, bad_arg)   # QATTN_ERR_UNSUPPORTED_FMT
    assert call(fp8=_native.FMT_BF16) == call(in_fmt=_native.fmt_of(torch.float8_e4m3fn))

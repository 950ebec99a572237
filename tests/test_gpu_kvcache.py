"""The appendable FP8 K/V cache on the MI355X (quantumattention_amd/kvcache.py, include/qattn_kvcache.h).

Byte oracle: for any scale the expected image is `_native.pack_fp8(ref, LAYOUT_KFRAG / _VFRAG)` of the row-major bytes
ref = fp8(clamp(round_to_dtype(fp32(x) / scale), +-qmax)), restated in tests/kvcache_cases.py -- compared on the keys below seqlens, plus the
rule that every other byte keeps what it held (a fresh cache: zero; the caches here are pre-filled through the kernel and rolled back, so
the bytes around an appended range are non-zero).  Shapes: capacity 200 (no multiple of 64), B = 2, Hkv = 2, the smallest that reach every
store path -- a wholly covered chunk, chunks covered from the left, from the right and in the middle, 4-key groups split at either end."""
import math

import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import kvcache_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV, CAP = 2, 2, 200
# D x 16-bit dtype x fp8 format: a cross, not the full product
CFGS = [(64, torch.bfloat16, "e4m3"), (128, torch.bfloat16, "e4m3"), (256, torch.bfloat16, "e4m3"), (128, torch.float16, "e4m3"),
        (128, torch.bfloat16, "e5m2"), (64, torch.float16, "e5m2"), (256, torch.float16, "e5m2")]
CFG_IDS = [f"d{d}-{str(t)[6:]}-{f}" for d, t, f in CFGS]


def _rand(shape, dtype, seed, mul=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * mul).to(dtype).to(DEV)


def _su(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class Model:
    """the expected row-major bytes of a cache [B, Hkv, capacity, D] and its lengths, advanced by the header's rules"""

    def __init__(self, cache):
        self.cache = cache
        self.fp8 = C.FP8[cache.fp8_format]
        Bc, H, cap, D = cache.shape
        self.k, self.v = (torch.zeros(Bc, H, cap, D, dtype=torch.uint8, device=DEV) for _ in range(2))
        self.lens = [0] * Bc

    def append(self, k_new, v_new, new_lens=None, advance=True):
        cap, T = self.cache.shape[2], k_new.shape[2]
        qk, qv = C.quant_ref(k_new, self.cache.scale_k, self.fp8), C.quant_ref(v_new, self.cache.scale_v, self.fp8)
        for b, p in enumerate(self.lens):
            n = T if new_lens is None else min(max(new_lens[b], 0), T)
            n = min(n, cap - p)
            self.k[b, :, p:p + n] = qk[b, :, :n]
            self.v[b, :, p:p + n] = qv[b, :, :n]
            if advance:
                self.lens[b] = p + n

    def images(self):
        return (_native.pack_fp8(self.k.view(self.fp8), _native.LAYOUT_KFRAG), _native.pack_fp8(self.v.view(self.fp8), _native.LAYOUT_VFRAG))

    def check(self, what=""):
        ik, iv = self.images()
        c = self.cache
        assert c.seqlens.tolist() == self.lens, (what, c.seqlens.tolist(), self.lens)
        for name, got, want in (("k", c.k, ik), ("v", c.v, iv)):
            if not torch.equal(got, want):
                Bc, H, cap, D = c.shape
                layout = C.KFRAG if name == "k" else C.VFRAG
                bad = (C.from_image(got, layout, Bc, H, cap, D) != C.from_image(want, layout, Bc, H, cap, D)).any(-1).nonzero()
                raise AssertionError(f"{what}: {name} image differs at (b, h, key) {bad[:8].tolist()} ... {bad.shape[0]} keys")


def _filled(D, dtype, fmt, seed, scale=0.01):
    """a cache whose 200 keys were all written once (through the kernel, checked), then rolled back to empty: the bytes an append must
    leave alone are non-zero"""
    sk = torch.tensor([[1.0, 1.5], [0.75, 2.0]]) * scale
    c = qa.alloc_kv_cache_fp8(B, HKV, CAP, D, scale_k=sk, scale_v=scale * 2, dtype=dtype, device=DEV, fp8_format=fmt)
    m = Model(c)
    k, v = _rand((B, HKV, CAP, D), dtype, seed), _rand((B, HKV, CAP, D), dtype, seed + 1)
    qa.kv_cache_append_fp8(c, k, v)
    m.append(k, v)
    m.check("fill")
    return c, m


def _set_lens(c, m, lens):
    c.seqlens.copy_(_su(lens))
    m.lens = list(lens)


def test_the_numpy_byte_maps_are_the_librarys():
    for D in (64, 128, 256):
        rows = torch.randint(0, 256, (1, 2, 70, D), dtype=torch.uint8)
        for layout, mine in ((_native.LAYOUT_KFRAG, C.KFRAG), (_native.LAYOUT_VFRAG, C.VFRAG)):
            img = _native.pack_fp8(rows.to(DEV).view(torch.float8_e4m3fn), layout)
            assert torch.equal(img.cpu(), torch.from_numpy(C.to_image(rows.numpy(), mine)))
            assert torch.equal(C.from_image(img, mine, 1, 2, 70, D)[:, :, :70].cpu(), rows)


@pytest.mark.parametrize("D,dtype,fmt", CFGS, ids=CFG_IDS)
def test_bytes_at_the_store_path_boundaries(D, dtype, fmt):
    c, m = _filled(D, dtype, fmt, 10 * D)
    steps = [
        ("T7 at (0, 61): a chunk boundary crossed, a 4-key group split at both ends", [0, 61], 7, None),
        ("T1 at 3 and 63", [3, 63], 1, None),
        ("T1 at 64 and 199", [64, 199], 1, None),
        ("T130 from 5: two partly covered chunks around a whole one", [5, 5], 130, None),
        ("T4 with new_lens (0, 3)", [17, 126], 4, [0, 3]),
        ("T64 at (64, 128): exactly one whole chunk each", [64, 128], 64, None),
    ]
    for i, (what, lens, T, nl) in enumerate(steps):
        _set_lens(c, m, lens)
        k, v = _rand((B, HKV, T, D), dtype, 100 + i, mul=2.0), _rand((B, HKV, T, D), dtype, 200 + i, mul=2.0)
        assert qa.kv_cache_append_fp8(c, k, v, new_lens=None if nl is None else _su(nl)) is c
        m.append(k, v, nl)
        m.check(what)
    # advance=False writes the bytes and leaves seqlens alone
    _set_lens(c, m, [30, 62])
    k, v = _rand((B, HKV, 5, D), dtype, 300), _rand((B, HKV, 5, D), dtype, 301)
    qa.kv_cache_append_fp8(c, k, v, advance=False)
    m.append(k, v, advance=False)
    m.check("advance=False")


@pytest.mark.parametrize("D,dtype,fmt", CFGS, ids=CFG_IDS)
def test_with_the_scales_of_prepare_kv_the_images_are_prepare_kvs(D, dtype, fmt):
    S = 192
    k, v = _rand((B, HKV, S, D), dtype, 7 * D), _rand((B, HKV, S, D), dtype, 7 * D + 1)
    kv = qa.prepare_kv_fp8(k, v, fp8_format=fmt)
    c = qa.alloc_kv_cache_fp8(B, HKV, S, D, scale_k=kv.scale_k, scale_v=kv.scale_v, dtype=dtype, device=DEV, fp8_format=fmt)
    at = 0
    for n in (1, 7, 56, 128):
        qa.kv_cache_append_fp8(c, k[:, :, at:at + n], v[:, :, at:at + n])
        at += n
    assert at == S and c.seqlens.tolist() == [S, S]
    assert torch.equal(c.k, kv.k) and torch.equal(c.v, kv.v)
    for numerics in ("compiled", "eager"):
        kv = qa.prepare_kv_fp8(k, v, fp8_format=fmt, numerics=numerics)
        p = qa.kv_cache_from_prefill_fp8(k, v, S, headroom=1.0, fp8_format=fmt, numerics=numerics)
        assert _same_bits(p.scale_k, kv.scale_k) and _same_bits(p.scale_v, kv.scale_v) and p.seqlens.tolist() == [S, S]
        assert torch.equal(p.k, kv.k) and torch.equal(p.v, kv.v)
    h = qa.kv_cache_from_prefill_fp8(k, v, 300, fp8_format=fmt, numerics="eager")
    assert torch.equal(h.scale_k, kv.scale_k * 2.0) and torch.equal(h.scale_v, kv.scale_v * 2.0) and h.shape == (B, HKV, 300, D) and h.seqlens.tolist() == [S, S]


@pytest.mark.parametrize("D,dtype,fmt", CFGS, ids=CFG_IDS)
def test_nan_in_k_becomes_a_nan_byte_and_inf_clamps_to_qmax(D, dtype, fmt):
    """the cache's scale is finite whatever the data hold, so the kernel itself must route a vector with a non-finite element to the exact
    sequence.  Against quant_ref byte for byte; where quant_ref holds a NaN byte, any NaN byte of the format counts (a NaN has no value to
    compare: e4m3 0x7f / 0xff, e5m2 0x7d .. 0x7f and their negatives), and its seven neighbours in the vector are compared like all others"""
    c, m = _filled(D, dtype, fmt, 20 * D)
    for T, lens in ((9, [61, 0]), (64, [64, 128])):            # the key-by-key stores and the whole-chunk stores
        _set_lens(c, m, lens)
        k, v = _rand((B, HKV, T, D), dtype, 400 + T, mul=2.0), _rand((B, HKV, T, D), dtype, 500 + T, mul=2.0)
        k[0, 0, 0, 0], k[0, 1, 2, 13], k[1, 0, T - 1, D - 1], k[1, 1, 5, 8] = float("nan"), float("inf"), float("-inf"), float("nan")
        k[1, 1, 5, 9] = float("inf")                           # a NaN and an inf in one vector
        qa.kv_cache_append_fp8(c, k, v)
        m.append(k, v)
        isnan = (lambda b: (b & 0x7F) == 0x7F) if fmt == "e4m3" else (lambda b: (b & 0x7F) > 0x7C)
        want_nan = isnan(m.k)
        got = C.from_image(c.k, C.KFRAG, B, HKV, CAP, D)[:, :, :CAP]
        assert want_nan[0, 0, lens[0], 0] and want_nan[1, 1, lens[1] + 5, 8]
        assert torch.equal(isnan(got), want_nan), "NaN elements of k_new must be NaN bytes, and no other byte may be"
        assert torch.equal(got[~want_nan], m.k[~want_nan])
        m.k[want_nan] = got[want_nan]                          # (whatever NaN byte the device chose)
        m.check(f"non-finite K, T{T}")
        qmax_byte = 0x7E if fmt == "e4m3" else 0x7B
        p0, p1 = lens
        assert got[0, 1, p0 + 2, 13] == qmax_byte and got[1, 0, p1 + T - 1, D - 1] == (qmax_byte | 0x80) and got[1, 1, p1 + 5, 9] == qmax_byte


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_saturation_gives_qmax_bytes_no_nan_byte_and_a_finite_attention(fmt):
    D, S = 128, 150
    k, v = _rand((B, HKV, S, D), torch.bfloat16, 41), _rand((B, HKV, S, D), torch.bfloat16, 42)
    kv = qa.prepare_kv_fp8(k, v, fp8_format=fmt)
    c = qa.alloc_kv_cache_fp8(B, HKV, CAP, D, scale_k=kv.scale_k / 4, scale_v=kv.scale_v / 4, dtype=torch.bfloat16, device=DEV, fp8_format=fmt)
    m = Model(c)
    qa.kv_cache_append_fp8(c, k, v)
    m.append(k, v)
    m.check("saturated")
    qmax_byte, nan_from = (0x7E, 0x7F) if fmt == "e4m3" else (0x7B, 0x7C)   # the largest finite magnitude; the first non-finite one
    for rows in (m.k, m.v):
        mag = rows[:, :, :S] & 0x7F
        assert (mag == qmax_byte).float().mean() > 0.01 and not (mag >= nan_from).any()
    q = _rand((B, 4, 2, D), torch.bfloat16, 43)
    out, lse = qa.fp8_attn_splitkv_func(q, c, seqused_k=c.seqlens, causal=True, return_lse=True)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()


def test_overflow_drops_tokens_saturates_seqlens_and_stays_inside_the_images():
    D, dtype, GUARD = 64, torch.bfloat16, 1 << 16
    c, m = _filled(D, dtype, "e4m3", 50)
    bufs = []
    for name in ("k", "v"):                       # the images re-homed between guards
        img = getattr(c, name)
        buf = torch.full((img.numel() + 2 * GUARD,), 0xC3, dtype=torch.uint8, device=DEV)
        buf[GUARD:GUARD + img.numel()] = img
        setattr(c, name, buf[GUARD:GUARD + img.numel()])
        bufs.append(buf)
    _set_lens(c, m, [190, 200])
    k, v = _rand((B, HKV, 16, D), dtype, 51), _rand((B, HKV, 16, D), dtype, 52)
    qa.kv_cache_append_fp8(c, k, v)
    m.append(k, v)
    assert m.lens == [200, 200]
    m.check("T16 at 190 and at 200 of 200")
    qa.kv_cache_append_fp8(c, k, v)               # full: nothing written
    m.check("full cache")
    for buf in bufs:
        assert (buf[:GUARD] == 0xC3).all() and (buf[-GUARD:] == 0xC3).all()


@pytest.mark.parametrize("D,dtype,fmt", CFGS[:4], ids=CFG_IDS[:4])
def test_transposed_and_padded_views_give_the_bits_of_their_contiguous_copies(D, dtype, fmt):
    T = 70
    bthd_k, bthd_v = _rand((B, T, HKV, D), dtype, 60), _rand((B, T, HKV, D), dtype, 61)
    padded = _rand((B, HKV, T, D + 8), dtype, 62)
    for kx, vx in ((bthd_k.transpose(1, 2), bthd_v.transpose(1, 2)), (padded[..., :D], bthd_v.transpose(1, 2)),
                   (bthd_k.transpose(1, 2)[:, :, 3:4], padded[:, :, 5:6, 8:])):
        assert not kx.is_contiguous() or kx.shape[2] == 1
        c, m = _filled(D, dtype, fmt, 63)
        _set_lens(c, m, [61, 2])
        qa.kv_cache_append_fp8(c, kx, vx)
        m.append(kx.contiguous(), vx.contiguous())
        m.check("view")


def _decode_inputs(step, D, dtype):
    return (_rand((B, 8, 1, D), dtype, 700 + step), _rand((B, 2, 1, D), dtype, 800 + step, mul=1.5), _rand((B, 2, 1, D), dtype, 900 + step, mul=1.5))


def test_decode_loop_eager_equals_one_replayed_graph_equals_fresh_prepared_kv():
    D, dtype, cap, S0, steps = 128, torch.bfloat16, 1100, 1030, 6
    k0, v0 = _rand((B, 2, S0, D), dtype, 70), _rand((B, 2, S0, D), dtype, 71)
    attend = lambda q, kv, su: qa.fp8_attn_splitkv_func(q, kv, causal=True, seqused_k=su, num_splits=3, return_lse=True)
    eager = qa.kv_cache_from_prefill_fp8(k0, v0, cap, headroom=2)
    m = Model(eager)
    m.append(k0, v0)
    m.check("prefill")
    want = []
    for s in range(steps):
        q, kn, vn = _decode_inputs(s, D, dtype)
        qa.kv_cache_append_fp8(eager, kn, vn)
        out, lse = attend(q, eager, eager.seqlens)
        m.append(kn, vn)
        m.check(f"step {s}")
        # a fresh PreparedKV from the oracle image of the keys so far, same scales
        L = S0 + s + 1
        fresh = qa.PreparedKV(_native.pack_fp8(m.k[:, :, :L].contiguous().view(m.fp8), _native.LAYOUT_KFRAG),
                              _native.pack_fp8(m.v[:, :, :L].contiguous().view(m.fp8), _native.LAYOUT_VFRAG), eager.scale_k, eager.scale_v,
                              (B, 2, L, D), eager.fp8_format, dtype, eager.numerics, "frag")
        fo, fl = attend(q, fresh, None)
        assert _same_bits(out, fo) and _same_bits(lse, fl), s
        want.append((out, lse))
    # ONE captured graph of "append 1, attend", replayed with refreshed static inputs
    graphed = qa.kv_cache_from_prefill_fp8(k0, v0, cap, headroom=2)
    warm = qa.kv_cache_from_prefill_fp8(k0, v0, cap, headroom=2)
    qs, ks, vs = (t.clone() for t in _decode_inputs(0, D, dtype))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        qa.kv_cache_append_fp8(warm, ks, vs)
        attend(qs, warm, warm.seqlens)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        qa.kv_cache_append_fp8(graphed, ks, vs)
        out_s, lse_s = attend(qs, graphed, graphed.seqlens)
    assert graphed.seqlens.tolist() == [S0, S0]   # capture ran nothing
    for s in range(steps):
        for dst, src in zip((qs, ks, vs), _decode_inputs(s, D, dtype)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert graphed.seqlens.tolist() == [S0 + s + 1] * B
        assert _same_bits(out_s, want[s][0]) and _same_bits(lse_s, want[s][1]), s
    assert torch.equal(graphed.k, eager.k) and torch.equal(graphed.v, eager.v)


def test_rollback_then_append_equals_the_straight_append_of_the_survivors():
    D, dtype = 128, torch.bfloat16
    k0, v0 = _rand((B, HKV, 61, D), dtype, 80), _rand((B, HKV, 61, D), dtype, 81)
    kn, vn = _rand((B, HKV, 8, D), dtype, 82), _rand((B, HKV, 8, D), dtype, 83)
    a, b = (qa.kv_cache_from_prefill_fp8(k0, v0, CAP) for _ in range(2))
    qa.kv_cache_append_fp8(a, kn[:, :, :4], vn[:, :, :4])
    a.seqlens.sub_(2)
    qa.kv_cache_append_fp8(a, kn[:, :, 6:8], vn[:, :, 6:8])
    keep = [0, 1, 6, 7]
    qa.kv_cache_append_fp8(b, kn[:, :, keep], vn[:, :, keep])
    assert a.seqlens.tolist() == b.seqlens.tolist() == [65, 65]
    for layout, x, y in ((C.KFRAG, a.k, b.k), (C.VFRAG, a.v, b.v)):
        assert torch.equal(C.from_image(x, layout, B, HKV, CAP, D)[:, :, :65], C.from_image(y, layout, B, HKV, CAP, D)[:, :, :65])
    # a draft of 4, 3 rejected: the rejected tokens' bytes stay behind seqlens and influence no bit
    qa.kv_cache_append_fp8(a, kn[:, :, 2:6], vn[:, :, 2:6])
    a.seqlens.sub_(3)
    qa.kv_cache_append_fp8(b, kn[:, :, 2:3], vn[:, :, 2:3])
    assert not torch.equal(a.k, b.k)
    q = _rand((B, 4, 3, D), dtype, 84)
    for ns in (1, 2):
        got = qa.fp8_attn_splitkv_func(q, a, causal=True, seqused_k=a.seqlens, num_splits=ns, return_lse=True)
        want = qa.fp8_attn_splitkv_func(q, b, causal=True, seqused_k=b.seqlens, num_splits=ns, return_lse=True)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])


def test_the_library_op_called_directly_is_the_function():
    D, dtype = 128, torch.bfloat16
    a, ma = _filled(D, dtype, "e4m3", 95)
    _set_lens(a, ma, [61, 130])
    kn, vn = _rand((B, HKV, 9, D), dtype, 96), _rand((B, HKV, 9, D), dtype, 97)
    nl = _su([9, 2])
    assert qa.ops.fp8_kv_cache_append_(a.k, a.v, a.scale_k, a.scale_v, a.seqlens, kn, vn, nl, CAP, "e4m3", True) is None
    ma.append(kn, vn, [9, 2])
    ma.check("op")


def test_torch_compile_fullgraph_of_append_then_attend_gives_the_eager_bits():
    D, dtype = 64, torch.float16
    k0, v0 = _rand((B, HKV, 130, D), dtype, 90), _rand((B, HKV, 130, D), dtype, 91)
    q, kn, vn = _rand((B, 4, 2, D), dtype, 92), _rand((B, HKV, 2, D), dtype, 93), _rand((B, HKV, 2, D), dtype, 94)
    ca, cb = (qa.kv_cache_from_prefill_fp8(k0, v0, CAP) for _ in range(2))

    def step(cache):
        def f(q, kn, vn):
            qa.kv_cache_append_fp8(cache, kn, vn)
            return qa.fp8_attn_splitkv_func(q * 2, cache, causal=True, seqused_k=cache.seqlens, num_splits=2, return_lse=True)
        return f

    torch._dynamo.reset()
    got = torch.compile(step(ca), fullgraph=True)(q, kn, vn)
    want = step(cb)(q, kn, vn)
    assert all(_same_bits(x, y) for x, y in zip(got, want))
    assert ca.seqlens.tolist() == cb.seqlens.tolist() == [132, 132] and torch.equal(ca.k, cb.k) and torch.equal(ca.v, cb.v)
    assert not math.isnan(float(got[0].float().sum()))

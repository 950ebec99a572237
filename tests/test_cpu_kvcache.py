"""The appendable FP8 K/V cache (quantumattention_amd/kvcache.py, include/qattn_kvcache.h) without a GPU: exports and signatures, the
validation reasons, the C entry's error codes (returned before any device call), the eager definition -- piecewise = at once, rollback,
overflow, attention over the cache -- and the teeth of the layout facts the kernel's store scheme for partly covered chunks rests on."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, kvcache
from tests import kvcache_cases as C


def _kv(seed, B=2, Hkv=2, S=200, D=64, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, Hkv, S, D, generator=g).to(dtype) for _ in range(2))


def _cache(B=2, Hkv=2, capacity=200, D=64, dtype=torch.bfloat16, sk=0.01, sv=0.02, **kw):
    return qa.alloc_kv_cache_fp8(B, Hkv, capacity, D, scale_k=sk, scale_v=sv, dtype=dtype, device="cpu", **kw)


def _u8(t):
    return t.view(torch.uint8)


# ---- surface ------------------------------------------------------------------------------------------------------------------------------
def test_exports_and_signatures():
    assert qa.KVCacheFP8 is kvcache.KVCacheFP8 and issubclass(qa.KVCacheFP8, qa.PreparedKV)
    for name in ("alloc_kv_cache_fp8", "kv_cache_from_prefill_fp8", "kv_cache_append_fp8"):
        assert getattr(qa, name) is getattr(kvcache, name) and name not in qa.__all__
    assert hasattr(qa.ops, "fp8_kv_cache_append_")
    sig = lambda f: str(inspect.signature(f)).replace("typing.", "").replace("torch.Tensor", "Tensor")
    assert sig(qa.alloc_kv_cache_fp8) == ("(B: int, Hkv: int, capacity: int, D: int, *, scale_k, scale_v, dtype, device, fp8_format: Optional[str] = None, "
                                          "numerics: Optional[str] = None) -> quantumattention_amd.kvcache.KVCacheFP8")
    assert sig(qa.kv_cache_from_prefill_fp8) == ("(k: Tensor, v: Tensor, capacity: int, *, headroom: float = 2.0, fp8_format: Optional[str] = None, "
                                                 "numerics: Optional[str] = None) -> quantumattention_amd.kvcache.KVCacheFP8")
    assert sig(qa.kv_cache_append_fp8) == ("(cache: quantumattention_amd.kvcache.KVCacheFP8, k_new: Tensor, v_new: Tensor, *, "
                                           "new_lens: Optional[Tensor] = None, advance: bool = True) -> quantumattention_amd.kvcache.KVCacheFP8")
    assert "qattn_kv_cache_append_fp8" in _native.EXPORTS


def test_alloc_gives_zero_images_zero_lengths_and_fp32_scales_per_head():
    per_head = torch.tensor([0.5, 0.25], dtype=torch.float64)
    per_bh = torch.tensor([[1.0, 2.0], [3.0, 4.0]])
    for sk, want in ((0.125, torch.full((2, 2), 0.125)), (per_head, torch.tensor([[0.5, 0.25]] * 2)), (per_bh, per_bh)):
        c = _cache(sk=sk, sv=3, fp8_format="e5m2", numerics="eager")
        assert isinstance(c, qa.KVCacheFP8) and c.shape == (2, 2, 200, 64) and c.capacity == 200 and c.layout == "rowmajor"
        assert c.fp8_format == "e5m2" and c.numerics == "eager" and c.dtype == torch.bfloat16
        assert c.k.dtype == torch.float8_e5m2 and c.k.shape == (2, 2, 200, 64) and not _u8(c.k).any() and not _u8(c.v).any()
        assert c.seqlens.dtype == torch.int32 and c.seqlens.tolist() == [0, 0]
        assert c.scale_k.dtype == torch.float32 and c.scale_k.shape == (2, 2) and c.scale_k.is_contiguous() and torch.equal(c.scale_k, want)
        assert torch.equal(c.scale_v, torch.full((2, 2), 3.0))
    with qa.config.patch({"attention.fp8_format": "e5m2"}):
        assert _cache().fp8_format == "e5m2"


@pytest.mark.parametrize("bad", ["B", "capacity", "cap_bool", "D", "dtype", "scale_zero", "scale_neg", "scale_inf", "scale_nan", "scale_tensor_zero",
                                 "scale_tensor_nan", "scale_shape", "scale_type", "scale_bool", "fmt", "numerics"])
def test_alloc_refuses(bad):
    a = dict(B=2, Hkv=2, capacity=200, D=64)
    kw = dict(scale_k=0.01, scale_v=0.01, dtype=torch.bfloat16, device="cpu")
    if bad == "B":
        a["B"] = 0
    elif bad == "capacity":
        a["capacity"] = -1
    elif bad == "cap_bool":
        a["capacity"] = True
    elif bad == "D":
        a["D"] = 48
    elif bad == "dtype":
        kw["dtype"] = torch.float32
    elif bad == "scale_zero":
        kw["scale_k"] = 0.0
    elif bad == "scale_neg":
        kw["scale_v"] = -1.0
    elif bad == "scale_inf":
        kw["scale_k"] = float("inf")
    elif bad == "scale_nan":
        kw["scale_v"] = float("nan")
    elif bad == "scale_tensor_zero":
        kw["scale_k"] = torch.tensor([1.0, 0.0])
    elif bad == "scale_tensor_nan":
        kw["scale_v"] = torch.tensor([[1.0, 1.0], [float("nan"), 1.0]])
    elif bad == "scale_shape":
        kw["scale_k"] = torch.ones(3)
    elif bad == "scale_type":
        kw["scale_k"] = "1.0"
    elif bad == "scale_bool":
        kw["scale_k"] = True
    elif bad == "fmt":
        kw["fp8_format"] = "e3m4"
    else:
        kw["numerics"] = "exact"
    with pytest.raises(ValueError):
        qa.alloc_kv_cache_fp8(a["B"], a["Hkv"], a["capacity"], a["D"], **kw)


@pytest.mark.parametrize("bad", ["headroom_lt1", "headroom_nan", "headroom_inf", "headroom_str", "capacity_small", "capacity_float", "f32", "kv_shape", "D"])
def test_from_prefill_refuses(bad):
    k, v = _kv(1, S=70)
    cap, kw = 100, {}
    if bad == "headroom_lt1":
        kw["headroom"] = 0.99
    elif bad == "headroom_nan":
        kw["headroom"] = float("nan")
    elif bad == "headroom_inf":
        kw["headroom"] = float("inf")
    elif bad == "headroom_str":
        kw["headroom"] = "2"
    elif bad == "capacity_small":
        cap = 69
    elif bad == "capacity_float":
        cap = 100.0
    elif bad == "f32":
        k, v = k.float(), v.float()
    elif bad == "kv_shape":
        v = v[:, :, :-1]
    else:
        k, v = k[..., :48], v[..., :48]
    with pytest.raises(ValueError):
        qa.kv_cache_from_prefill_fp8(k, v, cap, **kw)


@pytest.mark.parametrize("bad", ["cache_type", "k3d", "dtype", "f32", "kv_shape", "B", "Hkv", "D", "T0", "misaligned", "odd_stride", "d_strided", "grad",
                                 "device", "lens_device", "lens_dtype", "lens_shape", "seqlens_dtype", "fmt_bytes"])
def test_append_refuses(bad):
    c = _cache()
    k, v = _kv(2, S=3)
    kw = {}
    if bad == "cache_type":
        c = qa.prepare_kv_fp8(*_kv(3))
    elif bad == "k3d":
        k = k[0]
    elif bad == "dtype":
        k, v = k.to(torch.float16), v.to(torch.float16)
    elif bad == "f32":
        k, v = k.float(), v.float()
    elif bad == "kv_shape":
        v = v[:, :, :2]
    elif bad == "B":
        k, v = k[:1], v[:1]
    elif bad == "Hkv":
        k, v = k[:, :1], v[:, :1]
    elif bad == "D":
        k, v = torch.cat([k, k], -1), torch.cat([v, v], -1)
    elif bad == "T0":
        k, v = k[:, :, :0], v[:, :, :0]
    elif bad == "misaligned":      # dense rows that start 8 bytes into the storage
        k = torch.zeros(k.numel() + 4, dtype=k.dtype)[4:].view(k.shape)
    elif bad == "odd_stride":      # rows 68 elements apart: every other row starts 8 bytes off a 16-byte boundary
        k = torch.zeros(2, 2, 3, 68, dtype=k.dtype)[..., :64]
    elif bad == "d_strided":       # head_dim not innermost
        k = torch.zeros(2, 2, 64, 3, dtype=k.dtype).transpose(2, 3)
    elif bad == "grad":
        k = k.float().requires_grad_().to(torch.bfloat16)
    elif bad == "device":
        k, v = k.to("meta"), v.to("meta")
    elif bad == "lens_device":
        kw["new_lens"] = torch.tensor([1, 1], dtype=torch.int32, device="meta")
    elif bad == "lens_dtype":
        kw["new_lens"] = torch.tensor([1, 1])
    elif bad == "lens_shape":
        kw["new_lens"] = torch.tensor([1], dtype=torch.int32)
    elif bad == "seqlens_dtype":
        c.seqlens = c.seqlens.long()
    elif bad == "fmt_bytes":
        c.fp8_format = "e5m2"
    with pytest.raises(ValueError) as e:
        qa.kv_cache_append_fp8(c, k, v, **kw)
    assert str(e.value) == kvcache.kv_cache_append_input_reason(c, k, v, kw.get("new_lens"))


def test_the_views_a_projection_produces_are_accepted():
    c = _cache()
    bthd = torch.zeros(2, 5, 2, 64, dtype=torch.bfloat16)
    padded = torch.zeros(2, 2, 5, 72, dtype=torch.bfloat16)[..., :64]          # rows 144 bytes apart
    for t in (bthd.transpose(1, 2), padded, bthd.transpose(1, 2)[:, :, 1:2]):
        assert not t.is_contiguous() or t.shape[2] == 1
        assert kvcache.kv_cache_append_input_reason(c, t, t) is None


def test_the_c_entry_refuses_before_any_device_call():
    """the codes of include/qattn_kvcache.h; the pointers are never dereferenced on these paths"""
    L = _native.lib()
    s3 = (ctypes.c_longlong * 3)(2 * 3 * 64, 3 * 64, 64)
    ok = dict(k16=4096, v16=8192, in_fmt=_native.FMT_BF16, ks=s3, vs=s3, k8=1 << 20, v8=2 << 20, sk=256, sv=512, seqlens=1024, new_lens=None,
              advance=1, B=2, Hkv=2, T=3, capacity=200, D=64, fp8_fmt=_native.FMT_E4M3, stream=None)
    INVALID, DIM, FMT = -1, -2, -3        # include/qattn.h QATTN_ERR_INVALID_ARG / _UNSUPPORTED_DIM / _UNSUPPORTED_FMT (literal)

    def call(**over):
        a = dict(ok, **over)
        return L.qattn_kv_cache_append_fp8(*[a[n] for n in ("k16", "v16", "in_fmt", "ks", "vs", "k8", "v8", "sk", "sv", "seqlens", "new_lens", "advance",
                                                            "B", "Hkv", "T", "capacity", "D", "fp8_fmt", "stream")])

    for name in ("k16", "v16", "ks", "vs", "k8", "v8", "sk", "sv", "seqlens"):
        assert call(**{name: None}) == INVALID, name
    for name in ("k8", "v8", "k16", "v16"):
        assert call(**{name: ok[name] + 8}) == INVALID, name                       # misaligned image / row
    assert call(ks=(ctypes.c_longlong * 3)(2 * 3 * 68, 3 * 68, 68)) == INVALID     # misaligned rows
    assert call(vs=(ctypes.c_longlong * 3)(2 * 3 * 64, 3 * 64, -64)) == INVALID    # a negative stride would read in front of the base
    for name in ("B", "Hkv", "T", "capacity", "D"):
        assert call(**{name: 0}) == INVALID and call(**{name: -1}) == INVALID, name
    assert call(B=1 << 20, Hkv=1 << 11) == INVALID                                 # a grid beyond 2^31 - 1
    assert call(D=96) == DIM and call(D=32) == DIM
    assert call(in_fmt=_native.FMT_E4M3) == FMT and call(fp8_fmt=_native.FMT_BF16) == FMT


# ---- the eager definition -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,dtype", [("e4m3", torch.bfloat16), ("e5m2", torch.float16)])
def test_eager_append_writes_the_formula_piece_by_piece_as_at_once(fmt, dtype):
    k, v = _kv(4, S=150, dtype=dtype)
    sk, sv = torch.tensor([[0.01, 0.02], [0.005, 0.03]]), torch.tensor([0.02, 0.01])
    whole = _cache(dtype=dtype, sk=sk, sv=sv, fp8_format=fmt)
    assert qa.kv_cache_append_fp8(whole, k, v) is whole and whole.seqlens.tolist() == [150, 150]
    for img, x, s in ((whole.k, k, whole.scale_k), (whole.v, v, whole.scale_v)):
        assert torch.equal(_u8(img)[:, :, :150], C.quant_ref(x, s, C.FP8[fmt])) and not _u8(img)[:, :, 150:].any()
    pieces = _cache(dtype=dtype, sk=sk, sv=sv, fp8_format=fmt)
    for a, b in ((0, 1), (1, 8), (8, 64), (64, 150)):
        qa.kv_cache_append_fp8(pieces, k[:, :, a:b], v[:, :, a:b])
    assert torch.equal(_u8(pieces.k), _u8(whole.k)) and torch.equal(_u8(pieces.v), _u8(whole.v)) and pieces.seqlens.tolist() == [150, 150]


def test_eager_new_lens_advance_rollback_and_overflow():
    k, v = _kv(5, S=16)
    c = _cache()
    c.seqlens.copy_(torch.tensor([3, 190], dtype=torch.int32))
    qa.kv_cache_append_fp8(c, k, v, new_lens=torch.tensor([5, 99], dtype=torch.int32), advance=False)
    assert c.seqlens.tolist() == [3, 190]                                          # not advanced
    want = C.quant_ref(k, c.scale_k, C.FP8["e4m3"])
    assert torch.equal(_u8(c.k)[0, :, 3:8], want[0, :, :5]) and not _u8(c.k)[0, :, 8:].any() and not _u8(c.k)[0, :, :3].any()
    assert torch.equal(_u8(c.k)[1, :, 190:200], want[1, :, :10])                   # 16 tokens at 190 of 200: 10 written, 6 dropped
    qa.kv_cache_append_fp8(c, k, v, new_lens=torch.tensor([5, 99], dtype=torch.int32))
    assert c.seqlens.tolist() == [8, 200]                                          # saturates at the capacity
    qa.kv_cache_append_fp8(c, k, v)
    assert c.seqlens.tolist() == [24, 200]
    # rollback: append 4, take 2 back, append 2 others = the straight append of the 4 survivors, below seqlens
    a, b = _cache(), _cache()
    qa.kv_cache_append_fp8(a, k[:, :, :4], v[:, :, :4])
    a.seqlens.sub_(2)
    qa.kv_cache_append_fp8(a, k[:, :, 6:8], v[:, :, 6:8])
    keep = [0, 1, 6, 7]
    qa.kv_cache_append_fp8(b, k[:, :, keep], v[:, :, keep])
    assert a.seqlens.tolist() == b.seqlens.tolist() == [4, 4]
    assert torch.equal(_u8(a.k)[:, :, :4], _u8(b.k)[:, :, :4]) and torch.equal(_u8(a.v)[:, :, :4], _u8(b.v)[:, :, :4])


def test_eager_prefill_with_headroom_1_reproduces_prepare_kv_and_the_cache_is_attended_through_seqlens():
    k, v = _kv(6, S=192)
    kv = qa.prepare_kv_fp8(k, v)
    c = qa.kv_cache_from_prefill_fp8(k, v, 192, headroom=1.0)
    assert torch.equal(_u8(c.k), _u8(kv.k)) and torch.equal(_u8(c.v), _u8(kv.v))
    assert torch.equal(c.scale_k, kv.scale_k) and torch.equal(c.scale_v, kv.scale_v) and c.seqlens.tolist() == [192, 192]
    big = qa.kv_cache_from_prefill_fp8(k[:, :, :150], v[:, :, :150], 300)
    assert torch.equal(big.scale_k, qa.prepare_kv_fp8(k[:, :, :150], v[:, :, :150]).scale_k * 2.0) and big.seqlens.tolist() == [150, 150]
    qa.kv_cache_append_fp8(big, k[:, :, 150:], v[:, :, 150:])
    g = torch.Generator().manual_seed(7)
    q = torch.randn(2, 4, 3, 64, generator=g).to(torch.bfloat16)
    got = qa.fp8_attn_splitkv_func(q, big, seqused_k=big.seqlens, causal=True, num_splits=2)
    # a PreparedKV of exactly the used keys, same bytes and scales
    ref = qa.PreparedKV(big.k[:, :, :192].contiguous(), big.v[:, :, :192].contiguous(), big.scale_k, big.scale_v, (2, 2, 192, 64), "e4m3",
                        torch.bfloat16, big.numerics, "rowmajor")
    want = qa.fp8_attn_splitkv_func(q, ref, causal=True, num_splits=2)
    assert torch.equal(got, want) and torch.isfinite(got.float()).all()
    # bytes behind seqlens influence no bit: the largest finite value there (NaN bytes: the kernel's contract, tests/test_gpu_kvcache.py --
    # the eager definition multiplies a masked key's V by an exact zero, which keeps a NaN)
    _u8(big.k)[:, :, 192:] = 0x7E
    _u8(big.v)[:, :, 192:] = 0x7E
    assert torch.equal(qa.fp8_attn_splitkv_func(q, big, seqused_k=big.seqlens, causal=True, num_splits=2), want)


def test_eager_nan_in_k_stays_a_nan_byte_and_inf_clamps():
    k, v = _kv(9, S=4)
    k[0, 0, 1, 3], k[1, 1, 2, 5], k[0, 1, 0, 7] = float("nan"), float("inf"), float("-inf")
    c = _cache()
    qa.kv_cache_append_fp8(c, k, v)
    kb = _u8(c.k)[:, :, :4]
    assert kb[0, 0, 1, 3] & 0x7F == 0x7F and kb[1, 1, 2, 5] == 0x7E and kb[0, 1, 0, 7] == 0xFE and ((kb & 0x7F) == 0x7F).sum() == 1


def test_prefill_scales_are_prepare_kvs_also_with_a_nan_and_on_a_view():
    k, v = _kv(10, S=70)
    kt = k.transpose(1, 2).contiguous().transpose(1, 2)                             # [B, T, H, D]-backed
    for kk in (k, kt):
        c, kv = qa.kv_cache_from_prefill_fp8(kk, v, 70, headroom=1.0), qa.prepare_kv_fp8(kk, v)
        assert torch.equal(c.scale_k, kv.scale_k) and torch.equal(c.scale_v, kv.scale_v) and torch.equal(_u8(c.k), _u8(kv.k))
    k[1, 0, 5, 5] = float("nan")
    c, kv = qa.kv_cache_from_prefill_fp8(k, v, 70, headroom=1.0), qa.prepare_kv_fp8(k, v)
    assert torch.isnan(c.scale_k[1, 0]) and torch.equal(torch.isnan(c.scale_k), torch.isnan(kv.scale_k))


def test_saturation_clamps_and_never_makes_a_nan_byte():
    k, v = _kv(8, S=40)
    tight = qa.kv_cache_from_prefill_fp8(k, v, 64, headroom=1.0)
    c = _cache(capacity=64, sk=tight.scale_k / 4, sv=tight.scale_v / 4)
    qa.kv_cache_append_fp8(c, k, v)
    kb = _u8(c.k)[:, :, :40]
    assert ((kb & 0x7F) == 0x7E).any() and not ((kb & 0x7F) == 0x7F).any()         # e4m3: 0x7e = 448, 0x7f = NaN
    assert torch.equal(kb, C.quant_ref(k, c.scale_k, C.FP8["e4m3"]))
    back = c.k[:, :, :40].float() * c.scale_k[:, :, None, None]
    lim = (448 * c.scale_k)[:, :, None, None]
    sat = k.float().abs() > lim
    assert sat.any() and torch.equal(back[sat].abs(), lim.expand_as(back)[sat])     # a saturated element sits at scale * qmax: its error is its excess


# ---- the layout facts the store scheme rests on ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128, 256])
def test_layout_maps_are_bijections_and_their_units_belong_to_one_key_or_one_aligned_group(D):
    for layout in (C.KFRAG, C.VFRAG):
        m = C.chunk_map(layout, D)
        assert sorted(m.reshape(-1).tolist()) == list(range(64 * D))
    key_of = np.empty(64 * D, np.int64)
    key_of[C.chunk_map(C.KFRAG, D).reshape(-1)] = np.repeat(np.arange(64), D)
    pieces = key_of.reshape(-1, 16)
    assert (pieces == pieces[:, :1]).all()                                          # a 16-byte KFRAG piece holds bytes of ONE key ...
    assert np.array_equal(pieces[:, 0], [32 * (i // (2 * D)) + (i & 31) for i in range(4 * D)])   # ... the key the kernel derives from the piece number
    d_of = np.empty(64 * D, np.int64)
    key_of[C.chunk_map(C.VFRAG, D).reshape(-1)] = np.repeat(np.arange(64), D)
    d_of[C.chunk_map(C.VFRAG, D).reshape(-1)] = np.tile(np.arange(D), 64)
    words, wd = key_of.reshape(-1, 4), d_of.reshape(-1, 4)
    assert (words % 4 == np.arange(4)).all() and (words // 4 == words[:, :1] // 4).all() and (wd == wd[:, :1]).all()   # a VFRAG word: one aligned 4-key group, one channel
    for w in range(16 * D):                                                         # the decode of a word number the kernel uses
        kb = 32 * ((w >> 7) & 1) + 8 * (w & 3) + 4 * ((w >> 8) & 1)
        assert words[w, 0] == kb and wd[w, 0] == 32 * (w >> 9) + ((w >> 2) & 31)
    rows = np.random.default_rng(D).integers(0, 256, (2, 70, D), dtype=np.uint8)
    for layout in (C.KFRAG, C.VFRAG):
        img = torch.from_numpy(C.to_image(rows, layout))
        back = C.from_image(img, layout, 1, 2, 70, D)
        assert np.array_equal(back[0, :, :70].numpy(), rows) and not back[0, :, 70:].any()


@pytest.mark.parametrize("lo,hi", [(61, 64), (0, 4 - 1), (2, 3), (5, 64), (63, 64)])
def test_a_word_store_for_a_half_covered_group_changes_an_existing_key(lo, hi):
    """the mutant the GPU buffer test must catch: [lo, hi) splits a 4-key group, and a whole-word store for that group overwrites the bytes
    of the keys before lo (already in the cache) or behind hi (another call's, or poison a test planted)"""
    D = 64
    rng = np.random.default_rng(lo * 64 + hi)
    old = rng.integers(1, 256, (64, D), dtype=np.uint8)          # the chunk as it is: every key holds non-zero bytes
    new = rng.integers(1, 256, (64, D), dtype=np.uint8)
    staged = np.zeros_like(new)
    staged[lo:hi] = new[lo:hi]
    want = old.copy()
    want[lo:hi] = new[lo:hi]
    good = C.to_image(old, C.VFRAG)
    C.store_vfrag_chunk(good, staged, lo, hi, D)
    assert np.array_equal(good, C.to_image(want, C.VFRAG))
    bad = C.to_image(old, C.VFRAG)
    C.store_vfrag_chunk(bad, staged, lo, hi, D, mutant=True)
    rows = C.from_image(torch.from_numpy(bad), C.VFRAG, 1, 1, 64, D)[0, 0].numpy()
    assert np.array_equal(rows[lo:hi], new[lo:hi])
    changed = [r for r in range(64) if not (lo <= r < hi) and not np.array_equal(rows[r], old[r])]
    assert changed and all(lo // 4 * 4 <= r < (hi + 3) // 4 * 4 for r in changed), changed

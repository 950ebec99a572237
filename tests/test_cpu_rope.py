"""CPU tests of the RoPE-fused pre-pass's Python surface (quantumattention_amd/rope.py, include/qattn_rope.h): the eager definition against
an independent numpy fp32 restatement bit for bit, the quarter-turn probe's closed form and its teeth, signatures, every ValueError
reason, and the fake registration of the op.  No GPU: tests/test_gpu_rope.py holds the kernels against the same definition."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, rope
from tests import rope_probe as RP


# ---- an independent restatement: numpy float32, one rounding per operation, explicit round-to-nearest-even to 16 bits
def _to_f32(x):
    if x.dtype == torch.bfloat16:
        return (x.contiguous().view(torch.int16).numpy().astype(np.uint16).astype(np.uint32) << 16).view(np.float32)
    return x.numpy().astype(np.float32)


def _round16_bits(y, dtype):
    """float32 array -> the uint16 bit patterns of y rounded to nearest even in `dtype`"""
    if dtype == torch.float16:
        return y.astype(np.float16).view(np.uint16)
    u = y.view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)      # finite inputs


def _np_rope_bits(x, cos, sin, interleaved):
    xf = _to_f32(x)
    S, D = xf.shape[-2], xf.shape[-1]
    c, s = cos.numpy()[..., :S, :].astype(np.float32), sin.numpy()[..., :S, :].astype(np.float32)
    if c.ndim == 3:
        c, s = c[:, None], s[:, None]
    out = np.empty_like(xf)
    h = D // 2
    for i in range(h):
        ia, ib = (2 * i, 2 * i + 1) if interleaved else (i, i + h)
        a, b = xf[..., ia], xf[..., ib]
        out[..., ia] = np.float32(a * c[..., i]) - np.float32(b * s[..., i])
        out[..., ib] = np.float32(b * c[..., i]) + np.float32(a * s[..., i])
    return _round16_bits(out, x.dtype)


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().astype(np.uint16)


def _angle_tables(T, half, seed, batch=None):
    g = torch.Generator().manual_seed(seed)
    shape = (T, half) if batch is None else (batch, T, half)
    ang = torch.rand(shape, generator=g, dtype=torch.float64) * 6.283185307179586
    return torch.cos(ang).to(torch.float32), torch.sin(ang).to(torch.float32)


@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("table", ["shared", "batched", "sliced"])
def test_eager_definition_equals_the_numpy_restatement_bit_for_bit(table, dtype, interleaved):
    B, H, S, D = 2, 3, 37, 64
    x = torch.randn(B, H, S, D, generator=torch.Generator().manual_seed(5)).to(dtype)
    if table == "shared":
        cos, sin = _angle_tables(S + 5, D // 2, 1)
    elif table == "batched":
        cos, sin = _angle_tables(S, D // 2, 2, batch=B)
    else:
        big_c, big_s = _angle_tables(S + 90, D // 2, 3)
        cos, sin = big_c[77:77 + S], big_s[77:77 + S]          # a view: positions 77 .. 77 + S - 1
        assert cos.data_ptr() != big_c.data_ptr()
    got = qa.apply_rope_eager(x, cos, sin, interleaved=interleaved)
    assert got.dtype == dtype and got.shape == x.shape and got.is_contiguous()
    np.testing.assert_array_equal(_bits(got), _np_rope_bits(x, cos, sin, interleaved))
    # 16-bit tables are up-cast exactly: the same bits as the fp32 tables holding those 16-bit values
    c16, s16 = cos.to(torch.bfloat16), sin.to(torch.bfloat16)
    np.testing.assert_array_equal(_bits(qa.apply_rope_eager(x, c16, s16, interleaved=interleaved)),
                                  _np_rope_bits(x, c16.to(torch.float32), s16.to(torch.float32), interleaved))
    # the transposed [B,S,H,D]-backed view gives the dense tensor's bits
    xv = x.transpose(1, 2).contiguous().transpose(1, 2)
    assert not xv.is_contiguous()
    assert torch.equal(qa.apply_rope_eager(xv, cos, sin, interleaved=interleaved), got)


def test_identity_table_and_the_two_conventions_differ():
    x = torch.randn(1, 2, 9, 64, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    one, zero = torch.ones(9, 32), torch.zeros(9, 32)
    for il in (False, True):
        assert torch.equal(qa.apply_rope_eager(x, one, zero, interleaved=il), x)
    cos, sin = _angle_tables(9, 32, 4)
    assert not torch.equal(qa.apply_rope_eager(x, cos, sin, interleaved=False), qa.apply_rope_eager(x, cos, sin, interleaved=True))


# ---- the quarter-turn probe: closed form and teeth
B, HQ, HKV, SQ, SKV, OFF = 2, 4, 2, 40, 75, 77


@pytest.fixture(scope="module", params=[(64, False), (64, True), (128, True)], ids=["d64-neox", "d64-gptj", "d128-gptj"])
def probe(request):
    D, il = request.param
    return RP.Probe(B, HQ, HKV, SQ, SKV, D, il, k_offset=OFF, seed=1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_probe_rotation_is_the_exact_signed_permutation(probe, dtype):
    q, k, _ = probe.tensors(dtype)
    ck, sk = probe.k_tables()
    qr = qa.apply_rope_eager(q, probe.cos, probe.sin, interleaved=probe.interleaved)
    kr = qa.apply_rope_eager(k, ck, sk, interleaved=probe.interleaved)
    assert np.array_equal(qr.to(torch.float64).numpy(), probe.q_rot) and np.array_equal(kr.to(torch.float64).numpy(), probe.k_rot)
    # every output is a signed permutation of its input row: the same multiset of magnitudes
    assert np.array_equal(np.sort(np.abs(qr.float().numpy()), axis=-1), np.sort(np.abs(q.float().numpy()), axis=-1))
    # and the CPU entry points agree with it: the quantiser returns the probe's values unchanged (they are exact in fp8), SDPA finds the pointer
    for scaling in ("head-wise", "token-wise"):
        q8, s = qa.rope_quantize_fp8(q, probe.cos, probe.sin, interleaved=probe.interleaved, scaling=scaling)
        # (the torch quantiser of the CPU path rounds its scale to the input dtype, so the bytes are compared, not the product: every
        # rotated q value is +-gain = the head's / row's abs-max, i.e. the byte +-fmax with the rotated value's sign)
        assert s.shape == ((B, HQ) if scaling == "head-wise" else (B, HQ, SQ))
        assert np.array_equal(q8.to(torch.float64).numpy(), 448.0 * np.sign(probe.q_rot))
    out, lse = qa.fp8_attn_rope_func(q, k, probe.tensors(dtype)[2], probe.cos, probe.sin, cos_k=ck, sin_k=sk, interleaved=probe.interleaved,
                                     return_lse=True)
    assert np.abs(out.double().numpy() - probe.ref).max() <= RP.TOL_V16     # (CPU path: 16-bit SDPA on exact inputs)
    assert np.abs(lse.double().numpy() - probe.ref_lse).max() <= 1e-4


def test_probe_has_teeth(probe):
    """Each way of being wrong changes the rotated tensors EXACTLY (they are no longer the expected permutation) and moves the attention
    answer by more than TEETH x the project's bound -- on every row for a wrong position / a wrong table; for the other pairing convention
    on every row whose turn is EVEN: the conventions agree on turns 0 and 2 (identity and minus identity) and differ by ONE signed
    permutation M on turns 1 and 3, so such a row keeps its query while its target -- the probe's targets all have odd turns -- becomes
    M u, and the pointer is lost (an odd-turn row and its odd-turn target are both multiplied by M: that score survives)."""
    il, q64, k64 = probe.interleaved, probe.q, probe.k
    rot = lambda x, turns, conv=il: RP.turn_rows(x, turns, conv)
    mutants = {
        # the other pairing convention, applied to q and k alike
        "convention": (rot(q64, probe.turns_q, not il), rot(k64, probe.turns_k, not il)),
        # the keys' positions off by one
        "k position + 1": (probe.q_rot, rot(k64, probe.turns_k + 1)),
        # q's table applied to k: the keys' offset of 77 positions is lost
        "q table on k": (probe.q_rot, rot(k64, np.arange(SKV) % 4)),
        # the queries' positions off by one
        "q position + 1": (rot(q64, probe.turns_q + 1), probe.k_rot),
    }
    bound = RP.TEETH * RP.TOL
    for name, (qm, km) in mutants.items():
        assert not (np.array_equal(qm, probe.q_rot) and np.array_equal(km, probe.k_rot)), name
        out, _ = RP.sdpa64(qm, km, probe.v)
        moved = np.abs(out - probe.ref).max(-1)                                  # [B, Hq, Sq]: the largest move within each row
        rows = (probe.turns_q % 2 == 0) if name == "convention" else np.ones(SQ, bool)
        assert moved[..., rows].min() > bound, (name, float(moved[..., rows].min()), bound)
    # shifting q AND k by one position is invisible to attention (RoPE is relative) but not to the rotated tensors: the exact check sees it
    qs, ks = rot(q64, probe.turns_q + 1), rot(k64, probe.turns_k + 1)
    assert not np.array_equal(qs, probe.q_rot)
    assert np.abs(RP.sdpa64(qs, ks, probe.v)[0] - probe.ref).max() < 1e-9
    # the eager definition itself, fed each mistake, is caught by the exact check
    q, k, _ = probe.tensors(torch.bfloat16)
    wrong = qa.apply_rope_eager(k, probe.cos, probe.sin, interleaved=il)        # q's table on k
    assert not np.array_equal(wrong.double().numpy(), probe.k_rot)
    wrong = qa.apply_rope_eager(q, probe.cos, probe.sin, interleaved=not il)
    assert not np.array_equal(wrong.double().numpy(), probe.q_rot)
    wrong = qa.apply_rope_eager(q, probe.cos[1:], probe.sin[1:], interleaved=il)
    assert not np.array_equal(wrong.double().numpy(), probe.q_rot)


# ---- the call surface
def test_signatures_are_pinned():
    def sig(f):
        return [(n, p.kind is inspect.Parameter.KEYWORD_ONLY, p.default) for n, p in inspect.signature(f).parameters.items()]

    E = inspect.Parameter.empty
    assert sig(qa.apply_rope_eager) == [("x", False, E), ("cos", False, E), ("sin", False, E), ("interleaved", True, False)]
    assert sig(qa.rope_quantize_fp8) == [("x", False, E), ("cos", False, E), ("sin", False, E), ("interleaved", True, False),
                                         ("scaling", True, "head-wise"), ("fp8_dtype", True, torch.float8_e4m3fn), ("numerics", True, "compiled")]
    assert sig(qa.fp8_attn_rope_func) == [("q", False, E), ("k", False, E), ("v", False, E), ("cos", False, E), ("sin", False, E),
                                          ("cos_k", True, None), ("sin_k", True, None), ("interleaved", True, False), ("is_causal", True, False),
                                          ("scale", True, None), ("scaling", True, "head-wise"), ("pv_precision", True, "fp8"),
                                          ("precision", True, "auto"), ("return_lse", True, False)]
    assert qa.apply_rope_eager is rope.apply_rope_eager and qa.fp8_attn_rope_func is rope.fp8_attn_rope_func
    assert not {"apply_rope_eager", "rope_quantize_fp8", "fp8_attn_rope_func"} & set(qa.__all__)    # __all__ stays the reference's seven names
    assert len(qa.__all__) == 7


def test_every_rejection_has_a_reason():
    x = torch.zeros(2, 2, 8, 64, dtype=torch.bfloat16)
    c = torch.zeros(8, 32)
    bad_tables = [
        (c[:, :16], c[:, :16], "partial rotary_dim"),                               # a partial rotary_dim
        (torch.zeros(8, 64), torch.zeros(8, 64), r"duplicated \[T, D\] table"),     # the HF-style full-width table
        (c[:5], c[:5], "fewer than the sequence length"),                           # T < S
        (c, torch.zeros(9, 32), "same shape"),
        (c.to(torch.float64), c.to(torch.float64), "dtype"),
        (c, c.to(torch.bfloat16), "dtype"),
        (c.to(torch.int32), c.to(torch.int32), "dtype"),
        (torch.zeros(32), torch.zeros(32), r"\[T, D/2\] or \[B, T, D/2\]"),
        (torch.zeros(3, 8, 32), torch.zeros(3, 8, 32), "same batch size"),
        (c.to("meta"), c.to("meta"), "device"),
        ([[1.0] * 32] * 8, c, "must be tensors"),
    ]
    for cos, sin, why in bad_tables:
        for fn in (lambda: qa.apply_rope_eager(x, cos, sin), lambda: qa.rope_quantize_fp8(x, cos, sin),
                   lambda: qa.fp8_attn_rope_func(x, x, x, cos, sin), lambda: qa.fp8_attn_rope_func(x, x, x, c, c, cos_k=cos, sin_k=sin)):
            with pytest.raises(ValueError, match=why):
                fn()
    with pytest.raises(ValueError, match="bf16 or fp16"):
        qa.apply_rope_eager(x.float(), c, c)
    with pytest.raises(ValueError, match="4-D"):
        qa.rope_quantize_fp8(x[0], c, c)
    for kw, why in (({"scaling": "row-wise"}, "scaling"), ({"fp8_dtype": torch.int8}, "fp8_dtype"), ({"numerics": "jit"}, "numerics")):
        with pytest.raises(ValueError, match=why):
            qa.rope_quantize_fp8(x, c, c, **kw)
    f = qa.fp8_attn_rope_func
    with pytest.raises(ValueError, match="both provided"):
        f(x, x, x, c, c, cos_k=c)
    with pytest.raises(ValueError, match="4-D"):
        f(x[0], x, x, c, c)
    with pytest.raises(ValueError, match="share bf16 or fp16"):
        f(x, x.half(), x, c, c)
    with pytest.raises(ValueError, match="do not match query"):
        f(x, x[:1], x[:1], c, c)
    with pytest.raises(ValueError, match="do not match query"):
        f(x, x, x[:, :, :4], c, c)
    with pytest.raises(ValueError, match="not a multiple"):
        f(torch.zeros(2, 3, 8, 64, dtype=torch.bfloat16), x, x, c, c)
    for kw, why in (({"scaling": "row-wise"}, "scaling"), ({"pv_precision": "fp32"}, "pv_precision"), ({"precision": "exact"}, "precision"),
                    ({"scale": -1.0}, "scale must be positive")):
        with pytest.raises(ValueError, match=why):
            f(x, x, x, c, c, **kw)
    # an odd number of pairs per row has no D/2 table: head_dim must be even
    with pytest.raises(ValueError, match="even"):
        qa.apply_rope_eager(torch.zeros(1, 1, 4, 7, dtype=torch.bfloat16), torch.zeros(4, 3), torch.zeros(4, 3))


def test_cpu_paths_compose_the_eager_definition():
    g = torch.Generator().manual_seed(3)
    q = torch.randn(1, 4, 20, 64, generator=g).to(torch.float16)
    k, v = (torch.randn(1, 2, 33, 64, generator=g).to(torch.float16) for _ in range(2))
    cos, sin = _angle_tables(140, 32, 7)
    ck, sk = cos[100:133], sin[100:133]
    for il in (False, True):
        qr, kr = qa.apply_rope_eager(q, cos, sin, interleaved=il), qa.apply_rope_eager(k, ck, sk, interleaved=il)
        out = qa.fp8_attn_rope_func(q, k, v, cos, sin, cos_k=ck, sin_k=sk, interleaved=il)
        rep = lambda t: t.repeat_interleave(2, dim=1)
        assert torch.equal(out, torch.nn.functional.scaled_dot_product_attention(qr, rep(kr), rep(v)))
        for scaling, dims in (("head-wise", [2, 3]), ("token-wise", [3])):
            x8, s = qa.rope_quantize_fp8(q, cos, sin, interleaved=il, scaling=scaling, fp8_dtype=torch.float8_e5m2)
            w8, ws = qa.nn._dynamically_quantize_fp8(qr, reduction_dim=dims, fp8_dtype=torch.float8_e5m2)
            assert x8.dtype == torch.float8_e5m2 and torch.equal(x8.view(torch.uint8), w8.view(torch.uint8)) and torch.equal(s, ws)


def test_fake_registration_of_the_op_on_meta_tensors():
    from quantumattention_amd import ops  # noqa: F401  (registers the ops)

    op = torch.ops.quantumattention_amd.fp8_rope_attention_forward
    q = torch.empty(2, 8, 300, 128, dtype=torch.bfloat16, device="meta")
    k = torch.empty(2, 2, 512, 128, dtype=torch.bfloat16, device="meta")
    cos = torch.empty(600, 64, dtype=torch.float32, device="meta")
    out, lse = op(q, k, k, cos, cos)
    assert out.shape == q.shape and out.dtype == torch.bfloat16 and out.device.type == "meta" and lse.shape == (0,) and lse.dtype == torch.float32
    out, lse = op(q.half(), k.half(), k.half(), cos, cos, cos[88:], cos[88:], True, True, "token-wise", "e5m2", "eager", "fast", True, True, scale=0.1)
    assert out.shape == q.shape and out.dtype == torch.float16 and lse.shape == (2, 8, 300) and lse.dtype == torch.float32 and lse.device.type == "meta"


def test_argument_errors_come_before_any_launch():
    """codes of include/qattn_rope.h, checked without touching a buffer: every pointer below is a bare aligned address"""
    L = _native.lib()
    one = 4096
    ok = dict(q=one, k=one, strides=None, in_fmt=_native.FMT_BF16, cq=one, sq=one, qtb=0, qtr=64, ck=one, sk=one, ktb=0, ktr=64, il=0, q8=one,
              k8=one, lay=_native.LAYOUT_KFRAG, scq=one, sck=one, B=1, Hq=2, Hkv=1, Sq=8, Skv=8, D=128, fmt=_native.FMT_E4M3, mode=1, num=0,
              ws=None, wsb=0, st=None)

    def rc(**kw):
        a = dict(ok, **kw)
        return L.qattn_rope_quant_qk_fp8(*[a[n] for n in ok])

    assert rc(q=None, k=None) == -1 and rc(q8=None) == -1 and rc(D=96) == -2 and rc(in_fmt=_native.FMT_E4M3) == -3 and rc(fmt=_native.FMT_BF16) == -3
    assert rc(lay=_native.LAYOUT_VFRAG) == -3 and rc(il=2) == -1 and rc(cq=None) == -1 and rc(cq=one + 4) == -1 and rc(qtr=62) == -1 and rc(ktb=-4) == -1
    assert rc(q=one + 8) == -1 and rc(mode=0) == -4 and rc(mode=7) == -1 and rc(num=3) == -1 and rc(Sq=0) == -1
    assert rc(strides=(ctypes.c_longlong * 6)(2048, 1024, 120, 2048, 1024, 128)) == -1      # a row stride below D
    assert rc(strides=(ctypes.c_longlong * 6)(2048, 1024, 128, 2048, 1020, 128)) == -1      # not a multiple of 8 elements
    assert L.qattn_rope_quant_qk_workspace_bytes(4, 32, 8) == 256 * 4 * (4 * 32 + 4 * 8)
    assert L.qattn_fp8_rope_quant_attention_workspace_bytes(1, 2, 1, 8, 8, 96) == 0

"""CPU-only tests of key smoothing on the packed variable-length and block-sparse entries (include/qattn_smooth.h): how the
public functions follow config.attention.smooth_k, the C entries' argument codes before any device call, the ops' fake
implementations, and the eager restatements behind config.attention.force_eager_fallback -- fp32 mean over the used keys, one fp32
subtraction, the same eager quantiser, LSE corrected by scale * q.m.

The mean pass's split rule exists once (`mean_splits`, csrc/qattn_smooth_dev.h, a host and device function over `amax_splits` of
csrc/qattn_common.h): there is no device duplicate to pin against the host rule."""
import ctypes
import inspect
import math

import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native

BAR = 1e-2   # the reference's accuracy bar: RMSE against the unquantised computation
EAGER = {"attention.force_eager_fallback": True, "attention.skip_supported_check": True}


def _with_flag(f, args, smooth_k, kw):
    """the public call under config.attention.smooth_k = smooth_k (None: the config as it stands)"""
    if smooth_k is None:
        return f(*args, **kw)
    with qa.config.patch({"attention.smooth_k": bool(smooth_k)}):
        return f(*args, **kw)


def _varlen(*args, smooth_k=None, **kw):
    return _with_flag(qa.fp8_attn_varlen_func, args, smooth_k, kw)


def _sparse(*args, smooth_k=None, **kw):
    return _with_flag(qa.fp8_block_sparse_attn_func, args, smooth_k, kw)


def _rmse(a, b):
    return (a.double() - b.double()).pow(2).mean().sqrt().item()


def _sdpa64(q, k, v, causal=False, mask=None):
    """fp64 attention of [H, L, D] tensors (GQA by repetition), rows without a key -> 0"""
    rep = q.shape[0] // k.shape[0]
    k, v = (t.double().repeat_interleave(rep, dim=0) for t in (k, v))
    s = q.double() @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if causal:
        s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool).triu(1), -math.inf)
    if mask is not None:
        s = s.masked_fill(~mask, -math.inf)
    p = torch.softmax(s, dim=-1).nan_to_num(0.0)
    return p @ v, torch.logsumexp(s, dim=-1)


def _lse_tol(q, k):
    """Bound on |LSE of the fp8 scores - LSE of the true scores| for [H, L, D] q and k: an LSE moves by at most the largest score error,
    and e4m3 (3 mantissa bits, scale = amax / 448 so nothing clips) rounds q and k - m with a relative error of at most 2^-4 each, so
    |ds| <= sm * sum_d |q_d| |k_d - m_d| * (2 * 2^-4 + 2^-8); 0.15 leaves room for the values below e4m3's normal range."""
    rep = q.shape[0] // k.shape[0]
    ks = (k.double() - k.double().mean(dim=-2, keepdim=True)).repeat_interleave(rep, dim=0)
    return 0.15 * (q.double().abs() @ ks.abs().transpose(-1, -2)).max().item() / math.sqrt(q.shape[-1])


def _packed(seed, dtype, lens, Hq, Hkv, D, sigma=16.0):
    torch.manual_seed(seed)
    total = sum(lens)
    q = torch.randn(total, Hq, D)
    v = torch.randn(total, Hkv, D)
    k = torch.cat([torch.randn(n, Hkv, D) + sigma * torch.randn(1, Hkv, D) for n in lens])   # every sequence its own offset
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    return q.to(dtype), k.to(dtype), v.to(dtype), cu


def test_public_signatures_are_unchanged_and_the_bindings_and_exports_carry_the_flag():
    """the public functions follow config.attention.smooth_k (their parameter lists stay those of flash-attn's varlen call / the block-sparse
    call); the flag is an argument from the op down"""
    assert "smooth_k" not in inspect.signature(qa.fp8_attn_varlen_func).parameters
    assert "smooth_k" not in inspect.signature(qa.fp8_block_sparse_attn_func).parameters
    for f in (_native.fp8_quant_attention_varlen, _native.fp8_block_sparse_attention):
        assert inspect.signature(f).parameters["smooth_k"].default is False
    for name in ("qattn_fp8_quant_attention_varlen_forward_smooth", "qattn_fp8_quant_attention_varlen_smooth_workspace_bytes",
                 "qattn_fp8_block_sparse_attention_forward_smooth", "qattn_fp8_block_sparse_attention_smooth_workspace_bytes"):
        assert name in _native.EXPORTS
    assert len(qa.__all__) == 7


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_varlen_eager_with_smoothing_clears_the_bar_on_offset_keys_and_beats_the_unsmoothed_call(causal, dtype):
    torch.set_num_threads(4)
    lens, Hq, Hkv, D = [300, 64, 517], 4, 2, 64
    q, k, v, cu = _packed(0, dtype, lens, Hq, Hkv, D)
    with qa.config.patch(EAGER):
        on, lse_on = _varlen(q, k, v, cu, cu, max(lens), max(lens), causal=causal, smooth_k=True, return_lse=True)
        off = _varlen(q, k, v, cu, cu, max(lens), max(lens), causal=causal, smooth_k=False)
    ref = torch.empty(q.shape, dtype=torch.float64)
    ref_lse = torch.empty((Hq, q.shape[0]), dtype=torch.float64)
    tol = corr = 0.0
    for a, b in zip(cu[:-1].tolist(), cu[1:].tolist()):
        o, l = _sdpa64(q[a:b].transpose(0, 1), k[a:b].transpose(0, 1), v[a:b].transpose(0, 1), causal)
        ref[a:b], ref_lse[:, a:b] = o.transpose(0, 1), l
        tol = max(tol, _lse_tol(q[a:b].transpose(0, 1), k[a:b].transpose(0, 1)))
        corr = max(corr, (q[a:b].double().transpose(0, 1) @ k[a:b].double().mean(0).repeat_interleave(Hq // Hkv, dim=0)[..., None]).abs().max().item() / math.sqrt(D))
    r_on, r_off = _rmse(on, ref), _rmse(off, ref)
    print(f"varlen eager: rmse smooth_k on {r_on:.5f} off {r_off:.5f}")
    assert r_on < BAR, r_on
    assert r_on < r_off, (r_on, r_off)
    # the corrected LSE is that of the true scores up to the fp8 error of the scores; the uncorrected one lies sm_scale * q.m away
    err = (lse_on.double() - ref_lse).abs().max().item()
    print(f"lse: max err {err:.4f}, bound {tol:.4f}, max |correction| {corr:.2f}")
    assert err < tol and corr > 10 * tol, (err, tol, corr)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_block_sparse_eager_with_smoothing_clears_the_bar_over_the_listed_keys(dtype):
    torch.set_num_threads(4)
    torch.manual_seed(1)
    B, Hq, Hkv, Sq, Skv, D = 1, 4, 2, 500, 700, 64
    q = torch.randn(B, Hq, Sq, D).to(dtype)
    k = (torch.randn(B, Hkv, Skv, D) + 16.0 * torch.randn(B, Hkv, 1, D)).to(dtype)
    v = torch.randn(B, Hkv, Skv, D).to(dtype)
    nqb, nkb = -(-Sq // 128), -(-Skv // 128)
    mask = torch.rand(B, Hq, nqb, nkb) < 0.5
    mask[..., 0] = True      # every query block lists a key block ...
    mask[:, 1, 2, :] = False  # ... but one: zero rows, LSE -inf
    with qa.config.patch(EAGER):
        on, lse_on = _sparse(q, k, v, mask, smooth_k=True, return_lse=True)
        off = _sparse(q, k, v, mask, smooth_k=False)
    em = mask.repeat_interleave(128, dim=2)[:, :, :Sq].repeat_interleave(128, dim=3)[..., :Skv]
    ref, ref_lse = _sdpa64(q[0], k[0], v[0], mask=em[0])   # the fp64 reference over the listed keys only
    r_on, r_off = _rmse(on[0], ref), _rmse(off[0], ref)
    print(f"block-sparse eager: rmse smooth_k on {r_on:.5f} off {r_off:.5f}")
    assert r_on < BAR, r_on
    assert r_on < r_off, (r_on, r_off)
    assert (on[0, 1, 256:384] == 0).all() and (lse_on[0, 1, 256:384] == -math.inf).all()
    live = torch.isfinite(ref_lse)
    err, tol = (lse_on[0].double() - ref_lse)[live].abs().max().item(), _lse_tol(q[0], k[0])
    corr = (q[0].double() @ k[0].double().mean(-2).repeat_interleave(Hq // Hkv, dim=0)[..., None]).abs().max().item() / math.sqrt(D)
    print(f"lse: max err {err:.4f}, bound {tol:.4f}, max |correction| {corr:.2f}")
    assert err < tol and corr > 10 * tol, (err, tol, corr)


def test_varlen_eager_means_ignore_keys_beyond_seqused_k():
    torch.set_num_threads(4)
    torch.manual_seed(2)
    lq, lk, S_pad, Hq, Hkv, D = [40, 70, 9], [33, 100, 0], 128, 4, 2, 64
    q = torch.randn(sum(lq), Hq, D).to(torch.bfloat16)
    k = (torch.randn(len(lk), S_pad, Hkv, D) + 16.0 * torch.randn(len(lk), 1, Hkv, D)).to(torch.bfloat16)
    v = torch.randn(len(lk), S_pad, Hkv, D).to(torch.bfloat16)
    cu_q = torch.tensor([0, 40, 110, 119], dtype=torch.int32)
    cu_k = torch.arange(len(lk) + 1, dtype=torch.int32) * S_pad
    used = torch.tensor(lk, dtype=torch.int32)
    k2, v2 = k.clone(), v.clone()
    for i, n in enumerate(lk):
        k2[i, n:], v2[i, n:] = float("nan"), float("nan")
    with qa.config.patch(EAGER):
        call = lambda kk, vv: _varlen(q, kk.flatten(0, 1), vv.flatten(0, 1), cu_q, cu_k, 70, S_pad, seqused_k=used, smooth_k=True,
                                                      return_lse=True)
        out, lse = call(k, v)
        out2, lse2 = call(k2, v2)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    assert torch.isfinite(out).all() and (out[110:] == 0).all() and (lse[:, 110:] == -math.inf).all() and torch.isfinite(lse[:, :110]).all()


def test_calls_follow_the_config_flag_and_a_patch_around_a_call_overrides_it():
    torch.set_num_threads(4)
    q, k, v, cu = _packed(3, torch.bfloat16, [70, 130], 2, 2, 64)
    qd, kd, vd = (t[:128].transpose(0, 1)[None].contiguous() for t in (q, k, v))
    mask = torch.ones(1, 1, 1, 1, dtype=torch.bool)
    vl = lambda: qa.fp8_attn_varlen_func(q, k, v, cu, cu, 130, 130)
    bs = lambda: qa.fp8_block_sparse_attn_func(qd, kd, vd, mask)
    with qa.config.patch(EAGER):
        for f in (vl, bs):
            assert qa.config.attention.smooth_k is False
            off = f()
            with qa.config.patch({"attention.smooth_k": True}):
                on = f()
                with qa.config.patch({"attention.smooth_k": False}):
                    assert torch.equal(f(), off)
                assert torch.equal(f(), on)
            assert not torch.equal(on, off) and torch.equal(f(), off)


def test_fake_impls_accept_the_flag_and_keep_their_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from quantumattention_amd import ops  # noqa: F401  (registers the ops)

    with FakeTensorMode():
        q, k = torch.empty(300, 8, 64, dtype=torch.float16, device="cuda"), torch.empty(500, 2, 64, dtype=torch.float16, device="cuda")
        cu = torch.empty(4, dtype=torch.int32, device="cuda")
        out, lse = torch.ops.quantumattention_amd.fp8_varlen_attention_forward(q, k, k, cu, cu, None, 200, 200, True, "e4m3", "compiled", True, True)
        assert out.shape == (300, 8, 64) and out.dtype == torch.float16 and lse.shape == (8, 300)
        out, lse = torch.ops.quantumattention_amd.fp8_varlen_attention_forward(q, k, k, cu, cu, smooth_k=True)
        assert out.shape == (300, 8, 64) and lse.shape == (0,)
        qb, kb = torch.empty(2, 8, 1000, 128, dtype=torch.bfloat16, device="cuda"), torch.empty(2, 2, 999, 128, dtype=torch.bfloat16, device="cuda")
        m = torch.empty(2, 8, 8, 8, dtype=torch.bool, device="cuda")
        out, lse = torch.ops.quantumattention_amd.fp8_block_sparse_attention_forward(qb, kb, kb, m, "e4m3", "compiled", True, True)
        assert out.shape == (2, 8, 1000, 128) and out.dtype == torch.bfloat16 and lse.shape == (2, 8, 1000)
        out, lse = torch.ops.quantumattention_amd.fp8_block_sparse_attention_forward(qb, kb, kb, m, smooth_k=True)
        assert out.shape == (2, 8, 1000, 128) and lse.shape == (0,)


def test_c_entries_reject_bad_arguments_before_any_device_call():
    L = _native.lib()
    one = ctypes.c_void_p(256)   # any non-NULL, 16-byte aligned pointer: the checks come first
    ws = 1 << 40

    def varlen(k_mean=one, D=128, wsb=ws, tq=100, q=one):
        return L.qattn_fp8_quant_attention_varlen_forward_smooth(q, one, one, None, 2, one, None, one, one, None, 2, 4, 2, tq, 100, D, 0, 0, 0, 0.0,
                                                                 None, None, None, None, one, wsb, None, k_mean)

    assert varlen(k_mean=None) == -1 and varlen(k_mean=ctypes.c_void_p(260)) == -1 and varlen(q=None) == -1
    assert varlen(D=96) == -2
    plain = L.qattn_fp8_quant_attention_varlen_workspace_bytes(2, 4, 2, 100, 100, 128)
    need = L.qattn_fp8_quant_attention_varlen_smooth_workspace_bytes(2, 4, 2, 100, 100, 128)
    assert need >= plain + 4 * 2 * 2 * 128 and varlen(wsb=plain) == -4 and varlen(wsb=need - 1) == -4
    assert varlen(tq=0, wsb=need) == 0   # no query row: nothing to launch
    assert L.qattn_fp8_quant_attention_varlen_smooth_workspace_bytes(0, 4, 2, 100, 100, 128) == 0

    def sparse(k_mean=one, D=128, wsb=ws, q=one):
        return L.qattn_fp8_block_sparse_attention_forward_smooth(q, one, one, 2, one, None, one, None, 2, 4, 2, 300, 300, D, 0, 0, 0.0, None, None,
                                                                 None, None, one, wsb, None, k_mean)

    assert sparse(k_mean=None) == -1 and sparse(k_mean=ctypes.c_void_p(260)) == -1 and sparse(q=None) == -1
    assert sparse(D=96) == -2
    plain = L.qattn_fp8_block_sparse_attention_workspace_bytes(2, 4, 2, 300, 300, 128)
    need = L.qattn_fp8_block_sparse_attention_smooth_workspace_bytes(2, 4, 2, 300, 300, 128)
    assert need >= plain + 4 * 2 * 2 * 128 and sparse(wsb=plain) == -4 and sparse(wsb=need - 1) == -4
    assert L.qattn_fp8_block_sparse_attention_smooth_workspace_bytes(2, 4, 2, 0, 300, 128) == 0

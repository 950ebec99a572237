"""-m gpu: key smoothing (config.attention.smooth_k; include/qattn_smooth.h, qattn_fp8_quant_attention_forward_smooth).

The contract restated (header): m = fp32 mean of K over the sequence per (batch, kv head, channel), deterministic; ks = fp32(k) - m;
scale_k and the fp8 bytes = the existing quantiser's arithmetic applied to ks; the attention kernels unchanged; LSE corrected by
sm_scale * q.m; out mathematically unchanged.  The quantiser arithmetic is restated here in torch, not imported from the package."""
import math

import numpy as np
import pytest
import torch

import oracle
import quantumattention_amd as qa
from quantumattention_amd import _native
from tests.gpu_utils import (FMT, PATH_ONE_TERM, PATH_V16, TDT, assert_within_bound, bits16, fmt16, fused_step_uses_block_v, grade,
                             oracle_for_fp8_path, out_to_f32, unpack_frag)

pytestmark = pytest.mark.gpu
BAR = 1e-2   # the reference's accuracy bar (tests/test_interface.py): RMSE against the unquantised computation


def offset_qkv(seed, dtype, B, Hq, Hkv, Sq, Skv, D, sigma=16.0):
    """q, v ~ N(0,1); k = N(0,1) + c, c[b,h,1,d] ~ N(0, sigma^2): a per-channel offset shared by all tokens of a head."""
    torch.manual_seed(seed)
    q = torch.randn(B, Hq, Sq, D)
    k = torch.randn(B, Hkv, Skv, D) + sigma * torch.randn(B, Hkv, 1, D)
    v = torch.randn(B, Hkv, Skv, D)
    return q.to(dtype), k.to(dtype), v.to(dtype)


def smooth_call(q, k, v, *, causal=False, scaling="head-wise", fp8="e4m3", **kw):
    """The smoothing entry through the binding: (out, [lse,] path, quant dict) as torch tensors on the device."""
    dev = lambda t: t if t.is_cuda else t.cuda()
    return _native.fp8_quant_attention_forward(dev(q), dev(k), dev(v), is_causal=causal, scaling=scaling, fp8_dtype=TDT[fp8], smooth_k=True,
                                               return_path=True, return_quant=True, **kw)


def restate_quantiser(k, mean, scaling, fp8, numerics):
    """Steps 2-3 of the contract on the CPU: (fp8 bytes [B,H,S,D], fp32 scale [B,H] or [B,H,S])."""
    dtype, f8 = k.dtype, TDT[fp8]
    qmax = torch.finfo(f8).max
    ks = k.to(torch.float32) - mean[:, :, None, :]                       # one fp32 subtraction, never rounded to 16 bits
    amax = ks.abs().amax(dim=(-2, -1) if scaling == "head-wise" else -1, keepdim=True)
    scale = amax.mul(1.0 / qmax)
    eps = torch.tensor(torch.finfo(torch.float32).eps, dtype=torch.float32)
    if numerics == "eager":                                             # scale and eps rounded to the input dtype
        scale, eps = scale.to(dtype).to(torch.float32), eps.to(dtype).to(torch.float32)
    scale = torch.maximum(scale, eps)
    t = (ks / scale).to(dtype).to(torch.float32).clamp(-qmax, qmax).to(f8)   # IEEE fp32 quotient, rounded to the input dtype, clamped, RNE
    return t.view(torch.uint8).numpy(), scale.reshape(scale.shape[:2] if scaling == "head-wise" else scale.shape[:3]).numpy()


def k8_of(quant, B, Hkv, Skv, D):
    return unpack_frag(quant["k8"].cpu().numpy(), _native.LAYOUT_KFRAG, B, Hkv, Skv, D)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,H,S,D,view", [(2, 3, 1000, 128, "dense"), (1, 2, 4096, 128, "bshd"), (2, 2, 333, 64, "bshd"), (1, 2, 2500, 256, "dense"),
                                          (1, 1, 70000, 64, "dense")])
def test_mean_is_within_the_fp32_summation_bound_and_deterministic(B, H, S, D, view, dtype):
    """|k_mean - fp64 mean| <= (Skv + 2) 2^-24 max|k|: the first-order forward error bound of ANY fp32 summation order over the Skv values of a
    channel ((n - 1) u sum|x| <= (n - 1) u n max|x|, divided by n), plus one rounding each for the division and the store."""
    q, k, v = offset_qkv(3, dtype, B, H, H, 64, S, D)
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    if view == "bshd":   # the same values as a transposed view of a [B,S,H,D] tensor
        k = k.transpose(1, 2).contiguous().transpose(1, 2)
        assert not k.is_contiguous()
    call = lambda: smooth_call(q, k, v)[-1]["k_mean"]
    m1 = call()
    ref = k.double().mean(dim=-2)
    bound = (S + 2) * 2.0 ** -24 * k.double().abs().amax(dim=-2)
    err = (m1.double() - ref).abs()
    print(f"mean: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.4f}")
    assert (err <= bound).all(), (err / bound).max().item()
    assert torch.equal(m1, call()), "two calls must give the same bits"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mg = call()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(mg, m1), "a graph replay must give the eager call's bits"


QUANT_CASES = [
    # B, Hq, Hkv, S, D
    (1, 4, 2, 300, 64), (2, 2, 2, 1000, 128), (1, 4, 2, 1100, 128), (1, 2, 1, 257, 256),
]


@pytest.mark.parametrize("numerics", ["compiled", "eager"])
@pytest.mark.parametrize("fp8", ["e4m3", "e5m2"])
@pytest.mark.parametrize("scaling", ["head-wise", "token-wise"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,Hq,Hkv,S,D", QUANT_CASES)
def test_k8_and_scale_k_are_the_existing_quantiser_on_k_minus_mean_bit_for_bit(B, Hq, Hkv, S, D, dtype, scaling, fp8, numerics):
    q, k, v = offset_qkv(B + S, dtype, B, Hq, Hkv, S, S, D)
    quant = smooth_call(q, k, v, scaling=scaling, fp8=fp8, numerics=numerics)[-1]
    mean = quant["k_mean"].cpu()
    want8, want_scale = restate_quantiser(k, mean, scaling, fp8, numerics)
    got8 = k8_of(quant, B, Hkv, S, D)
    assert np.array_equal(quant["scale_k"].cpu().numpy(), want_scale), "scale_k"
    mism = got8[:, :, :S] != want8
    assert not mism.any(), (int(mism.sum()), np.argwhere(mism)[:4])
    assert (got8[:, :, S:] == 0).all(), "the padding rows of the last chunk stay zero bytes"


PARITY_CASES = [
    # B, Hq, Hkv, Sq, Skv, D, causal, fp8, scaling, dtype -- every PATH TABLE row of the fused entry (include/qattn.h), causal and not
    (1, 2, 2, 1300, 1300, 128, False, "e4m3", "head-wise", torch.bfloat16),     # D 128, head, <= 16384 keys
    (1, 4, 2, 1300, 1300, 128, True, "e4m3", "head-wise", torch.float16),
    (1, 1, 1, 1100, 16448, 128, False, "e4m3", "head-wise", torch.bfloat16),    # D 128, head, > 16384 keys
    (1, 1, 1, 16448, 16448, 128, True, "e5m2", "head-wise", torch.bfloat16),
    (1, 2, 2, 1100, 1100, 64, False, "e4m3", "head-wise", torch.bfloat16),      # D 64 / 256, head, <= 16384 keys
    (1, 4, 2, 2100, 2100, 256, True, "e4m3", "head-wise", torch.float16),
    (1, 1, 1, 1100, 16448, 256, False, "e4m3", "head-wise", torch.bfloat16),    # D 64 / 256, head, > 16384 keys
    (1, 1, 1, 16448, 16448, 64, True, "e4m3", "head-wise", torch.bfloat16),
    (1, 2, 2, 1100, 1100, 128, False, "e4m3", "token-wise", torch.bfloat16),    # token-wise
    (1, 2, 2, 1300, 1300, 64, True, "e5m2", "token-wise", torch.float16),
]


@pytest.mark.parametrize("case", PARITY_CASES, ids=lambda c: "B{}Hq{}Hkv{}Sq{}Skv{}D{}{}_{}_{}_{}".format(
    c[0], c[1], c[2], c[3], c[4], c[5], "c" if c[6] else "f", c[7], c[8][:4], "bf16" if c[9] == torch.bfloat16 else "fp16"))
def test_attention_and_lse_on_smoothed_keys_vs_the_per_row_path_oracle(case):
    """The attention kernels run unchanged on the smoothed k8 / scale_k: every row against THE oracle of the path the kernel reports, on the
    q8 / k8 / scales the call produced, at the bounds of tests/gpu_utils.py.  LSE: the oracle's on the quantised operands plus
    sm_scale * q.k_mean in fp64 (the caller's 16-bit q, the k_mean the call returned), at the per-path tolerances of tests/test_gpu_attention.py
    (one-term rows of the D = 128 head-wise kernel 2e-2, 16-bit-V rows 4e-3, every other row 2e-3), in both layouts."""
    B, Hq, Hkv, Sq, Skv, D, causal, fp8, scaling, dtype = case
    q, k, v = offset_qkv(1, dtype, B, Hq, Hkv, Sq, Skv, D)
    m = "head" if scaling == "head-wise" else "token"
    out, path, quant = smooth_call(q, k, v, causal=causal, scaling=scaling, fp8=fp8)
    out_l, lse, path_l, quant_l = smooth_call(q, k, v, causal=causal, scaling=scaling, fp8=fp8, return_lse=True)
    out_r, lse_r, _, _ = smooth_call(q, k, v, causal=causal, scaling=scaling, fp8=fp8, return_lse=True, lse_layout=_native.LSE_REFERENCE)
    for key in ("k8", "scale_k", "k_mean"):
        assert torch.equal(quant[key], quant_l[key]), key
    d128_head = D == 128 and scaling == "head-wise"
    if d128_head:   # (elsewhere an LSE request selects the exact-exponential one-term sweep: same bound, other bits -- as without smoothing)
        assert torch.equal(out, out_l), "asking for the LSE must not change the output"
    assert torch.equal(out_l, out_r), "the LSE layout must not change the output"
    q8, sq = oracle.quantize_fp8(bits16(q), fmt16(dtype), m, FMT[fp8])     # (bit-exact to the pre-pass / the in-kernel Q quantisation)
    k8 = np.ascontiguousarray(k8_of(quant, B, Hkv, Skv, D)[:, :, :Skv])
    sk = quant["scale_k"].cpu().numpy()
    if d128_head:
        assert np.array_equal(quant["scale_q"].cpu().numpy(), sq)
    vb = fused_step_uses_block_v(D, scaling, dtype, Skv)
    ref, ref_lse = oracle_for_fp8_path(q8, k8, bits16(v), sq, sk, fp8=fp8, v_dtype=dtype, scaling=m, causal=causal, v_block=vb, fused=True,
                                       return_lse=True)
    for what, o, p in (("plain", out, path), ("with lse", out_l, path_l)):
        mx, rmse, worst = grade(out_to_f32(o), ref, p.cpu().numpy())
        print(f"{what}: max-abs {mx:.5f} rmse {rmse:.6f} worst |err| / bound {worst:.3f}")
        assert_within_bound(out_to_f32(o), ref, p.cpu().numpy(), what)
    rep = Hq // Hkv
    mean = quant["k_mean"].double().cpu().repeat_interleave(rep, dim=1)                 # [B,Hq,D]
    corr = (q.double() * mean[:, :, None, :]).sum(-1).numpy() / math.sqrt(D)
    want_lse = ref_lse + corr
    pl = path_l.cpu().numpy()
    tol = np.where(pl == PATH_ONE_TERM, 2e-2 if d128_head else 2e-3, np.where(pl == PATH_V16, 4e-3, 2e-3))
    err = np.abs(lse.cpu().numpy() - want_lse)
    err_r = np.abs(lse_r.cpu().numpy() / -math.sqrt(D) - want_lse)
    print(f"lse: max err {err.max():.5f} (reference layout {err_r.max():.5f}), max |correction| {np.abs(corr).max():.2f}")
    assert (err < tol).all(), float((err / tol).max())
    assert (err_r < tol).all(), float((err_r / tol).max())
    assert np.abs(corr).max() > 1.0, "the inputs must make the correction matter"


@pytest.mark.parametrize("scaling", ["head-wise", "token-wise"])
def test_a_constant_added_to_some_channels_changes_nothing_but_the_mean(scaling):
    """fp16 keys that are multiples of 2^-4 within +-4, Skv a power of two: every partial sum, the division by Skv and k - m are exact in
    fp32 whatever the summation order -- so +8 on every key of some channels must leave k8, scale_k and out bit for bit as they were."""
    torch.manual_seed(4)
    B, H, S, D = 1, 2, 1024, 128
    q, v = (torch.randn(B, H, S, D).to(torch.float16) for _ in range(2))
    k = (torch.randint(-64, 65, (B, H, S, D)).float() / 16).to(torch.float16)
    shift = torch.zeros(D)
    shift[[3, 17, 64, 100]] = 8.0
    k2 = (k.float() + shift).to(torch.float16)
    assert torch.equal(k2.float(), k.float() + shift)
    out1, _, q1 = smooth_call(q, k, v, scaling=scaling)
    out2, _, q2 = smooth_call(q, k2, v, scaling=scaling)
    assert torch.equal(q1["k_mean"].cpu(), k.double().mean(-2).float()), "the mean of such keys is exact"
    assert torch.equal(q2["k_mean"] - q1["k_mean"], shift.cuda().expand(B, H, D))
    assert torch.equal(q1["k8"], q2["k8"]) and torch.equal(q1["scale_k"], q2["scale_k"])
    assert torch.equal(out1, out2)


def _rmse(out, q, k, v, causal=False):
    ref = torch.nn.functional.scaled_dot_product_attention(q.double().cpu(), k.double().cpu(), v.double().cpu(), is_causal=causal)
    return (out.double().cpu() - ref).pow(2).mean().sqrt().item()


@pytest.mark.parametrize("func", ["fp8_attn_func", "fp8_token_wise_attn_func"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_end_to_end_offset_keys_clear_the_bar_only_with_the_flag(seed, dtype, func):
    """The point of the feature, through the public functions at precision="auto": B 1, H 4, S 2048, D 128, keys with a sigma = 16 channel
    offset; RMSE against fp64 SDPA on the unquantised inputs."""
    f = getattr(qa, func)
    q, k, v = (t.cuda() for t in offset_qkv(seed, dtype, 1, 4, 4, 2048, 2048, 128))
    with qa.config.patch({"attention.smooth_k": True, "attention.precision": "auto"}):
        on = f(q, k, v)
    with qa.config.patch({"attention.smooth_k": False, "attention.precision": "auto"}):
        off = f(q, k, v)
    r_on, r_off = _rmse(on, q, k, v), _rmse(off, q, k, v)
    print(f"{func} seed {seed} {dtype}: rmse smooth_k on {r_on:.5f} off {r_off:.5f}")
    assert r_on < BAR, r_on
    assert r_off > BAR, r_off   # guards that the inputs are hard


def test_flag_on_under_torch_compile_and_on_transposed_views_gives_the_eager_dense_bits():
    q, k, v = (t.cuda() for t in offset_qkv(5, torch.bfloat16, 2, 4, 2, 1300, 1300, 128))
    with qa.config.patch({"attention.smooth_k": True}):
        want = qa.fp8_attn_func(q, k, v, is_causal=True)
        with qa.config.patch({"attention.smooth_k": False}):
            assert not torch.equal(qa.fp8_attn_func(q, k, v, is_causal=True), want)
        qv, kv, vv = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (q, k, v))   # = x.view(B,S,H,D).transpose(1,2)
        assert not kv.is_contiguous()
        assert torch.equal(qa.fp8_attn_func(qv, kv, vv, is_causal=True), want)
        want_lse = smooth_call(q, k, v, causal=True, return_lse=True)[1]
        assert torch.equal(smooth_call(qv, kv, vv, causal=True, return_lse=True)[1], want_lse)
        torch._dynamo.reset()
        cf = torch.compile(lambda a, b, c: qa.fp8_attn_func(a * 1.0, b, c, is_causal=True), backend="aot_eager")
        assert torch.equal(cf(q, k, v), want)
    torch._dynamo.reset()


@pytest.mark.parametrize("func,scaling", [("fp8_attn_func", "head-wise"), ("fp8_token_wise_attn_func", "token-wise")])
def test_flag_off_is_the_existing_entry_bit_for_bit(func, scaling):
    q, k, v = (t.cuda() for t in offset_qkv(6, torch.bfloat16, 1, 4, 4, 1300, 1300, 128))
    assert qa.config.attention.smooth_k is False
    got = getattr(qa, func)(q, k, v, is_causal=True)
    want = _native.fp8_quant_attention_forward(q, k, v, is_causal=True, scaling=scaling)   # qattn_fp8_quant_attention_forward_strided
    assert torch.equal(got, want)
    with qa.config.patch({"attention.smooth_k": True}):   # pre-quantised q / k ignore the flag: the caller quantised
        q8, sq = qa.nn.dynamically_quantize_fp8(q, reduction_dim=[2, 3])
        k8, sk = qa.nn.dynamically_quantize_fp8(k, reduction_dim=[2, 3])
        a = qa.fp8_attn_func(q8, k8, v, scale_q=sq, scale_k=sk)
    assert torch.equal(a, qa.fp8_attn_func(q8, k8, v, scale_q=sq, scale_k=sk))


def test_c_entry_refuses_figures_of_the_unsmoothed_key_and_a_short_workspace():
    import ctypes
    L = _native.lib()
    B, H, S, D = 1, 2, 256, 128
    q, k, v = (torch.randn(B, H, S, D, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    out = torch.empty_like(q)
    q8 = torch.empty((B, H, S, D), dtype=torch.uint8, device="cuda")
    kf, vf = (torch.empty((L.qattn_fp8_tensor_bytes(lay, B, H, S, D),), dtype=torch.uint8, device="cuda") for lay in (_native.LAYOUT_KFRAG, _native.LAYOUT_VFRAG))
    sq, sk, sv, fig = (torch.ones((B, H), dtype=torch.float32, device="cuda") for _ in range(4))
    mean = torch.empty((B, H, D), dtype=torch.float32, device="cuda")
    n = L.qattn_fp8_quant_attention_smooth_workspace_bytes(B, H, H, S, S, D)
    ws = torch.empty((n,), dtype=torch.uint8, device="cuda")

    def call(amax_k=None, ssq_q=None, ssq_k=None, ws_bytes=n, k_mean=mean.data_ptr()):
        return L.qattn_fp8_quant_attention_forward_smooth(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), None, _native.FMT_BF16, out.data_ptr(), q8.data_ptr(), kf.data_ptr(), vf.data_ptr(),
            sq.data_ptr(), sk.data_ptr(), sv.data_ptr(), None, amax_k, None, ssq_q, ssq_k, B, H, H, S, S, D, _native.FMT_E4M3, _native.SCALE_HEAD, 0, 0,
            ctypes.c_float(0.0), 0, None, 0, None, ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream, k_mean)

    assert call(amax_k=fig.data_ptr()) == -1 and call(ssq_q=fig.data_ptr(), ssq_k=fig.data_ptr()) == -1 and call(k_mean=None) == -1
    assert call(ws_bytes=L.qattn_fp8_quant_attention_workspace_bytes(B, H, H, S)) == -4
    assert call() == 0 and call(ssq_q=fig.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()

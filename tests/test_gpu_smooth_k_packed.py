"""-m gpu: key smoothing on the packed variable-length and block-sparse entries (include/qattn_smooth.h:
qattn_fp8_quant_attention_varlen_forward_smooth, qattn_fp8_block_sparse_attention_forward_smooth).

The contract restated: per sequence (varlen, over its USED keys) or per (batch, kv head) over the whole Skv (block-sparse), k_mean /
scale_k / k8 are, bit for bit, what the dense smoothing entry leaves for that K alone; the attention kernels run unchanged on the smoothed
operands; the LSE is corrected by sm_scale * q.k_mean; `out` is mathematically unchanged.  The quantiser arithmetic is restated here in
torch (restate_quantiser, as in tests/test_gpu_smooth_k.py), not imported from the package."""
import math

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests.gpu_utils import TDT, unpack_frag

pytestmark = pytest.mark.gpu
DEV = "cuda"
NB = 128
BAR = 1e-2       # the reference's accuracy bar: RMSE against the unquantised computation
LSE_TOL = 4e-3   # the project's tolerance for 16-bit-V rows (tests/test_gpu_attention.py, as used by the dense smoothing test)


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


def _cdiv(a, b):
    return (a + b - 1) // b


def _cu(lengths):
    return torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32, device=DEV)


def _seq(t, a, n):
    """rows a .. a + n of a packed [total, H, D] tensor as the [1, H, n, D] view the dense entries take"""
    return t[a:a + n].transpose(0, 1)[None]


def _same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32),
                       y.contiguous().view(torch.int16 if y.element_size() == 2 else torch.int32))


def _offset_packed(seed, dtype, lq, lk_alloc, Hq, Hkv, D, sigma=16.0):
    """packed q, k, v: q, v ~ N(0,1); every sequence's keys N(0,1) + c with c ~ N(0, sigma^2) per (head, channel) (offset_qkv of
    tests/test_gpu_smooth_k.py, one offset per sequence)"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(sum(lq), Hq, D, generator=g)
    k = torch.cat([torch.randn(n, Hkv, D, generator=g) + sigma * torch.randn(1, Hkv, D, generator=g) for n in lk_alloc])
    v = torch.randn(sum(lk_alloc), Hkv, D, generator=g)
    return q.to(dtype).to(DEV), k.to(dtype).to(DEV), v.to(dtype).to(DEV)


def _k8_of_sequence(k8, i, start, used, Hkv, D):
    """sequence i's KFRAG image, unpacked to row-major [1, Hkv, ceil(used/64) 64, D] bytes"""
    mp = (used + 63) // 64 * 64
    off = Hkv * D * (start + 64 * i)
    return unpack_frag(k8[off:off + Hkv * mp * D], _native.LAYOUT_KFRAG, 1, Hkv, used, D)


def _check_varlen(q, k, v, lq, starts_k, lk, *, causal, fp8, numerics, seqused, sm_scale=0.0):
    """every claim of the varlen smoothing contract for one call; returns (out, lse, k_mean)"""
    dtype, (_, Hq, D), Hkv = q.dtype, q.shape, k.shape[1]
    B = len(lq)
    cu_q = _cu(lq)
    cu_k = torch.tensor(list(starts_k) + [k.shape[0]], dtype=torch.int32, device=DEV)
    used = torch.tensor(lk, dtype=torch.int32, device=DEV) if seqused else None
    kw = dict(is_causal=causal, fp8_dtype=TDT[fp8], numerics=numerics, sm_scale=sm_scale, smooth_k=True)
    out, lse, q8, k8, sq, sk, mean = _native.fp8_quant_attention_varlen(q, k, v, cu_q, cu_k, used, return_lse=True, return_quant=True, **kw)
    out_plain = _native.fp8_quant_attention_varlen(q, k, v, cu_q, cu_k, used, **kw)
    assert _same_bits(out, out_plain), "asking for the LSE or the operands must not change the output"
    assert mean.shape == (B, Hkv, D) and mean.dtype == torch.float32
    k8n, q8n = k8.cpu().numpy(), q8.cpu().numpy()
    sm = sm_scale if sm_scale > 0 else 1.0 / math.sqrt(D)
    max_corr, a = 0.0, 0
    for i, (n, b, m) in enumerate(zip(lq, starts_k, lk)):
        rows = slice(a, a + n)
        if m == 0:
            assert not mean[i].any(), "no used key: k_mean = 0"
            assert not out[rows].any() and (lse[:, rows] == -math.inf).all(), "no used key: zero rows, LSE -inf"
            a += n
            continue
        ki, vi = _seq(k, b, m), _seq(v, b, m)
        # 1. the dense smoothing entry on the sequence alone (any q serves when the sequence has no query: K's passes do not read it)
        qi = _seq(q, a, n) if n else torch.zeros((1, Hq, 1, D), dtype=dtype, device=DEV)
        dense = _native.fp8_quant_attention_forward(qi, ki, vi, is_causal=causal, scaling="head-wise", fp8_dtype=TDT[fp8], numerics=numerics,
                                                    smooth_k=True, return_quant=True)[-1]
        assert torch.equal(mean[i], dense["k_mean"][0]), ("k_mean", i, m)
        assert torch.equal(sk[i], dense["scale_k"][0]), ("scale_k", i, m)
        mine = _k8_of_sequence(k8n, i, b, m, Hkv, D)
        assert np.array_equal(mine, unpack_frag(dense["k8"].cpu().numpy(), _native.LAYOUT_KFRAG, 1, Hkv, m, D)), ("k8", i, m)
        assert not mine[:, :, m:].any(), "the padding rows of the last chunk stay zero bytes"
        # 2. independently: the torch restatement of the quantiser applied to the returned mean
        want8, want_scale = restate_quantiser(ki.cpu(), mean[i:i + 1].cpu(), "head-wise", fp8, numerics)
        assert np.array_equal(mine[:, :, :m], want8) and np.array_equal(sk[i:i + 1].cpu().numpy(), want_scale), ("restated", i, m)
        # 3. the mean within the first-order bound of any fp32 summation order
        ref_mean = ki[0].double().mean(dim=-2)
        bound = (m + 2) * 2.0 ** -24 * ki[0].double().abs().amax(dim=-2)
        assert ((mean[i].double() - ref_mean).abs() <= bound).all(), ("mean bound", i, m)
        if n == 0:
            continue
        # 4. out rows: the rowmajor 16-bit-V call on the returned operands; LSE: that call's plus sm_scale * q.k_mean in fp64
        q8i = torch.from_numpy(q8n[Hq * D * a:Hq * D * (a + n)].reshape(1, Hq, n, D)).to(DEV).view(TDT[fp8])
        k8i = torch.from_numpy(np.ascontiguousarray(mine[:, :, :m])).to(DEV).view(TDT[fp8])
        o, l = _native.fp8_attention_forward_rowmajor(q8i, k8i, vi, sq[i:i + 1], sk[i:i + 1], is_causal=causal, pv_16bit=True, sm_scale=sm_scale,
                                                      return_lse=True)
        assert _same_bits(out[rows], o[0].transpose(0, 1)), ("out", i, n, m)
        corr = sm * (qi[0].double() * mean[i].double().repeat_interleave(Hq // Hkv, dim=0)[:, None, :]).sum(-1)   # [Hq, n]
        err = (lse[:, rows].double() - (l[0].double() + corr)).abs().max().item()
        assert err < LSE_TOL, ("lse", i, n, m, err)
        max_corr = max(max_corr, corr.abs().max().item())
        a += n
    assert torch.isfinite(out).all()
    return out, lse, mean, max_corr


LENGTHS = [1, 63, 64, 65, 257, 1000, 4097]


@pytest.mark.parametrize("numerics", ["compiled", "eager"])
@pytest.mark.parametrize("fp8", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,causal", [(64, False), (128, True), (256, False), (128, False), (64, True), (256, True)])
def test_varlen_per_sequence_bits_are_the_dense_smoothing_entry_on_the_sequence_alone(D, causal, dtype, fp8, numerics):
    Hq, Hkv = (8, 2) if dtype == torch.float16 else (4, 2)
    lens = LENGTHS[::-1] if dtype == torch.float16 else LENGTHS
    q, k, v = _offset_packed(D + causal, dtype, lens, lens, Hq, Hkv, D)
    starts = list(np.cumsum([0] + lens)[:-1])
    out, lse, mean, max_corr = _check_varlen(q, k, v, lens, starts, lens, causal=causal, fp8=fp8, numerics=numerics, seqused=False)
    print(f"D {D} causal {causal} {dtype} {fp8} {numerics}: max |lse correction| {max_corr:.2f}")
    assert max_corr > 1.0, "the inputs must make the correction matter"
    # the public function: the same bits
    with qa.config.patch({"attention.fp8_format": fp8, "attention.quant_numerics": numerics}):
        cu = _cu(lens)
        o2, l2 = _varlen(q, k, v, cu, cu, max(lens), max(lens), causal=causal, return_lse=True, smooth_k=True)
    assert _same_bits(out, o2) and _same_bits(lse, l2)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype,pad_value", [(torch.bfloat16, 1e4), (torch.float16, float("nan"))], ids=["bf16-1e4", "fp16-nan"])
def test_varlen_cross_attention_with_seqused_k_ignores_the_padding_and_defines_empty_sequences(dtype, pad_value, causal):
    """Wan-style cross-attention: padded K / V [B, S_pad, H, D] as a packed view, seqused_k = k_lens; one sequence without a query, one
    without a used key."""
    D, Hq, Hkv, S_pad = 128, 8, 2, 512
    lq = [300, 0, 700, 257, 64]
    lk = [77, 130, 512, 0, 333]
    q, k, v = _offset_packed(7, dtype, lq, [S_pad] * len(lk), Hq, Hkv, D)
    starts = [S_pad * i for i in range(len(lk))]
    out, lse, mean, max_corr = _check_varlen(q, k, v, lq, starts, lk, causal=causal, fp8="e4m3", numerics="compiled", seqused=True, sm_scale=0.11)
    assert max_corr > 1.0
    k2, v2 = k.clone(), v.clone()
    for b, m in zip(starts, lk):
        k2[b + m:b + S_pad], v2[b + m:b + S_pad] = pad_value, pad_value
    cu_q, cu_k = _cu(lq), torch.tensor(starts + [S_pad * len(lk)], dtype=torch.int32, device=DEV)
    used = torch.tensor(lk, dtype=torch.int32, device=DEV)
    res = _native.fp8_quant_attention_varlen(q, k2, v2, cu_q, cu_k, used, is_causal=causal, sm_scale=0.11, smooth_k=True, return_lse=True, return_quant=True)
    assert _same_bits(res[0], out) and _same_bits(res[1], lse) and torch.equal(res[-1], mean), "keys beyond seqused_k influence no output bit"
    assert not torch.isnan(res[0]).any() and not torch.isnan(res[-1]).any()


def test_varlen_mean_is_deterministic_across_calls_and_graph_replay():
    lens = [4097, 1, 1000]
    q, k, v = _offset_packed(11, torch.bfloat16, lens, lens, 4, 4, 128)
    cu = _cu(lens)
    call = lambda: _native.fp8_quant_attention_varlen(q, k, v, cu, cu, None, smooth_k=True, return_quant=True)[-1]
    m1 = call()
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


def test_varlen_a_constant_added_to_some_channels_changes_nothing_but_the_mean():
    """fp16 keys that are multiples of 2^-4 within +-4, every L_i a power of two: every partial sum, the division by L_i and k - m are exact
    in fp32 whatever the summation order -- so +8 on every key of some channels must leave k8, scale_k and out bit for bit as they were."""
    torch.manual_seed(4)
    lens, H, D = [1024, 64, 256, 2048], 2, 128
    total = sum(lens)
    q, v = (torch.randn(total, H, D).to(torch.float16).to(DEV) for _ in range(2))
    k = (torch.randint(-64, 65, (total, H, D)).float() / 16).to(torch.float16)
    shift = torch.zeros(D)
    shift[[3, 17, 64, 100]] = 8.0
    k2 = (k.float() + shift).to(torch.float16)
    assert torch.equal(k2.float(), k.float() + shift)
    cu = _cu(lens)
    r1 = _native.fp8_quant_attention_varlen(q, k.to(DEV), v, cu, cu, None, smooth_k=True, return_quant=True)
    r2 = _native.fp8_quant_attention_varlen(q, k2.to(DEV), v, cu, cu, None, smooth_k=True, return_quant=True)
    a = 0
    for i, n in enumerate(lens):
        assert torch.equal(r1[-1][i].cpu(), k[a:a + n].double().mean(0).float()), "the mean of such keys is exact"
        a += n
    assert torch.equal(r2[-1] - r1[-1], shift.to(DEV).expand(len(lens), H, D))
    assert torch.equal(r1[3], r2[3]), "scale_k"
    for i, (b, n) in enumerate(zip(np.cumsum([0] + lens)[:-1], lens)):   # (the images only: the gaps between them are never written)
        assert np.array_equal(_k8_of_sequence(r1[2].cpu().numpy(), i, int(b), n, H, D), _k8_of_sequence(r2[2].cpu().numpy(), i, int(b), n, H, D))
    assert _same_bits(r1[0], r2[0])


def test_varlen_graph_replay_follows_rewritten_tables():
    D, Hq, Hkv, S_pad = 128, 4, 2, 640
    lq1, lk1 = [300, 200, 524], [640, 100, 333]
    lq2, lk2 = [100, 0, 924], [65, 640, 0]
    q, k, v = _offset_packed(13, torch.bfloat16, lq1, [S_pad] * 3, Hq, Hkv, D)
    cu_q, used = _cu(lq1), torch.tensor(lk1, dtype=torch.int32, device=DEV)
    cu_k = torch.arange(4, dtype=torch.int32, device=DEV) * S_pad
    f = lambda: _varlen(q, k, v, cu_q, cu_k, 1024, S_pad, seqused_k=used, return_lse=True, smooth_k=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, lse = f()
    g.replay()
    torch.cuda.synchronize()
    want, want_lse = f()
    assert _same_bits(out, want) and _same_bits(lse, want_lse)
    cu_q.copy_(_cu(lq2))
    used.copy_(torch.tensor(lk2, dtype=torch.int32, device=DEV))
    g.replay()
    torch.cuda.synchronize()
    want, want_lse = f()
    assert _same_bits(out, want) and _same_bits(lse, want_lse), "a replay must follow the new tables"
    assert not want[100:].any() and (want_lse[:, 100:] == -math.inf).all()


def test_varlen_torch_compile_fullgraph_gives_the_eager_bits_and_the_flag_off_is_the_plain_call():
    lens = [300, 65, 1000]
    q, k, v = _offset_packed(17, torch.bfloat16, lens, lens, 4, 2, 128)
    cu = _cu(lens)
    assert qa.config.attention.smooth_k is False
    plain = _varlen(q, k, v, cu, cu, 1000, 1000, causal=True, return_lse=True)
    off = _varlen(q, k, v, cu, cu, 1000, 1000, causal=True, return_lse=True, smooth_k=False)
    on = _varlen(q, k, v, cu, cu, 1000, 1000, causal=True, return_lse=True, smooth_k=True)
    assert _same_bits(plain[0], off[0]) and _same_bits(plain[1], off[1])
    assert not _same_bits(plain[0], on[0])
    with qa.config.patch({"attention.smooth_k": True}):
        cfg = _varlen(q, k, v, cu, cu, 1000, 1000, causal=True, return_lse=True)
        assert _same_bits(cfg[0], on[0]) and _same_bits(cfg[1], on[1])
        assert _same_bits(_varlen(q, k, v, cu, cu, 1000, 1000, causal=True, smooth_k=False), plain[0])
    torch._dynamo.reset()

    def f(q, k, v, cu):
        return qa.fp8_attn_varlen_func(q * 1.0, k, v, cu, cu, 1000, 1000, causal=True, return_lse=True)

    with qa.config.patch({"attention.smooth_k": True}):   # (baked in at trace time)
        got = torch.compile(f, fullgraph=True, backend="aot_eager")(q, k, v, cu)
    assert _same_bits(got[0], on[0]) and _same_bits(got[1], on[1])
    torch._dynamo.reset()


# ---- block-sparse ------------------------------------------------------------------------------------------------------------------
def _offset_dense(seed, dtype, B, Hq, Hkv, Sq, Skv, D, sigma=16.0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Hq, Sq, D, generator=g)
    k = torch.randn(B, Hkv, Skv, D, generator=g) + sigma * torch.randn(B, Hkv, 1, D, generator=g)
    v = torch.randn(B, Hkv, Skv, D, generator=g)
    return q.to(dtype).to(DEV), k.to(dtype).to(DEV), v.to(dtype).to(DEV)


def _random_mask(B, H, Sq, Skv, density, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, H, _cdiv(Sq, NB), _cdiv(Skv, NB), generator=g) < density).to(DEV)


def _band_mask(B, H, Sq, Skv, width=1):
    nq, nk = _cdiv(Sq, NB), _cdiv(Skv, NB)
    i = torch.arange(nq, device=DEV)[:, None].float() * nk / nq
    j = torch.arange(nk, device=DEV)[None, :].float()
    return ((j - i).abs() <= width).expand(B, H, nq, nk).clone()


BS_CASES = [   # D, dtype, fp8, B, Hq, Hkv, Sq, Skv, mask, scale
    (64, torch.bfloat16, "e4m3", 2, 2, 2, 1000, 999, "rand0.5", None),
    (64, torch.float16, "e5m2", 1, 2, 1, 256, 3000, "rand0.1", 0.07),
    (64, torch.bfloat16, "e4m3", 1, 4, 2, 1000, 999, "band", None),
    (128, torch.bfloat16, "e4m3", 1, 8, 2, 1000, 999, "band", None),
    (128, torch.float16, "e5m2", 2, 2, 2, 256, 3000, "rand0.5", 0.05),
    (128, torch.float16, "e4m3", 1, 4, 2, 1000, 999, "rand0.1", None),
    (256, torch.bfloat16, "e5m2", 1, 2, 1, 1000, 999, "rand0.5", None),
    (256, torch.float16, "e4m3", 1, 2, 2, 256, 3000, "band", 0.1),
    (256, torch.bfloat16, "e4m3", 1, 4, 2, 256, 3000, "rand0.1", None),
]


@pytest.mark.parametrize("D,dtype,fp8,B,Hq,Hkv,Sq,Skv,kind,scale", BS_CASES)
def test_block_sparse_operands_are_the_dense_smoothing_entrys_and_every_query_block_the_gathered_call(D, dtype, fp8, B, Hq, Hkv, Sq, Skv, kind, scale):
    q, k, v = _offset_dense(D + Sq + Hq, dtype, B, Hq, Hkv, Sq, Skv, D)
    mask = _band_mask(B, Hq, Sq, Skv) if kind == "band" else _random_mask(B, Hq, Sq, Skv, float(kind[4:]), D + Skv)
    sm_scale = 0.0 if scale is None else scale
    out, lse, q8, k8, sq, sk, mean = _native.fp8_block_sparse_attention(q, k, v, mask, fp8_dtype=TDT[fp8], sm_scale=sm_scale, smooth_k=True,
                                                                        return_lse=True, return_quant=True)
    assert _same_bits(out, _native.fp8_block_sparse_attention(q, k, v, mask, fp8_dtype=TDT[fp8], sm_scale=sm_scale, smooth_k=True))
    dense = _native.fp8_quant_attention_forward(q, k, v, is_causal=False, scaling="head-wise", fp8_dtype=TDT[fp8], smooth_k=True, return_quant=True)[-1]
    assert torch.equal(mean, dense["k_mean"]) and torch.equal(sk, dense["scale_k"]) and torch.equal(k8, dense["k8"])
    k8r = unpack_frag(k8.cpu().numpy(), _native.LAYOUT_KFRAG, B, Hkv, Skv, D)
    want8, want_scale = restate_quantiser(k.cpu(), mean.cpu(), "head-wise", fp8, "compiled")
    assert np.array_equal(k8r[:, :, :Skv], want8) and np.array_equal(sk.cpu().numpy(), want_scale) and not k8r[:, :, Skv:].any()
    k8t = torch.from_numpy(np.ascontiguousarray(k8r[:, :, :Skv])).to(DEV).view(TDT[fp8])
    sm = scale if scale is not None else 1.0 / math.sqrt(D)
    corr = sm * (q.double() * mean.double().repeat_interleave(Hq // Hkv, dim=1)[:, :, None, :]).sum(-1)   # [B, Hq, Sq]
    m = mask.cpu()
    memo, worst, empty = {}, 0.0, 0
    for b in range(B):
        for h in range(Hq):
            hk = h // (Hq // Hkv)
            for i in range(m.shape[2]):
                r = slice(NB * i, min(NB * i + NB, Sq))
                js = tuple(m[b, h, i].nonzero().flatten().tolist())
                if not js:
                    empty += 1
                    assert not out[b, h, r].any() and (lse[b, h, r] == -math.inf).all(), "an empty query block: zero rows, LSE -inf"
                    continue
                if (b, h, js) not in memo:
                    idx = torch.cat([torch.arange(NB * j, min(NB * j + NB, Skv)) for j in js]).to(DEV)
                    memo[(b, h, js)] = _native.fp8_attention_forward_rowmajor(
                        q8[b:b + 1, h:h + 1], k8t[b:b + 1, hk:hk + 1, idx], v[b:b + 1, hk:hk + 1, idx], sq[b:b + 1, h:h + 1], sk[b:b + 1, hk:hk + 1],
                        is_causal=False, pv_16bit=True, sm_scale=sm_scale, return_lse=True)
                o, l = memo[(b, h, js)]
                assert _same_bits(out[b, h, r], o[0, 0, r]), (b, h, i)
                worst = max(worst, (lse[b, h, r].double() - (l[0, 0, r].double() + corr[b, h, r])).abs().max().item())
    print(f"D {D} {dtype} {fp8} {kind}: lse max err {worst:.5f}, max |correction| {corr.abs().max().item():.2f}, empty query blocks {empty}")
    assert worst < LSE_TOL, worst
    assert corr.abs().max().item() > 1.0, "the inputs must make the correction matter"


@pytest.mark.parametrize("D", [64, 128, 256])
def test_block_sparse_all_true_mask_equals_the_varlen_smoothing_call_on_one_sequence_per_batch_element(D):
    B, H, S = 2, 4, 1000
    q, k, v = _offset_dense(D, torch.bfloat16, B, H, H, S, S, D)
    mask = torch.ones(1, 1, 1, 1, dtype=torch.bool, device=DEV)
    out, lse = _sparse(q, k, v, mask, return_lse=True, smooth_k=True)
    pk = lambda t: t.transpose(1, 2).reshape(B * S, H, D).contiguous()
    cu = _cu([S] * B)
    vo, vl = _varlen(pk(q), pk(k), pk(v), cu, cu, S, S, return_lse=True, smooth_k=True)
    assert _same_bits(out, vo.view(B, S, H, D).transpose(1, 2))
    assert (lse - vl.view(H, B, S).transpose(0, 1)).abs().max().item() < LSE_TOL   # (the two corrections add in different orders)


def test_block_sparse_graph_replay_follows_a_rewritten_mask_and_compile_gives_the_eager_bits():
    B, Hq, Hkv, S, D = 1, 4, 2, 1000, 128
    q, k, v = _offset_dense(23, torch.bfloat16, B, Hq, Hkv, S, S, D)
    mask = _random_mask(B, Hq, S, S, 0.5, 1)
    mask[:, 0, 1] = False
    f = lambda: _sparse(q, k, v, mask, return_lse=True, smooth_k=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, lse = f()
    g.replay()
    torch.cuda.synchronize()
    want, want_lse = f()
    assert _same_bits(out, want) and _same_bits(lse, want_lse)
    assert not want[0, 0, 128:256].any() and (want_lse[0, 0, 128:256] == -math.inf).all()
    mask.copy_(_random_mask(B, Hq, S, S, 0.3, 2))
    g.replay()
    torch.cuda.synchronize()
    want2, want_lse2 = f()
    assert _same_bits(out, want2) and _same_bits(lse, want_lse2) and not _same_bits(want, want2), "a replay must follow the new mask"
    # flag off: the plain call; flag on through the config: the smoothing entry's bits
    assert qa.config.attention.smooth_k is False
    plain = _sparse(q, k, v, mask, return_lse=True)
    off = _sparse(q, k, v, mask, return_lse=True, smooth_k=False)
    assert _same_bits(plain[0], off[0]) and _same_bits(plain[1], off[1]) and not _same_bits(plain[0], want2)
    with qa.config.patch({"attention.smooth_k": True}):
        cfg = _sparse(q, k, v, mask, return_lse=True)
    assert _same_bits(cfg[0], want2) and _same_bits(cfg[1], want_lse2)
    torch._dynamo.reset()

    def fc(q, k, v, mask):
        return qa.fp8_block_sparse_attn_func(q * 1.0, k, v, mask, return_lse=True)

    with qa.config.patch({"attention.smooth_k": True}):   # (baked in at trace time)
        got = torch.compile(fc, fullgraph=True, backend="aot_eager")(q, k, v, mask)
    assert _same_bits(got[0], want2) and _same_bits(got[1], want_lse2)
    torch._dynamo.reset()


# ---- accuracy end to end -----------------------------------------------------------------------------------------------------------
def _sdpa64(q, k, v, mask=None):
    """fp64 attention of [H, L, D] device tensors (GQA by repetition); rows without a key -> 0"""
    rep = q.shape[0] // k.shape[0]
    k, v = (t.double().repeat_interleave(rep, dim=0) for t in (k, v))
    s = q.double() @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if mask is not None:
        s = s.masked_fill(~mask, -math.inf)
    return torch.softmax(s, dim=-1).nan_to_num(0.0) @ v


def _rmse(a, b):
    return (a.double() - b.double()).pow(2).mean().sqrt().item()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_end_to_end_varlen_offset_keys_clear_the_bar_with_smoothing(seed, dtype):
    """A DiT-like packed batch: 4 sequences of 512 .. 2048 tokens, H 8, D 128, keys with a sigma = 16 channel offset per sequence; RMSE
    against fp64 SDPA on the unquantised inputs, per sequence.
    Measured on the MI355X: see profiles/smooth_k_packed/pytest_gpu_figures.log."""
    lens, H, D = [2048, 512, 1536, 1024], 8, 128
    q, k, v = _offset_packed(seed, dtype, lens, lens, H, H, D)
    cu = _cu(lens)
    on = _varlen(q, k, v, cu, cu, max(lens), max(lens), smooth_k=True)
    off = _varlen(q, k, v, cu, cu, max(lens), max(lens), smooth_k=False)
    ref = torch.cat([_sdpa64(q[a:b].transpose(0, 1), k[a:b].transpose(0, 1), v[a:b].transpose(0, 1)).transpose(0, 1)
                     for a, b in zip(cu[:-1].tolist(), cu[1:].tolist())])
    r_on, r_off = _rmse(on, ref), _rmse(off, ref)
    print(f"varlen seed {seed} {dtype}: rmse smooth_k on {r_on:.5f} off {r_off:.5f}")
    assert r_on < BAR, r_on
    assert r_on < r_off, (r_on, r_off)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_end_to_end_block_sparse_offset_keys_clear_the_bar_with_smoothing(seed, dtype):
    """B 1, H 8, S 2048, D 128, a band mask of width 2 (5 of 16 key blocks per query block), keys with a sigma = 16 channel offset; RMSE
    against fp64 SDPA on the unquantised inputs over the listed keys.
    Measured on the MI355X: see profiles/smooth_k_packed/pytest_gpu_figures.log."""
    B, H, S, D = 1, 8, 2048, 128
    q, k, v = _offset_dense(seed, dtype, B, H, H, S, S, D)
    mask = _band_mask(B, H, S, S, width=2)
    on = _sparse(q, k, v, mask, smooth_k=True)
    off = _sparse(q, k, v, mask, smooth_k=False)
    em = mask.repeat_interleave(NB, dim=2)[:, :, :S].repeat_interleave(NB, dim=3)[..., :S]
    ref = _sdpa64(q[0], k[0], v[0], em[0])
    r_on, r_off = _rmse(on[0], ref), _rmse(off[0], ref)
    print(f"block-sparse seed {seed} {dtype}: rmse smooth_k on {r_on:.5f} off {r_off:.5f}")
    assert r_on < BAR, r_on
    assert r_on < r_off, (r_on, r_off)

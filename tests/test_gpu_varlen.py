"""-m gpu: packed variable-length FP8 attention (quantumattention_amd.fp8_attn_varlen_func, include/qattn_varlen.h) on the MI355X.

The central property is bit identity: every sequence's rows and LSE columns equal the per-sequence dense path -- dynamically_quantize_fp8
of the sequence's q and (used) k, then fp8_attention_forward_rowmajor(..., pv_16bit=True, return_lse=True) -- bit for bit.  Besides: the
quantiser bytes against dynamically_quantize_fp8, seqused_k on padded K / V, empty sequences, an independent fp64 oracle, graph capture with
rewritten tables, torch.compile, and element offsets beyond 2^31."""
import math

import numpy as np
import pytest
import torch

import oracle
import quantumattention_amd as qa
from quantumattention_amd import _native
from tests.gpu_utils import FMT, TDT, bits8, bits16, fmt16, unpack_frag

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cu(lengths):
    return torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32, device=DEV)


def _seq(t, a, n):
    """rows a .. a + n of a packed [total, H, D] tensor as the [1, H, n, D] view the dense entries take"""
    return t[a:a + n].transpose(0, 1)[None]


def _dense_loop(q, k, v, lq, lk, *, causal, sm_scale=0.0, starts_k=None):
    """the per-sequence dense path: (out [total_q, Hq, D], lse [Hq, total_q]); sequences without a key give zero rows and -inf"""
    total_q, Hq, D = q.shape
    out = torch.zeros_like(q)
    lse = torch.full((Hq, total_q), -math.inf, dtype=torch.float32, device=DEV)
    a = 0
    starts_k = starts_k if starts_k is not None else list(np.cumsum([0] + list(lk))[:-1])
    for n, m, b in zip(lq, lk, starts_k):
        if n and m:
            q8, sq = qa.dynamically_quantize_fp8(_seq(q, a, n), reduction_dim=[2, 3])
            k8, sk = qa.dynamically_quantize_fp8(_seq(k, b, m), reduction_dim=[2, 3])
            o, l = _native.fp8_attention_forward_rowmajor(q8, k8, _seq(v, b, m), sq, sk, is_causal=causal, pv_16bit=True, sm_scale=sm_scale,
                                                          return_lse=True)
            out[a:a + n] = o[0].transpose(0, 1)
            lse[:, a:a + n] = l[0]
        a += n
    return out, lse


def _same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32),
                       y.contiguous().view(torch.int16 if y.element_size() == 2 else torch.int32))


def _rand(n, H, D, dtype, g):
    return torch.randn(n, H, D, generator=g, device=DEV, dtype=torch.float32).to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("fp8", ["e4m3", "e5m2"])
@pytest.mark.parametrize("numerics", ["compiled", "eager"])
def test_quantiser_bytes_and_scales_equal_dynamically_quantize_fp8_per_sequence(dtype, fp8, numerics):
    g = torch.Generator(device=DEV).manual_seed(1)
    D, Hq, Hkv = 128, 4, 2
    lq, lk, pad = [1, 63, 64, 65, 200], [70, 1, 64, 129, 5], 3
    q = _rand(sum(lq), Hq, D, dtype, g) * 3
    kp = _rand(sum(lk) + pad * len(lk), Hkv, D, dtype, g)
    starts = list(np.cumsum([0] + [n + pad for n in lk])[:-1])
    for b, n in zip(starts, lk):
        kp[b + n:b + n + pad] = 1e4 if dtype == torch.float16 else 1e30   # unused keys: must not reach the scale
    cu_k = torch.tensor(starts + [kp.shape[0]], dtype=torch.int32, device=DEV)
    used = torch.tensor(lk, dtype=torch.int32, device=DEV)
    _, q8, k8, sq, sk = _native.fp8_quant_attention_varlen(q, kp, kp, _cu(lq), cu_k, used, fp8_dtype=TDT[fp8], numerics=numerics,
                                                          return_quant=True)
    q8, k8 = bits8(q8), bits8(k8)
    with qa.config.patch({"attention.fp8_format": fp8, "attention.quant_numerics": numerics}):
        a = 0
        for i, (n, m, b) in enumerate(zip(lq, lk, starts)):
            rq, rsq = qa.dynamically_quantize_fp8(_seq(q, a, n), reduction_dim=[2, 3])
            rk, rsk = qa.dynamically_quantize_fp8(_seq(kp, b, m), reduction_dim=[2, 3])
            assert np.array_equal(q8[Hq * D * a:Hq * D * (a + n)], bits8(rq).ravel()), i
            mp = (m + 63) // 64 * 64
            off = Hkv * D * (b + 64 * i)
            kr = unpack_frag(k8[off:off + Hkv * mp * D], _native.LAYOUT_KFRAG, 1, Hkv, m, D)
            assert np.array_equal(kr[:, :, :m], bits8(rk)), i
            assert not kr[:, :, m:].any()   # the last chunk's padding: zeros, as the dense pack
            assert torch.equal(sq[i], rsq[0]) and torch.equal(sk[i], rsk[0]), i
            a += n


def test_quantiser_reads_strided_slices_of_a_packed_qkv_projection():
    g = torch.Generator(device=DEV).manual_seed(2)
    lens, H, D = [33, 300, 64], 4, 64
    qkv = _rand(sum(lens), 3 * H, D, torch.bfloat16, g).view(sum(lens), 3, H, D)
    q, k, v = qkv.unbind(1)
    assert not q.is_contiguous() and _native.varlen_strided_ok(q)
    cu = _cu(lens)
    res = _native.fp8_quant_attention_varlen(q, k, v, cu, cu, None, return_lse=True, return_quant=True)
    dense = _native.fp8_quant_attention_varlen(q.contiguous(), k.contiguous(), v.contiguous(), cu, cu, None, return_lse=True, return_quant=True)
    for j in (0, 1, 2, 4, 5):   # (k8: the KFRAG images only -- the buffer's gaps between them are never written)
        assert torch.equal(res[j], dense[j]), j
    a = 0
    for i, n in enumerate(lens):
        rq, rsq = qa.dynamically_quantize_fp8(_seq(q, a, n), reduction_dim=[2, 3])
        assert np.array_equal(bits8(res[2])[H * D * a:H * D * (a + n)], bits8(rq).ravel()) and torch.equal(res[4][i], rsq[0])
        a += n


LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1000, 4097]


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("causal", [False, True])
def test_bit_for_bit_against_the_per_sequence_dense_path(D, causal):
    g = torch.Generator(device=DEV).manual_seed(D + causal)
    for dtype, (Hq, Hkv) in ((torch.bfloat16, (4, 4)), (torch.float16, (8, 2))):
        lens = LENGTHS[::-1] if dtype == torch.float16 else LENGTHS
        q, k, v = (_rand(sum(lens), h, D, dtype, g) for h in (Hq, Hkv, Hkv))
        cu = _cu(lens)
        out, lse = qa.fp8_attn_varlen_func(q, k, v, cu, cu, max(lens), max(lens), causal=causal, return_lse=True)
        ref, ref_lse = _dense_loop(q, k, v, lens, lens, causal=causal)
        assert _same_bits(out, ref), (dtype, Hq, Hkv)
        assert _same_bits(lse, ref_lse), (dtype, Hq, Hkv)
        assert torch.equal(qa.fp8_attn_varlen_func(q, k, v, cu, cu, max(lens), max(lens), causal=causal), out)


@pytest.mark.parametrize("causal", [False, True])
def test_cross_attention_with_other_key_lengths_and_an_explicit_scale(causal):
    g = torch.Generator(device=DEV).manual_seed(7)
    lq, lk, D = [300, 1, 1000, 64, 257], [77, 520, 64, 1300, 1], 128
    q, k, v = _rand(sum(lq), 8, D, torch.bfloat16, g), _rand(sum(lk), 2, D, torch.bfloat16, g), _rand(sum(lk), 2, D, torch.bfloat16, g)
    for scale in (None, 0.3):
        out, lse = qa.fp8_attn_varlen_func(q, k, v, _cu(lq), _cu(lk), 1000, 1300, softmax_scale=scale, causal=causal, return_lse=True)
        ref, ref_lse = _dense_loop(q, k, v, lq, lk, causal=causal, sm_scale=0.0 if scale is None else scale)
        assert _same_bits(out, ref) and _same_bits(lse, ref_lse), scale


def test_seqused_k_on_padded_kv_equals_the_trimmed_call_whatever_the_padding_holds():
    g = torch.Generator(device=DEV).manual_seed(3)
    B, S_pad, H, D = 4, 512, 8, 128
    k_lens = [512, 100, 1, 333]
    lq = [1024, 700, 64, 1500]
    q = _rand(sum(lq), H, D, torch.bfloat16, g)
    kp, vp = (torch.randn(B, S_pad, H, D, generator=g, device=DEV).bfloat16() for _ in range(2))
    cu_k = torch.arange(B + 1, dtype=torch.int32, device=DEV) * S_pad
    used = torch.tensor(k_lens, dtype=torch.int32, device=DEV)
    kt = torch.cat([kp[i, :n] for i, n in enumerate(k_lens)])
    vt = torch.cat([vp[i, :n] for i, n in enumerate(k_lens)])
    want = qa.fp8_attn_varlen_func(q, kt, vt, _cu(lq), _cu(k_lens), 1500, 512, return_lse=True)
    for fill in (None, 1e4, float("nan")):
        k2, v2 = kp.clone(), vp.clone()
        if fill is not None:
            for i, n in enumerate(k_lens):
                k2[i, n:], v2[i, n:] = fill, fill
        got = qa.fp8_attn_varlen_func(q, k2.view(B * S_pad, H, D), v2.view(B * S_pad, H, D), _cu(lq), cu_k, 1500, S_pad, seqused_k=used,
                                      return_lse=True)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), fill


def test_empty_sequences_are_defined():
    g = torch.Generator(device=DEV).manual_seed(4)
    lq, lk, H, D = [300, 0, 257, 40], [500, 9, 0, 70], 4, 64
    q, k, v = _rand(sum(lq), H, D, torch.bfloat16, g), _rand(sum(lk), H, D, torch.bfloat16, g), _rand(sum(lk), H, D, torch.bfloat16, g)
    for causal in (False, True):
        out, lse = qa.fp8_attn_varlen_func(q, k, v, _cu(lq), _cu(lk), 300, 500, causal=causal, return_lse=True)
        ref, ref_lse = _dense_loop(q, k, v, lq, lk, causal=causal)
        assert _same_bits(out, ref) and _same_bits(lse, ref_lse)
        assert (out[300:557] == 0).all() and (lse[:, 300:557] == -math.inf).all()


@pytest.mark.parametrize("causal", [False, True])
def test_every_row_within_the_v16_bound_of_the_fp64_oracle_on_a_dit_batch(causal):
    g = torch.Generator(device=DEV).manual_seed(5)
    lens, H, D = [1024, 2600, 1800, 3100, 1500, 2200], 8, 128
    q, k, v = (_rand(sum(lens), H, D, torch.bfloat16, g) for _ in range(3))
    out = qa.fp8_attn_varlen_func(q, k, v, _cu(lens), _cu(lens), max(lens), max(lens), causal=causal).float().cpu().numpy()
    a, worst = 0, 0.0
    for n in lens:
        q8, sq = qa.dynamically_quantize_fp8(_seq(q, a, n), reduction_dim=[2, 3])
        k8, sk = qa.dynamically_quantize_fp8(_seq(k, a, n), reduction_dim=[2, 3])
        ref = oracle.attention_forward(bits8(q8), bits8(k8), bits16(_seq(v, a, n)), FMT["e4m3"], FMT["e4m3"], fmt16(torch.bfloat16),
                                       sq.cpu().numpy(), sk.cpu().numpy(), None, causal=causal)[0].transpose(1, 0, 2)
        ratio = np.abs(out[a:a + n] - ref) / (2.0 ** -7 * np.maximum(1.0, np.abs(ref)))
        worst = max(worst, float(ratio.max()))
        a += n
    assert worst < 1.0, worst


def test_graph_replay_follows_rewritten_tables():
    g = torch.Generator(device=DEV).manual_seed(6)
    H, D, total = 8, 128, 1200
    q, k, v = (_rand(total, H, D, torch.bfloat16, g) for _ in range(3))
    cu_q, cu_k = _cu([100, 700, 400]), _cu([300, 200, 700])
    call = lambda: qa.fp8_attn_varlen_func(q, k, v, cu_q, cu_k, 700, 700, causal=True, return_lse=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = call()
    cu_q.copy_(_cu([650, 50, 500]))
    cu_k.copy_(_cu([1, 1000, 199]))
    graph.replay()
    torch.cuda.synchronize()
    want = call()
    assert _same_bits(out, want[0]) and _same_bits(lse, want[1])
    ref, ref_lse = _dense_loop(q, k, v, [650, 50, 500], [1, 1000, 199], causal=True)
    assert _same_bits(out, ref) and _same_bits(lse, ref_lse)


def test_torch_compile_fullgraph_gives_the_eager_bits():
    g = torch.Generator(device=DEV).manual_seed(8)
    lens, H, D = [200, 1000, 77], 8, 128
    q, k, v = (_rand(sum(lens), H, D, torch.float16, g) for _ in range(3))
    cu = _cu(lens)

    def f(q, k, v, cu):
        return qa.fp8_attn_varlen_func(q * 2, k, v, cu, cu, 1000, 1000, causal=True, return_lse=True)

    torch._dynamo.reset()
    got = torch.compile(f, fullgraph=True)(q, k, v, cu)
    want = f(q, k, v, cu)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])


def test_element_offsets_beyond_2_to_the_31():
    B, L, H, D = 2048, 1024, 16, 128
    g = torch.Generator(device=DEV).manual_seed(9)
    total = B * L
    assert H * D * total > 2 ** 31
    q, k, v = (torch.randn(total, H, D, generator=g, device=DEV, dtype=torch.bfloat16) for _ in range(3))
    cu = torch.arange(B + 1, dtype=torch.int32, device=DEV) * L
    out, lse = qa.fp8_attn_varlen_func(q, k, v, cu, cu, L, L, causal=True, return_lse=True)
    for i in (0, B // 2, B - 1):
        a = i * L
        ref, ref_lse = _dense_loop(q[a:a + L], k[a:a + L], v[a:a + L], [L], [L], causal=True)
        assert _same_bits(out[a:a + L], ref) and _same_bits(lse[:, a:a + L], ref_lse), i

"""-m gpu: block-sparse FP8 attention (quantumattention_amd.fp8_block_sparse_attn_func, include/qattn_block_sparse.h) on the MI355X.

The central property is bit identity: rows 128 i .. 128 i + 127 of every head equal the dense 16-bit-V path -- the whole-tensor
dynamically_quantize_fp8 of q and k, then fp8_attention_forward_rowmajor(..., pv_16bit=True, return_lse=True) on the keys of the blocks that
query block i lists, gathered in ascending order -- bit for bit.  Besides: the dense call under an all-true mask, empty query blocks, NaN /
1e4 in keys nobody lists, broadcast masks, an fp64 oracle, graph replay after rewriting the mask, torch.compile, the eager fallback."""
import math

import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests.gpu_utils import TDT

pytestmark = pytest.mark.gpu
DEV = "cuda"
NB = 128


def _cdiv(a, b):
    return (a + b - 1) // b


def _rand(shape, dtype, g):
    return torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32).to(dtype)


def _same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32),
                       y.contiguous().view(torch.int16 if y.element_size() == 2 else torch.int32))


def _random_mask(B, H, Sq, Skv, density, g):
    return torch.rand(B, H, _cdiv(Sq, NB), _cdiv(Skv, NB), generator=g, device=DEV) < density


def _band_mask(B, H, Sq, Skv, width=1, global_cols=0):
    """|j - i nKB / nQB| <= width, plus the first `global_cols` key blocks for every query block"""
    nq, nk = _cdiv(Sq, NB), _cdiv(Skv, NB)
    i = torch.arange(nq, device=DEV)[:, None].float() * nk / nq
    j = torch.arange(nk, device=DEV)[None, :].float()
    m = ((j - i).abs() <= width) | (j < global_cols)
    return m.expand(B, H, nq, nk).clone()


def _gathered_reference(q, k, v, mask, *, sm_scale=0.0):
    """per (b, h, query block i): the dense 16-bit-V call on the whole-tensor q8 and on k8 / v gathered at the keys of the blocks i lists"""
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    q8, sq = qa.dynamically_quantize_fp8(q, reduction_dim=[2, 3])
    k8, sk = qa.dynamically_quantize_fp8(k, reduction_dim=[2, 3])
    m = mask.expand(B, Hq, _cdiv(Sq, NB), _cdiv(Skv, NB)).cpu()
    out = torch.zeros_like(q)
    lse = torch.full((B, Hq, Sq), -math.inf, dtype=torch.float32, device=DEV)
    memo = {}
    for b in range(B):
        for h in range(Hq):
            hk = h // (Hq // Hkv)
            for i in range(m.shape[2]):
                js = tuple(m[b, h, i].nonzero().flatten().tolist())
                if not js:
                    continue
                if (b, h, js) not in memo:
                    idx = torch.cat([torch.arange(NB * j, min(NB * j + NB, Skv)) for j in js]).to(DEV)
                    memo[(b, h, js)] = _native.fp8_attention_forward_rowmajor(
                        q8[b:b + 1, h:h + 1], k8[b:b + 1, hk:hk + 1, idx], v[b:b + 1, hk:hk + 1, idx], sq[b:b + 1, h:h + 1], sk[b:b + 1, hk:hk + 1],
                        is_causal=False, pv_16bit=True, sm_scale=sm_scale, return_lse=True)
                o, l = memo[(b, h, js)]
                r = slice(NB * i, min(NB * i + NB, Sq))
                out[b, h, r] = o[0, 0, r]
                lse[b, h, r] = l[0, 0, r]
    return out, lse


CASES = [   # D, dtype, fp8, B, Hq, Hkv, Sq, Skv, mask, scale
    (64, torch.bfloat16, "e4m3", 2, 2, 2, 1000, 999, "rand0.5", None),
    (64, torch.float16, "e4m3", 1, 2, 1, 4097, 4097, "rand0.1", None),
    (64, torch.bfloat16, "e5m2", 1, 2, 2, 256, 3000, "band", 0.07),
    (128, torch.bfloat16, "e4m3", 1, 8, 2, 1000, 999, "band", None),
    (128, torch.float16, "e5m2", 2, 2, 2, 256, 3000, "rand0.5", 0.05),
    (128, torch.bfloat16, "e4m3", 1, 2, 2, 4097, 4097, "rand0.1", None),
    (128, torch.float16, "e4m3", 1, 8, 2, 4097, 4097, "band", None),
    (256, torch.bfloat16, "e5m2", 1, 2, 1, 1000, 999, "rand0.5", None),
    (256, torch.float16, "e4m3", 1, 2, 2, 256, 3000, "band", 0.1),
    (256, torch.bfloat16, "e4m3", 1, 2, 2, 4097, 4097, "rand0.1", None),
]


@pytest.mark.parametrize("D,dtype,fp8,B,Hq,Hkv,Sq,Skv,kind,scale", CASES)
def test_every_query_block_equals_the_gathered_dense_call(D, dtype, fp8, B, Hq, Hkv, Sq, Skv, kind, scale):
    g = torch.Generator(device=DEV).manual_seed(D + Sq + Skv + Hq)
    q = _rand((B, Hq, Sq, D), dtype, g)
    k = _rand((B, Hkv, Skv, D), dtype, g)
    v = _rand((B, Hkv, Skv, D), dtype, g)
    mask = _band_mask(B, Hq, Sq, Skv) if kind == "band" else _random_mask(B, Hq, Sq, Skv, float(kind[4:]), g)
    with qa.config.patch({"attention.fp8_format": fp8}):
        out, lse = qa.fp8_block_sparse_attn_func(q, k, v, mask, scale=scale, return_lse=True)
        ref, ref_lse = _gathered_reference(q, k, v, mask, sm_scale=0.0 if scale is None else scale)
        # the quantiser: the bytes and scales of dynamically_quantize_fp8 on the whole tensors
        _, q8, k8, sq, sk = _native.fp8_block_sparse_attention(q, k, v, mask, fp8_dtype=TDT[fp8], return_quant=True)
        rq, rsq = qa.dynamically_quantize_fp8(q, reduction_dim=[2, 3])
        rk, rsk = qa.dynamically_quantize_fp8(k, reduction_dim=[2, 3])
    assert out.dtype == dtype and out.shape == q.shape and lse.shape == (B, Hq, Sq)
    assert torch.equal(q8.view(torch.uint8), rq.view(torch.uint8)) and torch.equal(k8.view(torch.uint8), rk.view(torch.uint8))
    assert torch.equal(sq, rsq) and torch.equal(sk, rsk)
    assert _same_bits(out, ref) and _same_bits(lse, ref_lse)


@pytest.mark.parametrize("D", [64, 128, 256])
def test_all_true_mask_is_the_dense_16bit_v_call(D):
    g = torch.Generator(device=DEV).manual_seed(2)
    B, Hq, Hkv, Sq, Skv = 2, 4, 2, 1000, 999
    q, k, v = _rand((B, Hq, Sq, D), torch.bfloat16, g), _rand((B, Hkv, Skv, D), torch.bfloat16, g), _rand((B, Hkv, Skv, D), torch.bfloat16, g)
    out, lse = qa.fp8_block_sparse_attn_func(q, k, v, torch.ones(1, dtype=torch.bool, device=DEV), return_lse=True)
    q8, sq = qa.dynamically_quantize_fp8(q, reduction_dim=[2, 3])
    k8, sk = qa.dynamically_quantize_fp8(k, reduction_dim=[2, 3])
    ref, ref_lse = _native.fp8_attention_forward_rowmajor(q8, k8, v, sq, sk, is_causal=False, pv_16bit=True, return_lse=True)
    assert _same_bits(out, ref) and _same_bits(lse, ref_lse)


def test_query_blocks_without_keys_give_zero_rows_and_minus_inf():
    g = torch.Generator(device=DEV).manual_seed(3)
    B, H, Sq, Skv, D = 1, 2, 700, 500, 128
    q, k, v = _rand((B, H, Sq, D), torch.bfloat16, g), _rand((B, H, Skv, D), torch.bfloat16, g), _rand((B, H, Skv, D), torch.bfloat16, g)
    mask = _random_mask(B, H, Sq, Skv, 0.6, g)
    mask[:, :, 0] = True
    mask[0, 0, 1] = False    # the second half of workgroup 0 in head 0: nothing
    mask[0, 1, 2:4] = False  # a whole workgroup of head 1: nothing
    out, lse = qa.fp8_block_sparse_attn_func(q, k, v, mask, return_lse=True)
    ref, ref_lse = _gathered_reference(q, k, v, mask)
    assert (out[0, 0, 128:256] == 0).all() and (lse[0, 0, 128:256] == -math.inf).all()
    assert (out[0, 1, 256:512] == 0).all() and (lse[0, 1, 256:512] == -math.inf).all()
    assert _same_bits(out, ref) and _same_bits(lse, ref_lse)
    out, lse = qa.fp8_block_sparse_attn_func(q, k, v, torch.zeros_like(mask), return_lse=True)
    assert (out == 0).all() and (lse == -math.inf).all()


def test_values_of_key_blocks_nobody_lists_change_no_bit():
    g = torch.Generator(device=DEV).manual_seed(4)
    B, Hq, Hkv, Sq, Skv, D = 1, 4, 2, 1000, 1300, 128
    q, k, v = _rand((B, Hq, Sq, D), torch.float16, g), _rand((B, Hkv, Skv, D), torch.float16, g), _rand((B, Hkv, Skv, D), torch.float16, g)
    mask = _random_mask(B, Hq, Sq, Skv, 0.5, g)
    off = [1, 4, 10]   # the last (ragged) block among them
    mask[..., off] = False
    out, lse = qa.fp8_block_sparse_attn_func(q, k, v, mask, return_lse=True)
    v2 = v.clone()
    for n, j in enumerate(off):
        v2[:, :, NB * j:NB * j + NB] = float("nan") if n % 2 == 0 else 1e4
    out2, lse2 = qa.fp8_block_sparse_attn_func(q, k, v2, mask, return_lse=True)
    assert _same_bits(out2, out) and _same_bits(lse2, lse)


def test_broadcast_mask_equals_the_materialised_one():
    g = torch.Generator(device=DEV).manual_seed(5)
    B, Hq, Hkv, Sq, Skv, D = 2, 4, 4, 900, 1100, 64
    q, k, v = _rand((B, Hq, Sq, D), torch.bfloat16, g), _rand((B, Hkv, Skv, D), torch.bfloat16, g), _rand((B, Hkv, Skv, D), torch.bfloat16, g)
    small = _random_mask(1, 1, Sq, Skv, 0.4, g)
    big = small.expand(B, Hq, -1, -1)
    got = qa.fp8_block_sparse_attn_func(q, k, v, big, return_lse=True)
    got2 = qa.fp8_block_sparse_attn_func(q, k, v, small[0, 0], return_lse=True)
    want = qa.fp8_block_sparse_attn_func(q, k, v, big.contiguous(), return_lse=True)
    for a in (got, got2):
        assert _same_bits(a[0], want[0]) and _same_bits(a[1], want[1])


def test_fp64_oracle_on_a_band_plus_global_mask():
    g = torch.Generator(device=DEV).manual_seed(6)
    B, H, S, D = 1, 8, 8192, 128
    q, k, v = (_rand((B, H, S, D), torch.bfloat16, g) for _ in range(3))
    mask = _band_mask(B, H, S, S, width=4, global_cols=2)
    out = qa.fp8_block_sparse_attn_func(q, k, v, mask)
    q8, sq = qa.dynamically_quantize_fp8(q, reduction_dim=[2, 3])
    k8, sk = qa.dynamically_quantize_fp8(k, reduction_dim=[2, 3])
    em = mask[0, 0].repeat_interleave(NB, 0)[:S].repeat_interleave(NB, 1)[:, :S]
    worst = 0.0
    for h in range(H):
        dq = q8[0, h].double() * sq[0, h].double()
        dk = k8[0, h].double() * sk[0, h].double()
        s = (dq @ dk.T) / math.sqrt(D)
        s = s.masked_fill(~em, -math.inf)
        ref = torch.softmax(s, dim=-1) @ v[0, h].double()
        err = ((out[0, h].double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
        worst = max(worst, err)
    assert worst < 2 ** -7, worst


def test_graph_replay_follows_a_rewritten_mask():
    g = torch.Generator(device=DEV).manual_seed(7)
    B, H, S, D = 1, 8, 1500, 128
    q, k, v = (_rand((B, H, S, D), torch.bfloat16, g) for _ in range(3))
    mask = _random_mask(B, H, S, S, 0.3, g)
    call = lambda: qa.fp8_block_sparse_attn_func(q, k, v, mask, return_lse=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = call()
    mask.copy_(_band_mask(B, H, S, S, width=2, global_cols=1))
    graph.replay()
    torch.cuda.synchronize()
    want = call()
    assert _same_bits(out, want[0]) and _same_bits(lse, want[1])
    ref, ref_lse = _gathered_reference(q, k, v, mask)
    assert _same_bits(out, ref) and _same_bits(lse, ref_lse)


def test_torch_compile_fullgraph_gives_the_eager_bits():
    g = torch.Generator(device=DEV).manual_seed(8)
    B, Hq, Hkv, S, D = 2, 8, 2, 1000, 128
    q, k, v = _rand((B, Hq, S, D), torch.float16, g), _rand((B, Hkv, S, D), torch.float16, g), _rand((B, Hkv, S, D), torch.float16, g)
    mask = _random_mask(1, Hq, S, S, 0.3, g)

    def f(q, k, v, mask):
        return qa.fp8_block_sparse_attn_func(q * 2, k, v, mask, scale=0.1, return_lse=True)

    torch._dynamo.reset()
    got = torch.compile(f, fullgraph=True)(q, k, v, mask)
    want = f(q, k, v, mask)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])


def test_eager_fallback_agrees_with_the_kernel():
    g = torch.Generator(device=DEV).manual_seed(9)
    B, Hq, Hkv, Sq, Skv, D = 1, 4, 2, 1000, 1200, 128
    q, k, v = _rand((B, Hq, Sq, D), torch.bfloat16, g), _rand((B, Hkv, Skv, D), torch.bfloat16, g), _rand((B, Hkv, Skv, D), torch.bfloat16, g)
    mask = _random_mask(B, Hq, Sq, Skv, 0.4, g)
    mask[0, 0, 2] = False
    # (the eager definition quantises with the torch quantiser: the kernel's pre-pass runs the same arithmetic under quant_numerics =
    # "eager", so that the two differ by P.V precision only -- with the compiled numerics some fp8 bytes round the other way, 2^-5 on
    # single outputs)
    with qa.config.patch({"attention.quant_numerics": "eager"}):
        out, lse = qa.fp8_block_sparse_attn_func(q, k, v, mask, return_lse=True)
    with qa.config.patch({"attention.force_eager_fallback": True}):
        eo, el = qa.fp8_block_sparse_attn_func(q, k, v, mask, return_lse=True)
    assert (eo[0, 0, 256:384] == 0).all() and (el[0, 0, 256:384] == -math.inf).all()
    err = ((out.double() - eo.double()).abs() / eo.double().abs().clamp_min(1.0)).max().item()
    assert err < 2 ** -7, err
    fin = torch.isfinite(el)
    assert torch.equal(fin, torch.isfinite(lse)) and (lse[fin] - el[fin]).abs().max().item() < 2 ** -7

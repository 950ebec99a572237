"""-m gpu: sliding-window (local) FP8 attention on packed sequences (quantumattention_amd.fp8_attn_varlen_window_func /
fp8_window_attn_func, include/qattn_window.h) on the MI355X.

The reference is built here: per sequence, dynamically_quantize_fp8 of its queries and used keys, de-quantised (q8 * sq, k8 * sk) in fp64,
the window mask r + delta - left <= j <= r + delta + right (delta = L_k - L_q), fp64 softmax, the ORIGINAL 16-bit V.  Bounds: `out` the
project's 16-bit-V bound |got - ref| < 2^-7 max(1, |ref|) (README tolerance rule), the LSE the 4e-3 of include/qattn.h for 16-bit-V rows;
rows whose window holds no key are exactly 0 and -inf.  Besides: bit identity with the packed entry where the window masks nothing or is
the causal mask, V rows nobody attends never read, graph replay, torch.compile, key smoothing, and the dense [B, H, S, D] call shape."""
import math

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests.gpu_utils import TDT, unpack_frag

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_V16 = 2.0 ** -7
LSE_TOL = 4e-3


def _cu(lengths):
    return torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32, device=DEV)


def _seq(t, a, n):
    """rows a .. a + n of a packed [total, H, D] tensor as the [1, H, n, D] view the dense entries take"""
    return t[a:a + n].transpose(0, 1)[None]


def _same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32),
                       y.contiguous().view(torch.int16 if y.element_size() == 2 else torch.int32))


def _rand(n, H, D, dtype, g):
    return torch.randn(n, H, D, generator=g, device=DEV, dtype=torch.float32).to(dtype)


def _scores64(q, k, lq, lk, starts_k=None, scale=None):
    """per sequence: fp64 scores [Hq, L_q, L_k] of the de-quantised q8 * sq and k8 * sk (None where a side is empty) -- computed once per
    set of tensors and shared by every window"""
    Hq, D = q.shape[1], q.shape[2]
    sm = 1.0 / math.sqrt(D) if scale is None else scale
    starts_k = starts_k if starts_k is not None else list(np.cumsum([0] + list(lk))[:-1])
    res, a = [], 0
    for n, m, b in zip(lq, lk, starts_k):
        if n and m:
            q8, sq = qa.dynamically_quantize_fp8(_seq(q, a, n), reduction_dim=[2, 3])
            k8, sk = qa.dynamically_quantize_fp8(_seq(k, b, m), reduction_dim=[2, 3])
            dq = q8[0].double() * sq[0].double()[:, None, None]
            dk = (k8[0].double() * sk[0].double()[:, None, None]).repeat_interleave(Hq // k.shape[1], dim=0)
            res.append((dq @ dk.transpose(-1, -2)) * sm)
        else:
            res.append(None)
        a += n
    return res


def _alive(n, m, window):
    d = torch.arange(m, device=DEV)[None, :] - torch.arange(n, device=DEV)[:, None] - (m - n)   # j - (r + delta)
    ok = torch.ones(n, m, dtype=torch.bool, device=DEV)
    if window[0] >= 0:
        ok &= d >= -window[0]
    if window[1] >= 0:
        ok &= d <= window[1]
    return ok


def _ref64(scores, v, lq, lk, window, starts_k=None, lse_shift=None):
    """fp64 windowed softmax on the shared scores and the original V: (out [total_q, Hq, D], lse [Hq, total_q], empty-row mask [total_q])"""
    Hq = next(s.shape[0] for s in scores if s is not None)
    total_q, D = sum(lq), v.shape[2]
    starts_k = starts_k if starts_k is not None else list(np.cumsum([0] + list(lk))[:-1])
    out = torch.zeros(total_q, Hq, D, dtype=torch.float64, device=DEV)
    lse = torch.full((Hq, total_q), -math.inf, dtype=torch.float64, device=DEV)
    a = 0
    for s, n, m, b in zip(scores, lq, lk, starts_k):
        if s is not None:
            sw = s.masked_fill(~_alive(n, m, window), -math.inf)
            l = torch.logsumexp(sw, dim=-1)
            p = torch.exp(sw - l.clamp_min(-1e300)[..., None])
            vv = v[b:b + m].transpose(0, 1).double().repeat_interleave(Hq // v.shape[1], dim=0)
            vv = torch.where(torch.isfinite(vv), vv, torch.zeros_like(vv))   # (V rows outside every window may hold anything: their P is 0)
            out[a:a + n] = (p @ vv).transpose(0, 1)
            lse[:, a:a + n] = l if lse_shift is None else l + lse_shift[:, a:a + n]
        a += n
    return out, lse, torch.isinf(lse[0])


def _check(got, got_lse, ref, ref_lse, empty, what):
    """every row: the V16 bound on out, 4e-3 on the LSE; rows without a key exactly 0 and -inf.  Returns the two worst ratios."""
    assert got.shape == ref.shape and got_lse.shape == ref_lse.shape
    assert (got[empty] == 0).all() and (got_lse[:, empty] == -math.inf).all(), (what, "rows without a key must be exactly 0 / -inf")
    assert torch.isfinite(got).all() and torch.isfinite(got_lse[:, ~empty]).all(), what
    worst = ((got.double() - ref).abs() / (TOL_V16 * ref.abs().clamp_min(1.0))).max().item()
    worst_lse = ((got_lse[:, ~empty].double() - ref_lse[:, ~empty]).abs().max().item() / LSE_TOL) if (~empty).any() else 0.0
    print(f"{what}: worst |out err| / bound {worst:.3f}, worst |lse err| / 4e-3 {worst_lse:.3f}, rows without a key {int(empty.sum())}")
    assert worst < 1.0 and worst_lse < 1.0, (what, worst, worst_lse)
    return worst, worst_lse


WINDOWS = [(0, 0), (16, 0), (63, 0), (64, 0), (65, 1), (100, 37), (0, 64), (-1, 0), (5, -1), (128, 128)]
GRID_LENS = [300, 1, 700, 0, 65]   # 700: three query blocks; 1 and 65: one key / one key past a chunk; 0: no rows


@pytest.mark.parametrize("D,dtype,fp8", [(D, t, "e4m3") for D in (64, 128, 256) for t in (torch.bfloat16, torch.float16)]
                         + [(128, torch.bfloat16, "e5m2")])
def test_every_row_against_the_fp64_window_reference(D, dtype, fp8):
    g = torch.Generator(device=DEV).manual_seed(D + (dtype == torch.float16))
    Hq, Hkv, lens = 8, 2, GRID_LENS
    q, k, v = (_rand(sum(lens), h, D, dtype, g) for h in (Hq, Hkv, Hkv))
    cu = _cu(lens)
    with qa.config.patch({"attention.fp8_format": fp8}):
        scores = _scores64(q, k, lens, lens)
        for window in WINDOWS:
            out, lse = qa.fp8_attn_varlen_window_func(q, k, v, cu, cu, max(lens), max(lens), window, return_lse=True)
            ref, ref_lse, empty = _ref64(scores, v, lens, lens, window)
            assert not empty.any()   # L_q = L_k: every row has its own key
            _check(out, lse, ref, ref_lse, empty, f"D {D} {dtype} {fp8} window {window}")
            assert _same_bits(qa.fp8_attn_varlen_window_func(q, k, v, cu, cu, max(lens), max(lens), window), out)


@pytest.mark.parametrize("D", [64, 128, 256])
def test_other_key_lengths_rows_without_a_key_and_seqused_k(D):
    g = torch.Generator(device=DEV).manual_seed(10 + D)
    Hq, Hkv, dtype = 8, 2, torch.bfloat16
    # delta > 0, delta < 0 (rows 0 .. 399 have no key under right = 0), and a sequence whose USED keys (130 of 400) set delta = -70
    lq, lk_alloc, lk = [100, 500, 200], [500, 100, 400], [500, 100, 130]
    q = _rand(sum(lq), Hq, D, dtype, g)
    k, v = _rand(sum(lk_alloc), Hkv, D, dtype, g), _rand(sum(lk_alloc), Hkv, D, dtype, g)
    starts = [0, 500, 600]
    cu_q, cu_k = _cu(lq), _cu(lk_alloc)
    used = torch.tensor(lk, dtype=torch.int32, device=DEV)
    scores = _scores64(q, k, lq, lk, starts)
    for window in ((-1, 0), (32, 0)):
        ref, ref_lse, empty = _ref64(scores, v, lq, lk, window, starts)
        assert empty[100:500].all() and not empty[:100].any() and not empty[500:600].any()
        assert empty[600:670].all() and not empty[670:].any()   # delta from the used count: 130 - 200
        for fill in (None, 1e4, float("nan")):
            k2, v2 = k.clone(), v.clone()
            if fill is not None:
                k2[600 + 130:], v2[600 + 130:] = fill, fill
            out, lse = qa.fp8_attn_varlen_window_func(q, k2, v2, cu_q, cu_k, 500, 500, window, seqused_k=used, return_lse=True)
            _check(out, lse, ref, ref_lse, empty, f"D {D} window {window} unused keys {fill}")
            if fill is None:
                first = (out, lse)
            else:
                assert _same_bits(out, first[0]) and _same_bits(lse, first[1]), "keys beyond seqused_k influence no bit"


@pytest.mark.parametrize("D", [64, 128, 256])
def test_exact_where_the_window_makes_it_exact(D):
    g = torch.Generator(device=DEV).manual_seed(20 + D)
    lens, H = [300, 1, 700, 65], 4
    for dtype in (torch.bfloat16, torch.float16):
        q, k, v = (_rand(sum(lens), H, D, dtype, g) for _ in range(3))
        cu = _cu(lens)
        win = lambda w, cq=cu, ck=cu: qa.fp8_attn_varlen_window_func(q, k, v, cq, ck, 700, 700, w, return_lse=True)
        # (0, 0), L_q = L_k, Hq = Hkv: every row sees its own key only -- P is exactly 1, out is v
        out, lse = win((0, 0))
        assert _same_bits(out, v) and torch.isfinite(lse).all()
        # nothing masked: the packed entry's non-causal bits, for the unbounded window and for finite ones wider than every sequence
        full = qa.fp8_attn_varlen_func(q, k, v, cu, cu, 700, 700, causal=False, return_lse=True)
        for w in ((-1, -1), (700, 700), (2 ** 31 - 1, 2 ** 31 - 1), (-1, 5000), (699, -1)):
            got = win(w)
            assert _same_bits(got[0], full[0]) and _same_bits(got[1], full[1]), (dtype, w)
        # (-1, 0) on equal tables: the packed entry's (top-left = bottom-right) causal bits
        causal = qa.fp8_attn_varlen_func(q, k, v, cu, cu, 700, 700, causal=True, return_lse=True)
        got = win((-1, 0))
        assert _same_bits(got[0], causal[0]) and _same_bits(got[1], causal[1]), dtype
        # other key lengths, nothing masked
        lk = [65, 700, 1, 300]
        ck = _cu(lk)
        full = qa.fp8_attn_varlen_func(q, k, v, cu, ck, 700, 700, causal=False, return_lse=True)
        got = win((1000, 1000), cu, ck)
        assert _same_bits(got[0], full[0]) and _same_bits(got[1], full[1]), dtype


@pytest.mark.parametrize("D", [64, 128, 256])
def test_value_rows_no_query_attends_are_never_read(D):
    g = torch.Generator(device=DEV).manual_seed(30 + D)
    Lq, Lk, Hq, Hkv, window = 1500, 1900, 8, 2, (64, 0)
    q, k, v = _rand(Lq, Hq, D, torch.bfloat16, g), _rand(Lk, Hkv, D, torch.bfloat16, g), _rand(Lk, Hkv, D, torch.bfloat16, g)
    v[:Lk - Lq - 64] = float("nan")   # rows below delta - left: outside row 0's window, and every later row's
    out, lse = qa.fp8_attn_varlen_window_func(q, k, v, _cu([Lq]), _cu([Lk]), Lq, Lk, window, return_lse=True)
    assert torch.isfinite(out).all()
    ref, ref_lse, empty = _ref64(_scores64(q, k, [Lq], [Lk]), v, [Lq], [Lk], window)
    _check(out, lse, ref, ref_lse, empty, f"D {D} NaN below the first window")


def test_graph_replay_follows_rewritten_tables():
    g = torch.Generator(device=DEV).manual_seed(40)
    H, D, total = 8, 128, 1200
    q, k, v = (_rand(total, H, D, torch.bfloat16, g) for _ in range(3))
    cu_q, cu_k = _cu([100, 700, 400]), _cu([300, 200, 700])
    call = lambda: qa.fp8_attn_varlen_window_func(q, k, v, cu_q, cu_k, 700, 1000, (100, 7), return_lse=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = call()
    lq, lk = [650, 50, 500], [1, 1000, 199]
    cu_q.copy_(_cu(lq))
    cu_k.copy_(_cu(lk))
    graph.replay()
    torch.cuda.synchronize()
    want = call()
    assert _same_bits(out, want[0]) and _same_bits(lse, want[1])
    ref, ref_lse, empty = _ref64(_scores64(q, k, lq, lk), v, lq, lk, (100, 7))
    assert empty.any() and not empty.all()
    _check(out, lse, ref, ref_lse, empty, "graph replay on rewritten tables")


def test_torch_compile_fullgraph_gives_the_eager_bits():
    g = torch.Generator(device=DEV).manual_seed(41)
    lens, H, D = [200, 1000, 77], 8, 128
    q, k, v = (_rand(sum(lens), H, D, torch.float16, g) for _ in range(3))
    cu = _cu(lens)

    def f(q, k, v, cu):
        return qa.fp8_attn_varlen_window_func(q * 2, k, v, cu, cu, 1000, 1000, (96, 3), return_lse=True)

    torch._dynamo.reset()
    got = torch.compile(f, fullgraph=True)(q, k, v, cu)
    want = f(q, k, v, cu)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])


@pytest.mark.parametrize("D", [64, 128, 256])
def test_key_smoothing_on_offset_keys(D):
    g = torch.Generator().manual_seed(50 + D)
    Hq, Hkv, dtype, window, sigma = 8, 2, torch.bfloat16, (100, 37), 16.0
    lq, lk = [300, 700, 165], [300, 900, 40]
    q = torch.randn(sum(lq), Hq, D, generator=g).to(dtype).to(DEV)
    k = torch.cat([torch.randn(n, Hkv, D, generator=g) + sigma * torch.randn(1, Hkv, D, generator=g) for n in lk]).to(dtype).to(DEV)
    v = torch.randn(sum(lk), Hkv, D, generator=g).to(dtype).to(DEV)
    cu_q, cu_k = _cu(lq), _cu(lk)
    with qa.config.patch({"attention.smooth_k": True}):
        out, lse = qa.fp8_attn_varlen_window_func(q, k, v, cu_q, cu_k, 700, 900, window, return_lse=True)
    res = _native.fp8_quant_attention_varlen_window(q, k, v, cu_q, cu_k, None, window_left=window[0], window_right=window[1], smooth_k=True,
                                                    return_lse=True, return_quant=True)
    assert _same_bits(res[0], out) and _same_bits(res[1], lse)
    q8, k8, sq, sk, mean = res[2:]
    packed = _native.fp8_quant_attention_varlen(q, k, v, cu_q, cu_k, None, smooth_k=True, return_quant=True)
    assert torch.equal(mean, packed[-1]) and torch.equal(sk, packed[-2]) and torch.equal(sq, packed[-3])   # the packed smoothing entry's bits
    # the reference on the operands the kernel read: q8 * sq, (k - mean)8 * sk; the LSE of the true scores lies sm q.mean higher
    sm = 1.0 / math.sqrt(D)
    scores, shift, a, b = [], torch.zeros(Hq, sum(lq), dtype=torch.float64, device=DEV), 0, 0
    k8n = k8.cpu().numpy()
    for i, (n, m) in enumerate(zip(lq, lk)):
        mp = (m + 63) // 64 * 64
        off = Hkv * D * (b + 64 * i)
        kb = unpack_frag(k8n[off:off + Hkv * mp * D], _native.LAYOUT_KFRAG, 1, Hkv, m, D)[0, :, :m]
        dk = torch.from_numpy(np.ascontiguousarray(kb)).to(DEV).view(TDT["e4m3"]).double() * sk[i].double()[:, None, None]
        dq = q8[Hq * D * a:Hq * D * (a + n)].view(Hq, n, D).view(TDT["e4m3"]).double() * sq[i].double()[:, None, None]
        scores.append((dq @ dk.repeat_interleave(Hq // Hkv, dim=0).transpose(-1, -2)) * sm)
        shift[:, a:a + n] = sm * (_seq(q, a, n)[0].double() * mean[i].double().repeat_interleave(Hq // Hkv, dim=0)[:, None, :]).sum(-1)
        a, b = a + n, b + m
    ref, ref_lse, empty = _ref64(scores, v, lq, lk, window, lse_shift=shift)
    assert empty[1000:1088].all() and not empty[1088:].any()   # sequence 2, delta = -125: rows 0 .. 87 end before key 0 under right = 37
    _check(out, lse, ref, ref_lse, empty, f"D {D} smooth_k, sigma {sigma} offset keys")


def test_dense_call_shape_is_the_packed_call_on_views():
    g = torch.Generator(device=DEV).manual_seed(60)
    B, Hq, Hkv, Sq, Skv, D, window = 2, 8, 2, 300, 420, 128, (64, 16)
    mk = lambda S, H: torch.randn(B, S, H, D, generator=g, device=DEV, dtype=torch.float32).bfloat16()
    qm, km, vm = mk(Sq, Hq), mk(Skv, Hkv), mk(Skv, Hkv)                      # [B, S, H, D] memory
    q, k, v = (t.transpose(1, 2) for t in (qm, km, vm))                      # the [B, H, S, D] views a model hands over
    steps = torch.arange(B + 1, dtype=torch.int32, device=DEV)
    want = qa.fp8_attn_varlen_window_func(qm.view(B * Sq, Hq, D), km.view(B * Skv, Hkv, D), vm.view(B * Skv, Hkv, D), steps * Sq, steps * Skv,
                                          Sq, Skv, window, return_lse=True)
    # no copy: the packed views the entry builds start at the callers' own bytes and keep their strides
    for t, S in ((q, Sq), (k, Skv), (v, Skv)):
        p = t.permute(0, 2, 1, 3).reshape(B * S, t.shape[1], D)
        assert p.data_ptr() == t.data_ptr() and p.stride() == (t.shape[1] * D, D, 1) and p.is_contiguous()
    # and the call's peak allocation is its results, its workspace and the two tables: a re-layout copy of q (1.2 MB) or k / v (430 KB) would show
    ws_bytes = _native.lib().qattn_fp8_quant_attention_varlen_window_workspace_bytes(B, Hq, Hkv, B * Sq, B * Skv, D)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out, lse = qa.fp8_window_attn_func(q, k, v, window, return_lse=True)
    grown = torch.cuda.max_memory_allocated() - before
    assert grown <= out.numel() * 2 + lse.numel() * 4 + ws_bytes + 16384, (grown, ws_bytes)
    assert out.shape == (B, Hq, Sq, D) and lse.shape == (B, Hq, Sq)
    assert _same_bits(out, want[0].view(B, Sq, Hq, D).permute(0, 2, 1, 3)) and _same_bits(lse, want[1].view(Hq, B, Sq).permute(1, 0, 2))
    assert _same_bits(qa.fp8_window_attn_func(q, k, v, window), out)
    # B = 1 from a contiguous [1, H, S, D]: a free view as well (token stride D, head stride S D)
    q1, k1, v1 = (t[:1].contiguous() for t in (q, k, v))
    p1 = q1.permute(0, 2, 1, 3).reshape(Sq, Hq, D)
    assert p1.data_ptr() == q1.data_ptr() and p1.stride() == (D, Sq * D, 1)
    o1, l1 = qa.fp8_window_attn_func(q1, k1, v1, window, return_lse=True)
    c1 = torch.arange(2, dtype=torch.int32, device=DEV)
    w1 = qa.fp8_attn_varlen_window_func(qm[0], km[0], vm[0], c1 * Sq, c1 * Skv, Sq, Skv, window, return_lse=True)
    assert _same_bits(o1[0], w1[0].transpose(0, 1)) and _same_bits(l1[0], w1[1])
    assert _same_bits(o1, out[:1]) and _same_bits(l1, lse[:1])

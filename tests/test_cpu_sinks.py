"""Learned attention sinks without a GPU (quantumattention_amd/sinks.py, include/qattn_sinks.h): the surface, every ValueError, the C
entries' sink checks, the fake registrations, the eager definitions against the fp64 oracle of tests/sinks_cases.py, the -inf-sink
identity, paged = contiguous and packed = paged per slot on the eager path, and the TEETH of the constant-V probe the GPU tests run:
every named way of getting the sink wrong moves a row of those very inputs by >= 4x the bound."""
import inspect
import math

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, merge, sinks, splitkv
from tests import paged_varlen_cases as V
from tests import sinks_cases as S


def _sig(f):
    return str(inspect.signature(f)).replace("typing.", "").replace("torch.Tensor", "Tensor")


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


NINF = torch.full((S.HQ,), -math.inf)


# ---- surface --------------------------------------------------------------------------------------------------------------------------------
def test_exports_and_literal_signatures():
    for name in ("fp8_attn_splitkv_sink_func", "fp8_attn_paged_sink_func", "fp8_attn_paged_varlen_sink_func", "merge_attn_states_with_sinks"):
        assert getattr(qa, name) is getattr(sinks, name) and name not in qa.__all__
    assert _sig(qa.fp8_attn_splitkv_sink_func) == (
        "(q, kv, sinks, window_size=(-1, 0), *, scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, num_splits: int = 0, "
        "precision: str = 'accurate', return_lse: bool = False, return_partials: bool = False)")
    assert _sig(qa.fp8_attn_paged_sink_func) == (
        "(q, cache: quantumattention_amd.paged.PagedKVCacheFP8, sinks, window_size=(-1, 0), *, scale: Optional[float] = None, "
        "seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, num_splits: int = 0, precision: str = 'accurate', "
        "return_lse: bool = False, return_partials: bool = False)")
    assert _sig(qa.fp8_attn_paged_varlen_sink_func) == (
        "(q, cache: quantumattention_amd.paged.PagedKVCacheFP8, cu_seqlens_q: Tensor, max_seqlen_q: int, sinks, window_size=(-1, 0), *, "
        "scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, num_splits: int = 0, "
        "precision: str = 'accurate', return_lse: bool = False, return_partials: bool = False)")
    assert _sig(qa.merge_attn_states_with_sinks) == (
        "(outs: Sequence[Tensor], lses: Sequence[Tensor], sinks: Tensor, *, out_dtype: Optional[torch.dtype] = None, return_lse: bool = True)")
    assert _sig(sinks.sinks_input_reason) == "(sinks, num_heads: int, device) -> Optional[str]"
    # the eager definitions' new argument is optional and defaults to no sink; `window` stays last
    for f in (splitkv._splitkv_eager, qa.paged._attend_eager, qa.paged_varlen._attend_varlen_eager):
        params = inspect.signature(f).parameters
        assert list(params)[-2:] == ["sinks", "window"] and params["sinks"].default is None
    assert inspect.signature(merge.merge_attn_states_eager).parameters["sinks"].default is None
    for op in ("fp8_splitkv_sink_attention_forward", "fp8_paged_splitkv_sink_attention_forward", "fp8_paged_varlen_splitkv_sink_attention_forward",
               "attention_state_merge_sink"):
        assert hasattr(qa.ops, op) and hasattr(torch.ops.quantumattention_amd, op)
    for name in ("qattn_attention_state_merge_sink", "qattn_fp8_attention_splitkv_sink_forward", "qattn_fp8_attention_paged_splitkv_sink_forward",
                 "qattn_fp8_attention_paged_varlen_sink_forward"):
        assert name in _native.EXPORTS and hasattr(_native.lib(), name)
    assert _native.ABI_VERSION == 8 == _native.lib().qattn_abi_version()


# ---- ValueErrors ----------------------------------------------------------------------------------------------------------------------------
def _small():
    p = S.Problem(64, 5)
    c, _ = p.cache("cpu")
    qp, cu, _ = p.packed_q("cpu")
    return p, c, qp, cu


def test_every_sink_value_error_carries_its_reason():
    p, c, qp, cu = _small()
    kv = qa.paged.gather_paged_eager(c)
    good = torch.zeros(S.HQ)
    calls = {
        "contig": lambda s, **kw: qa.fp8_attn_splitkv_sink_func(p.q, kv, s, (8, 0), seqused_k=c.seqlens, **kw),
        "paged": lambda s, **kw: qa.fp8_attn_paged_sink_func(p.q, c, s, (8, 0), **kw),
        "packed": lambda s, **kw: qa.fp8_attn_paged_varlen_sink_func(qp, c, cu, p.Sq, s, (8, 0), **kw),
        "merge": lambda s, **kw: qa.merge_attn_states_with_sinks([torch.zeros(1, S.HQ, 3, 64)], [torch.zeros(1, S.HQ, 3)], s),
    }
    bad = [(None, "tensor"), ([0.0] * S.HQ, "tensor"), (good.double(), "dtype"), (good.long(), "dtype"), (torch.zeros(S.HKV), "shape"),
           (torch.zeros(S.B, S.HQ), "shape"), (torch.zeros(S.HQ + 1), "shape"), (torch.zeros(()), "shape"),
           (torch.zeros(S.HQ, device="meta"), "to be on"), (torch.zeros(S.HQ, requires_grad=True), "grad")]
    for name, call in calls.items():
        call(good)                                                  # (the arguments are fine as they stand)
        call(good.bfloat16())
        call(good.half())
        for s, match in bad:
            with pytest.raises(ValueError, match=match):
                call(s)
            assert match in sinks.sinks_input_reason(s, S.HQ, "cpu")
    assert sinks.sinks_input_reason(good, S.HQ, "cpu") is None
    for name in ("contig", "paged", "packed"):
        with pytest.raises(ValueError, match="precision"):
            calls[name](good, precision="auto")
        with pytest.raises(ValueError, match="num_splits"):
            calls[name](good, num_splits=65)
    with pytest.raises(ValueError, match="window_size"):
        qa.fp8_attn_paged_sink_func(p.q, c, good, (-2, 0))
    # 16-bit sinks are up-cast: the bits of the fp32 call on the same values
    s16 = torch.tensor([0.5, -1.25, 3.0, -math.inf])
    for dt in (torch.bfloat16, torch.float16):
        a = qa.fp8_attn_paged_sink_func(p.q, c, s16.to(dt), (63, 0), num_splits=2, return_lse=True)
        b = qa.fp8_attn_paged_sink_func(p.q, c, s16, (63, 0), num_splits=2, return_lse=True)
        assert all(_same_bits(x, y) for x, y in zip(a, b))


def test_the_c_entries_refuse_a_null_or_misaligned_sink_before_any_device_call():
    L = _native.lib()
    INVALID = -1
    contig = lambda s: L.qattn_fp8_attention_splitkv_sink_forward(4096, _native.FMT_BF16, 1 << 20, 2 << 20, 256, 512, 8192, None, None, 2, 4, 2, 1, 256,
                                                                  64, _native.FMT_E4M3, 0, 127, 0, s, 0.0, 1, 1, None, None, None, None, None, None,
                                                                  None, 0, None)
    paged = lambda s: L.qattn_fp8_attention_paged_splitkv_sink_forward(4096, _native.FMT_BF16, 1 << 20, 2 << 20, 2048, 4, 8, 64, 4, 256, 512, 8192, None,
                                                                       1024, 2, 4, 2, 1, 256, 64, _native.FMT_E4M3, 0, 127, 0, s, 0.0, 1, 1, None, None,
                                                                       None, None, None, None, None, 0, None)
    packed = lambda s: L.qattn_fp8_attention_paged_varlen_sink_forward(4096, None, _native.FMT_BF16, 1 << 20, 2 << 20, 2048, 4, 8, 64, 4, 256, 512, 8192,
                                                                       None, 3072, 1024, 2, 4, 2, 5, 4, 256, 64, _native.FMT_E4M3, 0, 127, 0, s, 0.0, 1, 1,
                                                                       None, None, None, None, None, None, None, 0, None)
    workspace = L.qattn_fp8_attention_paged_splitkv_window_forward(4096, _native.FMT_BF16, 1 << 20, 2 << 20, 2048, 4, 8, 64, 4, 256, 512, 8192, None, 1024, 2,
                                                                   4, 2, 1, 256, 64, _native.FMT_E4M3, 0, 127, 0, 0.0, 1, 1, None, None, None, None, None,
                                                                   None, None, 0, None)
    assert workspace < 0 and workspace != INVALID
    for f in (contig, paged, packed):
        assert f(1 << 12) == workspace          # every argument check passed: the next one is the workspace's, as for the window sibling
        assert f(None) == INVALID and f((1 << 12) + 2) == INVALID
    # the merge entry: n = 1 is accepted, n = 0 / 9 and a NULL or misaligned sink are not
    import ctypes
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    def merge_rc(n, sink):
        m = max(n, 1)
        return L.qattn_attention_state_merge_sink(n, (vp * m)(*[1 << 20] * m), (ctypes.c_int * m)(*[_native.FMT_FP32] * m), (ll * (3 * m))(*[512, 128, 64] * m),
                                                  (vp * m)(*[1 << 21] * m), (ll * (3 * m))(*[8, 2, 1] * m), None, _native.FMT_BF16, (ll * 3)(512, 128, 64),
                                                  None, None, 1, 4, 2, 64, None, sink)
    assert merge_rc(0, 4096) == INVALID and merge_rc(9, 4096) == INVALID
    assert merge_rc(1, 4096) == INVALID         # (out is NULL: the sibling's own check, reached with n = 1)
    assert L.qattn_attention_state_merge(1, (vp * 1)(1 << 20), (ctypes.c_int * 1)(_native.FMT_FP32), (ll * 3)(512, 128, 64), (vp * 1)(1 << 21),
                                         (ll * 3)(8, 2, 1), 1 << 22, _native.FMT_BF16, (ll * 3)(512, 128, 64), None, None, 1, 4, 2, 64, None) == INVALID


def test_the_fake_registrations_give_the_shapes_and_dtypes_of_the_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        u8, f32, i32 = torch.empty(16, dtype=torch.uint8), torch.empty(3, 2), torch.empty(4, dtype=torch.int32)
        snk = torch.empty(8)
        ops = torch.ops.quantumattention_amd
        for ns, lse, parts in ((1, False, False), (1, True, True), (3, True, True), (9, False, True)):
            qd = torch.empty(3, 8, 5, 128, dtype=torch.float16)
            for res in (ops.fp8_splitkv_sink_attention_forward(qd, u8, u8, f32, f32, i32[:3], 1280, ns, 127, 0, snk, "e4m3", "compiled", "accurate", lse, parts),
                        ops.fp8_paged_splitkv_sink_attention_forward(qd, u8, u8, f32, f32, i32.view(1, 4).expand(3, 4), i32[:3], 1280, 20, 64, ns, 127, 0,
                                                                     snk, "e4m3", "compiled", "fast", lse, parts)):
                out, l, po, pl, pp = res
                assert out.shape == (3, 8, 5, 128) and out.dtype == torch.float16 and l.shape == ((3, 8, 5) if lse else (0,))
                assert l.dtype == pl.dtype == po.dtype == torch.float32 and pp.dtype == torch.uint8
                if parts and ns > 1:
                    assert po.shape == (ns, 3, 8, 5, 128) and pl.shape == pp.shape == (ns, 3, 8, 5)
                else:
                    assert po.numel() == pl.numel() == pp.numel() == 0
            qp = torch.empty(39, 8, 128, dtype=torch.bfloat16)
            out, l, po, pl, pp = ops.fp8_paged_varlen_splitkv_sink_attention_forward(qp, u8, u8, f32, f32, i32.view(1, 4).expand(3, 4), i32[:3], i32, 33,
                                                                                     1280, 20, 64, ns, 127, 0, snk, "e4m3", "compiled", "accurate", lse, parts)
            assert out.shape == (39, 8, 128) and out.dtype == torch.bfloat16 and l.shape == ((8, 39) if lse else (0,))
            if parts and ns > 1:
                assert po.shape == (ns, 39, 8, 128) and pl.shape == pp.shape == (ns, 8, 39) and pp.dtype == torch.uint8
        o, l = ops.attention_state_merge_sink([torch.empty(2, 8, 5, 64)] * 3, [torch.empty(2, 8, 5)] * 3, snk, torch.bfloat16)
        assert o.shape == (2, 8, 5, 64) and o.dtype == torch.bfloat16 and l.shape == (2, 8, 5) and l.dtype == torch.float32
        o, l = ops.attention_state_merge_sink([torch.empty(9, 8, 64, dtype=torch.float16)], [torch.empty(8, 9)], snk)
        assert o.shape == (9, 8, 64) and o.dtype == torch.float16 and l.shape == (8, 9)


# ---- the eager definitions against the oracle ---------------------------------------------------------------------------------------------------
def _entries(p, c, kv, qp, cud):
    """{name: call(sinks, window, **kw) -> (out [B, HQ, Sq, D], lse [B, HQ, Sq], ...)} of the three entries on the problem, all sequences
    with Sq queries; the packed outputs in the dense layout"""
    def packed(s, w, **kw):
        res = qa.fp8_attn_paged_varlen_sink_func(qp, c, cud, p.Sq, s, w, **kw)
        out, lse = res[0], res[1]
        return (out.view(S.B, p.Sq, S.HQ, p.D).transpose(1, 2), lse.view(S.HQ, S.B, p.Sq).transpose(0, 1)) + tuple(res[2:])
    return {"contig": lambda s, w, **kw: qa.fp8_attn_splitkv_sink_func(p.q.to(qp.device), kv, s, w, seqused_k=c.seqlens, **kw),
            "paged": lambda s, w, **kw: qa.fp8_attn_paged_sink_func(p.q.to(qp.device), c, s, w, **kw),
            "packed": packed}


@pytest.mark.parametrize("D,Sq", [(64, 1), (64, 5), (64, 130), (128, 5)])
def test_the_eager_definitions_are_the_fp64_oracle_with_the_sink_column(D, Sq):
    """out to one bf16 ulp + 1e-5 (fp32 softmax against fp64), lse to 1e-4; rows without a key: zero rows with lse = sink_h EXACTLY"""
    p = S.Problem(D, Sq)
    c, _ = p.cache("cpu")
    kv = qa.paged.gather_paged_eager(c)
    qp, cud, _ = p.packed_q("cpu")
    for window in S.WINDOWS:
        snk = p.ladder(window)
        st = torch.from_numpy(snk)
        empty = np.isneginf(p.keys_state(window)[1])
        assert empty.any() == (Sq == 130), "Sq 130 over 65 keys leaves rows without a key"
        for ns in S.SPLITS:
            ro, rl = p.reference(window, snk, ns)
            for name, call in _entries(p, c, kv, qp, cud).items():
                out, lse = call(st, window, num_splits=ns, return_lse=True)
                o, l = out.float().numpy(), lse.numpy()
                what = (name, D, Sq, window, ns)
                assert np.all(np.abs(o - ro) <= 2.0 ** -8 * np.abs(ro) + 1e-5), what
                assert np.all(np.abs(l - rl) <= 1e-4), what
                assert (o[empty] == 0).all() and np.array_equal(l[empty], np.broadcast_to(snk[None, :, None], l.shape)[empty]), what


def test_eager_minus_inf_sinks_are_the_window_siblings_bit_for_bit_and_nan_or_inf_sinks_poison_their_head_alone():
    p = S.Problem(64, 5)
    c, _ = p.cache("cpu")
    kv = qa.paged.gather_paged_eager(c)
    qp, cud, _ = p.packed_q("cpu")
    kw = dict(return_lse=True, return_partials=True)
    for window in ((-1, 0), (63, 0)):
        for ns in S.SPLITS:
            for precision in ("accurate", "fast")[:1 if ns == 2 else 2]:
                k2 = dict(num_splits=ns, precision=precision, **kw)
                pairs = ((qa.fp8_attn_splitkv_sink_func(p.q, kv, NINF, window, seqused_k=c.seqlens, **k2),
                          qa.fp8_attn_splitkv_window_func(p.q, kv, window, seqused_k=c.seqlens, **k2)),
                         (qa.fp8_attn_paged_sink_func(p.q, c, NINF, window, **k2), qa.fp8_attn_paged_window_func(p.q, c, window, **k2)),
                         (qa.fp8_attn_paged_varlen_sink_func(qp, c, cud, p.Sq, NINF, window, **k2),
                          qa.fp8_attn_paged_varlen_window_func(qp, c, cud, p.Sq, window, **k2)))
                for got, want in pairs:
                    assert len(got) == len(want) == 5 and all(_same_bits(x, y) for x, y in zip(got, want)), (window, ns, precision)
        # finite sinks: the partials are still the sibling's, and they merge to out, lse
        st = torch.from_numpy(p.ladder(window))
        for ns in (2, 9):
            got = qa.fp8_attn_paged_sink_func(p.q, c, st, window, num_splits=ns, **kw)
            want = qa.fp8_attn_paged_window_func(p.q, c, window, num_splits=ns, **kw)
            assert all(_same_bits(x, y) for x, y in zip(got[2:], want[2:])) and not _same_bits(got[0], want[0])
            mo, ml = qa.merge_attn_states_with_sinks(list(got[2]), list(got[3]), st, out_dtype=p.q.dtype)
            assert _same_bits(mo, got[0]) and _same_bits(ml, got[1])
        for poison in (math.nan, math.inf):
            st2 = st.clone()
            st2[2] = poison
            for ns in (1, 2):
                out, lse = qa.fp8_attn_paged_sink_func(p.q, c, st2, window, num_splits=ns, return_lse=True)
                ref = qa.fp8_attn_paged_sink_func(p.q, c, st, window, num_splits=ns, return_lse=True)
                assert torch.isnan(out[:, 2].float()).all() and torch.isnan(lse[:, 2]).all(), (window, poison, ns)
                keep = [0, 1, 3]
                assert _same_bits(out[:, keep], ref[0][:, keep]) and _same_bits(lse[:, keep], ref[1][:, keep])


def test_eager_paged_is_contiguous_on_the_gathered_cache_and_packed_is_paged_on_each_slot_alone_idle_slots_included():
    p = S.Problem(64, 5)
    c, _ = p.cache("cpu")
    kv = qa.paged.gather_paged_eager(c)
    sq = [5, 0, 3, 1]
    qp, cud, cu = p.packed_q("cpu", sq)
    for window in ((127, 0), (0, 0)):
        st = torch.from_numpy(p.ladder(window))
        for ns in (1, 2):
            kw = dict(num_splits=ns, return_lse=True, return_partials=True)
            a = qa.fp8_attn_paged_sink_func(p.q, c, st, window, **kw)
            b = qa.fp8_attn_splitkv_sink_func(p.q, kv, st, window, seqused_k=c.seqlens, **kw)
            assert all(_same_bits(x, y) for x, y in zip(a, b))
            got = qa.fp8_attn_paged_varlen_sink_func(qp, c, cud, max(sq), st, window, **kw)
            for s in range(S.B):
                if sq[s]:
                    want = qa.fp8_attn_paged_sink_func(V.alone(qp, cu, s), V.one_slot(c, s), st, window, **kw)
                    assert _same_bits(V.rows_of(got[0], "o", cu, s), want[0]) and _same_bits(V.rows_of(got[1], "l", cu, s), want[1])


def test_merge_with_sinks_eager_is_the_fp64_formula_for_one_to_nine_states():
    g = torch.Generator().manual_seed(3)
    H, Sn, D = 4, 7, 64
    snk = torch.tensor([0.3, -math.inf, 2.0, -1.0])
    for n in (1, 2, 8, 9):
        outs = [torch.randn(2, H, Sn, D, generator=g) for _ in range(n)]
        lses = [torch.randn(2, H, Sn, generator=g) * 2 for _ in range(n)]
        for l in lses:
            l[0, :, 0] = -math.inf                                   # a row empty in every state
        lses[0][1, :, 1] = -math.inf
        out, lse = qa.merge_attn_states_with_sinks(outs, lses, snk)
        Ls = torch.stack([l.double() for l in lses] + [snk.double()[None, :, None].expand(2, H, Sn)])
        ref_l = torch.logsumexp(Ls, 0)
        w = torch.exp(Ls[:-1] - ref_l.clamp_min(-1e300))
        ref_o = (w[..., None] * torch.stack(outs).double()).sum(0)
        live = ~torch.isneginf(ref_l)
        assert torch.allclose(out.double(), ref_o, atol=1e-5) and torch.allclose(lse.double()[live], ref_l[live], atol=1e-5)
        assert (out[0, :, 0] == 0).all() and torch.equal(lse[0, :, 0], snk), "all states empty: a zero row with lse = sink_h"
        # -inf sinks: merge_attn_states
        if n > 1:
            a = qa.merge_attn_states_with_sinks(outs, lses, NINF)
            b = qa.merge_attn_states(outs, lses)
            assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    # the packed convention: [total, H, D] / [H, total]
    outs, lses = [torch.randn(9, H, D, generator=g)], [torch.randn(H, 9, generator=g)]
    out, lse = qa.merge_attn_states_with_sinks(outs, lses, snk)
    want = torch.logaddexp(lses[0], snk[:, None])
    assert torch.allclose(lse, want, atol=1e-6) and torch.allclose(out, outs[0] * torch.exp(lses[0] - want).t()[..., None], atol=1e-6)


# ---- teeth ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", S.DS)
def test_every_named_mutant_moves_a_row_of_the_constant_v_probe_by_four_times_the_bound(D):
    """the inputs of tests/test_gpu_sinks.py's constant-V probe: at EVERY query count each mutant moves some element of some window and
    split count by >= TEETH x its bound (out: 2^-6 max(1, |ref| / 2); the empty-row mutant leaves out alone and shows in the LSE, against
    LSE_TOL, at Sq = 130 -- the one count with rows that hold no key).  (A single (window, ns) need not show a mutant: under (0, 0) a
    decode's one key lies in one split, and "once per split" is then the right rule.)"""
    best = {}
    for Sq in S.SQS:
        p = S.Problem(D, Sq, const_v=True)
        for window in S.WINDOWS:
            snk = p.ladder(window)
            # the probe's own claim: out = v (1 - p_sink), p_sink from the oracle's key LSE
            ro, rl = p.reference(window, snk)
            lse_k = p.keys_state(window)[1]
            share = 1.0 / (1.0 + np.exp(lse_k - snk[None, :, None].astype(np.float64)))
            v0 = p.v.double().numpy()[:, :, 0].repeat(S.G, axis=1)[:, :, None, :]
            assert np.allclose(ro, np.where(np.isneginf(lse_k)[..., None], 0.0, v0 * (1.0 - share)[..., None]), atol=1e-9)
            for m in S.MUTANTS:
                if m == "an empty row given lse = -inf" and Sq != 130:
                    continue                                         # (no row without a key)
                ns_set = (2, 9) if m == "sink added once per split" else (9,) if m == "sink added in every launch of the merge chain" else (1, 2, 9)
                for ns in ns_set:
                    best[m, Sq] = max(best.get((m, Sq), 0.0), S.teeth(p, window, snk, ns, m))
    assert {m for m, _ in best} == set(S.MUTANTS)
    assert all(t >= S.TEETH for t in best.values()), best

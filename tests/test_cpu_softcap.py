"""Logit soft-capping without a GPU (quantumattention_amd/softcap.py, include/qattn_softcap.h): the surface, every ValueError, the C
entries' softcap check, the fake registrations, the eager definitions against the fp64 oracle of tests/softcap_cases.py, softcap=None and
softcap=0.0, paged = contiguous and packed = paged per slot on the eager path, the cap probe's closed form, and the TEETH of the GPU tests:
every named way of getting the cap wrong moves an element of those very inputs by >= 4x the bound."""
import inspect
import math

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, softcap, splitkv
from tests import paged_varlen_cases as V
from tests import softcap_cases as C


def _sig(f):
    return str(inspect.signature(f)).replace("typing.", "").replace("torch.Tensor", "Tensor")


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- surface --------------------------------------------------------------------------------------------------------------------------------
def test_exports_and_literal_signatures():
    for name in ("fp8_attn_splitkv_softcap_func", "fp8_attn_paged_softcap_func", "fp8_attn_paged_varlen_softcap_func", "softcap_input_reason"):
        assert getattr(qa, name) is getattr(softcap, name) and name not in qa.__all__
    assert _sig(qa.fp8_attn_splitkv_softcap_func) == (
        "(q, kv, softcap, window_size=(-1, 0), *, scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, num_splits: int = 0, "
        "precision: str = 'accurate', return_lse: bool = False, return_partials: bool = False)")
    assert _sig(qa.fp8_attn_paged_softcap_func) == (
        "(q, cache: quantumattention_amd.paged.PagedKVCacheFP8, softcap, window_size=(-1, 0), *, scale: Optional[float] = None, "
        "seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, num_splits: int = 0, precision: str = 'accurate', "
        "return_lse: bool = False, return_partials: bool = False)")
    assert _sig(qa.fp8_attn_paged_varlen_softcap_func) == (
        "(q, cache: quantumattention_amd.paged.PagedKVCacheFP8, cu_seqlens_q: Tensor, max_seqlen_q: int, softcap, window_size=(-1, 0), *, "
        "scale: Optional[float] = None, seqused_k: Optional[Tensor] = None, max_seqlen_k: Optional[int] = None, num_splits: int = 0, "
        "precision: str = 'accurate', return_lse: bool = False, return_partials: bool = False)")
    assert _sig(softcap.softcap_input_reason) == "(softcap) -> Optional[str]"
    # the eager definitions' new argument is optional, defaults to no cap and stands before `window`, which stays last
    for f in (splitkv._splitkv_eager, qa.paged._attend_eager, qa.paged_varlen._attend_varlen_eager):
        params = inspect.signature(f).parameters
        names = list(params)
        assert names[-1] == "window" and "softcap" in names and names.index("softcap") < names.index("window")
        assert params["softcap"].default is None
    for op in ("fp8_splitkv_softcap_attention_forward", "fp8_paged_splitkv_softcap_attention_forward",
               "fp8_paged_varlen_splitkv_softcap_attention_forward"):
        assert hasattr(qa.ops, op) and hasattr(torch.ops.quantumattention_amd, op)
    for name in ("qattn_fp8_attention_splitkv_softcap_forward", "qattn_fp8_attention_paged_splitkv_softcap_forward",
                 "qattn_fp8_attention_paged_varlen_softcap_forward"):
        assert name in _native.EXPORTS and hasattr(_native.lib(), name)
    assert _native.ABI_VERSION == 8 == _native.lib().qattn_abi_version()


# ---- ValueErrors ----------------------------------------------------------------------------------------------------------------------------
def _small(D=64, Sq=5):
    p = C.Problem(D, Sq)
    c, _ = p.cache("cpu")
    qp, cu, _ = p.packed_q("cpu")
    return p, c, qp, cu


def _calls(p, c, qp, cu):
    kv = qa.paged.gather_paged_eager(c)
    return {
        "contig": lambda s, w=(8, 0), **kw: qa.fp8_attn_splitkv_softcap_func(p.q, kv, s, w, seqused_k=c.seqlens, **kw),
        "paged": lambda s, w=(8, 0), **kw: qa.fp8_attn_paged_softcap_func(p.q, c, s, w, **kw),
        "packed": lambda s, w=(8, 0), **kw: qa.fp8_attn_paged_varlen_softcap_func(qp, c, cu, p.Sq, s, w, **kw),
    }


def test_every_softcap_value_error_carries_its_reason():
    p, c, qp, cu = _small()
    bad = [(-1.0, "negative"), (-0.5, "negative"), (math.nan, "NaN"), (math.inf, "inf"), (-math.inf, "inf"), (None, "host float"),
           ("50", "host float"), (torch.tensor(50.0), "host float"), (True, "host float"), (1e39, "float32")]
    for name, call in _calls(p, c, qp, cu).items():
        call(50.0)                                                  # (the arguments are fine as they stand)
        call(30)                                                    # (an int is a host number too)
        call(0.0)
        for s, match in bad:
            with pytest.raises(ValueError, match=match):
                call(s)
            assert match in softcap.softcap_input_reason(s)
        with pytest.raises(ValueError, match="precision"):
            call(50.0, precision="auto")
        with pytest.raises(ValueError, match="num_splits"):
            call(50.0, num_splits=65)
        with pytest.raises(ValueError, match="window_size"):
            call(50.0, (-2, 0))
    for ok in (0.0, 0, 0.5, 50.0, 30):
        assert softcap.softcap_input_reason(ok) is None


def test_the_c_entries_refuse_a_softcap_that_is_not_finite_or_not_positive_before_any_device_call():
    L = _native.lib()
    INVALID = -1
    contig = lambda s: L.qattn_fp8_attention_splitkv_softcap_forward(4096, _native.FMT_BF16, 1 << 20, 2 << 20, 256, 512, 8192, None, None, 2, 4, 2, 1, 256,
                                                                     64, _native.FMT_E4M3, 0, 127, 0, s, 0.0, 1, 1, None, None, None, None, None, None,
                                                                     None, 0, None)
    paged = lambda s: L.qattn_fp8_attention_paged_splitkv_softcap_forward(4096, _native.FMT_BF16, 1 << 20, 2 << 20, 2048, 4, 8, 64, 4, 256, 512, 8192,
                                                                          None, 1024, 2, 4, 2, 1, 256, 64, _native.FMT_E4M3, 0, 127, 0, s, 0.0, 1, 1, None,
                                                                          None, None, None, None, None, None, 0, None)
    packed = lambda s: L.qattn_fp8_attention_paged_varlen_softcap_forward(4096, None, _native.FMT_BF16, 1 << 20, 2 << 20, 2048, 4, 8, 64, 4, 256, 512,
                                                                          8192, None, 3072, 1024, 2, 4, 2, 5, 4, 256, 64, _native.FMT_E4M3, 0, 127, 0, s,
                                                                          0.0, 1, 1, None, None, None, None, None, None, None, 0, None)
    workspace = L.qattn_fp8_attention_paged_splitkv_window_forward(4096, _native.FMT_BF16, 1 << 20, 2 << 20, 2048, 4, 8, 64, 4, 256, 512, 8192, None, 1024, 2,
                                                                   4, 2, 1, 256, 64, _native.FMT_E4M3, 0, 127, 0, 0.0, 1, 1, None, None, None, None, None,
                                                                   None, None, 0, None)
    assert workspace < 0 and workspace != INVALID
    for f in (contig, paged, packed):
        for good in (50.0, 30.0, 0.5, 1e-30, 3e38):
            assert f(good) == workspace         # every argument check passed: the next one is the workspace's, as for the window sibling
        for bad in (0.0, -0.0, -50.0, math.nan, math.inf, -math.inf):
            assert f(bad) == INVALID, bad


def test_the_fake_registrations_give_the_shapes_and_dtypes_of_the_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        u8, f32, i32 = torch.empty(16, dtype=torch.uint8), torch.empty(3, 2), torch.empty(4, dtype=torch.int32)
        ops = torch.ops.quantumattention_amd
        for ns, lse, parts in ((1, False, False), (1, True, True), (3, True, True), (9, False, True)):
            qd = torch.empty(3, 8, 5, 128, dtype=torch.float16)
            for res in (ops.fp8_splitkv_softcap_attention_forward(qd, u8, u8, f32, f32, i32[:3], 1280, ns, 4095, 0, 50.0, "e4m3", "compiled", "accurate",
                                                                  lse, parts),
                        ops.fp8_paged_splitkv_softcap_attention_forward(qd, u8, u8, f32, f32, i32.view(1, 4).expand(3, 4), i32[:3], 1280, 20, 64, ns,
                                                                        -1, 0, 30.0, "e4m3", "compiled", "fast", lse, parts, scale=0.0625)):
                out, l, po, pl, pp = res
                assert out.shape == (3, 8, 5, 128) and out.dtype == torch.float16 and l.shape == ((3, 8, 5) if lse else (0,))
                assert l.dtype == pl.dtype == po.dtype == torch.float32 and pp.dtype == torch.uint8
                if parts and ns > 1:
                    assert po.shape == (ns, 3, 8, 5, 128) and pl.shape == pp.shape == (ns, 3, 8, 5)
                else:
                    assert po.numel() == pl.numel() == pp.numel() == 0
            qp = torch.empty(39, 8, 128, dtype=torch.bfloat16)
            out, l, po, pl, pp = ops.fp8_paged_varlen_splitkv_softcap_attention_forward(qp, u8, u8, f32, f32, i32.view(1, 4).expand(3, 4), i32[:3], i32,
                                                                                        33, 1280, 20, 64, ns, 127, 0, 50.0, "e4m3", "compiled",
                                                                                        "accurate", lse, parts)
            assert out.shape == (39, 8, 128) and out.dtype == torch.bfloat16 and l.shape == ((8, 39) if lse else (0,))
            if parts and ns > 1:
                assert po.shape == (ns, 39, 8, 128) and pl.shape == pp.shape == (ns, 8, 39) and pp.dtype == torch.uint8


# ---- the eager definitions against the oracle ---------------------------------------------------------------------------------------------------
def _dense(p, res):
    """a packed result in the dense layout [B, HQ, Sq, D] / [B, HQ, Sq]"""
    return (res[0].view(C.B, p.Sq, C.HQ, p.D).transpose(1, 2), res[1].view(C.HQ, C.B, p.Sq).transpose(0, 1)) + tuple(res[2:])


@pytest.mark.parametrize("D,Sq", [(64, 1), (64, 5), (64, 130), (128, 5), (256, 5)])
def test_the_eager_definitions_are_the_fp64_oracle_over_the_cap_ladder(D, Sq):
    """out to one bf16 ulp + 1e-5 (fp32 softmax against fp64) -- far inside the fp8-V bound the GPU tests apply --, lse to 1e-4; rows
    without a key: zero rows with lse = -inf"""
    p, c, qp, cu = _small(D, Sq)
    calls = _calls(p, c, qp, cu)
    for window in C.WINDOWS:
        empty = p.empty(window)
        assert empty.any() == (Sq == 130 and window != (-1, -1)), "Sq 130 over 65 keys leaves rows without a key under a causal window"
        for cap in C.CAPS:
            for gain in C.GAINS:
                ro, rl = p.reference(window, cap, gain)
                for ns in C.SPLITS if (D, Sq) == (64, 5) else (2,):
                    for name, call in calls.items():
                        res = call(cap, window, scale=p.scale(gain), num_splits=ns, return_lse=True)
                        out, lse = _dense(p, res) if name == "packed" else res
                        o, l = out.float().numpy(), lse.numpy()
                        what = (name, D, Sq, window, cap, gain, ns)
                        assert np.all(np.abs(o - ro) <= 2.0 ** -8 * np.abs(ro) + 1e-5), what
                        assert np.all(np.abs(o - ro) <= C.bound(ro)), what
                        live = ~empty
                        assert np.all(np.abs(l[live] - rl[live]) <= 1e-4) and np.abs(l[live] - rl[live]).max() <= C.LSE_TOL, what
                        assert (o[empty] == 0).all() and np.isneginf(l[empty]).all() and np.isneginf(rl[empty]).all(), what


def test_softcap_none_leaves_the_eager_results_bit_equal_and_softcap_zero_is_the_window_sibling():
    p, c, qp, cu = _small()
    kv = qa.paged.gather_paged_eager(c)
    kw = dict(return_lse=True, return_partials=True)
    for window in ((-1, 0), (127, 0)):
        for ns in (1, 2, 9):
            k2 = dict(num_splits=ns, scale=p.scale(4.0), **kw)
            sib = (qa.fp8_attn_splitkv_window_func(p.q, kv, window, seqused_k=c.seqlens, **k2), qa.fp8_attn_paged_window_func(p.q, c, window, **k2),
                   qa.fp8_attn_paged_varlen_window_func(qp, c, cu, p.Sq, window, **k2))
            zero = (qa.fp8_attn_splitkv_softcap_func(p.q, kv, 0.0, window, seqused_k=c.seqlens, **k2),
                    qa.fp8_attn_paged_softcap_func(p.q, c, 0.0, window, **k2), qa.fp8_attn_paged_varlen_softcap_func(qp, c, cu, p.Sq, 0, window, **k2))
            capped = qa.fp8_attn_paged_softcap_func(p.q, c, 2.0, window, **k2)
            for got, want in zip(zero, sib):
                assert len(got) == len(want) == 5 and all(_same_bits(x, y) for x, y in zip(got, want)), (window, ns)
            assert not _same_bits(capped[0], sib[1][0]) and not _same_bits(capped[1], sib[1][1]), "the cap is felt"
            # the eager definitions themselves: softcap=None is the call without the argument
            a = splitkv._splitkv_eager(p.q, kv, False, p.scale(4.0), c.seqlens, ns, "accurate", window=window)
            b = splitkv._splitkv_eager(p.q, kv, False, p.scale(4.0), c.seqlens, ns, "accurate", softcap=None, window=window)
            assert all(_same_bits(x, y) for x, y in zip(a, b)) and all(_same_bits(x, y) for x, y in zip(a, sib[0]))
            a = qa.paged._attend_eager(p.q, c, False, p.scale(4.0), c.seqlens, C.CAP, ns, "accurate", softcap=None, window=window)
            assert all(_same_bits(x, y) for x, y in zip(a, sib[1]))
            a = qa.paged_varlen._attend_varlen_eager(qp, c, cu, False, p.scale(4.0), c.seqlens, C.CAP, ns, "accurate", softcap=None, window=window)
            assert all(_same_bits(x, y) for x, y in zip(a, sib[2]))
            # the partials are states over capped scores: they merge to out, lse
            if ns > 1:
                mo, ml = qa.merge_attn_states(list(capped[2]), list(capped[3]), out_dtype=p.q.dtype)
                assert _same_bits(mo, capped[0]) and _same_bits(ml, capped[1])


def test_eager_paged_is_contiguous_on_the_gathered_cache_and_packed_is_paged_on_each_slot_alone_idle_slots_included():
    p, c, _, _ = _small()
    kv = qa.paged.gather_paged_eager(c)
    sq = [5, 0, 3, 1]
    qp, cud, cu = p.packed_q("cpu", sq)
    for window in ((127, 0), (-1, -1)):
        for cap, gain in ((2.0, 4.0), (50.0, 1.0)):
            for ns in (1, 2):
                kw = dict(num_splits=ns, scale=p.scale(gain), return_lse=True, return_partials=True)
                a = qa.fp8_attn_paged_softcap_func(p.q, c, cap, window, **kw)
                b = qa.fp8_attn_splitkv_softcap_func(p.q, kv, cap, window, seqused_k=c.seqlens, **kw)
                assert all(_same_bits(x, y) for x, y in zip(a, b))
                got = qa.fp8_attn_paged_varlen_softcap_func(qp, c, cud, max(sq), cap, window, **kw)
                for s in range(C.B):
                    if sq[s]:
                        want = qa.fp8_attn_paged_softcap_func(V.alone(qp, cu, s), V.one_slot(c, s), cap, window, **kw)
                        assert _same_bits(V.rows_of(got[0], "o", cu, s), want[0]) and _same_bits(V.rows_of(got[1], "l", cu, s), want[1])


# ---- teeth ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Sq", C.CASES)
def test_every_named_mutant_moves_an_element_of_the_gpu_tests_inputs_by_four_times_the_bound(D, Sq):
    """the inputs of tests/test_gpu_softcap.py's oracle test: on EVERY (D, Sq) each mutant moves some element of some rung of the ladder
    and some window by >= TEETH x its bound (out: 2^-6 max(1, |ref| / 2); lse: LSE_TOL).  No single rung shows them all: under (-1, -1)
    nothing is masked and "after the mask" is right; at cap 50 the masked keys' exp(-50) is invisible."""
    p = C.Problem(D, Sq)
    best = {}
    for m in C.MUTANTS:
        for window in C.WINDOWS:
            for cap in C.CAPS:
                for gain in C.GAINS:
                    best[m] = max(best.get(m, 0.0), C.teeth(p, window, cap, gain, m))
    assert set(best) == set(C.MUTANTS)
    assert all(t >= C.TEETH for t in best.values()), best
    # the LSE mutant leaves out alone: it bites through the LSE only
    ro, _ = p.reference((-1, 0), 2.0, 4.0)
    mo, _ = p.reference((-1, 0), 2.0, 4.0, "LSE returned for the uncapped scores")
    assert np.array_equal(ro, mo)


@pytest.mark.parametrize("D", (64, 128, 256))
def test_the_cap_probe_has_its_closed_form_its_teeth_and_an_eager_path_inside_its_bound(D):
    for Sq in C.PROBE_SQS:
        pr = C.Probe(D, Sq)
        c, _ = pr.cache("cpu")
        qp, cu, _ = pr.packed_q("cpu")
        calls = _calls(pr, c, qp, cu)
        # the closed form is the fp64 softmax of the capped scores on these inputs
        kx = pr.k.double().numpy().repeat(C.G, axis=1)
        x = np.einsum("bhsd,bhkd->bhsk", pr.q.double().numpy(), kx) * C.PROBE_SCALE
        for b, j in enumerate(pr.star):
            assert np.array_equal(x[b, :, :, j], np.broadcast_to(pr.X[:, None], (C.HQ, Sq))) and np.count_nonzero(x[b]) == C.HQ * Sq
        for window in C.WINDOWS:
            n = pr.counts(window)
            for cap in C.PROBE_CAPS:
                ro, rl = pr.expected(window, cap)
                if cap == 2.0 and window == (-1, -1):
                    w = math.exp(2.0 * math.tanh(4.0)) / (math.exp(2.0 * math.tanh(4.0)) + 64.0)
                    assert n[0, 0] == 65 and abs(w - 0.10) < 0.005 and math.exp(8.0) / (math.exp(8.0) + 64.0) > 0.975
                for precision in ("accurate", "fast"):
                    bnd = C.probe_bound(ro, precision)
                    for name, call in calls.items():
                        res = call(cap, window, scale=C.PROBE_SCALE, num_splits=2, precision=precision, return_lse=True)
                        out, lse = _dense(pr, res) if name == "packed" else res
                        o = out.float().numpy()
                        assert np.all(np.abs(o - ro) <= bnd) and (o[ro == 0] == 0).all(), (name, D, Sq, window, cap, precision)
                        assert np.abs(lse.numpy() - rl).max() <= 1e-4
                    # teeth, against the tighter of the two bounds' widest: FAST's
                    for m in ("cap dropped", "cap applied after the mask"):
                        if cap == 50.0 or (m == "cap applied after the mask" and window != (127, 0)):
                            continue                                # (cap 50 moves X = 8 by 0.07, exp(-50) is invisible / few or no keys masked inside [0, L))
                        mo, _ = pr.expected(window, cap, m)
                        live = ro != 0
                        t = float((np.abs(mo - ro)[live] / C.probe_bound(ro, "fast")[live]).max())
                        assert t >= C.TEETH, (m, D, Sq, window, cap, t)
        # "with the cap after the mask a (127, 0) window at 1280 keys loses more than half the weight" (cap 2, the even heads)
        ro, _ = pr.expected((127, 0), 2.0)
        mo, _ = pr.expected((127, 0), 2.0, "cap applied after the mask")
        live = ro[3, 0] != 0
        assert np.all(np.abs(mo[3, 0][live]) < 0.5 * np.abs(ro[3, 0][live]))

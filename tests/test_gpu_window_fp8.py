"""-m gpu: the FP8 P.V mode of sliding-window attention (fp8_attn_varlen_window_pv_func / fp8_window_attn_pv_func with pv_precision="fp8",
qattn_fp8_quant_attention_varlen_window_forward_fp8pv, include/qattn_window.h) on the MI355X.

Grading: per sequence an fp64 windowed softmax written here (torch.float64) on the operands the call RETURNS -- its q8 slab, its k8 / v8
images and the three scales, unpacked as tests/test_gpu_varlen_fp8.py does; bound gpu_utils.grade with a plain array,
|got - ref| < 2^-6 max(1, |ref| / 2); LSE within 2e-3 (exact exponentials whenever the LSE is asked for); the -inf pattern equal to the
reference's.  The returned bytes and scales equal the CPU quantiser's per sequence over the used keys, bit for bit, and row_path equals the
literal rule of tests/window_fp8_cases.py.  Then what needs no tolerance (windows that mask nothing or the causal triangle against the
packed FP8-PV entry, the 16-bit default against the released function, the one-key window), other key lengths, seqused_k, keys outside a
tile's swept chunks, the membership probes, and the structure of the entry."""
import functools
import math

import numpy as np
import pytest
import torch

import oracle
import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import gpu_utils
from tests import probes as P
from tests import window_fp8_cases as W
from tests.gpu_utils import TDT, bits8
from tests.gpu_utils import FMT, bits16, fmt16
from tests.test_gpu_varlen_fp8 import _image, _operands

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE, TWO = W.ONE, W.TWO
LSE_TOL = 2e-3
LENS = [300, 1, 700, 0, 65, 1300]      # 1300 crosses the 1024-key rule; 700: six tiles; 1 and 65: one key / one key past a chunk; 0: no rows
LENS_256 = [300, 1, 0, 65, 1300]
# tests/test_gpu_window.py's ten (edges at 63 / 64 / 65 and 0 / 1 / 64), and two whose FAST one-term tiles start above chunk 0
WINDOWS = [(0, 0), (16, 0), (63, 0), (64, 0), (65, 1), (100, 37), (0, 64), (-1, 0), (5, -1), (128, 128), (1024, 0), (600, 500)]


def _cu(lengths):
    return torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32, device=DEV)


def _starts(lengths):
    return [int(x) for x in np.cumsum([0] + list(lengths))[:-1]]


def _rand(n, H, D, dtype, g):
    return torch.randn(n, H, D, generator=g, device=DEV, dtype=torch.float32).to(dtype)


def _same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32),
                       y.contiguous().view(torch.int16 if y.element_size() == 2 else torch.int32))


def _batch(D, dtype, seed, lq=None, lk=None, Hq=None, Hkv=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    lq = lq or (LENS_256 if D == 256 else LENS)
    lk = lk or lq
    Hq, Hkv = Hq or (2 if D == 256 else 4), Hkv or (1 if D == 256 else 2)
    return _rand(sum(lq), Hq, D, dtype, g), _rand(sum(lk), Hkv, D, dtype, g), _rand(sum(lk), Hkv, D, dtype, g), lq, lk


def _call(q, k, v, lq, lk, window, *, used=None, cu_k=None, fp8="e4m3", precision="accurate", scale=None, lse=True, smooth_k=False):
    """(out, lse | None, q8, k8, v8, sq, sk, sv, [k_mean], path)"""
    res = _native.fp8_quant_attention_varlen_window_fp8pv(
        q, k, v, _cu(lq), _cu(lk) if cu_k is None else cu_k, used, window_left=window[0], window_right=window[1], fp8_dtype=TDT[fp8],
        sm_scale=0.0 if scale is None else scale, precision=precision, return_lse=lse, return_quant=True, return_path=True, smooth_k=smooth_k)
    return res if lse else (res[0], None) + tuple(res[1:])


def _pub(q, k, v, lq, lk, window, precision, *, lse=True, **kw):
    return qa.fp8_attn_varlen_window_pv_func(q, k, v, _cu(lq), _cu(lk), max(lq), max(lk), window, return_lse=lse, pv_precision="fp8",
                                             precision=precision, **kw)


def _check_quantiser(res, q, k, v, lq, lk, fp8):
    """the returned bytes and scales are oracle.quantize_fp8's per sequence over the used keys (a sequence without rows / keys: nothing)"""
    ops = _operands(res, lq, lk)
    for i, (a, n, b, m) in enumerate(zip(_starts(lq), lq, _starts(lk), lk)):
        for x, s0, cnt, got8, gots in ((q, a, n, ops[i][0], ops[i][3]), (k, b, m, ops[i][1], ops[i][4]), (v, b, m, ops[i][2], ops[i][5])):
            if cnt == 0:
                continue
            rb, rs = oracle.quantize_fp8(bits16(x[s0:s0 + cnt].transpose(0, 1)[None]), fmt16(x.dtype), "head", FMT[fp8], "compiled")
            assert np.array_equal(got8, rb), (i, "bytes")
            assert np.array_equal(gots.view(np.uint32), rs.view(np.uint32)), (i, "scale")


def _deq(b, fp8, s):
    """bytes [1, H, n, D] (numpy) and scales [1, H] -> float64 [H, n, D] on the device"""
    t = torch.from_numpy(np.ascontiguousarray(b)).to(DEV).view(TDT[fp8]).double()[0]
    return t * torch.from_numpy(np.asarray(s, np.float64)).to(DEV)[0][:, None, None]


def _ref64(ops, window, scale, fp8, D):
    """fp64 windowed softmax on the returned operands: (out [total_q, Hq, D], lse [Hq, total_q]); a row without a key: zeros, -inf"""
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    outs, lses = [], []
    for qi, ki, vi, sq, sk, sv in ops:
        Hq, n, m = qi.shape[1], qi.shape[2], ki.shape[2]
        if n == 0 or m == 0:
            outs.append(np.zeros((n, Hq, D)))
            lses.append(np.full((Hq, n), -np.inf))
            continue
        q, k, v = _deq(qi, fp8, sq), _deq(ki, fp8, sk), _deq(vi, fp8, sv)
        rep = Hq // k.shape[0]
        k, v = k.repeat_interleave(rep, 0), v.repeat_interleave(rep, 0)
        s = (q @ k.transpose(-1, -2)) * scale
        s = s.masked_fill(~torch.from_numpy(W.alive(n, m, window)).to(DEV)[None], -math.inf)
        l = torch.logsumexp(s, -1)
        p = torch.exp(s - l.clamp_min(-1e300)[..., None])
        outs.append((p @ v).transpose(0, 1).cpu().numpy())
        lses.append(l.cpu().numpy())
    return np.concatenate(outs, 0), np.concatenate(lses, 1)


def _grade(res, ref, ref_lse, what, lse_shift=None):
    out = gpu_utils.out_to_f32(res[0])
    dead = np.isneginf(ref_lse)
    assert not np.isnan(out).any(), what
    assert (out[dead.T] == 0).all(), (what, "rows without a key must be exactly 0")
    worst = gpu_utils.grade(out, ref)[2]
    worst_lse = 0.0
    if res[1] is not None:
        l = res[1].cpu().numpy()
        assert np.array_equal(np.isneginf(l), dead), what
        want = ref_lse if lse_shift is None else ref_lse + lse_shift
        worst_lse = float(np.abs(l[~dead] - want[~dead]).max()) if (~dead).any() else 0.0
    print(f"{what}: worst |err| / bound {worst:.3f}, worst LSE error {worst_lse:.2e}")
    assert worst < 1.0, (what, worst)
    assert worst_lse < LSE_TOL, (what, worst_lse)
    return worst, worst_lse


# ---- 1. / 2. parity on the returned operands, the quantiser, the path table -----------------------------------------------------------------
@pytest.mark.parametrize("dtype,fp8", [(torch.bfloat16, "e4m3"), (torch.float16, "e5m2")], ids=["bf16-e4m3", "fp16-e5m2"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_every_row_is_within_the_fp8_v_bound_of_the_fp64_windowed_softmax(D, dtype, fp8):
    q, k, v, lq, lk = _batch(D, dtype, 500 + D)
    Hq = q.shape[1]
    ops = None
    top = (0.0, 0.0)
    saw_one_above_chunk0 = False
    for window in WINDOWS:
        ref = None
        for precision in ("accurate", "fast"):   # (default scale: scale^2 D = 1 on N(0, 1) data, FAST's stated domain)
            what = f"D{D} {fp8} {window} {precision}"
            res = _call(q, k, v, lq, lk, window, fp8=fp8, precision=precision)
            if ops is None:   # (the quantised operands depend on neither the window nor the precision)
                _check_quantiser(res, q, k, v, lq, lk, fp8)
                ops = _operands(res, lq, lk)
                first = res
            else:
                assert all(torch.equal(res[j], first[j]) for j in (2, 5, 6, 7)), what
            if ref is None:
                ref = _ref64(ops, window, None, fp8, D)
            want_path = W.expected_path(lq, lk, Hq, window, precision)
            assert np.array_equal(res[-1].cpu().numpy(), want_path), what
            assert precision == "fast" or (want_path == TWO).all()
            top = tuple(max(a, b) for a, b in zip(top, _grade(res, ref[0], ref[1], what)))
            res_n = _call(q, k, v, lq, lk, window, fp8=fp8, precision=precision, lse=False)
            assert np.array_equal(res_n[-1].cpu().numpy(), want_path), what
            if precision == "accurate":   # asking for the LSE changes no bit of out
                assert _same_bits(res_n[0], res[0]), what
            else:                         # the one-term tiles run the byte-exponential sweep without the LSE: the same bound and table
                top = (max(top[0], _grade(res_n, ref[0], ref[1], what + " (byte)")[0]), top[1])
                two = torch.from_numpy(want_path.T == TWO).to(DEV)
                assert torch.equal(res_n[0][two], res[0][two]), what
                if window in ((1024, 0), (600, 500)):
                    n = lq[-1]
                    tiles = [t for t in range((n + 127) // 128) if W.tile_is_one_term(n, n, window[0], window[1], t, "fast")]
                    saw_one_above_chunk0 |= any(W.tile_interval(n, n, window[0], window[1], t)[0] >= 64 for t in tiles)
    assert saw_one_above_chunk0, "FAST must have one-term tiles whose interval starts above chunk 0"
    print(f"D{D} {fp8}: worst |err| / bound {top[0]:.3f}, worst LSE error {top[1]:.2e} over {len(WINDOWS)} windows x 2 precisions")


# ---- 3. what needs no tolerance --------------------------------------------------------------------------------------------------------------
def _packed(q, k, v, lq, lk, causal, precision, lse):
    res = _native.fp8_quant_attention_varlen_fp8pv(q, k, v, _cu(lq), _cu(lk), None, is_causal=causal, precision=precision, return_lse=lse,
                                                   return_path=True)
    return res if lse else (res[0], None, res[1])


@pytest.mark.parametrize("precision", ["accurate", "fast"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_windows_that_mask_nothing_or_the_causal_triangle_equal_the_packed_fp8pv_entry(D, precision):
    q, k, v, lq, _ = _batch(D, torch.bfloat16, 600 + D)
    g = torch.Generator(device=DEV).manual_seed(601)
    lk = [170, 40, 1300, 9, 500, 1100][:len(lq)] if D != 256 else [170, 40, 9, 500, 1100]
    kx, vx = _rand(sum(lk), k.shape[1], D, torch.bfloat16, g), _rand(sum(lk), k.shape[1], D, torch.bfloat16, g)
    for lse in (True, False):
        for kk, vv, lkk in ((k, v, lq), (kx, vx, lk)):
            want = _packed(q, kk, vv, lq, lkk, False, precision, lse)
            for window in ((-1, -1), (5000, 5000), (5000, -1), (-1, 2 ** 31 - 1)):
                got = _call(q, kk, vv, lq, lkk, window, precision=precision, lse=lse)
                assert _same_bits(got[0], want[0]) and torch.equal(got[-1], want[-1]), (window, lse)
                assert not lse or _same_bits(got[1], want[1]), window
        want = _packed(q, k, v, lq, lq, True, precision, lse)
        got = _call(q, k, v, lq, lq, (-1, 0), precision=precision, lse=lse)
        assert _same_bits(got[0], want[0]) and torch.equal(got[-1], want[-1]) and (not lse or _same_bits(got[1], want[1])), ("causal", lse)


def test_the_default_call_gives_the_released_functions_bits():
    q, k, v, lq, _ = _batch(128, torch.bfloat16, 30)
    cu = _cu(lq)
    for window in ((16, 0), (100, 37)):
        want = qa.fp8_attn_varlen_window_func(q, k, v, cu, cu, max(lq), max(lq), window, return_lse=True)
        for kw in ({}, {"pv_precision": "16bit"}, {"pv_precision": "16bit", "precision": "accurate"}):
            got = qa.fp8_attn_varlen_window_pv_func(q, k, v, cu, cu, max(lq), max(lq), window, return_lse=True, **kw)
            assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), kw
        assert not _same_bits(_pub(q, k, v, lq, lq, window, "accurate")[0], want[0])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_the_one_key_window_returns_each_rows_dequantised_fp8_v(D, dtype):
    """(0, 0) with Hq = Hkv and L_q = L_k under ACCURATE: every row attends its own key alone, so out is v8 scale_v in the output format.
    Not bit for bit on the machine (measured, bf16: 76 of 302848 elements at D = 64, 1 of 605696 at D = 128, 732 of 852992 at D = 256): the
    exponent's argument fma(s, c, shift - fl(m c)) is rounded, P' = 2^(shift + eps) has the power of two as its e4m3 high term but the fp32
    row sum keeps eps, and sv / l' moves the product across a rounding boundary of the output format on a few elements.
    Held to the parity bound against v8 scale_v in fp64; the count of differing elements is printed."""
    H = 2
    q, k, v, lq, _ = _batch(D, dtype, 700 + D, Hq=H, Hkv=H)
    res = _call(q, k, v, lq, lq, (0, 0))
    ops = _operands(res, lq, lq)
    # fp32(v8) * scale_v: one rounding, then the output format's
    want = (torch.cat([torch.from_numpy(np.ascontiguousarray(o[2])).to(DEV).view(TDT["e4m3"]).float()[0]
                       * torch.from_numpy(o[5]).to(DEV)[0][:, None, None] for o in ops if o[0].shape[2]], 1)).transpose(0, 1).to(dtype)
    bad = int((res[0].view(torch.int16) != want.contiguous().view(torch.int16)).sum())
    print(f"one-key window D{D} {dtype}: {bad} of {want.numel()} elements differ from round(v8 scale_v)")
    # A ceiling on the count, from the arithmetic and not from the measurement: the exponent's argument is a few units in size (shift
    # and (s - m) c = 0), rounded to fp32 with |s c| up to 2^5: an absolute error of at most 2^-19, so l' is off by a relative
    # 2^-19 ln 2 (+ 2^-23 of exp2 itself) < 2^-19.  An element flips iff v8 scale_v lies that close to a rounding boundary of the output
    # format, whose boundaries are a relative 2^-8 (bf16) apart or more: a share of at most 2 * 2^-19 / 2^-8 = 2^-10 of the elements
    # for values spread over a binade.  Twice that is allowed; more means something other than this rounding moved the output.
    assert bad <= want.numel() * 2.0 ** -9, (bad, want.numel())
    ref = np.concatenate([(_deq(o[2], "e4m3", o[5])).transpose(0, 1).cpu().numpy() for o in ops if o[0].shape[2]], 0)
    worst = gpu_utils.grade(gpu_utils.out_to_f32(res[0]), ref)[2]
    print(f"one-key window D{D} {dtype}: worst |err| / bound {worst:.4f}")
    assert worst < 1.0
    assert (res[-1] == TWO).all() and torch.isfinite(res[1]).all()


# ---- 4. other key lengths, seqused_k, keys outside a tile's swept chunks --------------------------------------------------------------------
CROSS_LQ, CROSS_LK = [300, 200, 100, 1300], [170, 500, 100, 1090]   # L_q > L_k: rows 0 .. 129 of sequence 0 have no key under right = 0 --
#                                                                     tile 1 holds rows 128, 129 without a key beside rows with keys


@pytest.mark.parametrize("D", [64, 128, 256])
def test_other_key_lengths_with_rows_without_a_key_inside_a_tile_that_sweeps(D):
    q, k, v, lq, lk = _batch(D, torch.bfloat16, 800 + D, lq=CROSS_LQ, lk=CROSS_LK)
    Hq = q.shape[1]
    ops = None
    for window in ((16, 0), (0, 0), (100, 37), (-1, 0), (1024, 0), (0, 64)):
        ref = None
        for precision in ("accurate", "fast"):
            for lse in (True, False):
                res = _call(q, k, v, lq, lk, window, precision=precision, lse=lse)
                ops = ops or _operands(res, lq, lk)
                ref = ref or _ref64(ops, window, None, "e4m3", D)
                want_path = W.expected_path(lq, lk, Hq, window, precision)
                assert np.array_equal(res[-1].cpu().numpy(), want_path), (window, precision)
                _grade(res, ref[0], ref[1], f"cross D{D} {window} {precision} lse {lse}")
        if window[1] == 0:
            dead = np.isneginf(ref[1])
            assert dead[:, :130].all() and not dead[:, 130:300].any()
            assert (want_path[:, :128] == ONE).all() and (want_path[:, 128:300] == TWO).all()   # a keyless row carries its tile's code


@pytest.mark.parametrize("precision", ["accurate", "fast"])
def test_seqused_k_on_padded_kv_equals_the_trimmed_call_whatever_the_padding_holds(precision):
    g = torch.Generator(device=DEV).manual_seed(3)
    B, S_pad, H, D = 3, 1344, 4, 128
    k_lens, lq = [1300, 100, 1], [1300, 300, 64]
    q = _rand(sum(lq), H, D, torch.bfloat16, g)
    kp, vp = (torch.randn(B, S_pad, H, D, generator=g, device=DEV).bfloat16() for _ in range(2))
    cu_k = torch.arange(B + 1, dtype=torch.int32, device=DEV) * S_pad
    used = torch.tensor(k_lens, dtype=torch.int32, device=DEV)
    kt = torch.cat([kp[i, :n] for i, n in enumerate(k_lens)])
    vt = torch.cat([vp[i, :n] for i, n in enumerate(k_lens)])
    for window in ((1024, 0), (37, 100)):
        want = _call(q, kt, vt, lq, k_lens, window, precision=precision)
        w_ops = _operands(want, lq, k_lens)
        for fill in (1e4, float("nan")):
            k2, v2 = kp.clone(), vp.clone()
            for i, n in enumerate(k_lens):
                k2[i, n:], v2[i, n:] = fill, fill
            got = _call(q, k2.view(B * S_pad, H, D), v2.view(B * S_pad, H, D), lq, k_lens, window, used=used, cu_k=cu_k, precision=precision)
            assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), fill
            assert torch.equal(got[7], want[7]) and torch.equal(got[-1], want[-1]), fill
            for go, wo in zip(_operands(got, lq, k_lens, [i * S_pad for i in range(B)]), w_ops):
                assert all(np.array_equal(x, y) for x, y in zip(go, wo)), fill


@pytest.mark.parametrize("precision", ["accurate", "fast"])
def test_keys_outside_a_tiles_swept_chunks_change_no_bit_of_its_rows(precision):
    """K and V negated at every key outside the 64-key chunks klo / 64 .. khi / 64 of a tile: the head's abs-max element sits at key 600,
    inside the interval of every tile under test, so no scale moves -- and no bit of the tile's rows may"""
    g = torch.Generator(device=DEV).manual_seed(56)
    n, H, D = 1300, 2, 128
    q, k, v = (_rand(n, H, D, torch.bfloat16, g) for _ in range(3))
    k[600, :, 0] = 8.0
    v[600, :, 0] = 8.0
    for window, t in (((100, 37), 5), ((1024, 0), 9), ((600, 500), 4)):
        klo, khi = W.tile_interval(n, n, window[0], window[1], t)
        lo, hi = klo // 64 * 64, min((khi // 64 + 1) * 64, n)
        assert lo <= 600 < hi and (lo > 0 or hi < n)
        assert W.tile_is_one_term(n, n, window[0], window[1], t, precision) == (precision == "fast" and window != (100, 37))
        k2, v2 = k.clone(), v.clone()
        for x in (k2, v2):
            x[:lo] *= -1
            x[hi:] *= -1
        rows = slice(128 * t, min(128 * (t + 1), n))
        for lse in (False, True):
            a = _call(q, k, v, [n], [n], window, precision=precision, lse=lse)
            b = _call(q, k2, v2, [n], [n], window, precision=precision, lse=lse)
            assert torch.equal(a[5], b[5]) and torch.equal(a[6], b[6]) and torch.equal(a[7], b[7])   # the scales
            assert _same_bits(a[0][rows], b[0][rows]) and (not lse or _same_bits(a[1][:, rows], b[1][:, rows])), (window, lse)
            assert not _same_bits(a[0], b[0]), "the negated keys are attended by other tiles"


# ---- 5. membership probes (tests/probes.py; teeth: tests/test_cpu_window_fp8.py) ----------------------------------------------------------------
def _T(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _probe_case(probe, D, window, lq, lk):
    case = W.make_probe(probe, D, window, list(lq), list(lk))
    return case, case.reference()


@pytest.mark.parametrize("D", [64, 128, 256])
def test_count_decoy_and_pointer_probes_through_the_window_fp8pv_entry(D):
    """exact-answer inputs on which one misplaced key moves the output by >= 4x the bound.  The count probe's rows are flat: both
    precisions; the decoy and pointer probes' rows are peaked: ACCURATE (FAST has no rescue)."""
    res = {}
    for probe, window, lq, lk in W.probe_cases(D):
        case, (ref, ref_lse) = _probe_case(probe, D, window, tuple(lq), tuple(lk))
        q, k, v = _T(case.q, torch.bfloat16), _T(case.k, torch.bfloat16), _T(case.v, torch.bfloat16)
        dead = np.isneginf(ref_lse).T
        for precision in ("accurate", "fast") if probe == "count" else ("accurate",):
            for lse in (True, False):
                got = _pub(q, k, v, case.lq, case.alloc, window, precision, lse=lse)
                out = gpu_utils.out_to_f32(got[0] if lse else got)
                name = f"{probe} {window} {'cross' if lq != lk else 'self'} {precision}{'' if lse else ' (no lse)'}"
                assert (out[dead] == 0).all(), (name, "rows without a key must be exactly 0")
                res[name] = float((np.abs(out - ref) / P.project_bound(ref, False)).max())
                if lse:
                    l = got[1].cpu().numpy()
                    assert np.array_equal(np.isneginf(l), dead.T), name
                    if probe != "count":   # (the count probe's expected LSE reads the quantised q: graded by the parity sweep instead)
                        live = ~dead.T
                        res[name + " lse"] = float(np.abs(l[live] - ref_lse[live]).max() / LSE_TOL)
    print(f"probes D {D}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert all(v < 1.0 for v in res.values()), {k: v for k, v in res.items() if v >= 1.0}


# ---- 6. structure ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["accurate", "fast"])
def test_empty_batch_entries_are_defined(precision):
    g = torch.Generator(device=DEV).manual_seed(4)
    lq, lk, H, D = [300, 0, 257, 40], [1100, 9, 0, 70], 4, 64
    q, k, v = _rand(sum(lq), H, D, torch.bfloat16, g), _rand(sum(lk), H, D, torch.bfloat16, g), _rand(sum(lk), H, D, torch.bfloat16, g)
    for window in ((16, 0), (-1, -1)):
        for lse in (True, False):
            res = _call(q, k, v, lq, lk, window, precision=precision, lse=lse)
            assert (res[0][300:557] == 0).all() and (res[-1][:, 300:557] == ONE).all()
            assert not lse or (res[1][:, 300:557] == -math.inf).all()
            assert np.array_equal(res[-1].cpu().numpy(), W.expected_path(lq, lk, H, window, precision))
            ref = _ref64(_operands(res, lq, lk), window, None, "e4m3", D)
            _grade(res, ref[0], ref[1], f"empty {window} {precision} lse {lse}")


def test_strided_slices_of_a_packed_qkv_projection_equal_the_contiguous_call():
    g = torch.Generator(device=DEV).manual_seed(2)
    lens, H, D = [33, 300, 64], 4, 64
    qkv = _rand(sum(lens), 3 * H, D, torch.bfloat16, g).view(sum(lens), 3, H, D)
    q, k, v = qkv.unbind(1)
    assert not v.is_contiguous() and _native.varlen_strided_ok(v)
    for window in ((16, 0), (37, 100)):
        res = _call(q, k, v, lens, lens, window)
        dense = _call(q.contiguous(), k.contiguous(), v.contiguous(), lens, lens, window)
        assert _same_bits(res[0], dense[0]) and _same_bits(res[1], dense[1])
        assert all(torch.equal(res[j], dense[j]) for j in (2, 5, 6, 7, 8))
        for go, wo in zip(_operands(res, lens, lens), _operands(dense, lens, lens)):
            assert all(np.array_equal(x, y) for x, y in zip(go, wo))


def test_graph_replay_follows_rewritten_tables():
    g = torch.Generator(device=DEV).manual_seed(6)
    H, D, total = 8, 128, 2400
    q, k, v = (_rand(total, H, D, torch.bfloat16, g) for _ in range(3))
    cu_q, cu_k = _cu([100, 1500, 800]), _cu([300, 1300, 800])
    used = torch.tensor([300, 1200, 800], dtype=torch.int32, device=DEV)
    call = lambda: qa.fp8_attn_varlen_window_pv_func(q, k, v, cu_q, cu_k, 1500, 1500, (1024, 0), seqused_k=used, return_lse=True,
                                                     pv_precision="fp8", precision="fast")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = call()
    cu_q.copy_(_cu([1250, 50, 1100]))
    cu_k.copy_(_cu([1, 1299, 1100]))
    used.copy_(torch.tensor([1, 1111, 64], dtype=torch.int32, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    want = call()
    assert _same_bits(out, want[0]) and _same_bits(lse, want[1])
    # ... which is the call on fresh tables of the same contents
    kt = torch.cat([k[0:1], k[1:1112], k[1300:1364]])
    vt = torch.cat([v[0:1], v[1:1112], v[1300:1364]])
    fresh = _pub(q, kt, vt, [1250, 50, 1100], [1, 1111, 64], (1024, 0), "fast")
    assert _same_bits(out, fresh[0]) and _same_bits(lse, fresh[1])


def test_torch_compile_fullgraph_gives_the_eager_bits():
    g = torch.Generator(device=DEV).manual_seed(8)
    lens, H, D = [200, 1300, 77], 8, 128
    q, k, v = (_rand(sum(lens), H, D, torch.float16, g) for _ in range(3))
    cu = _cu(lens)

    def f(q, k, v, cu):
        return qa.fp8_attn_varlen_window_pv_func(q * 2, k, v, cu, cu, 1300, 1300, (1024, 5), softmax_scale=0.04, return_lse=True,
                                                 pv_precision="fp8", precision="fast")

    torch._dynamo.reset()
    got = torch.compile(f, fullgraph=True)(q, k, v, cu)
    want = f(q, k, v, cu)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])


@pytest.mark.parametrize("D", [64, 128, 256])
def test_key_smoothing_on_offset_keys(D):
    """k_mean / scale_k / k8 bit-equal to the packed smoothing entry; out against the fp64 reference on the returned (smoothed) operands;
    the LSE that of the true scores (corrected by scale * q.k_mean); rows without a key stay at -inf"""
    g = torch.Generator(device=DEV).manual_seed(28 + D)
    lq, lk = [300, 65, 700], [170, 65, 1100]
    Hq, Hkv = (2, 1) if D == 256 else (4, 2)
    q, k, v = _rand(sum(lq), Hq, D, torch.bfloat16, g), _rand(sum(lk), Hkv, D, torch.bfloat16, g), _rand(sum(lk), Hkv, D, torch.bfloat16, g)
    k = (k.float() + 16.0 * torch.randn(1, Hkv, D, generator=g, device=DEV)).to(torch.bfloat16)   # a sigma = 16 offset per channel
    r16 = _native.fp8_quant_attention_varlen(q, k, v, _cu(lq), _cu(lk), None, return_quant=True, smooth_k=True)   # (out, q8, k8, sq, sk, k_mean)
    for window in ((16, 0), (100, 37)):
        for precision in ("accurate", "fast"):
            res = _call(q, k, v, lq, lk, window, precision=precision, smooth_k=True)   # (out, lse, q8, k8, v8, sq, sk, sv, k_mean, path)
            assert torch.equal(res[6], r16[4]) and torch.equal(res[8], r16[5]) and torch.equal(res[2], r16[1])
            for i, (b, m) in enumerate(zip(_starts(lk), lk)):
                assert np.array_equal(_image(bits8(res[3]), _native.LAYOUT_KFRAG, b, i, m, Hkv, D), _image(bits8(r16[2]), _native.LAYOUT_KFRAG, b, i, m, Hkv, D))
            ref = _ref64(_operands(res, lq, lk), window, None, "e4m3", D)
            shift = np.concatenate([(q[a:a + n].double().transpose(0, 1) * res[8][i].double().repeat_interleave(Hq // Hkv, 0)[:, None, :]).sum(-1)
                                    .cpu().numpy() / math.sqrt(D) for i, (a, n) in enumerate(zip(_starts(lq), lq))], 1)
            _grade(res, ref[0], ref[1], f"smooth D{D} {window} {precision}", lse_shift=shift)
            if window[1] == 0:
                assert (res[1][:, :130] == -math.inf).all() and torch.isfinite(res[1][:, 130:]).all()
            with qa.config.patch({"attention.smooth_k": True}):
                po, pl = _pub(q, k, v, lq, lk, window, precision)
            assert _same_bits(po, res[0]) and _same_bits(pl, res[1])


@pytest.mark.parametrize("precision", ["accurate", "fast"])
def test_dense_call_shape_is_the_packed_call_on_views(precision):
    g = torch.Generator(device=DEV).manual_seed(12)
    B, Hq, Hkv, Sq, Skv, D = 2, 4, 2, 1200, 1300, 128
    q = torch.randn(B, Sq, Hq, D, generator=g, device=DEV).bfloat16().permute(0, 2, 1, 3)      # [B, S, H, D] memory: free views
    k, v = (torch.randn(B, Hkv, Skv, D, generator=g, device=DEV).bfloat16() for _ in range(2))  # contiguous [B, H, S, D]: one copy each
    out, lse = qa.fp8_window_attn_pv_func(q, k, v, (1024, 3), return_lse=True, pv_precision="fp8", precision=precision)
    assert out.shape == (B, Hq, Sq, D) and lse.shape == (B, Hq, Sq)
    pk = lambda t: t.permute(0, 2, 1, 3).reshape(-1, t.shape[1], D)
    po, pl = _pub(pk(q), pk(k), pk(v), [Sq] * B, [Skv] * B, (1024, 3), precision)
    assert _same_bits(out, po.view(B, Sq, Hq, D).permute(0, 2, 1, 3)) and _same_bits(lse, pl.view(Hq, B, Sq).permute(1, 0, 2))
    no = qa.fp8_window_attn_pv_func(q, k, v, (1024, 3), pv_precision="fp8", precision=precision)
    assert _same_bits(no, _pub(pk(q), pk(k), pk(v), [Sq] * B, [Skv] * B, (1024, 3), precision, lse=False).view(B, Sq, Hq, D).permute(0, 2, 1, 3))
    d16 = qa.fp8_window_attn_pv_func(q, k, v, (1024, 3), return_lse=True)
    w16 = qa.fp8_window_attn_func(q, k, v, (1024, 3), return_lse=True)
    assert _same_bits(d16[0], w16[0]) and _same_bits(d16[1], w16[1])


@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "smooth"])
@pytest.mark.parametrize("precision,window", [("accurate", (16, 0)), ("fast", (1024, 37))])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_the_c_entry_on_guarded_buffers_of_exactly_the_documented_sizes(D, precision, window, smooth):
    """tests/arena.py through the Plan of tests/test_gpu_buffer_contract.py: guards intact, every documented byte written, bits equal to the
    ordinary call, no dependence on what the workspace / scratch held or on bytes outside the inputs.  k8 / v8: the images of the used keys do
    not tile their buffers (scratch between them)."""
    from tests.test_gpu_buffer_contract import ALIGN1, ALIGN4, HKV, HQ, Plan, _stream

    L = _native.lib()
    LQ, LK_ALLOC, USED = [65, 3, 257, 1300], [130, 9, 300, 1344], [129, 0, 200, 1300]
    g = torch.Generator().manual_seed(77 + D)
    tq, tk, nb = sum(LQ), sum(LK_ALLOC), len(LQ)
    q = torch.randn(tq, HQ, D, generator=g)
    k, v = (torch.randn(tk, HKV, D, generator=g) for _ in range(2))
    cu_q, cu_k, used = _cu(LQ), _cu(LK_ALLOC), torch.tensor(USED, dtype=torch.int32, device=DEV)
    for b, u, a in zip(_starts(LK_ALLOC), USED, LK_ALLOC):   # keys beyond seqused_k influence no output bit: NaN there
        k[b + u:b + a] = float("nan")
        v[b + u:b + a] = float("nan")
    q, k, v = (t.to(torch.bfloat16).to(DEV) for t in (q, k, v))
    res = _call(q, k, v, LQ, LK_ALLOC, window, used=used, precision=precision, smooth_k=smooth)
    want = {"out": res[0], "lse": res[1], "q8": res[2], "scale_q": res[5], "scale_k": res[6], "scale_v": res[7], "row_path": res[-1]}
    p = Plan()
    pq, pk, pv = p.inp("q", q, row_bytes=2 * HQ * D), p.inp("k", k, row_bytes=2 * HKV * D), p.inp("v", v, row_bytes=2 * HKV * D)
    pcq, pck, pu = (p.inp(n, t, align=ALIGN4) for n, t in (("cu_seqlens_q", cu_q), ("cu_seqlens_k", cu_k), ("seqused_k", used)))
    po = p.out("out", 2 * tq * HQ * D, "bf16", row_bytes=2 * HQ * D)
    pl = p.out("lse", 4 * HQ * tq, "fp32", align=ALIGN4)
    pq8 = p.out("q8", L.qattn_varlen_tensor_bytes(_native.LAYOUT_ROWMAJOR, nb, HQ, tq, D), "fp8", row_bytes=D)
    psq, psk, psv = (p.out(n, 4 * nb * h, "fp32", align=ALIGN4) for n, h in (("scale_q", HQ), ("scale_k", HKV), ("scale_v", HKV)))
    pp = p.out("row_path", HQ * tq, "path", align=ALIGN1)
    frag = L.qattn_varlen_tensor_bytes(_native.LAYOUT_KFRAG, nb, HKV, tk, D)
    pk8, pv8 = p.scratch("k8", frag, row_bytes=D), p.scratch("v8", frag, row_bytes=D)
    pm = None
    if smooth:
        want["k_mean"] = res[8]
        pm = p.out("k_mean", 4 * nb * HKV * D, "fp32")
    ws_of = L.qattn_fp8_quant_attention_varlen_fp8pv_smooth_workspace_bytes if smooth else L.qattn_fp8_quant_attention_varlen_fp8pv_workspace_bytes
    wb = ws_of(nb, HQ, HKV, tq, tk, D)
    pw = p.scratch("workspace", wb, row_bytes=D)
    call = lambda: L.qattn_fp8_quant_attention_varlen_window_forward_fp8pv(
        pq, pk, pv, None, _native.fmt_of(torch.bfloat16), po, pl, pcq, pck, pu, nb, HQ, HKV, tq, tk, D, _native.FMT_E4M3, 0, window[0], window[1],
        0.0, _native.PRECISION[precision], pq8, pk8, pv8, psq, psk, psv, pp, pm, pw, wb, _stream())
    first = p.check(call, want)
    for name, j, layout in (("k8", 3, _native.LAYOUT_KFRAG), ("v8", 4, _native.LAYOUT_VFRAG)):
        got8 = p.ar[name].interior.cpu().numpy()
        for i, (b, m) in enumerate(zip(_starts(LK_ALLOC), USED)):
            assert np.array_equal(_image(got8, layout, b, i, m, HKV, D), _image(bits8(res[j]), layout, b, i, m, HKV, D)), (name, i)
    out = first["out"].view(torch.bfloat16).view(tq, HQ, D)
    assert (out[65:68].view(torch.int16) == 0).all() and (first["lse"].view(torch.float32).view(HQ, tq)[:, 65:68] == -math.inf).all()
    # sequence 2: 257 queries on 200 used keys -- under right = 0 its first 57 rows have no key
    if window[1] == 0:
        assert (out[68:68 + 57].view(torch.int16) == 0).all()

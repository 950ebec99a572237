"""-m gpu: the FP8 P.V mode of packed variable-length attention (fp8_attn_varlen_pv_func(..., pv_precision="fp8"),
qattn_fp8_quant_attention_varlen_forward_fp8pv, include/qattn_varlen.h) on the MI355X.

Grading: per sequence the fp64 oracle (oracle.attention_forward) on the entry's own q8 slab and k8 / v8 images with the three scales; bound
gpu_utils.grade with a plain array, |got - ref| < 2^-6 max(1, |ref| / 2); LSE within 2e-3 (exact exponentials whenever the LSE is asked
for).  The returned bytes and scales equal the CPU quantiser's per sequence over the used keys, bit for bit, and row_path equals a literal
restatement of the key-count rule.  Then what needs no tolerance: every non-causal sequence equals the block-sparse FP8-PV call on that
sequence alone, a per-sequence gain on V moves only that sequence's scale, keys no causal tile may read change no bit, padded K / V with
seqused_k equal the trimmed call -- and the structure of the entry: empty sequences, strided inputs, graph replay, torch.compile, the eager
fallback, key smoothing, the buffer contract and the default call."""
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
from tests.gpu_utils import FMT, TDT, bits8, bits16, fmt16, unpack_frag

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE, TWO = 0, 1   # include/qattn.h QATTN_PATH_ONE_TERM / _TWO_TERM (literal: the header is the contract)
LSE_TOL = 2e-3
TILE = 128
LENS = [1, 63, 64, 65, 129, 300, 1100]   # 1100 crosses the 1024-key rule; causal tiles from row 896 on are one-term under FAST
LENS_256 = [1, 65, 384, 1300]


def _cu(lengths):
    return torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32, device=DEV)


def _starts(lengths):
    return [int(x) for x in np.cumsum([0] + list(lengths))[:-1]]


def _rand(n, H, D, dtype, g):
    return torch.randn(n, H, D, generator=g, device=DEV, dtype=torch.float32).to(dtype)


def _same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32),
                       y.contiguous().view(torch.int16 if y.element_size() == 2 else torch.int32))


def _shape(D):
    """(lengths, Hq, Hkv) of the base batch"""
    return (LENS_256, 2, 1) if D == 256 else (LENS, 4, 2)


def _batch(D, dtype, seed, lens=None, Hq=None, Hkv=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    l0, h0, hk0 = _shape(D)
    lens, Hq, Hkv = lens or l0, Hq or h0, Hkv or hk0
    return _rand(sum(lens), Hq, D, dtype, g), _rand(sum(lens), Hkv, D, dtype, g), _rand(sum(lens), Hkv, D, dtype, g), lens


def _call(q, k, v, lq, lk, *, used=None, cu_k=None, causal=False, fp8="e4m3", precision="accurate", scale=None, lse=True, smooth_k=False,
          numerics="compiled"):
    """(out, lse | None, q8, k8, v8, sq, sk, sv, [k_mean], path)"""
    res = _native.fp8_quant_attention_varlen_fp8pv(q, k, v, _cu(lq), _cu(lk) if cu_k is None else cu_k, used, is_causal=causal, fp8_dtype=TDT[fp8],
                                                   numerics=numerics, sm_scale=0.0 if scale is None else scale, precision=precision, return_lse=lse,
                                                   return_quant=True, return_path=True, smooth_k=smooth_k)
    return res if lse else (res[0], None) + tuple(res[1:])


def _pub(q, k, v, lq, lk, precision, *, causal=False, lse=True, **kw):
    return qa.fp8_attn_varlen_pv_func(q, k, v, _cu(lq), _cu(lk), max(lq), max(lk), causal=causal, return_lse=lse, pv_precision="fp8",
                                      precision=precision, **kw)


def _image(buf, layout, start, i, m, Hkv, D):
    """sequence i's KFRAG / VFRAG image (m used keys from token `start`) as row-major bytes [1, Hkv, ceil(m/64) 64, D]"""
    mp = (m + 63) // 64 * 64
    off = Hkv * D * (start + 64 * i)
    return unpack_frag(buf[off:off + Hkv * mp * D], layout, 1, Hkv, m, D)


def _operands(res, lq, lk, starts_k=None):
    """per sequence: (q8 [1,Hq,n,D], k8 [1,Hkv,m,D], v8, sq [1,Hq], sk [1,Hkv], sv) as numpy, from what the call returned"""
    out, _, q8, k8, v8, sq, sk, sv = res[:8]
    _, Hq, D = out.shape
    Hkv = sk.shape[1]
    q8, k8, v8 = bits8(q8), bits8(k8), bits8(v8)
    sq, sk, sv = sq.cpu().numpy(), sk.cpu().numpy(), sv.cpu().numpy()
    starts_k = starts_k if starts_k is not None else _starts(lk)
    ops = []
    for i, (a, n, b, m) in enumerate(zip(_starts(lq), lq, starts_k, lk)):
        qi = q8[Hq * D * a:Hq * D * (a + n)].reshape(1, Hq, n, D)
        ki = _image(k8, _native.LAYOUT_KFRAG, b, i, m, Hkv, D)
        vi = _image(v8, _native.LAYOUT_VFRAG, b, i, m, Hkv, D)
        assert not ki[:, :, m:].any() and not vi[:, :, m:].any(), "the padding rows of the last chunk are zero bytes"
        ops.append((qi, ki[:, :, :m], vi[:, :, :m], sq[i:i + 1], sk[i:i + 1], sv[i:i + 1]))
    return ops


def _oracle(ops, causal, scale, fp8):
    """fp64 reference on the returned operands: (out [total_q, Hq, D], lse [Hq, total_q]); no key: zero rows, -inf"""
    f = FMT[fp8]
    outs, lses = [], []
    for qi, ki, vi, sq, sk, sv in ops:
        n, m = qi.shape[2], ki.shape[2]
        if n and m:
            o, l = oracle.attention_forward(qi, ki, vi, f, f, f, sq, sk, sv, causal=causal, sm_scale=0.0 if scale is None else scale, return_lse=True)
        else:
            o, l = np.zeros(qi.shape, np.float32), np.full(qi.shape[:3], -np.inf, np.float32)
        outs.append(np.asarray(o)[0].transpose(1, 0, 2))
        lses.append(np.asarray(l)[0])
    return np.concatenate(outs, 0), np.concatenate(lses, 1)


def _grade(res, ref, ref_lse, what):
    worst = gpu_utils.grade(gpu_utils.out_to_f32(res[0]), ref)[2]
    worst_lse = 0.0
    if res[1] is not None:
        l = res[1].cpu().numpy()
        dead = np.isneginf(ref_lse)
        assert np.array_equal(np.isneginf(l), dead), what
        worst_lse = float(np.abs(l[~dead] - ref_lse[~dead]).max()) if (~dead).any() else 0.0
    print(f"{what}: worst |err| / bound {worst:.3f}, worst LSE error {worst_lse:.2e}")
    assert worst < 1.0, (what, worst)
    assert worst_lse < LSE_TOL, (what, worst_lse)


def _expected_path(lq, lk, Hq, causal, precision):
    """the literal rule: tile t of a sequence sees n = used L_k keys (causal: min(L_k, 128 (t + 1))); ACCURATE two-term everywhere, FAST
    one-term iff n >= 1024; a sequence without a used key carries the one-term code"""
    cols = []
    for n_q, m in zip(lq, lk):
        r = np.arange(n_q)
        n = np.minimum(m, TILE * (r // TILE + 1)) if causal else np.full(n_q, m)
        one = (n == 0) | ((n >= 1024) if precision == "fast" else False)
        cols.append(np.where(one, ONE, TWO))
    return np.broadcast_to(np.concatenate(cols).astype(np.uint8), (Hq, sum(lq)))


def _check_quantiser(res, q, k, v, lq, lk, fp8, starts_k=None, numerics="compiled"):
    ops = _operands(res, lq, lk, starts_k)
    starts_k = starts_k if starts_k is not None else _starts(lk)
    for i, (a, n, b, m) in enumerate(zip(_starts(lq), lq, starts_k, lk)):
        for x, s0, cnt, got8, gots in ((q, a, n, ops[i][0], ops[i][3]), (k, b, m, ops[i][1], ops[i][4]), (v, b, m, ops[i][2], ops[i][5])):
            xi = x[s0:s0 + cnt].transpose(0, 1)[None]
            rb, rs = oracle.quantize_fp8(bits16(xi), fmt16(x.dtype), "head", FMT[fp8], numerics)
            assert np.array_equal(got8, rb), (i, "bytes")
            assert np.array_equal(gots.view(np.uint32), rs.view(np.uint32)), (i, "scale")


# ---- 1. / 2. the oracle sweep and the quantiser ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype,fp8", [(torch.bfloat16, "e4m3"), (torch.float16, "e5m2")], ids=["bf16-e4m3", "fp16-e5m2"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_every_sequence_is_within_the_fp8_v_bound_of_its_oracle(D, dtype, fp8, causal):
    q, k, v, lens = _batch(D, dtype, 100 + D + causal)
    Hq = q.shape[1]
    ref = None
    for precision in ("accurate", "fast"):
        what = f"D{D} {fp8} {'causal' if causal else 'full'} {precision}"
        res = _call(q, k, v, lens, lens, causal=causal, fp8=fp8, precision=precision)
        if ref is None:   # (the quantised operands do not depend on the precision: one reference serves every mode)
            _check_quantiser(res, q, k, v, lens, lens, fp8)
            r16 = _native.fp8_quant_attention_varlen(q, k, v, _cu(lens), _cu(lens), None, is_causal=causal, fp8_dtype=TDT[fp8], return_quant=True)
            assert torch.equal(res[2], r16[1]) and torch.equal(res[5], r16[3]) and torch.equal(res[6], r16[4])   # q8, scale_q, scale_k
            for i, (b, m) in enumerate(zip(_starts(lens), lens)):   # k8: the images (the gaps between them are never written)
                assert np.array_equal(_image(bits8(res[3]), _native.LAYOUT_KFRAG, b, i, m, k.shape[1], D),
                                      _image(bits8(r16[2]), _native.LAYOUT_KFRAG, b, i, m, k.shape[1], D))
            ref = _oracle(_operands(res, lens, lens), causal, None, fp8)
        want_path = _expected_path(lens, lens, Hq, causal, precision)
        assert np.array_equal(res[-1].cpu().numpy(), want_path), what
        assert (want_path == ONE).any() == (precision == "fast")
        _grade(res, ref[0], ref[1], what)
        with qa.config.patch({"attention.fp8_format": fp8}):   # the public function: the same bits
            po, pl = _pub(q, k, v, lens, lens, precision, causal=causal)
        assert _same_bits(po, res[0]) and _same_bits(pl, res[1])
        res_n = _call(q, k, v, lens, lens, causal=causal, fp8=fp8, precision=precision, lse=False)
        assert np.array_equal(res_n[-1].cpu().numpy(), want_path), what
        if precision == "fast":   # without the LSE the one-term tiles run the byte-exponential sweep: other bits, the same bound and table
            _grade(res_n, ref[0], ref[1], what + " (byte)")
            two = torch.from_numpy(want_path.T == TWO).to(DEV)   # [total_q, Hq]
            assert torch.equal(res_n[0][two], res[0][two])        # the two-term tiles do not depend on the LSE request
        else:                     # ACCURATE: requesting the LSE changes no bit of out
            assert _same_bits(res_n[0], res[0])


@pytest.mark.parametrize("numerics", ["compiled", "eager"])
def test_quantiser_over_used_keys_with_eager_numerics_too(numerics):
    q, k, v, lens = _batch(128, torch.float16, 7, lens=[70, 1, 200])
    res = _call(q, k, v, lens, lens, numerics=numerics)
    _check_quantiser(res, q, k, v, lens, lens, "e4m3", numerics=numerics)


# ---- 3. non-causal packing: every sequence is the block-sparse FP8-PV call on that sequence alone ------------------------------------------
@pytest.mark.parametrize("precision", ["accurate", "fast"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_a_non_causal_sequence_equals_the_block_sparse_fp8pv_call_on_it_alone(D, precision):
    q, k, v, lens = _batch(D, torch.bfloat16, 200 + D)
    out, lse = _pub(q, k, v, lens, lens, precision)
    out_n = _pub(q, k, v, lens, lens, precision, lse=False)
    for a, n in zip(_starts(lens), lens):
        qi, ki, vi = (t[a:a + n].transpose(0, 1)[None] for t in (q, k, v))
        mask = torch.ones(1, 1, (n + 127) // 128, (n + 127) // 128, dtype=torch.bool, device=DEV)
        ro, rl = qa.fp8_block_sparse_attn_pv_func(qi, ki, vi, mask, return_lse=True, pv_precision="fp8", precision=precision)
        assert _same_bits(out[a:a + n].transpose(0, 1), ro[0]) and _same_bits(lse[:, a:a + n], rl[0]), (n, "with the LSE")
        rn = qa.fp8_block_sparse_attn_pv_func(qi, ki, vi, mask, pv_precision="fp8", precision=precision)
        assert _same_bits(out_n[a:a + n].transpose(0, 1), rn[0]), (n, "without the LSE")


# ---- 4. V's scale is per (sequence, head) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("precision", ["accurate", "fast"])
def test_a_gain_on_one_sequences_v_moves_only_that_sequences_scale(precision, causal):
    q, k, v, lens = _batch(128, torch.bfloat16, 301)
    v2 = v.clone()
    for i, (a, n) in enumerate(zip(_starts(lens), lens)):
        v2[a:a + n] *= 2.0 ** (2 * i)   # (at most 2^12 on N(0,1) data: bf16 stays normal, and so does out)
    for lse in (True, False):
        r1 = _call(q, k, v, lens, lens, causal=causal, precision=precision, lse=lse)
        r2 = _call(q, k, v2, lens, lens, causal=causal, precision=precision, lse=lse)
        for i, (a, n) in enumerate(zip(_starts(lens), lens)):
            gain = 2.0 ** (2 * i)
            assert np.array_equal(_image(bits8(r1[4]), _native.LAYOUT_VFRAG, a, i, n, v.shape[1], 128),
                                  _image(bits8(r2[4]), _native.LAYOUT_VFRAG, a, i, n, v.shape[1], 128)), i
            assert torch.equal(r2[7][i], r1[7][i] * gain), i
            assert _same_bits(r2[0][a:a + n], (r1[0][a:a + n].float() * gain).to(torch.bfloat16)), i
        assert torch.equal(r1[2], r2[2]) and torch.equal(r1[5], r2[5]) and torch.equal(r1[6], r2[6])
        if lse:
            assert _same_bits(r1[1], r2[1])


# ---- 5. causal membership -----------------------------------------------------------------------------------------------------------------
PROBE_LENS = [64, 128, 129, 1100]   # the diagonal on a 64-key and on a 128-row edge, one row past it, and across the 1024-key rule


def _T(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _probe_case(probe, D, kind):
    Hq, Hkv = P.heads("packed", probe)
    case = P.make_case(probe, D, PROBE_LENS, PROBE_LENS, None, kind=kind, Hq=Hq, Hkv=Hkv)
    return case, case.reference()


@pytest.mark.parametrize("kind", ["causal", "full"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_count_and_pointer_probes_through_the_fp8pv_entry(D, kind):
    """tests/probes.py, unchanged: exact-answer inputs on which one misplaced key moves the output by >= 4x the bound (tests/test_cpu_probes.py).
    The count probe's rows are flat: both precisions; the pointer probe's rows are peaked: ACCURATE (FAST has no rescue)."""
    res = {}
    for probe, modes in (("count", ("accurate", "fast")), ("pointer", ("accurate",))):
        case, (ref, ref_lse) = _probe_case(probe, D, kind)
        q, k, v = _T(case.q, torch.bfloat16), _T(case.k, torch.bfloat16), _T(case.v, torch.bfloat16)
        for precision in modes:
            for lse in (True, False):
                got = _pub(q, k, v, case.lq, case.alloc, precision, causal=kind == "causal", lse=lse)
                out = gpu_utils.out_to_f32(got[0] if lse else got)
                res[f"{probe} {precision}{'' if lse else ' (no lse)'}"] = float((np.abs(out - ref) / P.project_bound(ref, False)).max())
                if lse and probe == "pointer":   # (the count probe's expected LSE reads the quantised q: graded by the oracle sweep instead)
                    res[f"{probe} {precision} lse"] = float(np.abs(got[1].cpu().numpy() - ref_lse).max() / LSE_TOL)
    print(f"probes {kind} D {D}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert all(v < 1.0 for v in res.values()), res


@pytest.mark.parametrize("precision", ["accurate", "fast"])
def test_keys_above_the_last_diagonal_chunk_are_never_read(precision):
    """causal, L_q < L_k: the sequence's last tile T sweeps chunks 0 .. ceil(min(L_k, 128 (T + 1)) / 64) - 1; K and V negated at every key
    beyond them (finite, abs-max and so the scales unchanged) change no bit"""
    g = torch.Generator(device=DEV).manual_seed(55)
    lq, lk, Hq, Hkv, D = [100, 300, 1090], [500, 1100, 1300], 4, 2, 128
    q, k, v = _rand(sum(lq), Hq, D, torch.bfloat16, g), _rand(sum(lk), Hkv, D, torch.bfloat16, g), _rand(sum(lk), Hkv, D, torch.bfloat16, g)
    k2, v2 = k.clone(), v.clone()
    for b, n, m in zip(_starts(lk), lq, lk):
        first_unread = 64 * -(-min(m, TILE * -(-n // TILE)) // 64)
        assert first_unread < m
        k2[b + first_unread:b + m] *= -1
        v2[b + first_unread:b + m] *= -1
    for lse in (False, True):
        a = _call(q, k, v, lq, lk, causal=True, precision=precision, lse=lse)
        b = _call(q, k2, v2, lq, lk, causal=True, precision=precision, lse=lse)
        assert torch.equal(a[5], b[5]) and torch.equal(a[6], b[6]) and torch.equal(a[7], b[7])   # the scales
        assert _same_bits(a[0], b[0]) and (not lse or _same_bits(a[1], b[1]))
    # ... and the token-exact diagonal inside the swept chunks: against the oracle
    ref = _oracle(_operands(a, lq, lk), True, None, "e4m3")
    _grade(a, ref[0], ref[1], f"causal cross {precision}")


# ---- 6. seqused_k ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["accurate", "fast"])
def test_seqused_k_on_padded_kv_equals_the_trimmed_call_whatever_the_padding_holds(precision):
    g = torch.Generator(device=DEV).manual_seed(3)
    B, S_pad, H, D = 4, 1152, 4, 128
    k_lens = [1152, 100, 1, 1100]
    lq = [300, 129, 64, 1100]
    q = _rand(sum(lq), H, D, torch.bfloat16, g)
    kp, vp = (torch.randn(B, S_pad, H, D, generator=g, device=DEV).bfloat16() for _ in range(2))
    cu_k = torch.arange(B + 1, dtype=torch.int32, device=DEV) * S_pad
    used = torch.tensor(k_lens, dtype=torch.int32, device=DEV)
    kt = torch.cat([kp[i, :n] for i, n in enumerate(k_lens)])
    vt = torch.cat([vp[i, :n] for i, n in enumerate(k_lens)])
    for causal in (False, True):
        want = _call(q, kt, vt, lq, k_lens, causal=causal, precision=precision)
        w_ops = _operands(want, lq, k_lens)
        for fill in (1e4, float("nan")):
            k2, v2 = kp.clone(), vp.clone()
            for i, n in enumerate(k_lens):
                k2[i, n:], v2[i, n:] = fill, fill
            got = _call(q, k2.view(B * S_pad, H, D), v2.view(B * S_pad, H, D), lq, k_lens, used=used, cu_k=cu_k, causal=causal, precision=precision)
            assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), fill
            assert torch.equal(got[7], want[7]) and torch.equal(got[-1], want[-1]), fill
            for go, wo in zip(_operands(got, lq, k_lens, [i * S_pad for i in range(B)]), w_ops):
                assert all(np.array_equal(x, y) for x, y in zip(go, wo)), fill


# ---- 7. empty sequences -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["accurate", "fast"])
def test_empty_sequences_are_defined(precision):
    g = torch.Generator(device=DEV).manual_seed(4)
    lq, lk, H, D = [300, 0, 257, 40], [1100, 9, 0, 70], 4, 64
    q, k, v = _rand(sum(lq), H, D, torch.bfloat16, g), _rand(sum(lk), H, D, torch.bfloat16, g), _rand(sum(lk), H, D, torch.bfloat16, g)
    for causal in (False, True):
        for lse in (True, False):
            res = _call(q, k, v, lq, lk, causal=causal, precision=precision, lse=lse)
            assert (res[0][300:557] == 0).all() and (res[-1][:, 300:557] == ONE).all()
            assert not lse or (res[1][:, 300:557] == -math.inf).all()
            assert np.array_equal(res[-1].cpu().numpy(), _expected_path(lq, lk, H, causal, precision))
            ref = _oracle(_operands(res, lq, lk), causal, None, "e4m3")
            _grade(res, ref[0], ref[1], f"empty {precision} causal {causal} lse {lse}")


# ---- 8. cross-attention --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_cross_attention_with_other_key_lengths_and_an_explicit_scale(causal):
    g = torch.Generator(device=DEV).manual_seed(8)
    lq, lk, Hq, Hkv, D, scale = [300, 5, 1200], [77, 1100, 300], 8, 2, 128, 0.05   # (scale^2 D = 0.32 <= 1: FAST's stated domain)
    q, k, v = _rand(sum(lq), Hq, D, torch.float16, g), _rand(sum(lk), Hkv, D, torch.float16, g), _rand(sum(lk), Hkv, D, torch.float16, g)
    ref = None
    for precision in ("accurate", "fast"):
        for lse in (True, False):
            res = _call(q, k, v, lq, lk, causal=causal, precision=precision, scale=scale, lse=lse)
            ref = ref or _oracle(_operands(res, lq, lk), causal, scale, "e4m3")
            assert np.array_equal(res[-1].cpu().numpy(), _expected_path(lq, lk, Hq, causal, precision))
            _grade(res, ref[0], ref[1], f"cross {precision} lse {lse}")
        po, pl = _pub(q, k, v, lq, lk, precision, causal=causal, softmax_scale=scale)
        assert _same_bits(po, _call(q, k, v, lq, lk, causal=causal, precision=precision, scale=scale)[0])


# ---- 9. a late jump of the running max -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_a_late_jump_of_the_running_max_rescales_accumulator_and_row_sums(causal):
    q, k, v, lens = _batch(128, torch.bfloat16, 11)
    a = _starts(lens)[-1]
    k[a + 1100 - 128:a + 1100] *= 8   # the 1100-token sequence's last 128 keys
    for lse in (True, False):
        res = _call(q, k, v, lens, lens, causal=causal, precision="accurate", lse=lse)
        ref = _oracle(_operands(res, lens, lens), causal, None, "e4m3")
        _grade(res, ref[0], ref[1], f"late max lse {lse}")


# ---- 10. strided inputs ------------------------------------------------------------------------------------------------------------------------
def test_strided_slices_of_a_packed_qkv_projection_equal_the_contiguous_call():
    g = torch.Generator(device=DEV).manual_seed(2)
    lens, H, D = [33, 300, 64], 4, 64
    qkv = _rand(sum(lens), 3 * H, D, torch.bfloat16, g).view(sum(lens), 3, H, D)
    q, k, v = qkv.unbind(1)
    assert not v.is_contiguous() and _native.varlen_strided_ok(v)
    for causal in (False, True):
        res = _call(q, k, v, lens, lens, causal=causal)
        dense = _call(q.contiguous(), k.contiguous(), v.contiguous(), lens, lens, causal=causal)
        assert _same_bits(res[0], dense[0]) and _same_bits(res[1], dense[1])
        assert all(torch.equal(res[j], dense[j]) for j in (2, 5, 6, 7, 8))
        for go, wo in zip(_operands(res, lens, lens), _operands(dense, lens, lens)):
            assert all(np.array_equal(x, y) for x, y in zip(go, wo))


# ---- 11. graph replay ----------------------------------------------------------------------------------------------------------------------
def test_graph_replay_follows_rewritten_tables():
    g = torch.Generator(device=DEV).manual_seed(6)
    H, D, total = 8, 128, 2400
    q, k, v = (_rand(total, H, D, torch.bfloat16, g) for _ in range(3))
    cu_q, cu_k = _cu([100, 1500, 800]), _cu([300, 1300, 800])
    used = torch.tensor([300, 1200, 800], dtype=torch.int32, device=DEV)
    call = lambda: qa.fp8_attn_varlen_pv_func(q, k, v, cu_q, cu_k, 1500, 1500, causal=True, seqused_k=used, return_lse=True, pv_precision="fp8",
                                              precision="fast")
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
    fresh = _pub(q, kt, vt, [1250, 50, 1100], [1, 1111, 64], "fast", causal=True)
    assert _same_bits(out, fresh[0]) and _same_bits(lse, fresh[1])


# ---- 12. torch.compile ----------------------------------------------------------------------------------------------------------------------
def test_torch_compile_fullgraph_gives_the_eager_bits():
    g = torch.Generator(device=DEV).manual_seed(8)
    lens, H, D = [200, 1100, 77], 8, 128
    q, k, v = (_rand(sum(lens), H, D, torch.float16, g) for _ in range(3))
    cu = _cu(lens)

    def f(q, k, v, cu):
        return qa.fp8_attn_varlen_pv_func(q * 2, k, v, cu, cu, 1100, 1100, softmax_scale=0.04, causal=True, return_lse=True, pv_precision="fp8",
                                          precision="fast")

    torch._dynamo.reset()
    got = torch.compile(f, fullgraph=True)(q, k, v, cu)
    want = f(q, k, v, cu)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])


# ---- 13. the eager fallback -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_eager_fallback_agrees_with_the_kernel(causal):
    q, k, v, lens = _batch(128, torch.bfloat16, 29, lens=[300, 0, 1100, 65])
    lk = [300, 40, 1100, 0]
    k, v = k[:sum(lk)], v[:sum(lk)]
    with qa.config.patch({"attention.quant_numerics": "eager"}):
        out, lse = _pub(q, k, v, lens, lk, "accurate", causal=causal)
    with qa.config.patch({"attention.force_eager_fallback": True}):
        eo, el = _pub(q, k, v, lens, lk, "accurate", causal=causal)
    assert (eo[1400:] == 0).all() and (el[:, 1400:] == -math.inf).all()
    assert gpu_utils.grade(out.float().cpu().numpy(), eo.float().cpu().numpy())[2] < 1.0
    fin = torch.isfinite(el)
    assert torch.equal(fin, torch.isfinite(lse)) and (lse[fin] - el[fin]).abs().max().item() < 2 ** -7


# ---- 14. key smoothing ------------------------------------------------------------------------------------------------------------------------
def test_key_smoothing_shares_k8_scale_k_and_k_mean_with_the_16bit_entry_and_lowers_the_error():
    g = torch.Generator(device=DEV).manual_seed(28)
    lens, Hq, Hkv, D = [300, 65, 1100], 4, 2, 128
    q, k, v = _rand(sum(lens), Hq, D, torch.bfloat16, g), _rand(sum(lens), Hkv, D, torch.bfloat16, g), _rand(sum(lens), Hkv, D, torch.bfloat16, g)
    k = (k.float() + 16.0 * torch.randn(1, Hkv, D, generator=g, device=DEV)).to(torch.bfloat16)   # a sigma = 16 offset per channel
    for causal in (False, True):
        r16 = _native.fp8_quant_attention_varlen(q, k, v, _cu(lens), _cu(lens), None, is_causal=causal, return_lse=True, return_quant=True,
                                                 smooth_k=True)   # (out, lse, q8, k8, sq, sk, k_mean)
        res = _call(q, k, v, lens, lens, causal=causal, smooth_k=True)   # (out, lse, q8, k8, v8, sq, sk, sv, k_mean, path)
        assert torch.equal(res[6], r16[5]) and torch.equal(res[8], r16[6]) and torch.equal(res[2], r16[2])
        for i, (b, m) in enumerate(zip(_starts(lens), lens)):
            assert np.array_equal(_image(bits8(res[3]), _native.LAYOUT_KFRAG, b, i, m, Hkv, D), _image(bits8(r16[3]), _native.LAYOUT_KFRAG, b, i, m, Hkv, D))
        assert (res[1] - r16[1]).abs().max().item() < 2 * LSE_TOL   # the LSE of the true scores, as the 16-bit-PV entry's
        # unquantised fp64 reference
        refs = []
        for a, n in zip(_starts(lens), lens):
            qi = q[a:a + n].transpose(0, 1).double()
            ki, vi = (t[a:a + n].transpose(0, 1).double().repeat_interleave(Hq // Hkv, 0) for t in (k, v))
            s = (qi @ ki.transpose(-1, -2)) / math.sqrt(D)
            if causal:
                s = s.masked_fill(torch.ones(n, n, dtype=torch.bool, device=DEV).triu(1), -math.inf)
            refs.append((torch.softmax(s, -1) @ vi).transpose(0, 1))
        ref = torch.cat(refs)
        for precision in ("accurate", "fast"):
            rmse = {}
            for on in (False, True):
                with qa.config.patch({"attention.smooth_k": on}):
                    out, _ = _pub(q, k, v, lens, lens, precision, causal=causal)
                rmse[on] = (out.double() - ref).pow(2).mean().sqrt().item()
            print(f"smooth_k {precision} causal {causal}: rmse against unquantised fp64 {rmse[False]:.4e} (off) -> {rmse[True]:.4e} (on)")
            assert rmse[True] < rmse[False]


# ---- 15. the buffer contract (include/qattn_buffers.h) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "smooth"])
@pytest.mark.parametrize("precision,causal", [("accurate", False), ("fast", True)])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_the_c_entry_on_guarded_buffers_of_exactly_the_documented_sizes(D, precision, causal, smooth):
    """tests/arena.py through the Plan of tests/test_gpu_buffer_contract.py: guards intact, every documented byte written, bits equal to the
    ordinary call, no dependence on what the workspace / scratch held or on bytes outside the inputs.  k8 / v8: the images of the used keys do
    not tile their buffers (scratch between them)."""
    from tests.test_gpu_buffer_contract import ALIGN1, ALIGN4, HKV, HQ, Plan, _stream

    L = _native.lib()
    LQ, LK_ALLOC, USED = [65, 3, 257, 1100], [130, 9, 300, 1200], [129, 0, 257, 1100]
    g = torch.Generator().manual_seed(77 + D)
    tq, tk, nb = sum(LQ), sum(LK_ALLOC), len(LQ)
    q = torch.randn(tq, HQ, D, generator=g)
    k, v = (torch.randn(tk, HKV, D, generator=g) for _ in range(2))
    cu_q, cu_k, used = _cu(LQ), _cu(LK_ALLOC), torch.tensor(USED, dtype=torch.int32, device=DEV)
    for b, u, a in zip(_starts(LK_ALLOC), USED, LK_ALLOC):   # keys beyond seqused_k influence no output bit: NaN there
        k[b + u:b + a] = float("nan")
        v[b + u:b + a] = float("nan")
    q, k, v = (t.to(torch.bfloat16).to(DEV) for t in (q, k, v))
    res = _call(q, k, v, LQ, LK_ALLOC, used=used, causal=causal, precision=precision, smooth_k=smooth)
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
    call = lambda: L.qattn_fp8_quant_attention_varlen_forward_fp8pv(
        pq, pk, pv, None, _native.fmt_of(torch.bfloat16), po, pl, pcq, pck, pu, nb, HQ, HKV, tq, tk, D, _native.FMT_E4M3, 0, int(causal), 0.0,
        _native.PRECISION[precision], pq8, pk8, pv8, psq, psk, psv, pp, pm, pw, wb, _stream())
    first = p.check(call, want)
    # the images inside the scratch-role k8 / v8: bit-equal to the ordinary call's
    for name, j, layout in (("k8", 3, _native.LAYOUT_KFRAG), ("v8", 4, _native.LAYOUT_VFRAG)):
        got8 = p.ar[name].interior.cpu().numpy()
        for i, (b, m) in enumerate(zip(_starts(LK_ALLOC), USED)):
            assert np.array_equal(_image(got8, layout, b, i, m, HKV, D), _image(bits8(res[j]), layout, b, i, m, HKV, D)), (name, i)
    out = first["out"].view(torch.bfloat16).view(tq, HQ, D)
    assert (out[65:68].view(torch.int16) == 0).all() and (first["lse"].view(torch.float32).view(HQ, tq)[:, 65:68] == -math.inf).all()


# ---- 16. the default call ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_the_default_call_gives_the_released_functions_bits(causal):
    q, k, v, lens = _batch(128, torch.bfloat16, 30)
    cu = _cu(lens)
    want = qa.fp8_attn_varlen_func(q, k, v, cu, cu, max(lens), max(lens), causal=causal, return_lse=True)
    for kw in ({}, {"pv_precision": "16bit"}, {"pv_precision": "16bit", "precision": "accurate"}):
        got = qa.fp8_attn_varlen_pv_func(q, k, v, cu, cu, max(lens), max(lens), causal=causal, return_lse=True, **kw)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), kw
    assert not _same_bits(_pub(q, k, v, lens, lens, "accurate", causal=causal)[0], want[0])

"""-m gpu: the scale ladder of tests/scale_ladder.py through every attention entry on the MI355X ("Scale ladder"): WHICH quant
scale -- of which batch entry, head, token, sequence or 64-key chunk -- each kernel applies to each element.

Neighbouring scale groups carry gains of 2^e, so a scale read at the wrong index makes some group's scores >= 4 x too large and its flat
rows collapse: tests/test_cpu_scale_ladder.py shows, on the very cases below, that every named mis-indexing moves the reference by >= 4 x
the bound applied here.  Three kinds of check:
1. oracle grading: every row against the fp64 masked softmax on the CPU quantiser's output (never on a scale a GPU call returned), per
   reported row_path, with tests/gpu_utils.grade -- no new bound; the LSE at the tolerances of include/qattn.h;
2. quantiser echo: the bytes an entry returns are those of the same call without gains, each scale exactly 2^e times the plain one;
3. exact equivariance, no oracle: with f = 0 the products scale_q scale_k do not move, so out, lse and row_path are the plain call's
   bit for bit; on the V head ladder out[b, h] = 2^e out_plain[b, h] bit for bit -- through the fused entry, the three separate C calls,
   the row-major entry and the op, head-wise and token-wise, under every precision, and through the packed, window, block-sparse and
   16-bit entries.
Each test prints one line: worst |err| / bound, share of the rows per path."""
import functools
import math

import numpy as np
import pytest
import torch

import oracle
import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import probes as P
from tests import scale_ladder as L
from tests.gpu_utils import (PATH_ONE_TERM, PATH_V16, TDT, PathRef, bits8, check_path_structure, fmt16, fused_call, grade,
                             oracle_for_fp8_path, out_to_f32, unpack_frag)
from tests.scale_ladder import B, HKV, HQ

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = ("fast", "auto", "accurate")
LSE_SWEEP128, LSE_V16, LSE_OTHER = P.LSE_TOL_SWEEP128, P.LSE_TOL_V16, P.LSE_TOL   # include/qattn.h: the D = 128 head-wise FP8 sweep, 16-bit-V rows, the others
ONE_TERM_SHARE = 0.90


def G(*ts):
    return tuple(t.to(DEV) for t in ts)


ROWS = ("one-term", "two-term", "16-bit V", "fp8 V, no row_path", "16-bit entry")


class Log:
    """worst |err| / bound, worst |lse err| / tolerance and the rows per path over the calls of one test"""

    def __init__(self, what):
        self.what, self.worst, self.lse, self.rows = what, 0.0, 0.0, np.zeros(len(ROWS), np.int64)

    def out(self, got, ref, path=None, v16=False, label="fp8 V, no row_path"):
        """grade one output with tests/gpu_utils.grade: a PathRef with the reported path; v16 -- an entry that runs 16-bit P on the
        16-bit V on every row (a full QATTN_PATH_V16 path); else a plain reference at the fp8-V bound, counted under `label`"""
        if v16:
            ref = np.asarray(ref, np.float64)
            path, ref = np.full(ref.shape[:-1], PATH_V16, np.uint8), PathRef(ref, ref)
        w = grade(got, ref, path)[2]
        if path is not None:
            self.rows[:3] += np.bincount(np.asarray(path).ravel(), minlength=3)
        else:
            self.rows[ROWS.index(label)] += np.asarray(ref)[..., 0].size
        self.worst = max(self.worst, w)
        return w

    def lse_err(self, got, ref, tol):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        dead = np.isneginf(ref)
        assert np.array_equal(np.isneginf(got), dead) and np.isfinite(got[~dead]).all(), (self.what, "LSE: -inf exactly on the rows without a key")
        w = float((np.abs(got - ref)[~dead] / np.broadcast_to(tol, ref.shape)[~dead]).max())
        self.lse = max(self.lse, w)
        return w

    def done(self):
        share = self.rows / max(1, self.rows.sum())
        print(f"{self.what}: worst |err| / bound {self.worst:.3f}, worst |lse err| / tolerance {self.lse:.3f}; rows " +
              ", ".join(f"{n} {x:.3f}" for n, x in zip(ROWS, share) if x > 0))
        assert self.worst < 1.0 and self.lse < 1.0, (self.what, self.worst, self.lse)


def fused_lse_tol(path, d128_head):
    return np.where(path == PATH_V16, LSE_V16, np.where(path == PATH_ONE_TERM, LSE_SWEEP128 if d128_head else LSE_OTHER, LSE_OTHER))


@functools.lru_cache(maxsize=None)
def fused_reference(kind, D, Sq, Skv, causal, dtype, fp8, side=None, v_head=False):
    """(ladder, its tensors on the CPU, the CPU quantiser's output, PathRef of the fused entry, the separate calls' reference (one fp8 V
    scale per head), the reference LSE) -- computed once per case, shared, left unchanged.  v_head: V carries the V head ladder"""
    mode = "head" if kind == "head" else "token"
    lad = L.head_ladder(D, Sq, Skv, v_head=v_head) if kind == "head" else L.token_ladder(D, Sq, Skv, side, v_head=v_head)
    t = lad.tensors(dtype)
    qz = L.quantise(t, dtype, fp8, mode)
    kw = dict(fp8=fp8, v_dtype=dtype, scaling=mode, causal=causal)
    ref, lse = oracle_for_fp8_path(qz.q8, qz.k8, qz.vb16, qz.sq, qz.sk, v_block=qz.v_block, fused=True, return_lse=True, **kw)
    sep = ref.fp8v if not qz.v_block else oracle_for_fp8_path(qz.q8, qz.k8, qz.vb16, qz.sq, qz.sk, **kw)
    return lad, t, qz, ref, sep, lse


def run_fused(log, tq, tk, tv, qz, ref, ref_lse, D, Sq, Skv, causal, fp8, scaling):
    """the fused entry under every precision, and once more with the LSE of the same launch"""
    d128_head = D == 128 and scaling == "head-wise"
    late = ~L.early_rows(Sq, Skv, causal)
    for prec in PRECISIONS:
        out, path = fused_call(tq, tk, tv, causal=causal, precision=prec, fp8=fp8, scaling=scaling)
        check_path_structure(path, Sq, Skv, causal, prec, d128_head)
        log.out(out, ref, path)
        if d128_head and prec != "accurate" and late.any():
            share = float((path[..., late] == PATH_ONE_TERM).mean())
            assert share >= ONE_TERM_SHARE, (log.what, prec, "the FP8 sweep must be what is graded", share)
    out, path, lse = fused_call(tq, tk, tv, causal=causal, precision="auto", fp8=fp8, scaling=scaling, return_lse=True)
    log.out(out, ref, path)
    log.lse_err(lse, ref_lse, fused_lse_tol(path, d128_head))


def run_separate(log, tq, tk, tv, qz, sep, ref_lse, Skv, causal, dtype, fp8, scaling):
    """the three separate C calls, and the pre-quantised row-major entry and op with the CPU ladder's bytes and scales handed over"""
    q8, sq = _native.quant_fp8(tq, scaling=scaling, fp8_dtype=TDT[fp8])
    kf, sk = _native.quant_fp8(tk, scaling=scaling, fp8_dtype=TDT[fp8], layout=_native.LAYOUT_KFRAG)
    vf, sv = _native.quant_fp8(tv, fp8_dtype=TDT[fp8], layout=_native.LAYOUT_VFRAG)
    assert np.array_equal(bits8(q8), qz.q8) and np.array_equal(sq.cpu().numpy(), qz.sq) and np.array_equal(sk.cpu().numpy(), qz.sk), \
        "quant_fp8 on the ladder: the CPU quantiser's bytes and scales"
    want_sv = oracle.quantize_fp8(qz.vb16, fmt16(dtype), "head", L.FMT[fp8], "compiled")[1]
    assert np.array_equal(sv.cpu().numpy(), want_sv), "scale_v: the CPU quantiser's, one per (batch, kv head)"
    kw = dict(Hkv=HKV, Skv=Skv, out_dtype=dtype, is_causal=causal, scaling=scaling)
    for prec in PRECISIONS:
        log.out(out_to_f32(_native.fp8_attention_forward(q8, kf, vf, sq, sk, sv, precision=prec, **kw)), sep)
    out, lse = _native.fp8_attention_forward(q8, kf, vf, sq, sk, sv, return_lse=True, **kw)
    log.out(out_to_f32(out), sep)
    log.lse_err(lse.cpu().numpy(), ref_lse, LSE_OTHER)
    # pre-quantised: q8, k8, scale_q, scale_k are the CALLER's tensors -- here the CPU quantiser's
    cq8, ck8 = (torch.from_numpy(x.copy()).view(TDT[fp8]).to(DEV) for x in (qz.q8, qz.k8))
    csq, csk = (torch.from_numpy(x.copy()).to(DEV) for x in (qz.sq, qz.sk))
    for prec in PRECISIONS:
        log.out(out_to_f32(_native.fp8_attention_forward_rowmajor(cq8, ck8, tv, csq, csk, is_causal=causal, precision=prec)), sep)
    out, lse = _native.fp8_attention_forward_rowmajor(cq8, ck8, tv, csq, csk, is_causal=causal, return_lse=True)
    log.out(out_to_f32(out), sep)
    log.lse_err(lse.cpu().numpy(), ref_lse, LSE_OTHER)
    if fp8 == "e4m3":
        log.out(out_to_f32(torch.ops.quantumattention_amd.fp8_attention_forward(cq8, ck8, tv, csq, csk, None, 0.0, causal)), sep)


def same(a, b, what):
    assert len(a) == len(b)
    for x, y, n in zip(a, b, ("1st", "2nd", "3rd")):
        assert np.array_equal(x, y, equal_nan=True), (what, n, "must equal the plain call bit for bit", int((np.asarray(x) != np.asarray(y)).sum()))


# ---- 1. the fused entry and the separate calls on the head ladder -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.HEAD_CASES, ids=L.case_id)
def test_fused_entry_on_the_head_ladder(case):
    D, Sq, Skv, causal, dtype, fp8 = case
    lad, t, qz, ref, sep, ref_lse = fused_reference("head", *case)
    tq, tk, tv = G(*t)
    log = Log(f"fused, head ladder {L.case_id(case)}")
    run_fused(log, tq, tk, tv, qz, ref, ref_lse, D, Sq, Skv, causal, fp8, "head-wise")
    # 2. the quantiser echo: k8, scale_q, scale_k (and the head's scale_v) against the plain call and against the CPU quantiser
    quant = lambda a, b, c: _native.fp8_quant_attention_forward(a, b, c, is_causal=causal, fp8_dtype=TDT[fp8], return_quant=True)[-1]
    plain = G(*L.head_ladder(D, Sq, Skv, gains=False).tensors(dtype))
    ql, qp = quant(tq, tk, tv), quant(*plain)
    assert torch.equal(ql["k8"], qp["k8"]), "k8: the bytes of the call without gains"
    assert np.array_equal(unpack_frag(ql["k8"].cpu().numpy(), _native.LAYOUT_KFRAG, B, HKV, Skv, D)[:, :, :Skv], qz.k8)
    for name, e, cpu in (("scale_q", lad.e_q, qz.sq), ("scale_k", lad.e_k, qz.sk)) + (() if qz.v_block else (("scale_v", lad.e_v, qz.sv),)):
        got, base = ql[name].cpu().numpy(), qp[name].cpu().numpy()
        assert np.array_equal(got, base * np.exp2(e).astype(np.float32)) and np.array_equal(got, cpu), (name, "exactly 2^e x the plain scale")
    # 3. exact equivariance: e only (f = 0) -- out, path and lse of the plain inputs; the V head ladder -- 2^e x the plain output
    e_only = G(*L.head_ladder(D, Sq, Skv, f=False).tensors(dtype))
    gain_v = np.exp2(L.E_VHEAD)[:, L.kv_of(), None, None]
    tvh = L.to16(L.head_ladder(D, Sq, Skv, gains=False).v * np.exp2(L.E_VHEAD)[..., None, None], dtype).to(DEV)
    # (fp16: 2^-24 is the spacing of the subnormal numbers.  An element whose plain value or whose scaled value lies below the smallest
    # normal number was rounded on that grid, once before the gain and once after it: such elements are held to that, the others exactly)
    tiny = float(torch.finfo(dtype).tiny)
    sub = tiny * float(torch.finfo(dtype).eps)
    for prec in PRECISIONS:
        kw = dict(causal=causal, precision=prec, fp8=fp8)
        base = fused_call(*plain, **kw)
        same(fused_call(*e_only, **kw), base, f"{log.what} {prec}, e only")
        if prec == "auto":   # (the LSE of the same launch; on the templated kernel its request selects the exact-exponential sweep)
            same(fused_call(*e_only, return_lse=True, **kw), fused_call(*plain, return_lse=True, **kw), f"{log.what} auto with the LSE, e only")
        out, path = fused_call(plain[0], plain[1], tvh, **kw)
        want = base[0] * gain_v
        normal = (np.abs(want) >= tiny) & (np.abs(base[0]) >= tiny)
        assert np.array_equal(path, base[1]) and np.array_equal(out[normal], want[normal]), (log.what, prec, "V head ladder: out = 2^e x the plain output")
        assert (np.abs(out - want) <= np.maximum(1.0, gain_v) * sub).all(), (log.what, prec, "V head ladder: subnormal elements")
    log.done()


@pytest.mark.parametrize("case", L.SEPARATE_HEAD, ids=L.case_id)
def test_separate_calls_and_prequantised_entry_on_the_head_ladder(case):
    """twice: with the chunk-ladder V (the q / k scale mutants have their teeth there) and with the V head ladder -- these entries keep ONE
    fp8 V scale per (batch, kv head), distinct by x2 .. x16 on that V"""
    D, Sq, Skv, causal, dtype, fp8 = case
    for v_head in (False, True):
        lad, t, qz, ref, sep, ref_lse = fused_reference("head", *case, v_head=v_head)
        log = Log(f"separate calls / pre-quantised, head ladder {L.case_id(case)}" + (", V head ladder" if v_head else ""))
        run_separate(log, *G(*t), qz, sep, ref_lse, Skv, causal, dtype, fp8, "head-wise")
        log.done()


# ---- the token ladder: fused entry, separate calls, pre-quantised entry -------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.TOKEN_CASES, ids=L.case_id)
def test_token_wise_entries_on_the_token_ladder(case):
    D, Sq, Skv, causal, dtype, fp8, side = case
    lad, t, qz, ref, sep, ref_lse = fused_reference("token", *case)
    tq, tk, tv = G(*t)
    log = Log(f"token-wise entries, token ladder {L.case_id(case)}")
    run_fused(log, tq, tk, tv, qz, ref, ref_lse, D, Sq, Skv, causal, fp8, "token-wise")
    quant = _native.fp8_quant_attention_forward(tq, tk, tv, is_causal=causal, scaling="token-wise", fp8_dtype=TDT[fp8], return_quant=True)[-1]
    assert np.array_equal(unpack_frag(quant["k8"].cpu().numpy(), _native.LAYOUT_KFRAG, B, HKV, Skv, D)[:, :, :Skv], qz.k8), "k8: 0 or +- the largest code"
    assert np.array_equal(quant["scale_k"].cpu().numpy(), qz.sk) and np.array_equal(quant["scale_q"].cpu().numpy(), qz.sq), "scale of token j: 2^(e_j) x one number"
    run_separate(log, tq, tk, tv, qz, sep, ref_lse, Skv, causal, dtype, fp8, "token-wise")
    log.done()


@pytest.mark.parametrize("case", L.VHEAD_TOKEN, ids=L.case_id)
def test_token_wise_entries_on_the_v_head_ladder(case):
    """token-wise scales keep ONE fp8 V scale per (batch, kv head) in every entry: the token ladder's q, k with V x 2^E_VHEAD"""
    D, Sq, Skv, causal, dtype, fp8, side = case
    lad, t, qz, ref, sep, ref_lse = fused_reference("token", *case, v_head=True)
    tq, tk, tv = G(*t)
    log = Log(f"token-wise entries, token ladder + V head ladder {L.case_id(case)}")
    run_fused(log, tq, tk, tv, qz, ref, ref_lse, D, Sq, Skv, causal, fp8, "token-wise")
    quant = _native.fp8_quant_attention_forward(tq, tk, tv, is_causal=causal, scaling="token-wise", fp8_dtype=TDT[fp8], return_quant=True)[-1]
    assert np.array_equal(quant["scale_v"].cpu().numpy(), qz.sv), "scale_v: the CPU quantiser's, one per (batch, kv head)"
    run_separate(log, tq, tk, tv, qz, sep, ref_lse, Skv, causal, dtype, fp8, "token-wise")
    log.done()


# ---- 3. exact equivariance through every dense entry, head-wise and token-wise ----------------------------------------------------------------
def dense_entries(causal, dtype, fp8, scaling):
    """{entry: f(tq, tk, tv, precision) -> tuple of numpy arrays, out first}: every dense entry that takes 16-bit q, k, v or what the
    quantiser made of them"""
    kw = dict(causal=causal, fp8=fp8, scaling=scaling)

    def quantised(tq, tk, tv):
        q8, sq = _native.quant_fp8(tq, scaling=scaling, fp8_dtype=TDT[fp8])
        k8, sk = _native.quant_fp8(tk, scaling=scaling, fp8_dtype=TDT[fp8])
        kf, sk2 = _native.quant_fp8(tk, scaling=scaling, fp8_dtype=TDT[fp8], layout=_native.LAYOUT_KFRAG)
        vf, sv = _native.quant_fp8(tv, fp8_dtype=TDT[fp8], layout=_native.LAYOUT_VFRAG)
        assert torch.equal(sk, sk2)
        return q8, k8, kf, vf, sq, sk, sv

    def separate(tq, tk, tv, prec, lse=False):
        q8, k8, kf, vf, sq, sk, sv = quantised(tq, tk, tv)
        r = _native.fp8_attention_forward(q8, kf, vf, sq, sk, sv, Hkv=HKV, Skv=tk.shape[2], out_dtype=dtype, is_causal=causal, scaling=scaling,
                                          precision=prec, return_lse=lse)
        return (out_to_f32(r[0]), r[1].cpu().numpy()) if lse else (out_to_f32(r),)

    def rowmajor(tq, tk, tv, prec, lse=False):
        q8, k8, kf, vf, sq, sk, sv = quantised(tq, tk, tv)
        r = _native.fp8_attention_forward_rowmajor(q8, k8, tv, sq, sk, is_causal=causal, precision=prec, return_lse=lse)
        return (out_to_f32(r[0]), r[1].cpu().numpy()) if lse else (out_to_f32(r),)

    def op(tq, tk, tv, prec):
        q8, k8, kf, vf, sq, sk, sv = quantised(tq, tk, tv)
        return (out_to_f32(torch.ops.quantumattention_amd.fp8_attention_forward(q8, k8, tv, sq, sk, None, 0.0, causal)),)

    res = {"fused": lambda a, b, c, prec: fused_call(a, b, c, precision=prec, **kw),
           "fused with the LSE": lambda a, b, c, prec: fused_call(a, b, c, precision=prec, return_lse=True, **kw),
           "separate calls": separate, "separate calls with the LSE": lambda a, b, c, prec: separate(a, b, c, prec, True),
           "row-major entry": rowmajor, "row-major entry with the LSE": lambda a, b, c, prec: rowmajor(a, b, c, prec, True)}
    if fp8 == "e4m3":
        res["op on pre-quantised q / k"] = op
    return res


@pytest.mark.parametrize("scaling", ["head-wise", "token-wise"])
@pytest.mark.parametrize("case", L.EQUIVARIANCE_CASES, ids=L.case_id)
def test_exact_equivariance_of_every_dense_entry(case, scaling):
    """no oracle.  e only (k 2^e, q 2^-e per kv group; under token-wise scales every token's scale of the group moves by 2^e): every output
    of every entry and precision equals the plain inputs' bit for bit.  V head ladder (v[b, h_kv] 2^e) on the plain q, k: out = 2^e x the
    plain out bit for bit, row_path and lse unchanged.  (The fused head-wise entry up to 16384 keys block-scales V: there the V head ladder
    moves every chunk's exponent by e.)"""
    D, Sq, Skv, causal, dtype, fp8 = case
    plain = G(*L.head_ladder(D, Sq, Skv, gains=False).tensors(dtype))
    e_only = G(*L.head_ladder(D, Sq, Skv, f=False).tensors(dtype))
    tvh = G(L.head_ladder(D, Sq, Skv, gains=False, v_head=True).tensors(dtype)[2])[0]
    gain_v = np.exp2(L.E_VHEAD)[:, L.kv_of(), None, None]
    tiny = float(torch.finfo(dtype).tiny)     # (fp16 elements below the smallest normal number: test_fused_entry_on_the_head_ladder)
    sub = tiny * float(torch.finfo(dtype).eps)
    n = 0
    for name, f in dense_entries(causal, dtype, fp8, scaling).items():
        for prec in PRECISIONS if not name.startswith("op") else ("auto",):
            what = f"{name} {scaling} {prec} {L.case_id(case)}"
            base = f(*plain, prec)
            same(f(*e_only, prec), base, what + ", e only")
            got = f(plain[0], plain[1], tvh, prec)
            want = base[0] * gain_v
            normal = (np.abs(want) >= tiny) & (np.abs(base[0]) >= tiny)
            assert np.array_equal(got[0][normal], want[normal]) and (np.abs(got[0] - want) <= np.maximum(1.0, gain_v) * sub).all(), (what, "V head ladder: out = 2^e x plain")
            same(got[1:], base[1:], what + ", V head ladder")
            n += 1
    print(f"exact equivariance {scaling} {L.case_id(case)}: {n} (entry, precision) pairs bit for bit, e only and V head ladder")


# ---- the 16-bit-V entries: packed, window, block-sparse, attn_func -------------------------------------------------------------------------------
def _cu(n):
    return torch.tensor([0, n, 2 * n], dtype=torch.int32, device=DEV)


def pack(t):
    """[B, H, S, D] -> the packed [B S, H, D] (a batch entry is a sequence)"""
    return t.transpose(1, 2).reshape(-1, t.shape[1], t.shape[3]).contiguous()


def unpack(out, lse, S):
    return out_to_f32(out).reshape(B, S, HQ, -1).transpose(0, 2, 1, 3), lse.cpu().numpy().reshape(HQ, B, S).transpose(1, 0, 2)


def packed_quant(r, S, D):
    """(q8 [B, HQ, S, D], k8 [B, HKV, S, D] bytes, scale_q, scale_k) from the packed entries' images: q8 row-major per-sequence slabs, k8 the
    KFRAG image of every sequence (Hkv D (cu_k[i] + 64 i) bytes in)"""
    q8, k8 = bits8(r[0]), bits8(r[1])
    Sp = (S + 63) // 64 * 64
    k = [unpack_frag(k8[HKV * D * (S + 64) * i:][:HKV * Sp * D], _native.LAYOUT_KFRAG, 1, HKV, S, D)[0, :, :S] for i in range(B)]
    return q8[:B * HQ * S * D].reshape(B, HQ, S, D), np.stack(k), r[2].cpu().numpy(), r[3].cpu().numpy()


def v16_entries(tq, tk, tv, S, fp8, smooth=False):
    """{entry: (out [B, HQ, S, D] fp32, lse [B, HQ, S], (q8, k8 bytes [B, H, S, D], scale_q, scale_k) as returned; with smoothing the
    block-sparse k8 is left out)} of every 16-bit-V entry on one problem"""
    D = tq.shape[3]
    pq, pk, pv, cu = pack(tq), pack(tk), pack(tv), _cu(S)
    kw = dict(fp8_dtype=TDT[fp8], return_lse=True, return_quant=True, smooth_k=smooth)
    res = {}
    for causal in (False, True):
        r = _native.fp8_quant_attention_varlen(pq, pk, pv, cu, cu, None, is_causal=causal, **kw)
        res["packed causal" if causal else "packed"] = unpack(r[0], r[1], S) + (packed_quant(r[2:6], S, D),)
    r = _native.fp8_quant_attention_varlen_window(pq, pk, pv, cu, cu, None, window_left=L.WINDOW[0], window_right=L.WINDOW[1], **kw)
    res["window"] = unpack(r[0], r[1], S) + (packed_quant(r[2:6], S, D),)
    mask = torch.from_numpy(L.sparse_tiles(S)[None]).to(DEV)
    r = _native.fp8_block_sparse_attention(tq, tk, tv, mask, **kw)
    res["block-sparse"] = (out_to_f32(r[0]), r[1].cpu().numpy(), (bits8(r[2]), None if smooth else bits8(r[3]), r[4].cpu().numpy(), r[5].cpu().numpy()))
    return res


MASK_OF = {"packed": {}, "packed causal": {"causal": True}, "window": {"window": L.WINDOW}}


@functools.lru_cache(maxsize=2)
def v16_references(D, S, dtype, fp8, smoothed=False):
    """{entry: (ref out, ref lse)}: fp64 masked softmax on the CPU quantiser's q8, k8, scales and the caller's 16-bit V"""
    lad = L.head_ladder(D, S, S)
    mean = None
    if smoothed:
        _, lad, mean = L.antithetic(lad)
    qz = L.quantise(lad, dtype, fp8, "head")
    refs = {}
    for name in ("packed", "packed causal", "window", "block-sparse"):
        mask = L.mask_of(S, S, tiles=L.sparse_tiles(S)) if name == "block-sparse" else L.mask_of(S, S, **MASK_OF[name])
        if name in ("packed", "packed causal"):
            refs[name] = oracle.attention_forward(qz.q8, qz.k8, qz.vb16, L.FMT[fp8], L.FMT[fp8], fmt16(dtype), qz.sq, qz.sk, None, causal=name != "packed",
                                                  return_lse=True)
        else:
            refs[name] = L.Scores(qz, mask).softmax(v=qz.v16)
    return lad, qz, refs, mean


@pytest.mark.parametrize("case", L.PACKED_CASES, ids=lambda c: f"D{c[0]}_S{c[1]}_{L.NAME[c[2]]}_{c[3]}")
def test_16bit_v_entries_on_the_head_ladder(case):
    """packed (a batch entry is a sequence: e per (sequence, head)), window, block-sparse: 16-bit P on the caller's 16-bit V on every row"""
    D, S, dtype, fp8 = case
    lad, qz, refs, _ = v16_references(D, S, dtype, fp8)
    got = v16_entries(*G(*lad.tensors(dtype)), S, fp8)
    plain = v16_entries(*G(*L.head_ladder(D, S, S, gains=False).tensors(dtype)), S, fp8)
    e_only = v16_entries(*G(*L.head_ladder(D, S, S, f=False).tensors(dtype)), S, fp8)
    log = Log(f"packed / window / block-sparse, head ladder D {D} S {S} {L.NAME[dtype]} {fp8}")
    for name, (out, lse, quant) in got.items():
        ref, ref_lse = refs[name]
        dead = np.isneginf(ref_lse)
        assert (out[dead] == 0).all(), (name, "rows without a key must be exactly 0")
        w = log.out(out, ref, v16=True)
        wl = log.lse_err(lse, ref_lse, LSE_V16)
        assert w < 1.0 and wl < 1.0, (name, w, wl)
        # echo: the bytes of the plain call, the scales exactly 2^e times its scales and the CPU quantiser's
        for i, cpu in ((0, qz.q8), (1, qz.k8)):
            assert np.array_equal(quant[i], plain[name][2][i]) and np.array_equal(quant[i], cpu), (name, "q8 / k8: the bytes of the call without gains")
        for i, e, cpu in ((2, lad.e_q, qz.sq), (3, lad.e_k, qz.sk)):
            s, base = quant[i], plain[name][2][i]
            assert np.array_equal(s, base * np.exp2(e).astype(np.float32)) and np.array_equal(s, cpu), (name, "scale", i)
        # equivariance: e only
        assert np.array_equal(e_only[name][0], plain[name][0]) and np.array_equal(e_only[name][1], plain[name][1]), (name, "e only: the plain call bit for bit")
    log.done()


@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.float16), (256, torch.bfloat16)], ids=lambda x: str(x).replace("torch.", ""))
def test_16bit_attn_func_on_the_head_ladder(D, dtype):
    """no scale anywhere: the ladder still separates the heads and batch entries (k of the wrong kv group is 4 .. 64 x off)"""
    S = 1100
    lad = L.head_ladder(D, S, S)
    t = lad.tensors(dtype)
    b16 = lambda x: L.bits16(x)
    log = Log(f"16-bit attn_func, head ladder D {D} S {S} {L.NAME[dtype]}")
    for causal in (False, True):
        ref = oracle.attention_forward(b16(t[0]), b16(t[1]), b16(t[2]), fmt16(dtype), fmt16(dtype), fmt16(dtype), causal=causal)
        log.out(out_to_f32(qa.attn_func(*G(*t), is_causal=causal)), ref, label="16-bit entry")
        plain = qa.attn_func(*G(*L.head_ladder(D, S, S, gains=False).tensors(dtype)), is_causal=causal)
        e_only = qa.attn_func(*G(*L.head_ladder(D, S, S, f=False).tensors(dtype)), is_causal=causal)
        assert torch.equal(e_only, plain), "e only: q k^T does not move -- the plain call bit for bit"
    log.done()


# ---- key smoothing, dense and packed -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [L.HEAD_CASES[0], L.HEAD_CASES[5]], ids=L.case_id)
def test_dense_key_smoothing_on_the_head_ladder(case):
    """K = the ladder's keys in antithetic pairs + a channel offset c 2^e: the fp32 mean is c 2^e exactly, k - mean the ladder exactly.  The
    smoothed call must return that mean, quantise the ladder's own bytes and scales, and give the UNsmoothed call's out and path on the
    ladder bit for bit; its LSE moves by sm_scale q.mean"""
    D, Sq, Skv, causal, dtype, fp8 = case
    given, attend, mean = L.antithetic(L.head_ladder(D, Sq, Skv))
    qz = L.quantise(attend, dtype, fp8, "head")
    kw = dict(fp8=fp8, v_dtype=dtype, scaling="head", causal=causal)
    ref, ref_lse = oracle_for_fp8_path(qz.q8, qz.k8, qz.vb16, qz.sq, qz.sk, v_block=qz.v_block, fused=True, return_lse=True, **kw)
    corr = (attend.q * mean[:, L.kv_of(), None, :]).sum(-1) / math.sqrt(D)
    tq, tk, tv = G(*given.tensors(dtype))
    tka = attend.tensors(dtype)[1].to(DEV)
    log = Log(f"fused + smooth_k, head ladder {L.case_id(case)}")
    d128 = D == 128
    for prec in PRECISIONS:
        call = lambda k, smooth: _native.fp8_quant_attention_forward(tq, k, tv, is_causal=causal, fp8_dtype=TDT[fp8], precision=prec, smooth_k=smooth,
                                                                    return_lse=True, return_path=True, return_quant=True)
        out, lse, path, quant = call(tk, True)
        out0, lse0, path0, quant0 = call(tka, False)
        assert np.array_equal(quant["k_mean"].cpu().numpy(), mean.astype(np.float32)), "k_mean = c 2^e exactly"
        assert torch.equal(quant["k8"], quant0["k8"]) and torch.equal(quant["scale_k"], quant0["scale_k"]), "k - mean is the ladder: its bytes and scale_k"
        assert np.array_equal(quant["scale_k"].cpu().numpy(), qz.sk) and np.array_equal(quant["scale_q"].cpu().numpy(), qz.sq)
        assert torch.equal(out, out0) and torch.equal(path, path0), (prec, "the unsmoothed call on the ladder, bit for bit")
        p = path.cpu().numpy()
        log.out(out_to_f32(out), ref, p)
        log.lse_err(lse.cpu().numpy(), ref_lse + corr, fused_lse_tol(p, d128))
    log.done()


@pytest.mark.parametrize("case", L.PACKED_CASES[:2], ids=lambda c: f"D{c[0]}_S{c[1]}_{L.NAME[c[2]]}_{c[3]}")
def test_packed_key_smoothing_on_the_head_ladder(case):
    """the same construction per sequence (packed, window) and per batch entry (block-sparse)"""
    D, S, dtype, fp8 = case
    attend, qz, refs, mean = v16_references(D, S, dtype, fp8, smoothed=True)
    given = L.antithetic(L.head_ladder(D, S, S))[0]
    got = v16_entries(*G(*given.tensors(dtype)), S, fp8, smooth=True)
    base = v16_entries(*G(*attend.tensors(dtype)), S, fp8)
    corr = (attend.q * mean[:, L.kv_of(), None, :]).sum(-1) / math.sqrt(D)
    log = Log(f"packed / window / block-sparse + smooth_k, head ladder D {D} S {S} {L.NAME[dtype]} {fp8}")
    for name, (out, lse, quant) in got.items():
        ref, ref_lse = refs[name]
        w, wl = log.out(out, ref, v16=True), log.lse_err(lse, ref_lse + corr, LSE_V16)
        assert w < 1.0 and wl < 1.0, (name, w, wl)
        assert np.array_equal(quant[2], qz.sq) and np.array_equal(quant[3], qz.sk), (name, "the ladder's scales")
        assert np.array_equal(quant[0], qz.q8) and (quant[1] is None or np.array_equal(quant[1], qz.k8)), (name, "the ladder's bytes")
        assert np.array_equal(out, base[name][0]), (name, "k - mean is the ladder: the unsmoothed call on it, bit for bit")
    log.done()

"""Buffer contract of the C ABI (include/qattn*.h, DESIGN.md "Buffer contract"): every entry, called through ctypes with EVERY caller-provided
buffer carved from a guarded arena (tests/arena.py) of exactly the size the header's size function returns, at the minimum alignment the header
documents.  Per case:

  a. every guard of every buffer -- inputs included -- is intact after the call;
  b. out / lse / row_path / scales / k_mean (and the quantised tensors a header declares fully written) equal, BIT FOR BIT, the same call made
     the ordinary way (the `_native` wrapper the rest of the suite grades against the fp64 oracle): parity is inherited, no tolerance here;
  c. none of them holds leftover poison (NaN / 0x7f / 0xA5 pre-fill): every element was written;
  d. the bits do not depend on what the workspace and the scratch outputs held before the call (0x00, then 0xFF);
  e. nor on the bytes around the inputs: hostile (NaN, 0x7f, INT32_MIN / MAX, 0x01 mask bytes) and then benign (zero) guards, the pad
     elements between the rows and heads of a strided view included.

Exempt from b - e (assertion a only), each by the header line quoted where the buffer is carved: q8 of the fused entries where the kernel
quantises Q itself, their v8 / scale_v where V is block-scaled, k8 of the packed entries.  Every access these tests induce lies inside an allocation the test owns."""
import ctypes
import functools
import os
import re

import pytest
import torch

from quantumattention_amd import _native
from tests import arena as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HQ, HKV = 1, 4, 2
DENSE_SHAPES = [(1, 1), (65, 65), (257, 63), (1089, 1089)]
# (D, dtype, scaling): D in 64 / 128 / 256 bf16, fp16 at D = 128; head-wise, and token-wise at D = 64
CFGS = [(64, torch.bfloat16, "head-wise"), (64, torch.bfloat16, "token-wise"), (128, torch.bfloat16, "head-wise"),
        (128, torch.float16, "head-wise"), (256, torch.bfloat16, "head-wise")]
CFG_IDS = ["d64", "d64-token", "d128", "d128-fp16", "d256"]
# precision auto everywhere; at (1089, 1089) also accurate
DENSE_CASES = [(sq, skv, "auto") for sq, skv in DENSE_SHAPES] + [(1089, 1089, "accurate")]
DENSE_IDS = [f"{sq}x{skv}-{p}" for sq, skv, p in DENSE_CASES]
ALIGN16 = 16   # tensors, fragment images, workspaces, k_mean: include/qattn_buffers.h
ALIGN4 = 4     # fp32 scales / amax / lse, int32 tables
ALIGN1 = 1     # row_path, block_mask


def _kind(dtype):
    return A.KIND_OF_DTYPE[dtype]


def _bytes(t):
    t = t.contiguous()
    return (t.to(torch.uint8) if t.dtype == torch.bool else t).view(-1).view(torch.uint8)


class Plan:
    """The buffers of one C call and the five assertions."""

    def __init__(self):
        self.ar = A.Arena(DEV)
        self.views, self.logical, self.graded, self.padded = [], {}, [], {}

    def inp(self, name, t, align=ALIGN16, row_bytes=0):
        r = self.ar.carve(name, t.numel() * t.element_size(), align=align, row_bytes=row_bytes, role="in", kind=_kind(t.dtype))
        r.load(t)
        return r.ptr

    def inp_view(self, name, t, strides, span, row_bytes=0):
        """A strided view of `span` elements holding t; returns its address."""
        r = self.ar.carve(name, span * t.element_size(), align=ALIGN16, row_bytes=row_bytes, role="in", kind=_kind(t.dtype))
        self.views.append((r, t, strides))
        r.load_view(t, strides, hostile=True)
        return r.ptr

    def out(self, name, nbytes, kind, align=ALIGN16, row_bytes=0, logical=None):
        """A graded output (assertions a - e); logical: uint8 interior -> the bytes the header says are written (default: all).  What a
        `logical` leaves out -- the pads between the rows / heads of a strided `out`, the floats behind each REFERENCE-layout lse row -- must
        still hold the pre-fill after the call: nothing but the logical elements may be stored."""
        self.ar.carve(name, nbytes, align=align, row_bytes=row_bytes, role="out", kind=kind)
        self.graded.append(name)
        self.logical[name] = logical or (lambda b: b)
        self.padded[name] = logical is not None
        return self.ar[name].ptr

    def scratch(self, name, nbytes, align=ALIGN16, row_bytes=0):
        """Workspace, or an output the header declares scratch / partly unwritten: assertion a, and the pre-fill of d."""
        return self.ar.carve(name, nbytes, align=align, row_bytes=row_bytes, role="scratch").ptr

    def run(self, call, hostile, fill):
        self.ar.set_input_guards(hostile)
        for r, t, strides in self.views:
            r.load_view(t, strides, hostile=hostile)
        for r in self.ar.regions.values():
            if r.role == "out":
                r.fill_poison()
            elif r.role == "scratch":
                r.fill(fill)
        rc = call()
        torch.cuda.synchronize()
        assert rc == 0, (rc, _native.lib().qattn_strerror(rc))
        A.assert_guards_intact(self.ar)                                                     # a
        snap = {n: self.logical[n](self.ar[n].interior).contiguous().clone() for n in self.graded}
        for n in self.graded:                                                               # c
            left = self.ar[n].poison_left(snap[n])
            assert left == 0, f"{n}: {left} elements still hold the pre-fill: never written"
            if self.padded[n]:
                r = self.ar[n]
                esz = len(A.POISON[r.kind])
                pads, kept = (r.nbytes - snap[n].numel()) // esz, r.poison_left()
                assert kept == pads, f"{n}: {pads - kept} of the {pads} pad elements outside the logical view were overwritten"
        return snap

    def check(self, call, expected):
        first = self.run(call, True, 0x00)
        for n in self.graded:                                                               # b
            want = _bytes(expected[n])
            assert want.numel() == first[n].numel(), (n, want.numel(), first[n].numel())
            assert torch.equal(first[n].view(-1), want), f"{n}: bits differ from the ordinary call at {_first_diff(first[n].view(-1), want)}"
        ones = self.run(call, True, 0xFF)
        benign = self.run(call, False, 0x00)
        for n in self.graded:
            assert torch.equal(first[n], ones[n]), f"{n}: depends on what the workspace / scratch held (0x00 vs 0xFF)"      # d
            assert torch.equal(first[n], benign[n]), f"{n}: depends on bytes outside the inputs (hostile vs benign guards)"  # e
        return first


def _first_diff(a, b):
    idx = torch.nonzero(a != b).view(-1)
    return f"byte {int(idx[0])} .. {int(idx[-1])}, {idx.numel()} bytes"


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _qkv(Sq, Skv, D, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 * Sq + 10 * Skv + D + seed)
    q = torch.randn(B, HQ, Sq, D, generator=g)
    k, v = (torch.randn(B, HKV, Skv, D, generator=g) for _ in range(2))
    return tuple(t.to(dtype).to(DEV) for t in (q, k, v))


def _strided_rows(name, t):
    """(strides, span) of a view of t [B,H,S,D] with padded rows and heads: rows D + 8 elements apart, heads 16 elements further."""
    _, H, S, D = t.shape
    rs = D + 8
    hs = S * rs + 16
    return (H * hs, hs, rs, 1), t.shape[0] * H * hs


def _bshd(t):
    """(strides, span) of t [B,H,S,D] as the transpose of a dense [B,S,H,D] tensor."""
    _, H, S, D = t.shape
    return (S * H * D, D, H * D, 1), t.numel()


def _as_logical(dtype, shape, strides):
    return lambda b: torch.as_strided(b.view(dtype), shape, strides).contiguous().view(-1).view(torch.uint8)


def _c3(strides_list):
    flat = [s for st in strides_list for s in st[:3]]
    return (ctypes.c_longlong * len(flat))(*flat)


# ---------------------------------------------------------------------------------------------------------------- 1. qattn_quant_fp8
@pytest.mark.parametrize("layout", [_native.LAYOUT_ROWMAJOR, _native.LAYOUT_KFRAG, _native.LAYOUT_VFRAG], ids=["rowmajor", "kfrag", "vfrag"])
@pytest.mark.parametrize("S", [1, 65, 257, 1089])
@pytest.mark.parametrize("D,dtype,scaling", CFGS, ids=CFG_IDS)
def test_quant_fp8(D, dtype, scaling, S, layout):
    L = _native.lib()
    x = _qkv(S, S, D, dtype)[0]
    mode = _native._scale_mode(scaling)
    want8, wants = _native.quant_fp8(x, scaling=scaling, layout=layout)
    p = Plan()
    px = p.inp("x", x, row_bytes=2 * D)
    p8 = p.out("x8", L.qattn_fp8_tensor_bytes(layout, B, HQ, S, D), "fp8", row_bytes=D)   # (fragment layouts: S zero-padded to 64, include/qattn.h)
    ps = p.out("scale", 4 * wants.numel(), "fp32", align=ALIGN4)
    wb = L.qattn_quant_workspace_bytes(B, HQ, S, D, mode)
    pw = p.scratch("workspace", wb)
    p.check(lambda: L.qattn_quant_fp8(px, _native.fmt_of(dtype), p8, ps, B, HQ, S, D, _native.FMT_E4M3, mode, 0, layout, pw, wb, _stream()),
            {"x8": want8, "scale": wants})


# ------------------------------------------------------------------------------------------------------------ 2. qattn_quant_qkv_fp8
@pytest.mark.parametrize("Sq,Skv", DENSE_SHAPES)
@pytest.mark.parametrize("D,dtype,scaling", CFGS, ids=CFG_IDS)
def test_quant_qkv_fp8(D, dtype, scaling, Sq, Skv):
    L = _native.lib()
    q, k, v = _qkv(Sq, Skv, D, dtype)
    mode = _native._scale_mode(scaling)
    w = dict(zip(("q8", "k8", "v8", "scale_q", "scale_k", "scale_v"), _native.quant_qkv_fp8(q, k, v, scaling=scaling)))
    p = Plan()
    pq, pk, pv = (p.inp(n, t, row_bytes=2 * D) for n, t in (("q", q), ("k", k), ("v", v)))
    o = [p.out("q8", L.qattn_fp8_tensor_bytes(_native.LAYOUT_ROWMAJOR, B, HQ, Sq, D), "fp8", row_bytes=D),
         p.out("k8", L.qattn_fp8_tensor_bytes(_native.LAYOUT_KFRAG, B, HKV, Skv, D), "fp8", row_bytes=D),
         p.out("v8", L.qattn_fp8_tensor_bytes(_native.LAYOUT_VFRAG, B, HKV, Skv, D), "fp8", row_bytes=D)]
    o += [p.out(n, 4 * w[n].numel(), "fp32", align=ALIGN4) for n in ("scale_q", "scale_k", "scale_v")]
    wb = L.qattn_quant_qkv_workspace_bytes(B, HQ, HKV)
    pw = p.scratch("workspace", wb)
    p.check(lambda: L.qattn_quant_qkv_fp8(pq, pk, pv, _native.fmt_of(dtype), *o, B, HQ, HKV, Sq, Skv, D, _native.FMT_E4M3, mode, 0, pw, wb, _stream()), w)


# ------------------------------------------------------------------------------------------------------- 3. / 4. qattn_pack_fp8, _pack16
@pytest.mark.parametrize("layout", [_native.LAYOUT_KFRAG, _native.LAYOUT_VFRAG], ids=["kfrag", "vfrag"])
@pytest.mark.parametrize("S", [1, 65, 257, 1089])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_pack_fp8(D, S, layout):
    L = _native.lib()
    x8, _ = _native.quant_fp8(_qkv(S, S, D, torch.bfloat16)[0])     # (quantised bytes: never the 0x7f of the pre-fill)
    p = Plan()
    px = p.inp("x8", x8, row_bytes=D)
    po = p.out("packed", L.qattn_fp8_tensor_bytes(layout, B, HQ, S, D), "fp8", row_bytes=D)
    p.check(lambda: L.qattn_pack_fp8(px, po, B, HQ, S, D, layout, _stream()), {"packed": _native.pack_fp8(x8, layout)})


@pytest.mark.parametrize("layout", [_native.LAYOUT_K16FRAG, _native.LAYOUT_V16FRAG], ids=["k16frag", "v16frag"])
@pytest.mark.parametrize("S", [1, 65, 257, 1089])
@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.bfloat16), (128, torch.float16), (256, torch.bfloat16)])
def test_pack16(D, dtype, S, layout):
    L = _native.lib()
    x = _qkv(S, S, D, dtype)[0]
    p = Plan()
    px = p.inp("x", x, row_bytes=2 * D)
    po = p.out("packed", L.qattn_16bit_tensor_bytes(layout, B, HQ, S, D), _kind(dtype), row_bytes=2 * D)
    p.check(lambda: L.qattn_pack16(px, po, B, HQ, S, D, layout, _stream()), {"packed": _native.pack16(x, layout)})


# --------------------------------------------------------------------------- 5. / 6. qattn_fp8_attention_forward, fp8 V and 16-bit V
@pytest.mark.parametrize("v16", [False, True], ids=["fp8v", "v16"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Sq,Skv,precision", DENSE_CASES, ids=DENSE_IDS)
@pytest.mark.parametrize("D,dtype,scaling", CFGS, ids=CFG_IDS)
def test_fp8_attention_forward(D, dtype, scaling, Sq, Skv, precision, causal, v16):
    L = _native.lib()
    q, k, v = _qkv(Sq, Skv, D, dtype)
    mode = _native._scale_mode(scaling)
    q8, kf, vf, sq, sk, sv = _native.quant_qkv_fp8(q, k, v, scaling=scaling)
    wo, wl = _native.fp8_attention_forward(q8, kf, v if v16 else vf, sq, sk, None if v16 else sv, Hkv=HKV, Skv=Skv, out_dtype=dtype,
                                           is_causal=causal, scaling=scaling, return_lse=True, precision=precision)
    p = Plan()
    pq, pk = p.inp("q8", q8, row_bytes=D), p.inp("k8", kf, row_bytes=D)
    pv = p.inp("v16", v, row_bytes=2 * D) if v16 else p.inp("v8", vf, row_bytes=D)
    psq, psk = p.inp("scale_q", sq, align=ALIGN4), p.inp("scale_k", sk, align=ALIGN4)
    psv = None if v16 else p.inp("scale_v", sv, align=ALIGN4)
    po = p.out("out", 2 * B * HQ * Sq * D, _kind(dtype), row_bytes=2 * D)
    pl = p.out("lse", 4 * B * HQ * L.qattn_lse_row_stride(Sq, _native.LSE_NATURAL), "fp32", align=ALIGN4)
    wb = L.qattn_attention_workspace_bytes(B, HQ, Sq)
    pw = p.scratch("workspace", wb)
    f16, f8 = _native.fmt_of(dtype), _native.FMT_E4M3
    p.check(lambda: L.qattn_fp8_attention_forward(pq, pk, pv, po, pl, psq, psk, psv, B, HQ, HKV, Sq, Skv, D, f8, f16 if v16 else f8, f16, mode,
                                                  int(causal), 0.0, _native.PRECISION[precision], _native.LSE_NATURAL, pw, wb, _stream()),
            {"out": wo, "lse": wl})


# ------------------------------------------------------------------------------------------- 7. qattn_fp8_attention_forward_rowmajor
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Sq,Skv,precision", DENSE_CASES, ids=DENSE_IDS)
@pytest.mark.parametrize("D,dtype,scaling", CFGS, ids=CFG_IDS)
def test_fp8_attention_forward_rowmajor(D, dtype, scaling, Sq, Skv, precision, causal):
    L = _native.lib()
    q, k, v = _qkv(Sq, Skv, D, dtype)
    mode = _native._scale_mode(scaling)
    (q8, sq), (k8, sk) = _native.quant_fp8(q, scaling=scaling), _native.quant_fp8(k, scaling=scaling)
    wo, wl = _native.fp8_attention_forward_rowmajor(q8, k8, v, sq, sk, is_causal=causal, precision=precision, return_lse=True)
    p = Plan()
    pq, pk, pv = p.inp("q8", q8, row_bytes=D), p.inp("k8", k8, row_bytes=D), p.inp("v16", v, row_bytes=2 * D)
    psq, psk = p.inp("scale_q", sq, align=ALIGN4), p.inp("scale_k", sk, align=ALIGN4)
    po = p.out("out", 2 * B * HQ * Sq * D, _kind(dtype), row_bytes=2 * D)
    pl = p.out("lse", 4 * B * HQ * L.qattn_lse_row_stride(Sq, _native.LSE_NATURAL), "fp32", align=ALIGN4)
    wb = L.qattn_fp8_attention_rowmajor_workspace_bytes(B, HQ, HKV, Sq, Skv, D)
    pw = p.scratch("workspace", wb, row_bytes=D)
    f16, f8 = _native.fmt_of(dtype), _native.FMT_E4M3
    p.check(lambda: L.qattn_fp8_attention_forward_rowmajor(pq, pk, pv, po, pl, psq, psk, B, HQ, HKV, Sq, Skv, D, f8, f16, f8, mode, int(causal), 0.0,
                                                           _native.PRECISION[precision], _native.LSE_NATURAL, pw, wb, _stream()),
            {"out": wo, "lse": wl})


# ------------------------------------------------------- 8. / 9. / 10. the fused entries: ..._forward_ex, ..._forward_strided, ..._forward_smooth
def _fused_contract(entry, q, k, v, scaling, precision, causal, view=None, lse_layout=_native.LSE_REFERENCE):
    """entry: "ex" (dense, qattn_fp8_quant_attention_forward_ex), "strided" (view: "rows" = padded rows and heads of q, k, v AND out;
    "bshd" = all four the transposes of dense [B,S,H,D] tensors -- the `like_query` output layout), "smooth"."""
    L = _native.lib()
    Bq, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    dtype = q.dtype
    mode = _native._scale_mode(scaling)
    smooth = entry == "smooth"
    res = _native.fp8_quant_attention_forward(q, k, v, is_causal=causal, scaling=scaling, precision=precision, return_lse=True,
                                              lse_layout=lse_layout, return_path=True, return_quant=True, smooth_k=smooth)
    want = {"out": res[0], "lse": res[1], "row_path": res[2], "scale_q": res[3]["scale_q"], "scale_k": res[3]["scale_k"], "k8": res[3]["k8"]}
    desc = _native.describe_path("fused", D, dtype, scaling, Skv)
    p = Plan()
    strides = None
    oshape = (Bq, Hq, Sq, D)
    if view is None:
        pq, pk, pv = (p.inp(n, t, row_bytes=2 * D) for n, t in (("q", q), ("k", k), ("v", v)))
        po = p.out("out", 2 * q.numel(), _kind(dtype), row_bytes=2 * D)
    else:
        lay = _strided_rows if view == "rows" else (lambda name, t: _bshd(t))
        lays = [lay(n, t) for n, t in (("q", q), ("k", k), ("v", v), ("out", q))]
        pq, pk, pv = (p.inp_view(n, t, lays[i][0], lays[i][1], row_bytes=2 * lays[i][0][2]) for i, (n, t) in enumerate((("q", q), ("k", k), ("v", v))))
        po = p.out("out", 2 * lays[3][1], _kind(dtype), row_bytes=2 * lays[3][0][2], logical=_as_logical(dtype, oshape, lays[3][0]))
        strides = _c3([l[0] for l in lays])
    ld = L.qattn_lse_row_stride(Sq, lse_layout)
    # include/qattn.h: REFERENCE rows are qattn_lse_row_stride() floats apart; the floats between Sq and the stride are not written
    pl = p.out("lse", 4 * Bq * Hq * ld, "fp32", align=ALIGN4, logical=_as_logical(torch.float32, (Bq, Hq, Sq), (Hq * ld, ld, 1)))
    pp = p.out("row_path", Bq * Hq * Sq, "path", align=ALIGN1)
    n_sq, n_sk = (Bq * Hq, Bq * Hkv) if mode == _native.SCALE_HEAD else (Bq * Hq * Sq, Bq * Hkv * Skv)
    psq, psk = p.out("scale_q", 4 * n_sq, "fp32", align=ALIGN4), p.out("scale_k", 4 * n_sk, "fp32", align=ALIGN4)
    pk8 = p.out("k8", L.qattn_fp8_tensor_bytes(_native.LAYOUT_KFRAG, Bq, Hkv, Skv, D), "fp8", row_bytes=D)
    # include/qattn.h, qattn_fp8_quant_attention_forward: "q8 / k8 / v8 / scale_*: caller-provided outputs + scratch (qattn_quant_qkv_fp8's
    # sizes; q8 untouched where the kernel quantises Q; scale_v = 1 where V is block-scaled)".  So, by the PATH TABLE columns q_quant / v_format:
    #   q8            EXEMPT (a only) where q_quant = kernel (D = 128 head-wise); else the pre-pass's row-major image: graded, b against
    #                 qattn_quant_qkv_fp8's q8
    #   v8, scale_v   EXEMPT (a only) where v_format = block (head-wise, Skv <= 16384: the bytes carry per-chunk scales that live in the
    #                 workspace, scale_v is the constant 1); else the per-head VFRAG image and its scale: graded, b against qattn_quant_qkv_fp8's
    n_q8 = L.qattn_fp8_tensor_bytes(_native.LAYOUT_ROWMAJOR, Bq, Hq, Sq, D)
    n_v8 = L.qattn_fp8_tensor_bytes(_native.LAYOUT_VFRAG, Bq, Hkv, Skv, D)
    q_in_kernel, v_block = desc["q_quant"] == "kernel", desc["v_format"] == "block"
    img = None if (q_in_kernel and v_block) else _native.quant_qkv_fp8(q, k, v, scaling=scaling)
    if q_in_kernel:
        pq8 = p.scratch("q8", n_q8, row_bytes=D)
    else:
        pq8 = p.out("q8", n_q8, "fp8", row_bytes=D)
        want["q8"] = img[0]
    if v_block:
        pv8 = p.scratch("v8", n_v8, row_bytes=D)
        psv = p.scratch("scale_v", 4 * Bq * Hkv, align=ALIGN4)
    else:
        pv8 = p.out("v8", n_v8, "fp8", row_bytes=D)
        psv = p.out("scale_v", 4 * Bq * Hkv, "fp32", align=ALIGN4)
        want["v8"], want["scale_v"] = img[2], res[3]["scale_v"]
    args = [pq, pk, pv, strides, _native.fmt_of(dtype), po, pq8, pk8, pv8, psq, psk, psv, None, None, None, None, None, Bq, Hq, Hkv, Sq, Skv, D,
            _native.FMT_E4M3, mode, 0, int(causal), 0.0, _native.PRECISION[precision], pl, lse_layout, pp]
    if smooth:
        want["k_mean"] = res[3]["k_mean"]
        pm = p.out("k_mean", 4 * Bq * Hkv * D, "fp32")
        wb = L.qattn_fp8_quant_attention_smooth_workspace_bytes(Bq, Hq, Hkv, Sq, Skv, D)
        pw = p.scratch("workspace", wb)
        call = lambda: L.qattn_fp8_quant_attention_forward_smooth(*args, pw, wb, _stream(), pm)
    else:
        wb = L.qattn_fp8_quant_attention_workspace_bytes(Bq, Hq, Hkv, Sq)
        pw = p.scratch("workspace", wb)
        if entry == "ex":
            del args[3]
            call = lambda: L.qattn_fp8_quant_attention_forward_ex(*args, pw, wb, _stream())
        else:
            call = lambda: L.qattn_fp8_quant_attention_forward_strided(*args, pw, wb, _stream())
    return p.check(call, want), want


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Sq,Skv,precision", DENSE_CASES, ids=DENSE_IDS)
@pytest.mark.parametrize("D,dtype,scaling", CFGS, ids=CFG_IDS)
def test_fp8_quant_attention_forward_ex(D, dtype, scaling, Sq, Skv, precision, causal):
    """With lse (the reference layout: rows at the padded stride) and row_path."""
    _fused_contract("ex", *_qkv(Sq, Skv, D, dtype), scaling, precision, causal)


@pytest.mark.parametrize("view", ["rows", "bshd"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Sq,Skv,precision", DENSE_CASES, ids=DENSE_IDS)
@pytest.mark.parametrize("D,dtype,scaling", CFGS, ids=CFG_IDS)
def test_fp8_quant_attention_forward_strided(D, dtype, scaling, Sq, Skv, precision, causal, view):
    """q, k, v and out as views with hostile pads between rows and heads ("rows"), and as transposes of [B,S,H,D] tensors ("bshd": the
    output carved with [B,S,H,D] strides is the `like_query` layout -- the C entry takes output strides, include/qattn_strided.h)."""
    _fused_contract("strided", *_qkv(Sq, Skv, D, dtype), scaling, precision, causal, view=view, lse_layout=_native.LSE_NATURAL)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Sq,Skv,precision", DENSE_CASES, ids=DENSE_IDS)
@pytest.mark.parametrize("D,dtype,scaling", CFGS, ids=CFG_IDS)
def test_fp8_quant_attention_forward_smooth(D, dtype, scaling, Sq, Skv, precision, causal):
    _fused_contract("smooth", *_qkv(Sq, Skv, D, dtype), scaling, precision, causal, lse_layout=_native.LSE_NATURAL)


def test_dynamic_hand_out_and_rescue_lists_do_not_depend_on_the_workspace():
    """The one case that reaches the per-XCD block counters and the rescue lists in the workspace (assertion d's teeth): the shape of
    test_dynamic_hand_out_of_a_large_non_causal_launch_equals_static_shares (8 x 32 heads x 24 blocks, D = 128, non-causal, AUTO) with the
    sharp rows of test_scattered_peaked_rows_are_gathered_and_recomputed (33 of every 256-row block, q x 2.2)."""
    g = torch.Generator(device=DEV).manual_seed(133)
    Bb, H, S, D = 8, 32, 6144, 128
    # csrc/qattn_attn_v2.hip launch_attn_v2_chk: a non-causal launch with a workspace draws its blocks from the per-XCD counters iff
    # total_blocks >= kDynMinRounds x CUs (csrc/qattn_attn.h).  No host-side query reports the choice, so the condition is restated here on
    # the constant read from the source: a change of either leaves this case failing, not silently static.
    src = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "qattn_attn.h")).read()
    dyn_min_rounds = int(re.search(r"constexpr int kDynMinRounds = (\d+);", src).group(1))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert Bb * H * -(-S // 256) >= dyn_min_rounds * cus, (dyn_min_rounds, cus, "the launch would take static shares: enlarge the shape")
    q, k, v = (torch.randn(Bb, H, S, D, dtype=torch.bfloat16, device=DEV, generator=g) for _ in range(3))
    sharp = torch.zeros(S, dtype=torch.bool)
    gc = torch.Generator().manual_seed(133)
    for blk in range(S // 256):
        sharp[torch.randperm(256, generator=gc)[:33] + 256 * blk] = True
    q[:, :, sharp.to(DEV)] *= 2.2
    first, _ = _fused_contract("ex", q, k, v, "head-wise", "auto", False, lse_layout=_native.LSE_NATURAL)
    path = first["row_path"].view(Bb, H, S)
    # (what the case is for: with 6144 >= 1024 keys and no causal mask no block is "early", so a row off the one-term sweep was flagged, listed
    # in the workspace and recomputed.  Every head must have such rows; HOW MANY of the sharp rows are
    # flagged is the precision rule's business -- graded in tests/test_gpu_precision.py -- and falls with the key count.)
    rescued = path != _native.PATH_ONE_TERM
    assert rescued[:, :, sharp.to(DEV)].any(dim=2).all(), "every head must have sent sharp rows through the rescue lists"


# ----------------------------------------------------------------------- 11. / 12. qattn_attention_forward_16, ..._forward_16_strided
@pytest.mark.parametrize("view", [None, "rows", "bshd"], ids=["dense", "rows", "bshd"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Sq,Skv", DENSE_SHAPES)
@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.bfloat16), (128, torch.float16), (256, torch.bfloat16)])
def test_attention_forward_16(D, dtype, Sq, Skv, causal, view):
    """view None: qattn_attention_forward_16; else qattn_attention_forward_16_strided on q and out (six strides)."""
    L = _native.lib()
    q, k, v = _qkv(Sq, Skv, D, dtype)
    kf, vf = _native.pack16(k, _native.LAYOUT_K16FRAG), _native.pack16(v, _native.LAYOUT_V16FRAG)
    wo, wl = _native.attention_forward_16(q, kf, vf, Hkv=HKV, Skv=Skv, is_causal=causal, return_lse=True)
    p = Plan()
    pk, pv = p.inp("k16", kf, row_bytes=2 * D), p.inp("v16", vf, row_bytes=2 * D)
    pl = p.out("lse", 4 * B * HQ * Sq, "fp32", align=ALIGN4)
    f = _native.fmt_of(dtype)
    if view is None:
        pq = p.inp("q", q, row_bytes=2 * D)
        po = p.out("out", 2 * q.numel(), _kind(dtype), row_bytes=2 * D)
        call = lambda: L.qattn_attention_forward_16(pq, pk, pv, po, pl, B, HQ, HKV, Sq, Skv, D, f, int(causal), 0.0, 0, _stream())
    else:
        st, span = _strided_rows("q", q) if view == "rows" else _bshd(q)
        pq = p.inp_view("q", q, st, span, row_bytes=2 * st[2])
        po = p.out("out", 2 * span, _kind(dtype), row_bytes=2 * st[2], logical=_as_logical(dtype, tuple(q.shape), st))
        strides = _c3([st, st])
        call = lambda: L.qattn_attention_forward_16_strided(pq, strides, pk, pv, po, pl, B, HQ, HKV, Sq, Skv, D, f, int(causal), 0.0, 0, _stream())
    p.check(call, {"out": wo, "lse": wl})


# --------------------------------------------------------- 13. / 14. / 15. the packed entries: varlen, varlen smooth, varlen window
# "issue": the lengths the contract is stated on (every row has a key).  "keyless": sequence 1 has 3 queries and no used key; sequence 3 has
# 70 queries on 5 used keys, so under the windows (0, 0) and (64, 0) its rows r < 65 attend nothing (include/qattn_window.h: rows
# r < -delta - window_right).  Such rows must be WRITTEN as zeros with an LSE of -inf: on pre-filled memory, not by luck.
LENGTHS = {"issue": ([65, 0, 257, 1], [130, 9, 300, 64], [129, 0, 257, 1]),
           "keyless": ([65, 3, 257, 70], [130, 9, 300, 64], [129, 0, 257, 5])}


def _keyless_rows(lq, used, window):
    """bool [total_q]: rows that attend no key (include/qattn_varlen.h, include/qattn_window.h)."""
    rows = []
    for n, u in zip(lq, used):
        for r in range(n):
            lo, hi = 0, u - 1
            if window is not None:
                wl, wr = window
                lo = max(lo, r + (u - n) - wl) if wl >= 0 else lo
                hi = min(hi, r + (u - n) + wr) if wr >= 0 else hi
            rows.append(lo > hi)
    return torch.tensor(rows, dtype=torch.bool, device=DEV)


@functools.lru_cache(maxsize=None)
def _packed(D, lengths):
    LQ, LK_ALLOC, USED = LENGTHS[lengths]
    g = torch.Generator().manual_seed(77 + D)
    tq, tk = sum(LQ), sum(LK_ALLOC)
    q = torch.randn(tq, HQ, D, generator=g)
    k, v = (torch.randn(tk, HKV, D, generator=g) for _ in range(2))
    cu = lambda ls: torch.tensor([0] + torch.tensor(ls).cumsum(0).tolist(), dtype=torch.int32)
    cu_q, cu_k = cu(LQ), cu(LK_ALLOC)
    for i, used in enumerate(USED):   # keys beyond seqused_k influence no output bit (include/qattn_varlen.h): NaN there
        k[int(cu_k[i]) + used:int(cu_k[i + 1])] = float("nan")
        v[int(cu_k[i]) + used:int(cu_k[i + 1])] = float("nan")
    return tuple(t.to(torch.bfloat16).to(DEV) for t in (q, k, v)) + (cu_q.to(DEV), cu_k.to(DEV), torch.tensor(USED, dtype=torch.int32, device=DEV))


def _packed_contract(D, smooth, causal=False, window=None, lengths="issue"):
    L = _native.lib()
    LQ, LK_ALLOC, USED = LENGTHS[lengths]
    q, k, v, cu_q, cu_k, used = _packed(D, lengths)
    nb, tq, tk = len(LQ), sum(LQ), sum(LK_ALLOC)
    if window is None:
        res = _native.fp8_quant_attention_varlen(q, k, v, cu_q, cu_k, used, is_causal=causal, return_lse=True, return_quant=True, smooth_k=smooth)
    else:
        res = _native.fp8_quant_attention_varlen_window(q, k, v, cu_q, cu_k, used, window_left=window[0], window_right=window[1], return_lse=True,
                                                        return_quant=True, smooth_k=smooth)
    want = {"out": res[0], "lse": res[1], "q8": res[2], "scale_q": res[4], "scale_k": res[5]}
    p = Plan()
    pq, pk, pv = p.inp("q", q, row_bytes=2 * HQ * D), p.inp("k", k, row_bytes=2 * HKV * D), p.inp("v", v, row_bytes=2 * HKV * D)
    pcq, pck, pu = (p.inp(n, t, align=ALIGN4) for n, t in (("cu_seqlens_q", cu_q), ("cu_seqlens_k", cu_k), ("seqused_k", used)))
    po = p.out("out", 2 * tq * HQ * D, "bf16", row_bytes=2 * HQ * D)
    pl = p.out("lse", 4 * HQ * tq, "fp32", align=ALIGN4)
    pq8 = p.out("q8", L.qattn_varlen_tensor_bytes(_native.LAYOUT_ROWMAJOR, nb, HQ, tq, D), "fp8", row_bytes=D)
    psq, psk = p.out("scale_q", 4 * nb * HQ, "fp32", align=ALIGN4), p.out("scale_k", 4 * nb * HKV, "fp32", align=ALIGN4)
    # EXEMPT (a only) -- include/qattn_varlen.h: "k8 KFRAG ..., sequence i's [Hkv, ceil(L_k/64) 64, D] image at byte Hkv D (cu_k[i] + 64 i)":
    # the images of the USED keys do not tile the H D (total + 64 B) bytes; the gaps between them are not written.
    pk8 = p.scratch("k8", L.qattn_varlen_tensor_bytes(_native.LAYOUT_KFRAG, nb, HKV, tk, D), row_bytes=D)
    pm = None
    if smooth:
        want["k_mean"] = res[6]
        pm = p.out("k_mean", 4 * nb * HKV * D, "fp32")
    f = _native.fmt_of(torch.bfloat16)
    if window is None:
        ws_of = L.qattn_fp8_quant_attention_varlen_smooth_workspace_bytes if smooth else L.qattn_fp8_quant_attention_varlen_workspace_bytes
        wb = ws_of(nb, HQ, HKV, tq, tk, D)
        pw = p.scratch("workspace", wb, row_bytes=D)
        args = (pq, pk, pv, None, f, po, pl, pcq, pck, pu, nb, HQ, HKV, tq, tk, D, _native.FMT_E4M3, 0, int(causal), 0.0, pq8, pk8, psq, psk, pw, wb, _stream())
        call = (lambda: L.qattn_fp8_quant_attention_varlen_forward_smooth(*args, pm)) if smooth else (lambda: L.qattn_fp8_quant_attention_varlen_forward(*args))
    else:
        wb = L.qattn_fp8_quant_attention_varlen_window_workspace_bytes(nb, HQ, HKV, tq, tk, D)
        pw = p.scratch("workspace", wb, row_bytes=D)
        i32 = 2 ** 31 - 1
        call = lambda: L.qattn_fp8_quant_attention_varlen_window_forward(pq, pk, pv, None, f, po, pl, pcq, pck, pu, nb, HQ, HKV, tq, tk, D, _native.FMT_E4M3, 0,
                                                                         min(window[0], i32), min(window[1], i32), 0.0, pq8, pk8, psq, psk, pw, wb, _stream(), pm)
    first = p.check(call, want)
    # rows without a key: exact zeros and an LSE of -inf, as tests/test_gpu_varlen.py and tests/test_gpu_window.py assert on ordinary memory
    empty = _keyless_rows(LQ, USED, window)
    out = first["out"].view(torch.bfloat16).view(tq, HQ, D)
    lse = first["lse"].view(torch.float32).view(HQ, tq)
    assert (out[empty].view(torch.int16) == 0).all(), "a row without a key gets a zero output row"
    assert (lse[:, empty] == float("-inf")).all() and torch.isfinite(lse[:, ~empty]).all()
    if lengths == "keyless":
        assert int(empty.sum()) >= 3 + (65 if window in ((0, 0), (64, 0)) else 0)


@pytest.mark.parametrize("lengths", ["issue", "keyless"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_fp8_quant_attention_varlen_forward(D, causal, lengths):
    _packed_contract(D, False, causal, lengths=lengths)


@pytest.mark.parametrize("lengths", ["issue", "keyless"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_fp8_quant_attention_varlen_forward_smooth(D, causal, lengths):
    _packed_contract(D, True, causal, lengths=lengths)


@pytest.mark.parametrize("lengths", ["issue", "keyless"])
@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "smooth"])
@pytest.mark.parametrize("window", [(0, 0), (64, 0), (5, -1)])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_fp8_quant_attention_varlen_window_forward(D, window, smooth, lengths):
    _packed_contract(D, smooth, window=window, lengths=lengths)


# ----------------------------------------------------------------------------- 16. / 17. the block-sparse entries, plain and smoothing
@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "smooth"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_fp8_block_sparse_attention_forward(D, smooth):
    """(Sq, Skv) = (300, 385): 3 x 4 tiles, the last of each axis ragged.  Query block 1 lists nothing (zero rows, LSE -inf, asserted on the
    poisoned output), query block 2 lists every key block.  The mask is ONE [3, 4] byte table broadcast over batch and heads (strides 0)
    inside hostile guards of 0x01: a mask byte read one tile out of range turns a tile on."""
    L = _native.lib()
    Sq, Skv = 300, 385
    q, k, v = _qkv(Sq, Skv, D, torch.bfloat16, seed=5)
    m = torch.tensor([[1, 0, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1]], dtype=torch.bool, device=DEV)
    res = _native.fp8_block_sparse_attention(q, k, v, m.expand(B, HQ, 3, 4), return_lse=True, return_quant=True, smooth_k=smooth)
    want = {"out": res[0], "lse": res[1], "q8": res[2], "k8": res[3], "scale_q": res[4], "scale_k": res[5]}
    p = Plan()
    pq, pk, pv = (p.inp(n, t, row_bytes=2 * D) for n, t in (("q", q), ("k", k), ("v", v)))
    pmask = p.inp("block_mask", m, align=ALIGN1, row_bytes=4)
    mstr = (ctypes.c_longlong * 4)(0, 0, 4, 1)
    po = p.out("out", 2 * q.numel(), "bf16", row_bytes=2 * D)
    pl = p.out("lse", 4 * B * HQ * Sq, "fp32", align=ALIGN4)
    pq8 = p.out("q8", L.qattn_fp8_tensor_bytes(_native.LAYOUT_ROWMAJOR, B, HQ, Sq, D), "fp8", row_bytes=D)
    # include/qattn_block_sparse.h: k8 row-major [B, Hkv, Skv, D] (plain) / the KFRAG image, zero-padded to 64 keys (smoothing): fully written
    pk8 = p.out("k8", L.qattn_fp8_tensor_bytes(_native.LAYOUT_KFRAG if smooth else _native.LAYOUT_ROWMAJOR, B, HKV, Skv, D), "fp8", row_bytes=D)
    psq, psk = p.out("scale_q", 4 * B * HQ, "fp32", align=ALIGN4), p.out("scale_k", 4 * B * HKV, "fp32", align=ALIGN4)
    ws_of = L.qattn_fp8_block_sparse_attention_smooth_workspace_bytes if smooth else L.qattn_fp8_block_sparse_attention_workspace_bytes
    wb = ws_of(B, HQ, HKV, Sq, Skv, D)
    pw = p.scratch("workspace", wb, row_bytes=D)
    args = (pq, pk, pv, _native.fmt_of(torch.bfloat16), po, pl, pmask, mstr, B, HQ, HKV, Sq, Skv, D, _native.FMT_E4M3, 0, 0.0, pq8, pk8, psq, psk, pw, wb, _stream())
    if smooth:
        want["k_mean"] = res[6]
        pm = p.out("k_mean", 4 * B * HKV * D, "fp32")
        call = lambda: L.qattn_fp8_block_sparse_attention_forward_smooth(*args, pm)
    else:
        call = lambda: L.qattn_fp8_block_sparse_attention_forward(*args)
    first = p.check(call, want)
    out = first["out"].view(torch.bfloat16).view(B, HQ, Sq, D)
    lse = first["lse"].view(torch.float32).view(B, HQ, Sq)
    assert (out[:, :, 128:256].view(torch.int16) == 0).all(), "a query block without a key block gets zero rows"
    assert (lse[:, :, 128:256] == float("-inf")).all()
    assert torch.isfinite(lse[:, :, :128]).all() and torch.isfinite(lse[:, :, 256:]).all()

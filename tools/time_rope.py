#!/usr/bin/env python3
"""Time the RoPE-fused quant pre-pass and step (include/qattn_rope.h) against what they replace, in the same process.
Times are HIP events around blocks of `--iters` back-to-back calls, the candidates interleaved block by block over `--rounds` rounds
(>= 16), median over the rounds (clock and thermal drift hit all alike); min .. max over the rounds is printed as the spread.  Kernel
times come from a run of this script under `rocprofv3 --kernel-trace --stats` (rope_amax_kernel, rope_quant_kernel against
amax_multi_kernel, quant_multi_kernel).

  prepass   through the C entries on preallocated buffers (no allocation inside the timed window):
              plain        qattn_quant_qkv_fp8(q, k, v)                                   -- what a caller of rotated tensors pays today
              rope         qattn_rope_quant_qk_fp8(q, k, tables) + qattn_quant_fp8(v)      -- the same HBM bytes plus the tables
            for interleaved off and on; the plain pass is listed twice (plain, plain_again) so that its own run-to-run spread shows.
  step      fp8_attn_rope_func(q, k, v, cos, sin) against the composition it equals bit for bit: apply_rope_eager on the device, then
            _native.quant_qkv_fp8 + _native.fp8_attention_forward; and (reported whatever it shows) fp8_attn_func on rotated tensors with the
            rotation excluded (`fused_step_on_rotated`) and, with --compiled-rotation, included as one torch.compile'd kernel per tensor.
Shapes: bench.py's C2 (B4 H32 S4096 D128 bf16) and Wan's (B1 H40 S32760 D128).  Prints one JSON line per case."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import quantumattention_amd as qa  # noqa: E402
from quantumattention_amd import _native  # noqa: E402

CASES = {"c2": (4, 32, 4096, 128), "wan": (1, 40, 32760, 128)}


def block_ms(fns, iters, rounds, warmup=3):
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    laps = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            laps[i].append((e0, e1))
    torch.cuda.synchronize()
    times = [sorted(a.elapsed_time(b) / iters for a, b in lap) for lap in laps]
    return [{"median_ms": t[rounds // 2], "min_ms": t[0], "max_ms": t[-1]} for t in times]


def tables(T, half, device):
    inv = 10000.0 ** (-torch.arange(half, dtype=torch.float64) / half)
    ang = torch.arange(T, dtype=torch.float64)[:, None] * inv
    return torch.cos(ang).to(torch.float32).to(device), torch.sin(ang).to(torch.float32).to(device)


def prepass_fns(q, k, v, cos, sin):
    """closures over preallocated buffers: (plain, rope interleaved=0, rope interleaved=1)"""
    L = _native.lib()
    B, H, S, D = q.shape
    dev = q.device
    e = lambda *shape, dtype=torch.uint8: torch.empty(shape, dtype=dtype, device=dev)
    q8, kf, vf = e(B, H, S, D), e(L.qattn_fp8_tensor_bytes(_native.LAYOUT_KFRAG, B, H, S, D)), e(L.qattn_fp8_tensor_bytes(_native.LAYOUT_VFRAG, B, H, S, D))
    sq, sk, sv = (e(B, H, dtype=torch.float32) for _ in range(3))
    wb_plain, wb_rope, wb_v = L.qattn_quant_qkv_workspace_bytes(B, H, H), L.qattn_rope_quant_qk_workspace_bytes(B, H, H), L.qattn_quant_workspace_bytes(B, H, S, D, 0)
    ws_plain, ws_rope, ws_v = e(wb_plain), e(wb_rope), e(wb_v)
    st = torch.cuda.current_stream().cuda_stream
    f16, f8 = _native.fmt_of(q.dtype), _native.FMT_E4M3

    def plain():
        rc = L.qattn_quant_qkv_fp8(q.data_ptr(), k.data_ptr(), v.data_ptr(), f16, q8.data_ptr(), kf.data_ptr(), vf.data_ptr(), sq.data_ptr(),
                                   sk.data_ptr(), sv.data_ptr(), B, H, H, S, S, D, f8, 0, 0, ws_plain.data_ptr(), wb_plain, st)
        assert rc == 0, rc

    def rope(il):
        def f():
            rc = L.qattn_rope_quant_qk_fp8(q.data_ptr(), k.data_ptr(), None, f16, cos.data_ptr(), sin.data_ptr(), 0, D // 2, cos.data_ptr(),
                                           sin.data_ptr(), 0, D // 2, il, q8.data_ptr(), kf.data_ptr(), _native.LAYOUT_KFRAG, sq.data_ptr(),
                                           sk.data_ptr(), B, H, H, S, S, D, f8, 0, 0, ws_rope.data_ptr(), wb_rope, st)
            assert rc == 0, rc
            rc = L.qattn_quant_fp8(v.data_ptr(), f16, vf.data_ptr(), sv.data_ptr(), B, H, S, D, f8, 0, 0, _native.LAYOUT_VFRAG, ws_v.data_ptr(), wb_v, st)
            assert rc == 0, rc
        return f

    return plain, rope(0), rope(1)


def run_case(name, iters, rounds, compiled_rotation, prepass_only=False):
    B, H, S, D = CASES[name]
    torch.manual_seed(0)
    q, k, v = (torch.randn(B, H, S, D, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    cos, sin = tables(S, D // 2, q.device)
    res = {"case": name, "B": B, "H": H, "S": S, "D": D, "dtype": "bf16", "iters": iters, "rounds": rounds}
    # bytes the pre-pass has to move: two reads of q, k, v in 16 bit, one write in 8 bit; the tables once per batch element if they stay on-die
    res["prepass_hbm_mbytes"] = 3 * B * H * S * D * (2 + 2 + 1) / 1e6
    res["table_mbytes_once_per_batch"] = 2 * B * S * (D // 2) * 4 * 2 / 1e6    # cos + sin, for q and for k, read by both passes
    plain, rope0, rope1 = prepass_fns(q, k, v, cos, sin)
    t = block_ms([plain, rope0, rope1, plain], iters, rounds)
    res["prepass"] = dict(zip(("plain", "rope", "rope_interleaved", "plain_again"), t))
    res["prepass"]["rope_over_plain"] = t[1]["median_ms"] / t[0]["median_ms"]
    res["prepass"]["rope_interleaved_over_plain"] = t[2]["median_ms"] / t[0]["median_ms"]
    res["prepass"]["plain_spread_pct"] = (t[0]["max_ms"] / t[0]["min_ms"] - 1.0) * 100.0
    res["prepass"]["plain_again_over_plain"] = t[3]["median_ms"] / t[0]["median_ms"]
    if prepass_only:
        return res

    def composition(il):
        def f():
            qr, kr = qa.apply_rope_eager(q, cos, sin, interleaved=il), qa.apply_rope_eager(k, cos, sin, interleaved=il)
            q8, kf, vf, sq, sk, sv = _native.quant_qkv_fp8(qr, kr, v)
            return _native.fp8_attention_forward(q8, kf, vf, sq, sk, sv, Hkv=H, Skv=S, out_dtype=q.dtype, is_causal=False)
        return f

    qr, kr = qa.apply_rope_eager(q, cos, sin), qa.apply_rope_eager(k, cos, sin)
    fns = {"rope_func": lambda: qa.fp8_attn_rope_func(q, k, v, cos, sin), "composition": composition(False),
           "rope_func_interleaved": lambda: qa.fp8_attn_rope_func(q, k, v, cos, sin, interleaved=True), "composition_interleaved": composition(True),
           "fused_step_on_rotated": lambda: qa.fp8_attn_func(qr, kr, v)}
    assert torch.equal(fns["rope_func"](), fns["composition"]()) and torch.equal(fns["rope_func_interleaved"](), fns["composition_interleaved"]())
    if compiled_rotation:
        try:
            from quantumattention_amd.rope import _rotate
            rot = torch.compile(lambda x: _rotate(x, cos, sin, False))
            same = torch.equal(rot(q), qr)
            fns["compiled_rotation_plus_fused_step"] = lambda: qa.fp8_attn_func(rot(q), rot(k), v)
            res["compiled_rotation"] = {"compiled": True, "bit_equal_to_eager": bool(same)}
        except Exception as ex:   # no Inductor backend on the box: say so
            res["compiled_rotation"] = {"compiled": False, "error": f"{type(ex).__name__}: {str(ex)[:200]}"}
    t = block_ms(list(fns.values()), iters, rounds)
    res["step"] = dict(zip(fns, t))
    res["step"]["rope_func_over_composition"] = res["step"]["rope_func"]["median_ms"] / res["step"]["composition"]["median_ms"]
    res["step"]["rope_func_interleaved_over_composition"] = (res["step"]["rope_func_interleaved"]["median_ms"]
                                                             / res["step"]["composition_interleaved"]["median_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,wan")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--compiled-rotation", action="store_true", help="also time torch.compile of the eager rotation + fp8_attn_func")
    ap.add_argument("--prepass-only", action="store_true", help="the pre-pass launches alone (for a counter pass: rocprofv3 --pmc FETCH_SIZE)")
    args = ap.parse_args()
    assert args.rounds >= 1 and args.iters >= 1
    assert _native.lib().qattn_check_device() == 0, "needs the MI355X"
    for c in args.cases.split(","):
        print(json.dumps(run_case(c, args.iters, args.rounds, args.compiled_rotation, args.prepass_only)), flush=True)


if __name__ == "__main__":
    main()

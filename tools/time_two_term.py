"""Two-term P (hi + lo e4m3) of one build: launch times of the paths that run it, and their error against the fp64 oracle in units of
the bound.  QUANTUM_ATTN_LIBRARY selects the build, so two builds are compared by running this twice (profiles/vwitness/two_term_ab.log).
  time  : separate calls (quantise once, attend) fast / auto / accurate -- accurate is the two-term sweep on every row; the fused entry
          on q x 3 (every row peaked: AUTO repeats blocks in two-term mode or rescues rows) and on 3 % scattered sharp rows (rescue_pass)
  error : worst |got - ref| / bound (tests/gpu_utils.py::grade) on the peaked cases of tests/test_gpu_precision.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import oracle
from quantumattention_amd import _native
from tests.gpu_utils import bits16, fused_call, fused_step_uses_block_v, grade, oracle_for_fp8_path, out_to_f32


def timeit(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): fn()
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / n)
    return best


def inputs(H, S, D, sharp, seed):
    torch.manual_seed(seed)
    q = torch.randn(1, H, S, D)
    if sharp == "mixed": q = q * torch.linspace(0.5, 6.0, S)[torch.randperm(S)].view(1, 1, S, 1)
    elif sharp == "scattered": q[:, :, torch.randperm(S)[: S * 3 // 100]] *= 4.0
    else: q = q * float(sharp)
    return tuple(t.to(torch.bfloat16) for t in (q, torch.randn(1, H, S, D), torch.randn(1, H, S, D)))


print(f"library {_native.LIB_PATH}", flush=True)
if "time" in sys.argv[1:] or len(sys.argv) == 1:
    for D in (128, 64, 256):
        B, H, S = 4, 32, 4096
        torch.manual_seed(0)
        q, k, v = (torch.randn(B, H, S, D, dtype=torch.bfloat16, device="cuda") for _ in range(3))
        q8, kf, vf, sq, sk, sv = _native.quant_qkv_fp8(q, k, v)
        for causal in (False, True):
            row = [f"{prec} {timeit(lambda: _native.fp8_attention_forward(q8, kf, vf, sq, sk, sv, Hkv=H, Skv=S, out_dtype=torch.bfloat16, is_causal=causal, precision=prec)):.4f} ms"
                   for prec in ("fast", "auto", "accurate")]
            print(f"separate B{B} H{H} S{S} D{D} {'causal' if causal else 'full  '}: " + " | ".join(row), flush=True)
    for D, sharp in ((128, 3.0), (128, "scattered"), (64, 3.0), (64, "scattered")):
        q, k, v = (t.expand(4, -1, -1, -1).contiguous().cuda() for t in inputs(32, 4096, D, sharp, 1))
        row = [f"{prec} {timeit(lambda: _native.fp8_quant_attention_forward(q, k, v, is_causal=False, precision=prec)):.4f} ms" for prec in ("fast", "auto", "accurate")]
        print(f"fused    B4 H32 S4096 D{D} q {sharp}: " + " | ".join(row), flush=True)

if "error" in sys.argv[1:] or len(sys.argv) == 1:
    for S, D, sharp, causal in ((4096, 128, 3.0, False), (2048, 128, "mixed", True), (2048, 64, 3.0, False), (2048, 64, "mixed", True), (2048, 256, 3.0, True), (2048, 256, "mixed", False)):
        q, k, v = inputs(2, S, D, sharp, S + D)
        q8, sq = oracle.quantize_fp8(bits16(q), oracle.FMT_BF16, "head", oracle.FMT_E4M3)
        k8, sk = oracle.quantize_fp8(bits16(k), oracle.FMT_BF16, "head", oracle.FMT_E4M3)
        ref = oracle_for_fp8_path(q8, k8, bits16(v), sq, sk, causal=causal, fused=True, v_block=fused_step_uses_block_v(D, "head", q.dtype, S))
        ref_sep = oracle_for_fp8_path(q8, k8, bits16(v), sq, sk, causal=causal)
        row = []
        for prec in ("auto", "accurate"):
            got, path = fused_call(q, k, v, causal=causal, precision=prec)
            mx, rmse, worst = grade(got, ref, path)
            row.append(f"fused {prec} {worst:.3f} (rmse {rmse:.5f}, two-term rows {int((path == 1).sum())})")
        g8, gk, gv, gsq, gsk, gsv = _native.quant_qkv_fp8(q.cuda(), k.cuda(), v.cuda())
        got = out_to_f32(_native.fp8_attention_forward(g8, gk, gv, gsq, gsk, gsv, Hkv=2, Skv=S, out_dtype=torch.bfloat16, is_causal=causal, precision="accurate"))
        mx, rmse, worst = grade(got, ref_sep)
        row.append(f"separate accurate {worst:.3f} (rmse {rmse:.5f})")
        print(f"error / bound S{S} D{D} q {sharp} {'causal' if causal else 'full'}: " + " | ".join(row), flush=True)

"""What tests/test_cpu_mla_prefill.py and tests/test_gpu_mla_prefill.py share (include/qattn_mla_prefill.h): ONE packed call of seven
sequences and the plain fp64 reference -- softmax attention per (sequence, head) on the de-quantised operands the call returned (q8 x scale_q)
and on K / V quantised by the eager quantiser with the scales the call returned, as tests/mla_cases.py does for the decode entries.

(L_q, L_k): a one-key sequence; one key short of a chunk; one over a chunk with a row past a 128-row tile; L_q < L_k across three chunks and
two tiles; L_q > L_k (the first 40 rows have no key when causal); a sequence with no rows; a sequence with no keys."""
import math

import numpy as np
import torch

from quantumattention_amd import mla_prefill as P

LENS = ((1, 1), (63, 64), (129, 129), (130, 200), (70, 30), (0, 17), (5, 0))
HEADS = (1, 3)
SM_SCALE = 1.0 / math.sqrt(192.0)
PE_PEAK = 20.0      # planted in k_pe of sequence 3: the largest |k| of that sequence lies in the shared rotary slice
TDT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def tables(lens=LENS):
    """(cu_seqlens_q, cu_seqlens_k) int32 [B + 1]"""
    cq, ck = np.cumsum([0] + [a for a, _ in lens]), np.cumsum([0] + [b for _, b in lens])
    return torch.tensor(cq, dtype=torch.int32), torch.tensor(ck, dtype=torch.int32)


def make_inputs(H, dtype, lens=LENS, seed=0, pad=0):
    """(q [tq, H, 192], kv [tk, H, 256] = k_nope | v, k_pe [tk, 64]) with `pad` more tokens behind the last sequence"""
    g = torch.Generator().manual_seed(seed)
    tq, tk = sum(a for a, _ in lens) + pad, sum(b for _, b in lens) + pad
    q = torch.randn((tq, H, P.D_QK), generator=g)
    kv = torch.randn((tk, H, P.D_NOPE + P.D_V), generator=g)
    k_pe = torch.randn((tk, P.D_ROPE), generator=g)
    if len(lens) > 3:
        k_pe[sum(b for _, b in lens[:3]) + 5, 7] = PE_PEAK
    return q.to(dtype), kv.to(dtype), k_pe.to(dtype)


def dequantised_kv(kv, k_pe, sk, sv, fmt, lens=LENS, used=None):
    """fp64 (K [tk, H, 192], V [tk, H, 128]): the eager quantiser's bytes under the RETURNED scales, de-quantised; rows no sequence uses: 0"""
    tk, H, _ = kv.shape
    kd, vd = np.zeros((tk, H, P.D_QK)), np.zeros((tk, H, P.D_V))
    k0 = 0
    for i, (_, lk) in enumerate(lens):
        n = lk if used is None else min(used[i], lk)
        rows = slice(k0, k0 + n)
        k = torch.cat([kv[rows, :, :P.D_NOPE], k_pe[rows, None, :].expand(n, H, P.D_ROPE)], dim=-1)
        kd[rows] = (P.quantize_kv_eager(k, sk[i][None, :, None], TDT[fmt]).double() * sk[i].double()[None, :, None]).numpy()
        vd[rows] = (P.quantize_kv_eager(kv[rows, :, P.D_NOPE:], sv[i][None, :, None], TDT[fmt]).double() * sv[i].double()[None, :, None]).numpy()
        k0 += lk
    return kd, vd


def reference(qd, kd, vd, causal, lens=LENS, used=None, scale=SM_SCALE):
    """fp64 (out [tq, H, 128], lse [H, tq]); a row without a key is a zero row with lse -inf; causal is bottom-right"""
    qd = np.asarray(qd, np.float64)
    out, lse = np.zeros(qd.shape[:2] + (P.D_V,)), np.full((qd.shape[1], qd.shape[0]), -np.inf)
    q0 = k0 = 0
    for i, (lq, lk) in enumerate(lens):
        L = lk if used is None else min(used[i], lk)
        for r in range(lq):
            n = min(L, r + 1 + L - lq) if causal else L
            if n > 0:
                s = np.einsum("hd,khd->hk", qd[q0 + r], kd[k0:k0 + n]) * scale
                m = s.max(axis=-1, keepdims=True)
                p = np.exp(s - m)
                den = p.sum(axis=-1, keepdims=True)
                out[q0 + r] = np.einsum("hk,khd->hd", p / den, vd[k0:k0 + n])
                lse[:, q0 + r] = (m + np.log(den))[:, 0]
        q0, k0 = q0 + lq, k0 + lk
    return out, lse

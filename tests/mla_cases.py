"""What tests/test_cpu_mla.py and tests/test_gpu_mla.py share (include/qattn_mla.h): small problems whose inputs are EXACT in both fp8 formats,
so that the fp64 oracle needs no quantiser, and the oracle itself -- plain softmax attention with values = channels 0..511 of the latent.

q and the latent are drawn from a grid of values with two mantissa bits; the latent is grid x SCALE_KV (a power of two), q is the grid itself with
channel 0 of every row set to +-3.5 = 448 x 2^-7, so that the kernel's token-wise scale is exactly 2^-7 and q8 = q x 2^7 without rounding."""
import math

import numpy as np
import torch

D, DV = 576, 512
B = 4
LENS = ((0, 1, 63, 200), (64, 65, 200, 1))      # one batch of four slots each: empty, one key, around a chunk boundary, several chunks
SHAPES = ((16, 1), (16, 4), (20, 3), (128, 1))   # (Hq, Sq): one full tile / 4 padding rows / a tile that crosses head boundaries / two tiles
PAGES = (64, 128)
SPLITS = (1, 2, 3, 0)
CAP = 256                                        # keys a slot can hold
SCALE_KV, SCALE_Q = 2.0 ** -2, 2.0 ** -7
SM_SCALE = 1.0 / math.sqrt(192.0)                # DeepSeek's: the 128 + 64 channels of the non-absorbed head
LSE_TOL = 2e-3                                   # the FP8-P.V siblings' (tests/splitkv_window_cases.py)
GRID = torch.tensor([0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0])


def draw(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return GRID[torch.randint(0, len(GRID), shape, generator=g)]


def make_q(Hq, Sq, dtype, seed=0):
    q = draw((B, Hq, Sq, D), seed)
    sign = torch.where(draw((B, Hq, Sq), seed + 1) < 0, -1.0, 1.0)
    q[..., 0] = 3.5 * sign
    return q.to(dtype)   # amax 3.5 -> scale_q = 3.5 / 448 = 2^-7, and q x 2^7 is in e4m3


def make_latent(dtype, seed=100):
    """[B, CAP, 576] in dtype: grid x SCALE_KV"""
    return (draw((B, CAP, D), seed) * SCALE_KV).to(dtype)


def make_table(page_size, seed=7):
    """a shuffled table [B, M] over num_pages = B M + 3 pages; returns (table int32, num_pages)"""
    M = CAP // page_size
    num_pages = B * M + 3
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(num_pages, generator=g)[: B * M].reshape(B, M).to(torch.int32), num_pages


def reference(qd, lat, lens, scale, causal):
    """fp64: qd [B, Hq, Sq, 576], lat [B, >= L, 576] de-quantised -> (out [B, Hq, Sq, 512], lse [B, Hq, Sq]); a row without a key is a zero
    row with lse -inf; causal is bottom-right over Sq"""
    qd, lat = np.asarray(qd, np.float64), np.asarray(lat, np.float64)
    Bn, Hq, Sq, _ = qd.shape
    out, lse = np.zeros((Bn, Hq, Sq, DV)), np.full((Bn, Hq, Sq), -np.inf)
    for b, L in enumerate(lens):
        for i in range(Sq):
            n = min(L, L - Sq + i + 1) if causal else L
            if n <= 0:
                continue
            s = qd[b, :, i] @ lat[b, :n].T * scale                     # [Hq, n]
            m = s.max(axis=-1, keepdims=True)
            p = np.exp(s - m)
            den = p.sum(axis=-1, keepdims=True)
            out[b, :, i] = (p / den) @ lat[b, :n, :DV]
            lse[b, :, i] = (m + np.log(den))[:, 0]
    return out, lse

#!/usr/bin/env python3
"""The floor of the two-term fp8 P on a constant V ("V-format witness"): not a kernel run but the arithmetic of hi + lo e4m3 P
(RNE, subnormals down to 2^-9) normalised by the fp32 sum of the un-rounded weights, on one mixed case of tests/test_gpu_vwitness.py
(S 2304 causal, D 64, token-wise fp16).  With lo = e4m3(p' - hi), weights p' < 2^-10 vanish from hi and lo alike and a constant V comes
out as v sum(hi + lo) / l: the severe rows that keep 1 % of their mass on such keys are 0.0208 low at |v| = 1.75, beyond 2^-6 (the
MI355X returned 0.0205 on those rows).  With lo = e4m3((p' - hi) 2^5) 2^-5, the kernels' low term (csrc/qattn_attn.h, lo_terms), the
floor is 2^-15.  The row's top key is placed at 2^5 (the reference), at 2^8 (the most the deferred rescale lets it grow to) and at 2^2
(a running reference 3 binades above the true top: the wave rescales 32 rows together); |p' - hi| 2^5 <= 256 is checked on the way.

  python tools/models/sim_two_term_floor.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository root
import oracle  # noqa: E402
from tests import vwitness as W  # noqa: E402
from tests.vwitness import FMT, bits16, fmt16  # noqa: E402

HQ, HKV = 4, 2


def main():
    D, scaling, dtype, fp8 = 64, "token", torch.float16, "e4m3"
    S, causal = W.SHAPE_CAUSAL
    q, k = W.scores_case(S, D, "mixed", W.MIXED_SEED, causal)
    deq = []
    for t in (q, k):
        x8, s = oracle.quantize_fp8(bits16(t.to(dtype)), fmt16(dtype), scaling, FMT[fp8])
        deq.append(oracle.fp8_to_f32(x8, FMT[fp8]).astype(np.float64)[0] * s.astype(np.float64)[0][..., None])
    late = ~W.early_rows(S, S, causal)
    e4m3 = lambda x: oracle.fp8_to_f32(oracle.f32_to_fp8(x.astype(np.float32), oracle.FMT_E4M3), oracle.FMT_E4M3).astype(np.float64)
    low = {(top, gain): [] for top in (4.0, 32.0, 256.0) for gain in (1.0, 32.0)}
    for h in range(HQ):
        sc = deq[0][h] @ deq[1][h // (HQ // HKV)].T / np.sqrt(D)
        sc = np.where(np.arange(S)[None, :] <= np.arange(S)[:, None], sc, -np.inf)
        for top, gain in low:
            p = top * np.exp(sc - sc.max(-1, keepdims=True))
            hi = e4m3(p)
            assert np.abs((p - hi) * gain).max() <= 256.0
            lo = e4m3((p - hi) * gain) / gain
            low[top, gain].append(W.TOP * (1.0 - (hi + lo).sum(-1) / p.sum(-1))[late])
    for (top, gain), v in low.items():
        v = np.stack(v)
        print(f"S {S} causal D {D} token-wise fp16, top key at {top:g}, low term x {gain:g}: {int((np.abs(v) >= W.TOL).sum())} rows outside the early "
              f"blocks come out >= 2^-6 off at |v| = 1.75, worst {np.abs(v).max():.5f}")


if __name__ == "__main__":
    main()

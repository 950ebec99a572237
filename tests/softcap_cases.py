"""What tests/test_cpu_softcap.py and the GPU tests of the soft-cap entries share (include/qattn_softcap.h), restated here and NOT imported
from the product: the problems -- tests/sinks_cases.py's geometry and exact-in-e4m3 inputs, with the odd query heads doubled so that the
two heads of a GQA tile quantise under DIFFERENT scale_q --, an fp64 oracle that applies the cap in fp64 on tests/splitkv_window_cases.py's
literal window rules, the cap ladder, the closed-form cap probe and the named mutants a test of the cap must expose.

Geometry (tests/sinks_cases.py): Hq 4, Hkv 2, four sequences of 65 / 300 / 1100 / 1280 keys, Sq 1 / 5 / 130, D 64 / 128 and one D 256 case
at Sq 5, page 128 behind a shuffled table, 1 / 2 / 9 splits.  Windows: causal, a 128-key causal window, everything.
The ladder: caps 0.5 / 2 / 50, each at scale = g / sqrt(D), g 1 / 4.  The even heads' scores have standard deviation g, the odd heads' 2 g:
at g = 4 scores of 20 and more meet every cap (cap 50 moves a score of 20 by 1.0); at g = 1 and cap 50 a score of 3 moves by 0.004 -- the
rung on which a kernel that ignores the cap is hardest to tell, which is why the teeth are taken over the ladder (test_cpu_softcap.py)."""
import math

import numpy as np
import torch

from tests import sinks_cases as S
from tests import splitkv_window_cases as W

B, HQ, HKV, CAP, PAGE, G, LENS = S.B, S.HQ, S.HKV, S.CAP, S.PAGE, S.G, S.LENS
SCALE_Q, SCALE_K, SCALE_V, E4M3 = S.SCALE_Q, S.SCALE_K, S.SCALE_V, S.E4M3
CASES = ((64, 1), (64, 5), (64, 130), (128, 1), (128, 5), (128, 130), (256, 5))     # (D, Sq)
SPLITS = S.SPLITS
WINDOWS = ((-1, 0), (127, 0), (-1, -1))
CAPS = (0.5, 2.0, 50.0)
GAINS = (1.0, 4.0)
LSE_TOL = W.LSE_TOL
TEETH = S.TEETH
HEAD_GAIN = (1.0, 2.0, 1.0, 2.0)      # q of the odd heads is doubled: scale_q of head h is SCALE_Q HEAD_GAIN[h]
MUTANTS = ("cap dropped", "cap applied after the mask", "cap applied to the unscaled scores", "x / cap forgotten",
           "cap taken in base-2 units", "another head's scale_q inside a GQA tile", "LSE returned for the uncapped scores")
bound = S.bound


class Problem(S.Problem):
    """tests/sinks_cases.Problem with q of the odd heads doubled (exact in bf16; the head-wise quantiser finds 2 SCALE_Q there) and the
    raw products q.k kept, so that every scale of the ladder reads the same inputs."""

    def __init__(self, D, Sq, seed=0):
        super().__init__(D, Sq, seed)
        gain = torch.tensor(HEAD_GAIN)[None, :, None, None]
        q = self.q.float() * gain
        self.q = q.bfloat16()
        assert torch.equal(self.q.float(), q)
        kx = self.k.double().numpy().repeat(G, axis=1)
        self.raw = np.matmul(self.q.double().numpy(), kx.transpose(0, 1, 3, 2))                           # [B, HQ, Sq, CAP], unscaled
        self.vx = self.v.double().numpy().repeat(G, axis=1)
        self.scores = None                                                                             # (the parent's: one fixed scale)
        self._ref = {}

    def scale(self, gain):
        return gain / math.sqrt(self.D)

    def reference(self, window, cap, gain, mutant=None):
        """(out [B, HQ, Sq, D], lse [B, HQ, Sq]) in fp64: y = cap tanh(x / cap) on x = scale q.k, THEN the window's mask; a row without a
        key is a zero row with lse -inf.  cap None: no cap (the window sibling).  mutant: one of MUTANTS."""
        key = (window, cap, gain, mutant)
        if key in self._ref:
            return self._ref[key]
        sm = self.scale(gain)
        x = self.raw * sm
        cap_ = math.inf if cap is None else float(cap)
        capf = (lambda z: z) if cap is None else (lambda z: cap_ * np.tanh(z / cap_))
        if mutant == "cap dropped":
            y = x
        elif mutant == "cap applied to the unscaled scores":       # kin without sm_scale
            y = capf(self.raw)
        elif mutant == "x / cap forgotten":
            y = cap_ * np.tanh(x)
        elif mutant == "cap taken in base-2 units":                 # P = 2^y where e^y is meant
            y = capf(x) * math.log(2.0)
        elif mutant == "another head's scale_q inside a GQA tile":  # the tanh's argument scaled by the OTHER head of the pair's scale_q
            other = np.array([HEAD_GAIN[h ^ 1] / HEAD_GAIN[h] for h in range(HQ)])[None, :, None, None]
            y = capf(x * other)
        else:
            assert mutant in (None, "cap applied after the mask", "LSE returned for the uncapped scores"), mutant
            y = capf(x)
        out = np.zeros((B, HQ, self.Sq, self.D))
        lse = np.full((B, HQ, self.Sq), -np.inf)
        for b, L in enumerate(LENS):
            keep = W.alive(self.Sq, L, window, CAP)                                                    # [Sq, CAP]
            sc = np.where(keep[None], y[b], -np.inf)
            if mutant == "cap applied after the mask":              # the masked keys of the sequence weigh exp(-cap), with their V
                sc = np.where(~keep[None] & (np.arange(CAP) < L)[None, None], -cap_, sc)
            mx = sc.max(-1)
            live = np.isfinite(mx)
            e = np.exp(sc - np.where(live, mx, 0.0)[..., None])
            tot = e.sum(-1)
            with np.errstate(divide="ignore"):
                lse[b] = np.where(live, mx + np.log(tot), -np.inf)
            out[b] = np.matmul(e / np.maximum(tot, 1e-300)[..., None], self.vx[b]) * live[..., None]
            if mutant == "LSE returned for the uncapped scores":
                su = np.where(keep[None], x[b], -np.inf)
                mu = su.max(-1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    lse[b] = np.where(live, mu + np.log(np.exp(su - np.where(live, mu, 0.0)[..., None]).sum(-1)), -np.inf)
        self._ref[key] = (out, lse)
        return out, lse

    def empty(self, window):
        return np.stack([~W.alive(self.Sq, L, window, CAP).any(-1) for L in LENS])[:, None, :].repeat(HQ, axis=1)     # [B, HQ, Sq]


def graded_heads(precision, cap, gain):
    """the query heads whose OUT the oracle test grades against the fp8-V bound.  ACCURATE: all, on every rung.  FAST: the sibling states
    its one-term sweep "for sm_scale^2 D <= 1" on unit-variance q and k (include/qattn_window.h) -- scores of standard deviation <= 1,
    which span about 4 between their -2 sigma and +2 sigma keys.  Capped scores lie in [-cap, cap]: at cap <= 2 they span at most 4 at
    any gain and on any head, inside that domain; at cap 50 the cap is all but off, and only the even heads (HEAD_GAIN 1) at g = 1 are
    inside it -- the odd heads stand at sm_scale^2 D = 4, g = 4 at 16 and 64.  (The LSE is an fp32 sum of exact exponentials under both
    precisions: graded everywhere.)"""
    if precision == "accurate" or cap <= 2.0:
        return list(range(HQ))
    return [h for h in range(HQ) if HEAD_GAIN[h] == 1.0] if gain == 1.0 else []


def teeth(prob, window, cap, gain, mutant):
    """how far the mutant moves the worst element, in units of its bound: out against `bound`, lse against LSE_TOL"""
    ro, rl = prob.reference(window, cap, gain)
    mo, ml = prob.reference(window, cap, gain, mutant)
    with np.errstate(invalid="ignore"):
        dl = np.where(rl == ml, 0.0, np.abs(rl - ml))
    return max(float((np.abs(mo - ro) / bound(ro)).max()), float(dl.max() / LSE_TOL))


# ---- the cap probe: a closed form -------------------------------------------------------------------------------------------------------------
# Per (sequence, kv head) every key is zero except key j* = L - Sq -- inside every row's window under each of WINDOWS while Sq <= 128 -- and V
# is zero except row j*.  q (every row of a head the same vector) holds 448 SCALE_Q HEAD_GAIN[h] in channel 0, which pins scale_q, and
# 256 SCALE_Q HEAD_GAIN[h] in channel 1; k[j*] holds 256 SCALE_K in channel 1 alone: the raw product is 2^16 2^-12 HEAD_GAIN[h] = 16 or 32,
# and under PROBE_SCALE = 0.5 the scaled score is X = 8 (even heads) or 16 (odd heads), exactly.  Every other attended key scores 0, and
# tanh(0) = 0 in any arithmetic.  So, with y = cap tanh(X / cap) and n the row's count of attended keys,
#     out = v* e^y / (e^y + n - 1),    lse = log(e^y + n - 1).
# At cap 2 and n = 65 the weight is 0.10; without the cap 0.98; with the cap after the mask a (127, 0) window at 1280 keys adds 1152
# keys of weight e^-2 to a denominator of 134 and loses more than half the weight.
# The bound, derived as DESIGN.md "Membership probes" derives the count probe's: V is zero off row j*, so an output element is
# v*[c] P'(j*) / l -- ONE product, no cancellation.  l is the fp32 sum of the unquantised exponentials (2^-22 n relative, n <= 1280:
# < 2^-11); the star key's logit carries the tanh error cap 2^-20 <= 2^-14 at cap <= 50; P'(j*) is rounded to e4m3 -- two-term, hi + lo:
# 2^-4 2^-4 = 2^-8 relative; one-term (precision FAST on a tile with >= 1024 keys): 2^-4 -- and out is rounded to bf16, 2^-9.  Hence
# |got - ref| <= REL |ref| with REL = 2^-7 (ACCURATE) and 2^-4 + 2^-7 (FAST), exactly 0 where ref is 0.
PROBE_SCALE = 0.5
PROBE_SQS = (1, 5)
PROBE_CAPS = (2.0, 50.0)
PROBE_REL = {"accurate": 2.0 ** -7, "fast": 2.0 ** -4 + 2.0 ** -7}


class Probe(S.Problem):
    def __init__(self, D, Sq):
        gen = torch.Generator().manual_seed(77 * D + Sq)
        self.D, self.Sq, self.const_v = D, Sq, False
        q = torch.zeros(B, HQ, Sq, D)
        q[..., 0] = 448.0 * SCALE_Q
        q[..., 1] = 256.0 * SCALE_Q
        q = q * torch.tensor(HEAD_GAIN)[None, :, None, None]
        k = torch.zeros(B, HKV, CAP, D)
        v = torch.zeros(B, HKV, CAP, D)
        self.star = [L - Sq for L in LENS]
        for b, j in enumerate(self.star):
            k[b, :, j, 1] = 256.0 * SCALE_K
            v[b, :, j] = torch.randint(1, 9, (HKV, D), generator=gen).float() * torch.where(torch.rand(HKV, D, generator=gen) < 0.5, -1.0, 1.0) * SCALE_V
        self.q, self.k, self.v = q.bfloat16(), k.bfloat16(), v.bfloat16()
        assert torch.equal(self.q.float(), q) and torch.equal(self.k.float(), k) and torch.equal(self.v.float(), v)
        self.X = np.array([8.0 * g for g in HEAD_GAIN])                                                  # the scaled score of j*, per head

    def counts(self, window):
        """n [B, Sq]: the keys each row attends (j* among them)"""
        n = np.stack([W.alive(self.Sq, L, window, CAP).sum(-1) for L in LENS])
        for b, L in enumerate(LENS):
            assert W.alive(self.Sq, L, window, CAP)[:, self.star[b]].all(), "the star key lies inside every row's window"
        return n

    def expected(self, window, cap, mutant=None):
        """(out [B, HQ, Sq, D], lse [B, HQ, Sq]) of the closed form; mutant: "cap dropped" or "cap applied after the mask" """
        n = self.counts(window)[:, None, :].astype(np.float64)                                          # [B, 1, Sq]
        X = self.X[None, :, None]
        y = X if (cap is None or mutant == "cap dropped") else cap * np.tanh(X / cap)
        den = np.exp(y) + n - 1.0
        if mutant == "cap applied after the mask":
            den = den + (np.array(LENS, np.float64)[:, None, None] - n) * math.exp(-cap)
        vstar = np.stack([self.v[b, :, j].double().numpy() for b, j in enumerate(self.star)]).repeat(G, axis=1)   # [B, HQ, D]
        return vstar[:, :, None, :] * (np.exp(y) / den)[..., None], np.log(den)


def probe_bound(ref, precision):
    return PROBE_REL[precision] * np.abs(ref)

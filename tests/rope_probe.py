"""The quarter-turn RoPE probe (tests/test_cpu_rope.py: closed form and teeth; tests/test_gpu_rope.py: the kernels).

The table row of position s is the turn by (s mod 4) quarter-turns: (cos, sin) in {(1, 0), (0, 1), (-1, 0), (0, -1)} for every pair.  A
rotated row is then a SIGNED PERMUTATION of the input row -- exact in any arithmetic, fused or not, so the expected answer does not
depend on the implementation under test:

    turn 0: (a, b)    turn 1: (-b, a)    turn 2: (-a, -b)    turn 3: (b, -a)

The attention problem is a pointer probe in the ROTATED frame: rotated key j is a random +-1 code row u[j], rotated query r is
gain * u[target(r)], values are rows over {-1, 0, 1}.  The caller's (unrotated) q and k are the inverse turns of those rows, so a kernel
that rotates with the wrong pairing convention, the wrong position or the wrong tensor's table loses the pointer: the target's score drops
from gain * sqrt(D) to about zero and the row's output moves from v[target] to a broad mixture.  Every value is one of 0, +-1, +-gain
(gain = 2): exactly representable in bf16, fp16, e4m3 and e5m2 under head-wise and token-wise scales, so one fp64 reference serves all.
Plain numpy: nothing here knows about the device."""
import math

import numpy as np
import torch

GAIN = 2.0
TOL, TOL_V16 = 2.0 ** -6, 2.0 ** -7    # the project's bounds on |out - ref| (fp8 V / 16-bit V), as tests/probes.py
TEETH = 4.0


def quarter_tables(T, half, offset=0):
    """(cos, sin) fp32 torch [T, half]: row s turns by ((s + offset) mod 4) quarter-turns."""
    turn = (np.arange(T) + offset) % 4
    c = np.array([1.0, 0.0, -1.0, 0.0], np.float32)[turn]
    s = np.array([0.0, 1.0, 0.0, -1.0], np.float32)[turn]
    rep = lambda a: torch.from_numpy(np.repeat(a[:, None], half, axis=1).copy())
    return rep(c), rep(s)


def turn_rows(x, turns, interleaved, inverse=False):
    """x [..., S, D] (numpy) with row s turned by turns[s] quarter-turns (inverse: turned back) -- the exact signed permutation."""
    x = np.asarray(x, np.float64)
    S, D = x.shape[-2], x.shape[-1]
    h = D // 2
    t = (np.asarray(turns) % 4)
    if inverse:
        t = (4 - t) % 4
    a, b = (x[..., 0::2], x[..., 1::2]) if interleaved else (x[..., :h], x[..., h:])
    t = t.reshape((1,) * (x.ndim - 2) + (S, 1))
    y0 = np.where(t == 0, a, np.where(t == 1, -b, np.where(t == 2, -a, b)))
    y1 = np.where(t == 0, b, np.where(t == 1, a, np.where(t == 2, -b, -a)))
    if interleaved:
        return np.stack((y0, y1), axis=-1).reshape(x.shape)
    return np.concatenate((y0, y1), axis=-1)


def sdpa64(q, k, v, causal=False):
    """fp64 attention with grouped kv heads: q [B,Hq,Sq,D], k / v [B,Hkv,Skv,D] -> (out, natural lse)."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    rep = q.shape[1] // k.shape[1]
    k, v = np.repeat(k, rep, axis=1), np.repeat(v, rep, axis=1)
    s = q @ np.swapaxes(k, -1, -2) / math.sqrt(q.shape[-1])
    if causal:
        i, j = np.arange(s.shape[-2])[:, None], np.arange(s.shape[-1])[None, :]
        s = np.where(j > i, -np.inf, s)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    return (e / l) @ v, (m + np.log(l))[..., 0]


class Probe:
    """One pointer probe.  q, k, v: what the caller passes (unrotated q and k); q_rot, k_rot: the exact rotated tensors; turns_q / turns_k:
    each row's quarter-turns (k's positions start at k_offset); ref / ref_lse: fp64 attention on the rotated tensors."""

    def __init__(self, B, Hq, Hkv, Sq, Skv, D, interleaved, k_offset=0, causal=False, seed=0):
        rng = np.random.default_rng(7919 * seed + 31 * D + Sq + 1000 * Skv + int(interleaved))
        u = rng.integers(0, 2, (B, Hkv, Skv, D)) * 2.0 - 1.0
        w = rng.integers(-1, 2, (B, Hkv, Skv, D)).astype(np.float64)
        w[..., 0] = 1.0                                       # no value row is all zero
        # targets with an ODD turn (the two conventions agree on turns 0 and 2 -- identity and minus identity -- and differ on 1 and 3, so
        # under the wrong convention every even-turn row loses its pointer), allowed under a causal mask
        tgt = np.empty((B, Hq, Sq), np.int64)
        odd = np.nonzero((np.arange(Skv) + k_offset) % 2 == 1)[0]
        for r in range(Sq):
            pool = odd[odd <= r] if causal else odd
            tgt[:, :, r] = rng.choice(pool, size=(B, Hq)) if len(pool) else 0
        kvh = np.arange(Hq) // (Hq // Hkv)
        bi = np.arange(B)[:, None, None]
        self.q_rot = GAIN * u[bi, kvh[None, :, None], tgt]
        self.k_rot, self.v = u, w
        self.turns_q, self.turns_k = np.arange(Sq) % 4, (np.arange(Skv) + k_offset) % 4
        self.q = turn_rows(self.q_rot, self.turns_q, interleaved, inverse=True)
        self.k = turn_rows(self.k_rot, self.turns_k, interleaved, inverse=True)
        self.interleaved, self.k_offset, self.causal, self.target = interleaved, k_offset, causal, tgt
        self.ref, self.ref_lse = sdpa64(self.q_rot, self.k_rot, self.v, causal)
        T = max(Sq, Skv + k_offset) + 3
        self.cos, self.sin = quarter_tables(T, D // 2)

    def tensors(self, dtype, device="cpu"):
        return tuple(torch.from_numpy(t).to(dtype).to(device) for t in (self.q, self.k, self.v))

    def k_tables(self):
        """the slice of the tables that positions the keys (a view, no copy)"""
        n = self.k.shape[2]
        return self.cos[self.k_offset:self.k_offset + n], self.sin[self.k_offset:self.k_offset + n]

"""What tests/test_cpu_sinks.py and the GPU tests of the learned-sink entries share (include/qattn_sinks.h), restated here and NOT imported
from the product: the problems -- inputs every element of which is exact in its FP8 format, so that the de-quantised operands are known
without a quantiser --, an fp64 oracle with the sink column built on tests/splitkv_window_cases.py's literal window rules, the sink ladder,
the constant-V probe and the named mutants a test of the sink must expose.

Geometry: Hq 4, Hkv 2 (G = 2), four sequences of 65 / 300 / 1100 / 1280 keys in one batch (1100 reaches precision FAST's 1024 keys with
one split, 1280 is 10 key blocks), Sq 1 / 5 / 130 (a decode, a speculative step, a tile that crosses heads; 130 > 65: rows without a
key under every causal window)."""
import math

import numpy as np
import torch

import quantumattention_amd as qa
from tests import splitkv_window_cases as W

B, HQ, HKV, CAP, PAGE = 4, 4, 2, 1280, 128
G = HQ // HKV
LENS = (65, 300, 1100, 1280)
SQS = (1, 5, 130)
DS = (64, 128)
SPLITS = (1, 2, 9)                  # 9: the smallest count that reaches the chained merge
WINDOWS = ((-1, 0), (127, 0), (63, 0), (0, 0))
LADDER = (0.25, 1.0, 4.0, 16.0)     # exp(sink_h - lse_keys): the sink takes 1/5, 1/2, 4/5, 16/17 of the denominator
SCALE_Q, SCALE_K, SCALE_V = 2.0 ** -7, 2.0 ** -5, 2.0 ** -5
E4M3 = torch.float8_e4m3fn
LSE_TOL = W.LSE_TOL
TEETH = 4.0
MUTANTS = ("sink dropped", "sink read at the kv-head index", "sink read at b Hq + h", "sink multiplied by sm_scale",
           "sink taken as a base-2 logarithm", "sink added once per split", "sink added in every launch of the merge chain",
           "an empty row given lse = -inf")


def _exact(shape, gen, std, scale):
    """bf16 values x = e scale with e an e4m3 number: they quantise back to e under the power-of-two scale, whatever the rounding"""
    e = (torch.randn(*shape, generator=gen) * std).clamp(-448, 448).to(E4M3).float()
    return e * scale


class Problem:
    """q [B, HQ, Sq, D], k / v [B, HKV, CAP, D] bf16 on the CPU, exact in e4m3 under SCALE_Q / SCALE_K / SCALE_V.  Every (sequence, head)
    of q holds one element of magnitude 448 SCALE_Q, so the head-wise quantiser -- dense or per packed sequence -- finds SCALE_Q itself.
    q and k have unit variance: scores of variance sm_scale^2 D = 1, the domain precision FAST's one-term sweep is stated for
    (include/qattn_window.h).
    const_v: V equal along the key axis, the constant-V probe: out = v (1 - p_sink) whatever the weights of the keys are."""

    def __init__(self, D, Sq, seed=0, const_v=False):
        gen = torch.Generator().manual_seed(1000 * D + 10 * Sq + seed)
        self.D, self.Sq, self.const_v = D, Sq, const_v
        q = _exact((B, HQ, Sq, D), gen, 128.0, SCALE_Q)
        q[:, :, 0, 0] = 448.0 * SCALE_Q * torch.where(torch.rand(B, HQ, generator=gen) < 0.5, -1.0, 1.0)
        k = _exact((B, HKV, CAP, D), gen, 32.0, SCALE_K)
        if const_v:
            c = torch.randint(2, 9, (B, HKV, 1, D), generator=gen).float() * torch.where(torch.rand(B, HKV, 1, D, generator=gen) < 0.5, -1.0, 1.0)
            v = c.expand(B, HKV, CAP, D).contiguous()
        else:
            v = _exact((B, HKV, CAP, D), gen, 32.0, SCALE_V)
        self.q, self.k, self.v = q.bfloat16(), k.bfloat16(), v.bfloat16()
        assert torch.equal(self.q.float(), q) and torch.equal(self.k.float(), k) and torch.equal(self.v.float(), v)
        self.sm_scale = 1.0 / math.sqrt(D)
        kx = self.k.double().numpy().repeat(G, axis=1)
        self.scores = np.einsum("bhsd,bhkd->bhsk", self.q.double().numpy(), kx) * self.sm_scale      # [B, HQ, Sq, CAP]
        self._keys = {}

    # ---- the product's objects on a device
    def cache(self, device, dead=None, window=None):
        """(cache, table): the keys and values as e4m3 bytes in the pools of a paged cache behind a shuffled table, seqlens = LENS (fixed
        scales: every byte exact).  Keys at and beyond L_b hold zeros; dead = a byte: every key outside [lo_b, L_b) under `window` --
        below the first key any query attends, or behind the used ones -- holds that byte in K and V (0x7F: NaN)."""
        from quantumattention_amd import _native
        M = CAP // PAGE
        c = qa.alloc_paged_kv_cache_fp8(B * M + 1, HKV, PAGE, self.D, batch_size=B, max_pages_per_seq=M, scale_k=SCALE_K, scale_v=SCALE_V,
                                        dtype=torch.bfloat16, device=device, fp8_format="e4m3")
        table = np.random.RandomState(5).permutation(B * M).reshape(B, M) + 1
        pools = []
        for x, scale in ((self.k, SCALE_K), (self.v, SCALE_V)):
            x8 = (x.float() / scale).to(E4M3).view(torch.uint8).clone()                       # [B, HKV, CAP, D], exact
            for b, L in enumerate(LENS):
                x8[b, :, L:] = 0 if dead is None else dead
                if dead is not None:
                    x8[b, :, :W.interval_lo(L, self.Sq, window[0])] = dead
            rows = torch.zeros(B * M + 1, HKV, PAGE, self.D, dtype=torch.uint8)
            rows[torch.from_numpy(table).long().reshape(-1)] = x8.view(B, HKV, M, PAGE, self.D).permute(0, 2, 1, 3, 4).reshape(B * M, HKV, PAGE, self.D)
            pools.append(rows)
        if c.layout == "rowmajor":
            c.k.view(torch.uint8).copy_(pools[0])
            c.v.view(torch.uint8).copy_(pools[1])
        else:
            c.k.copy_(_native.pack_fp8(pools[0].to(device).view(E4M3), _native.LAYOUT_KFRAG))
            c.v.copy_(_native.pack_fp8(pools[1].to(device).view(E4M3), _native.LAYOUT_VFRAG))
        c.block_table.copy_(torch.tensor(table, dtype=torch.int32))
        c.seqlens.copy_(torch.tensor(LENS, dtype=torch.int32))
        return c, table

    def packed_q(self, device, sq=None):
        """q packed by token [total, HQ, D] with cu_seqlens_q; sq: queries per slot (default Sq each; 0: an idle slot)"""
        sq = [self.Sq] * B if sq is None else list(sq)
        rows = [self.q[b, :, :n].transpose(0, 1) for b, n in enumerate(sq)]
        cu = [0] + np.cumsum(sq).tolist()
        return torch.cat(rows).contiguous().to(device), torch.tensor(cu, dtype=torch.int32, device=device), cu

    # ---- the fp64 oracle
    def keys_state(self, window):
        """(out [B, HQ, Sq, D], lse [B, HQ, Sq]) of the keys alone: -inf and a zero row where the window holds no key"""
        if window not in self._keys:
            out = np.zeros((B, HQ, self.Sq, self.D))
            lse = np.full((B, HQ, self.Sq), -np.inf)
            vx = self.v.double().numpy().repeat(G, axis=1)
            for b, L in enumerate(LENS):
                keep = W.alive(self.Sq, L, window, CAP)                                                # [Sq, CAP]
                sc = np.where(keep[None], self.scores[b], -np.inf)
                mx = sc.max(-1)
                live = np.isfinite(mx)
                e = np.exp(sc - np.where(live, mx, 0.0)[..., None])
                tot = e.sum(-1)
                with np.errstate(divide="ignore"):
                    lse[b] = np.where(live, mx + np.log(tot), -np.inf)
                out[b] = np.einsum("hsk,hkd->hsd", e / np.maximum(tot, 1e-300)[..., None], vx[b]) * live[..., None]
            self._keys[window] = (out, lse)
        return self._keys[window]

    def ladder(self, window):
        """sink_h = lse_keys + log LADDER[h], lse_keys the median LSE of head h's rows that hold a key: fp32 [HQ]"""
        lse = self.keys_state(window)[1]
        return np.array([np.median(lse[:, h][np.isfinite(lse[:, h])]) + math.log(LADDER[h]) for h in range(HQ)], np.float32)

    def reference(self, window, sinks, ns=1, mutant=None):
        """(out, lse) with the sink column: L = logaddexp(lse_keys, sink_h), out = out_keys exp(lse_keys - L); a row without a key is a
        zero row with lse = sink_h.  mutant: one of MUTANTS -- a named way of getting the sink wrong, as a function of (b, h, ns)."""
        out_k, lse_k = self.keys_state(window)
        s = np.asarray(sinks, np.float64)
        eff = np.broadcast_to(s[None, :, None], lse_k.shape).copy()
        if mutant == "sink dropped":
            eff[:] = -np.inf
        elif mutant == "sink read at the kv-head index":
            eff[:] = s[np.arange(HQ) // G][None, :, None]
        elif mutant == "sink read at b Hq + h":          # (the floats behind the HQ sinks: zeros here)
            ext = np.concatenate([s, np.zeros(B * HQ)])
            eff[:] = ext[np.arange(B)[:, None] * HQ + np.arange(HQ)[None]][..., None]
        elif mutant == "sink multiplied by sm_scale":
            eff *= self.sm_scale
        elif mutant == "sink taken as a base-2 logarithm":
            eff *= math.log(2.0)
        elif mutant == "sink added once per split":
            for b, L in enumerate(LENS):
                eff[b] += math.log(max(sum(hi > lo for lo, hi in W.plan(L, self.Sq, window[0], ns)), 1))
        elif mutant == "sink added in every launch of the merge chain":
            eff += math.log(1 if ns <= 8 else 1 + -(-(ns - 8) // 7))
        else:
            assert mutant in (None, "an empty row given lse = -inf"), mutant
        with np.errstate(invalid="ignore"):
            lse = np.logaddexp(lse_k, eff)
            w = np.where(np.isneginf(lse_k), 0.0, np.exp(lse_k - lse))
        if mutant == "an empty row given lse = -inf":
            lse = np.where(np.isneginf(lse_k), -np.inf, lse)
        return out_k * w[..., None], lse


def bound(ref):
    """tests/gpu_utils.py's per-element bound of an fp8-V row: 2^-6 max(1, |ref| / 2)"""
    return 2.0 ** -6 * np.maximum(1.0, np.abs(ref) / 2.0)


def teeth(prob, window, sinks, ns, mutant):
    """how far the mutant moves the worst element, in units of its bound: out against `bound`, lse against LSE_TOL"""
    ro, rl = prob.reference(window, sinks, ns)
    mo, ml = prob.reference(window, sinks, ns, mutant)
    with np.errstate(invalid="ignore"):
        dl = np.where(rl == ml, 0.0, np.abs(rl - ml))
    return max(float((np.abs(mo - ro) / bound(ro)).max()), float(dl.max() / LSE_TOL))

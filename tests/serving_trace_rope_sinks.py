"""What tests/test_cpu_serving_trace_rope_sinks.py and tests/test_gpu_serving_trace_rope_sinks.py share: the serving traces of
tests/serving_trace.py (its schedules, seeds, flags, Shadow, state check and grading) driven through the step a gpt-oss layer is made of --

    q_rot = apply_rope_paged_varlen(q, cache, cu, cos, sin)                  rotate q at the cache's positions, BEFORE the append
    paged_kv_cache_append_varlen_rope_fp8(cache, k_new, v_new, cu, cos, sin)  the step's UNROTATED packed K, rotated inside the append
    fp8_attn_paged_varlen_sink_func(q_rot, cache, cu, max(T), sinks, window)  (-1, 0) on the causal traces, (left, 0) on the windowed ones

Plain numpy / torch-as-a-number-format; NO rule is imported from the product.

THE SHADOW'S ROTATION.  Key t of slot b's append has position lens0[b] + t.  The shadow rotates the step's 16-bit k_new in fp64 with the
fp32 tables' values -- pairs (i, i + D/2), or (2i, 2i + 1) when interleaved: y_a = a cos - b sin, y_b = b cos + a sin --, rounds ONCE to
the input dtype (`round_once`: torch's own fp64 -> 16-bit cast rounds twice) and quantises with kvcache_cases.quant_ref under the cache's
fixed scales, so saturation stays part of the model.  V is not rotated.

THE K RULE.  The product rotates in fp32; at ties the two roundings to 16 bits differ, and rarely that moves the fp8 byte by one code.  So
the K half of the state check (`k_rule`, given to serving_trace.state_failures) lets a live K byte differ from the shadow's by ONE CODE
(adjacent magnitude, same sign; +0 / -0 adjacent) and the differing bytes be at most K_SHARE_CAP = 2^-14 of a step's live K bytes.
Everything else of the state check is exact: V bytes, seqlens, the NaN of free / poison pages, the dead-page counts.

ROTATED q.  The attention reference de-quantises the call's own q8 * scale_q, so it cannot see a wrongly rotated q: q_rot is held to the
fp64 rotation by value, |q_rot - y| <= halfstep(y) + 2^-18 (|a| + |b|): the 16-bit type's half step AT y (2^-9 |y| < halfstep <= 2^-8 |y|
for bf16, 2^-12 |y| < halfstep <= 2^-11 |y| for fp16; the absolute half step for subnormal results) and the allowance
tests/test_cpu_paged_varlen_rope.py makes for the fp32 operations.  (A relative bound of 2^-9 |y| for bf16 is below the type's half step
at the bottom of a binade -- 1 + 2^-8 rounds to 1 or to 1 + 2^-7, off by 2^-8 --: the once-rounded fp64 rotation itself misses it, which
tests/test_cpu_serving_trace_rope_sinks.py shows.  halfstep(y) is the least bound a correctly rounded result meets.)

THE REFERENCE.  serving_trace.reference on the shadow's de-quantised keys, then the sink column as tests/sinks_cases.py states it:
L = logaddexp(lse_keys, sink_h), out = out_keys exp(lse_keys - L).  Graded by serving_trace.grade_step (gpu_utils.grade, LSE_TOL)
unchanged: the sink scales a row by at most 1 and logaddexp is 1-Lipschitz in the key LSE.  No row of a trace is without a key.
One code of a saturated e4m3 key is an eighth of its value; in a key a pointer row's whole weight rests on, that moves the row's LSE by
4 10^-3 (seen on the CPU, page 128, causal: one byte), twice LSE_TOL.  The attention check is about the attention of what the cache holds,
so the reference de-quantises `Shadow.held`: the fp64 rule's bytes, with each byte the cache holds ONE CODE beside them taken over from the
cache after the step's append (`Shadow.adopt`).  The state check keeps comparing against the fp64 rule's bytes themselves (`Shadow.k8`),
every live key in every step, so the 2^-14 cap counts a differing byte for as long as its key lives.  A byte further than one code away
is never taken over, and none is once a step's one-code bytes exceed the cap: the attention check cannot see a one-code K error in up to
2^-14 of the live bytes -- what the K rule admits -- and sees every other one.  The pointer rows are built from the fp64 rule's own keys
(`Shadow.kd_rule`), so a mutant run gets the queries of the clean run whose references it is graded against."""
import math

import numpy as np
import torch

from tests import kvcache_cases as KC
from tests import paged_cases as PC
from tests import serving_trace as ST

B, HKV, G, HQ, CAP = ST.B, ST.HKV, ST.G, ST.HQ, ST.CAP
# one logit per query head, pairwise distinct (half a ln 2 apart), fixed for every run: 4.61 .. 7.04.  The share condition of the CPU file
# (share > 0.1 on a quarter of a head's rows, < 0.9 on a quarter) holds iff Q25(lse_keys) - ln 9 <= sink_h <= Q75(lse_keys) + ln 9; over
# the nine traces the quartiles of the key LSE lie in 4.97 .. 6.20 and 6.13 .. 7.42 (pointer rows score about 6), so sink_h must lie in
# 4.0 .. 8.3.  (5 + ln 2 (-4 .. 3) = 2.2 .. 7.1 misses it: the two smallest sinks take a tenth of almost no row.)
SINKS = tuple(6.0 + 0.5 * math.log(2.0) * e for e in (-4, -2, 0, 2, 3, 1, -1, -3))
K_SHARE_CAP = 2.0 ** -14
SPLITS = 9                         # every fifth step's second call: the smallest count that reaches the chained merge
SIG_BITS = {torch.bfloat16: 8, torch.float16: 11}                 # significant bits, the hidden one included
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14}              # the exponent of the smallest normal number
FP32_OPS = 2.0 ** -18


def tables(D, rows=CAP, base=10000.0):
    """angle[p, i] = p base^(-i / (D/2)) in fp64; cos / sin cast to fp32 [rows, D/2]"""
    h = D // 2
    ang = np.arange(rows, dtype=np.float64)[:, None] * (base ** (-np.arange(h, dtype=np.float64) / h))[None]
    return torch.from_numpy(np.cos(ang)).to(torch.float32), torch.from_numpy(np.sin(ang)).to(torch.float32)


class Cfg(ST.Cfg):
    """serving_trace.Cfg and what the RoPE + sinks step adds: the pairing, the tables, the sinks as the call is given them"""

    def __init__(self, D, dtype, fmt, interleaved=False, sink_dtype=torch.float32, pointers=True, q_std=1.5):
        super().__init__(D, dtype, fmt, pointers, q_std)
        self.il = bool(interleaved)
        self.cos, self.sin = tables(D)
        self.sinks = torch.tensor(SINKS, dtype=torch.float64).to(sink_dtype)
        self.sinks64 = self.sinks.double().numpy()                                     # the values the kernel is given (16-bit sinks: rounded)


# ---- the shadow's rotation ----------------------------------------------------------------------------------------------------------------------
def rotate64(x, pos, cos, sin, il, inverse=False):
    """(y, |a| + |b|) fp64 numpy: x [n, H, D] (numpy or a torch tensor) rotated, row j at table row pos[j]; inverse: by the opposite angle"""
    x = x.double().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)
    h = x.shape[-1] // 2
    at = np.asarray(pos, np.int64)
    c, s = cos.double().numpy()[at][:, None], sin.double().numpy()[at][:, None]
    if inverse:
        s = -s
    y, mag = np.empty_like(x), np.empty_like(x)
    if il:
        a, b = x[..., 0::2], x[..., 1::2]
        y[..., 0::2], y[..., 1::2] = a * c - b * s, b * c + a * s
        mag[..., 0::2] = mag[..., 1::2] = np.abs(a) + np.abs(b)
    else:
        a, b = x[..., :h], x[..., h:]
        y[..., :h], y[..., h:] = a * c - b * s, b * c + a * s
        mag[..., :h] = mag[..., h:] = np.abs(a) + np.abs(b)
    return y, mag


def round_once(y, dtype):
    """fp64 numpy -> the nearest value of the 16-bit `dtype` (ties to even), as a torch tensor.  torch casts fp64 -> fp32 -> 16 bits, which
    can land one code beside the nearest; so: that cast, its two neighbours in the format, and whichever of the three is nearest in fp64
    (at an exact tie the cast is already right: a tie of the 16-bit format is an fp32 number)."""
    y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64))
    c = y.to(torch.float32).to(dtype)
    bits = c.view(torch.int16).to(torch.int32) & 0xFFFF
    sign, mag = bits & 0x8000, bits & 0x7FFF
    cands = []
    for m in (mag, mag + 1, (mag - 1).clamp_min(0)):
        v = sign | m
        cands.append(torch.where(v >= 0x8000, v - 0x10000, v).to(torch.int16).view(dtype))
    dist = torch.stack([(x.double() - y).abs().nan_to_num(nan=math.inf, posinf=math.inf) for x in cands])
    pick = dist.argmin(0)                                                             # (the first of equal distances: the cast)
    return torch.stack(cands).gather(0, pick[None])[0]


def halfstep(y, dtype):
    """half the distance between the two values of `dtype` around y (fp64 numpy): 2^(floor(log2 |y|) - p), the exponent not below the
    format's smallest normal one"""
    e = np.frexp(np.abs(y))[1] - 1
    return np.exp2(np.maximum(e, MIN_EXP[dtype]).astype(np.float64) - SIG_BITS[dtype])


def q_ratio(q_rot, want, dtype):
    """worst |q_rot - y| / (halfstep(y) + 2^-18 (|a| + |b|)) over a step's rows; q_rot fp64 numpy [total, HQ, D], want = (y, |a| + |b|)"""
    y, mag = want
    if not np.isfinite(q_rot).all():
        return math.inf
    return float((np.abs(q_rot - y) / (halfstep(y, dtype) + FP32_OPS * mag)).max()) if y.size else 0.0


# ---- the K rule ---------------------------------------------------------------------------------------------------------------------------------
def one_code(got, want, fmt):
    """bool, elementwise: the two fp8 bytes are equal or adjacent codes -- finite, same sign, magnitudes one apart; +0 and -0 are adjacent"""
    g, w = got.astype(np.int16), want.astype(np.int16)
    gm, wm = g & 0x7F, w & 0x7F
    top = 0x7E if fmt == "e4m3" else 0x7B                                             # the largest finite magnitude code
    near = ((g & 0x80) == (w & 0x80)) & (np.abs(gm - wm) == 1) & (gm <= top) & (wm <= top)
    return (g == w) | near | ((gm == 0) & (wm == 0))


def k_rule(fmt, seen=None):
    """the K half of serving_trace.state_failures on these traces (module docstring).  seen: a list that gets every step's
    (differing bytes, live bytes)"""
    def rule(got, want, spans):
        bad, diff, live = [], 0, 0
        for b, (lo, hi) in enumerate(spans):
            g, w = got[b][:, lo:hi], want[b][:, lo:hi]
            ok = one_code(g, w, fmt)
            if not ok.all():
                keys = np.nonzero((~ok).any((0, 2)))[0] + lo
                bad.append(f"K bytes of slot {b}: {len(keys)} live keys hold a byte more than one code from the shadow's, first {int(keys[0])}")
            diff += int((g != w).sum())
            live += g.size
        if seen is not None:
            seen.append((diff, live))
        if diff > K_SHARE_CAP * live:
            bad.append(f"K bytes: {diff} of {live} live bytes differ from the shadow's, share {diff / live:.2e} > 2^-14")
        return bad
    return rule


# ---- the data of a trace and the shadow's bytes -------------------------------------------------------------------------------------------------
class Shadow(ST.Shadow):
    """serving_trace.Shadow (k8: the fp64 rule's bytes, what the state check compares against) and `held`, what the reference
    de-quantises: k8 with the bytes the cache holds one code beside it (module docstring, THE REFERENCE)"""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.held = self.k8.copy()

    def write(self, b, at, k8, v8):
        super().write(b, at, k8, v8)
        self.held[b, :, at:at + k8.shape[1]] = k8

    def kd(self, b, lo, hi):
        return self._deq(self.held, self.cfg.scale_k, b, lo, hi)

    def kd_rule(self, b, lo, hi):
        """the fp64 rule's own keys, whatever the cache holds: what the pointer rows are built from, so that a clean run and a mutant run
        of one trace get the same queries"""
        return self._deq(self.k8, self.cfg.scale_k, b, lo, hi)

    def adopt(self, got, spans):
        """got: the cache's K bytes per slot [HKV, >= hi_b, D]; spans: the live keys (lo_b, hi_b) of every slot.  Returns the number of
        bytes taken over.  At most K_SHARE_CAP of the live bytes are ever taken over: beyond the cap (where the state check fails) none is,
        and the reference stays on the fp64 rule's bytes."""
        near, live = [], 0
        for b, (lo, hi) in enumerate(spans):
            g, w = got[b][:, lo:hi], self.k8[b][:, lo:hi]
            near.append((g != w) & one_code(g, w, self.cfg.fmt))
            live += g.size
        taken = sum(int(m.sum()) for m in near)
        if taken > K_SHARE_CAP * live:
            near, taken = [np.zeros_like(m) for m in near], 0
        for b, (lo, hi) in enumerate(spans):
            self.held[b][:, lo:hi] = np.where(near[b], got[b][:, lo:hi], self.k8[b][:, lo:hi])
        assert taken <= K_SHARE_CAP * live
        return taken


class StepData:
    """i, step, k_new / v_new [total, HKV, D] (packed as test_gpu_serving_trace_packed_append._packed packs them; K UNROTATED), q
    [total, HQ, D] unrotated, q_want = (y, |a| + |b|) of the fp64 rotation of q, saturated"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _packed(x, T):
    """[total, HKV, D] of a step's padded tokens x [B, HKV, Tmax, D]: slot b's first T_b rows, in slot order"""
    return torch.cat([x[b, :, :T[b]].transpose(0, 1) for b in range(B)])


def materialise(trace, cfg, shadow, k_shift=0):
    """serving_trace.materialise for the RoPE step, with its draws: the same k_new, v_new and q before any rotation.  The shadow gets the
    bytes of the ROTATED keys (module docstring), at positions lens0[b] + t (+ k_shift: the teeth of the K rule).  A pointer row is the
    INVERSE rotation, at the row's own position, of c k_j (k_j the shadow's de-quantised, rotated key): rotated by the product it points
    at key j as serving_trace's pointer rows do."""
    ps, left, D = trace.page_size, trace.left, cfg.D
    qmax_byte = KC.quant_ref(torch.full((1, 1, 1, 1), 1.0e9, dtype=cfg.dtype), torch.ones(1, 1), cfg.fp8).item()
    for i, st in enumerate(trace.steps):
        g = torch.Generator().manual_seed(100003 * trace.seed + 97 * i + D)
        Tmax = max(st.T)
        k_new = (torch.randn(B, HKV, Tmax, D, generator=g) * ST.K_STD).to(cfg.dtype)
        v_new = (torch.randn(B, HKV, Tmax, D, generator=g) * ST.V_STD).to(cfg.dtype)
        k_new, v_new = _packed(k_new, st.T), _packed(v_new, st.T)
        sat = 0
        for b in range(B):
            n, L0 = st.T[b], st.lens0[b]
            if n == 0:
                continue
            rows = slice(st.cu[b], st.cu[b + 1])
            y, _ = rotate64(k_new[rows], [min(L0 + t + k_shift, CAP - 1) for t in range(n)], cfg.cos, cfg.sin, cfg.il)
            k_rot = round_once(y, cfg.dtype).transpose(0, 1)[None]                     # [1, HKV, n, D]
            k8 = KC.quant_ref(k_rot, cfg.scale_k[b:b + 1], cfg.fp8).numpy()[0]
            v8 = KC.quant_ref(v_new[rows].transpose(0, 1)[None], cfg.scale_v[b:b + 1], cfg.fp8).numpy()[0]
            shadow.write(b, L0, k8, v8)
            sat += int(((k8 & 0x7F) == qmax_byte).sum())
        total = sum(st.T)
        q = torch.randn(total, HQ, D, generator=g) * cfg.q_std
        if cfg.pointers:
            rng = np.random.RandomState(31 * trace.seed + i)
            for b in range(B):
                n, L1, L0 = st.T[b], st.lens1[b], st.lens0[b]
                for p in range(0, n, 3):
                    hi = p + L1 - n                                                # the last key position p attends
                    lo = 0 if left is None else max(hi - left, 0)
                    cand = [j for j in (lo, hi, hi // ps * ps, hi // ps * ps - 1, hi // 64 * 64 - 1, L0, L0 - 1, st.evicted[b] * ps) if lo <= j <= hi]
                    j = int(rng.choice(cand))
                    kj = shadow.kd_rule(b, j, j + 1)[:, 0]                         # [HKV, D]
                    c = 6.0 * math.sqrt(D) / np.maximum((kj ** 2).sum(-1), 1e-6)
                    back, _ = rotate64(np.repeat(kj * c[:, None], G, 0)[None], [L0 + p], cfg.cos, cfg.sin, cfg.il, inverse=True)
                    q[st.cu[b] + p] = torch.from_numpy(back[0]).float()
        q = q.to(cfg.dtype)
        q_pos = [st.lens0[b] + t for b in range(B) for t in range(st.T[b])]
        yield StepData(i=i, step=st, k_new=k_new, v_new=v_new, q=q, q_want=rotate64(q, q_pos, cfg.cos, cfg.sin, cfg.il), saturated=sat)


# ---- the reference of a step ----------------------------------------------------------------------------------------------------------------------
def reference(shadow, st, qd, left, sinks64):
    """serving_trace.reference with the sink column: [(out [HQ, Sq_b, D], lse [HQ, Sq_b], lse_keys [HQ, Sq_b]) or None per slot]"""
    res = []
    for r in ST.reference(shadow, st, qd, left):
        if r is None:
            res.append(None)
            continue
        o, l = r
        assert np.isfinite(l).all(), "no row of a trace is without a key"
        L = np.logaddexp(l, sinks64[:, None])
        res.append((o * np.exp(l - L)[..., None], L, l))
    return res


class Result(ST.Result):
    def __init__(self):
        super().__init__()
        self.q_worst, self.k_seen, self.lse_keys = 0.0, [], []

    @property
    def k_share(self):
        """the largest share of differing bytes among a step's live K bytes, and the differing bytes of the last step"""
        return max((d / n for d, n in self.k_seen if n), default=0.0)

    def sink_shares(self, sinks64):
        """[HQ, rows of the whole trace]: 1 / (1 + exp(lse_keys - sink_h))"""
        return 1.0 / (1.0 + np.exp(np.concatenate(self.lse_keys, axis=1) - sinks64[:, None]))

    def __repr__(self):
        return (f"{super().__repr__()}, worst q error / bound {self.q_worst:.3f}, K bytes beside the shadow's: largest share {self.k_share:.2e} "
                f"({self.k_seen[-1][0] if self.k_seen else 0} of {self.k_seen[-1][1] if self.k_seen else 0} in the last step)")


def run(trace, cfg, ops, refs=None, steps=None, splits_every=5):
    """serving_trace.run for the RoPE + sinks step.  ops (duck-typed, see the two test files):
        start(trace, cfg), host(step), lens(), pool_rows(), dead_pages(left)      as serving_trace.run's
        step(sd) -> q_rot fp64 numpy [total, HQ, D]                               rotate q (before the append), then the fused append
        attend(sd, num_splits) -> out, lse, qd                                    the sink entry on the q_rot of step(sd)
    refs: the references of an earlier run of the same (trace, cfg), reused (the mutant runs).  Returns a Result; nothing is asserted here."""
    shadow = Shadow(cfg)
    res = Result()
    rule = k_rule(cfg.fmt, res.k_seen)
    ops.start(trace, cfg)
    for sd in materialise(trace, cfg, shadow):
        if steps is not None and sd.i >= steps:
            break
        st = sd.step
        ops.host(st)
        q_rot = ops.step(sd)
        res.q_worst = max(res.q_worst, q_ratio(q_rot, sd.q_want, cfg.dtype))
        shadow.adopt(PC.gather_rows(ops.pool_rows()[0], st.table, trace.page_size),
                     [(st.evicted[b] * trace.page_size, st.lens1[b]) for b in range(B)])
        out, lse, qd = ops.attend(sd, 0)
        ref = refs[sd.i] if refs is not None else reference(shadow, st, qd, trace.left, cfg.sinks64)
        res.refs.append(ref)
        res.lse_keys.append(np.concatenate([r[2] for r in ref if r is not None], axis=1))
        w, wl = ST.grade_step(st, out, lse, ref)
        if sd.i % splits_every == 0:
            out9, lse9, _ = ops.attend(sd, SPLITS)
            w9, wl9 = ST.grade_step(st, out9, lse9, ref)
            w, wl = max(w, w9), max(wl, wl9)
        res.worst, res.worst_lse = max(res.worst, w), max(res.worst_lse, wl)
        bad = ST.state_failures(trace, st, shadow, ops.lens(), ops.pool_rows(), None,
                                ops.dead_pages(trace.left) if trace.left is not None else None, k_rule=rule)
        res.state += [(sd.i, st.events, m) for m in bad]
        res.saturated += sd.saturated
        res.steps += 1
    return res


"""What tests/test_cpu_serving_trace.py and tests/test_gpu_serving_trace.py share: a SHADOW MODEL of a paged FP8 K/V cache that is driven
through a long mixed serving schedule, the seeded generator of such schedules with the coverage flags it computes from the schedule itself,
and the driver that runs one schedule through a set of entry points (`ops`, supplied by the test file: the eager definitions on the CPU,
the HIP entries on the device) and grades every step.

Plain numpy / Python / torch-as-a-number-format; NO rule is imported from the product.  The quantiser is kvcache_cases.quant_ref, the
key-level page lookup paged_cases.gather_rows, the references splitkv_cases.softmax64 and splitkv_window_cases.reference, the dead-page
count splitkv_window_cases.dead_pages, the bound gpu_utils.grade (2^-6 max(1, |ref| / 2)) and LSE_TOL.

The shadow NEVER reads the pool to learn what the pool should hold: it keeps, per slot, the bytes of every appended key (quantised under
the cache's fixed per-(slot, kv head) scales, so saturation is part of the model), the slot's length and page list, a LIFO free list (a
freed page is the next one handed out) and the block table it would write.  Every freed page is overwritten with NaN bytes before it can be
handed out again (the whole pool starts that way), and every table entry the contract calls unread points at POISON, an in-range page that
stays NaN: a kernel that reads one entry, one key or one page too far shows NaN, never a fault.  No out-of-range entry is ever written.

One STEP is: the host's edits (NaN fills, table, seqlens for rollback / finish), ONE padded append for all slots (new_lens), then one packed
attention call on the step's queries (Sq_b = T_b per slot), then the state check."""
import math

import numpy as np
import torch

from tests import kvcache_cases as KC
from tests import paged_cases as PC
from tests import splitkv_cases as S
from tests import splitkv_window_cases as W

B, HKV, G = 4, 2, 4
HQ = HKV * G
CAP = 1536                        # keys a slot can hold: max_pages_per_seq * page_size for every page size
MAX_LEN = 1500                    # a slot that would grow past this finishes instead
CHUNKS = (2, 7, 63, 64, 65, 130)  # prefill chunk sizes: appends begin and end on, before and after chunk and page edges
STEPS, TAIL = 40, 8               # the last TAIL steps are decode / idle only (the graph stretch replays them)
POISON = 2                        # the pool page that is never handed out and stays NaN
PAGE_SIZES = (64, 128, 256)
LEFTS = (63, 300)                 # the windowed traces' window_left (right = 0)
K_STD, V_STD = 1.0, 1.0
# what a value may reach before it saturates, in standard deviations, per (slot, kv head): 2.5 sigma saturates one value in 80
AMP = np.array([[2.5, 4.0], [3.0, 6.0], [4.0, 2.5], [6.0, 3.0]])
FLAGS = ("start_mid_chunk", "straddle_page", "fill_page_exactly", "rollback_over_page_edge", "reused_by_other_slot_partly",
         "idle_beside_128_rows", "idle_before_active", "empty_slot_with_neighbours", "cross_1024")
WINDOW_FLAGS = ("evict_reuse_append",)
# the seed of every (page size, window_left or None) the GPU file runs; chosen on the CPU so that every flag is set (test_cpu_serving_trace)
SEEDS = {(64, None): 1, (128, None): 1, (256, None): 1, (64, 63): 1, (128, 63): 3, (256, 63): 2, (64, 300): 1, (128, 300): 2, (256, 300): 4}
CONTIGUOUS_SEED = 1               # the contiguous-cache trace (page size 128 for its flags only: the cache has no pages)


def trace_of(page_size, left=None):
    return Trace(SEEDS[(page_size, left)], page_size, left)


class Step:
    __slots__ = ("events", "poison", "table", "lens0", "T", "lens1", "nan_pages", "evicted")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def cu(self):
        """cu_seqlens_q: every new token is a query, Sq_b = T_b"""
        return [0] + np.cumsum(self.T).tolist()


class Trace:
    """steps, flags and the pool geometry of one (seed, page size, window_left, paged) schedule"""

    def __init__(self, seed, page_size, left=None, paged=True, steps=STEPS):
        assert CAP % page_size == 0
        self.seed, self.page_size, self.left, self.paged = seed, page_size, left, paged
        self.M = CAP // page_size
        self.num_pages = B * self.M + 3
        self.steps = []
        self.flags = {f: False for f in FLAGS + (WINDOW_FLAGS if left is not None else ())}
        self._generate(steps)

    # -- the generator ---------------------------------------------------------------------------------------------------------------------
    def _generate(self, nsteps):
        ps, left, M = self.page_size, self.left, self.M
        rng = np.random.RandomState(7919 * self.seed + ps + (0 if left is None else 13 * left + 1))
        free = [p for p in range(self.num_pages - 1, -1, -1) if p != POISON]      # LIFO: pop() hands out page 0 first
        lens, pages, evicted = [0] * B, [[] for _ in range(B)], [0] * B
        last_owner, evicted_from = {}, {}
        evict_reused = [None] * B                                                   # the step in which a page the slot evicted was handed out again
        for s in range(nsteps):
            tail = s >= nsteps - TAIL
            events, poison, T, lens0 = [], [], [0] * B, [0] * B
            fresh = []                                                              # (slot, logical page) taken from another slot this step

            def release(b, idx):
                p = pages[b][idx]
                pages[b][idx] = None
                free.append(p)
                poison.append(p)
                last_owner[p] = b

            for b in range(B):
                L = lens[b]
                ev = self._draw(rng, s, b, L, tail, nsteps)
                dead = 0 if left is None else W.dead_pages(L, left, ps)
                if ev == "evict" and dead <= evicted[b]:
                    ev = "decode"
                if L == 0 and ev in ("decode", "rollback", "evict") and not tail:    # (in the tail an empty slot starts with one token)
                    ev = "chunk"
                t = 0
                if ev == "decode":
                    t = 1
                elif ev == "chunk":
                    t = int(rng.choice(CHUNKS))
                    if s < 10 and b == 0:
                        t = 130                                                     # slot 0 is in prefill: its length crosses 1024
                elif ev == "rollback":
                    # candidates: one token, a few, just over the last page edge, more than a page; never into an evicted page
                    floor = 0 if not evicted[b] else min(L, evicted[b] * ps + left + 1)
                    cand = [r for r in (1, 3, (L - 1) % ps + 2, ps + 3, 70) if 1 <= r <= L - floor]
                    if not cand:
                        ev, t = "decode", 1
                    else:
                        r = int(rng.choice(cand))
                        if (L - r) // ps < (L - 1) // ps:
                            self.flags["rollback_over_page_edge"] = True
                        L -= r
                        for idx in range(len(pages[b]) - 1, -(-L // ps) - 1, -1):   # the pages wholly behind the new length go back
                            release(b, idx)
                            pages[b].pop()
                        t = int(rng.choice(CHUNKS))
                        ev = f"rollback {r}"
                elif ev == "evict":
                    for idx in range(evicted[b], dead):
                        evicted_from[pages[b][idx]] = b
                        release(b, idx)
                    evicted[b] = dead
                    t = 1
                if not self.paged and t and L + t > MAX_LEN:
                    ev, t = "idle", 0                                               # a contiguous cache never finishes a sequence: it rests
                if ev.startswith("finish") or (t and L + t > MAX_LEN):
                    for idx in range(len(pages[b])):
                        if pages[b][idx] is not None:
                            release(b, idx)
                    pages[b], L, evicted[b], evict_reused[b] = [], 0, 0, None
                    t = 0 if ev == "finish idle" else (t or int(rng.choice(CHUNKS)))
                    ev = "finish idle" if t == 0 else "finish"
                lens0[b], T[b] = L, t
                # the pages that cover [L, L + t)
                for idx in range(len(pages[b]), -(-(L + t) // ps)):
                    p = free.pop()
                    pages[b].append(p)
                    if last_owner.get(p, b) != b:
                        fresh.append((b, idx))
                    if p in evicted_from:
                        evict_reused[evicted_from.pop(p)] = s
                events.append(ev)
                if t:
                    self.flags["start_mid_chunk"] |= L % 64 != 0
                    self.flags["straddle_page"] |= L % ps != 0 and L // ps != (L + t - 1) // ps
                    self.flags["fill_page_exactly"] |= (L + t) % ps == 0
                    self.flags["cross_1024"] |= L < 1024 <= L + t
                lens[b] = L + t
            if not any(T):                                                          # a step appends something: the entry needs T >= 1
                b = int(rng.randint(B))
                if lens[b] % ps == 0:
                    pages[b].append(free.pop())
                    evicted_from.pop(pages[b][-1], None)
                T[b], lens[b], events[b] = 1, lens[b] + 1, "decode"
            for b, idx in fresh:
                self.flags["reused_by_other_slot_partly"] |= lens[b] < (idx + 1) * ps
            idle = [t == 0 for t in T]
            self.flags["idle_beside_128_rows"] |= any(idle) and any(G * t >= 128 for t in T)
            self.flags["idle_before_active"] |= any(idle[b - 1] and T[b] for b in range(1, B))
            self.flags["empty_slot_with_neighbours"] |= any(idle[b] and lens[b] == 0 for b in range(B)) and any(T)
            if left is not None:
                # the evicting slot appends again in a LATER step than the one in which its page was handed out
                self.flags["evict_reuse_append"] |= any(evict_reused[b] is not None and evict_reused[b] < s and T[b] for b in range(B))
            table = np.full((B, M), POISON, np.int32)
            for b in range(B):
                for idx, p in enumerate(pages[b]):
                    if p is not None:
                        table[b, idx] = p
            assert len(set(free)) == len(free) and POISON not in free
            live = [p for b in range(B) for p in pages[b] if p is not None]
            assert len(set(live)) == len(live) and not set(live) & set(free), "a page has one owner"
            self.steps.append(Step(events=events, poison=list(poison), table=table, lens0=lens0, T=T, lens1=list(lens),
                                   nan_pages=sorted(set(free) | {POISON}), evicted=list(evicted)))

    def _draw(self, rng, s, b, L, tail, nsteps):
        if tail:
            return "decode" if rng.rand() < 0.8 else "idle"
        if s < 10 and b == 0:
            return "chunk"
        if s < 3 and b == 3:
            return "idle"                                                           # slot 3 starts late: a slot of length 0 beside queries
        if not self.paged:
            names, w = ("idle", "decode", "chunk", "rollback"), (0.15, 0.35, 0.3, 0.2)
        elif self.left is None:
            names, w = ("idle", "decode", "chunk", "rollback", "finish", "finish idle"), (0.14, 0.22, 0.36, 0.16, 0.07, 0.05)
        else:
            names, w = (("idle", "decode", "chunk", "rollback", "finish", "finish idle", "evict"), (0.12, 0.16, 0.34, 0.12, 0.06, 0.04, 0.16))
        return str(rng.choice(names, p=w))


# ---- the data of a trace and the shadow's bytes -----------------------------------------------------------------------------------------------
class Cfg:
    def __init__(self, D, dtype, fmt, pointers=True, q_std=1.5):
        self.D, self.dtype, self.fmt, self.pointers, self.q_std = D, dtype, fmt, pointers, q_std
        self.fp8 = KC.FP8[fmt]
        qmax = float(torch.finfo(self.fp8).max)
        self.scale_k = torch.tensor(AMP * K_STD / qmax, dtype=torch.float32)
        self.scale_v = torch.tensor(AMP[::-1].copy() * V_STD / qmax, dtype=torch.float32)


class StepData:
    __slots__ = ("i", "step", "k_new", "v_new", "q", "saturated")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


class Shadow:
    """the bytes every slot holds, as uint8 [HKV, CAP, D] per slot for K and V, and their fp64 values"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.k8 = np.zeros((B, HKV, CAP, cfg.D), np.uint8)
        self.v8 = np.zeros((B, HKV, CAP, cfg.D), np.uint8)

    def write(self, b, at, k8, v8):
        n = k8.shape[1]
        self.k8[b, :, at:at + n], self.v8[b, :, at:at + n] = k8, v8

    def _deq(self, bytes8, scale, b, lo, hi):
        x = torch.from_numpy(np.ascontiguousarray(bytes8[b, :, lo:hi])).view(self.cfg.fp8).to(torch.float64)
        return (x * scale[b].to(torch.float64)[:, None, None]).numpy()

    def kd(self, b, lo, hi):
        return self._deq(self.k8, self.cfg.scale_k, b, lo, hi)

    def vd(self, b, lo, hi):
        return self._deq(self.v8, self.cfg.scale_v, b, lo, hi)


def materialise(trace, cfg, shadow):
    """yields the StepData of every step, updating `shadow` as it goes: k_new / v_new [B, HKV, Tmax, D] (rows at and behind T_b hold a large
    finite value: written anywhere, they would saturate and show), q [total, HQ, D] in cfg.dtype (CPU tensors).  A third of the query rows
    POINT at one key (q = c k_j, a score of about 6 against about N(0, 0.3) for the others) -- the slot's first or last attended key, a key
    beside a page or chunk edge, the first key of this step's append or the key before it -- so that one wrong key moves an output."""
    ps, left, D = trace.page_size, trace.left, cfg.D
    for i, st in enumerate(trace.steps):
        g = torch.Generator().manual_seed(100003 * trace.seed + 97 * i + D)
        Tmax = max(st.T)
        k_new = (torch.randn(B, HKV, Tmax, D, generator=g) * K_STD).to(cfg.dtype)
        v_new = (torch.randn(B, HKV, Tmax, D, generator=g) * V_STD).to(cfg.dtype)
        for b in range(B):
            k_new[b, :, st.T[b]:] = 1.0e4
            v_new[b, :, st.T[b]:] = -1.0e4
        k8 = KC.quant_ref(k_new, cfg.scale_k, cfg.fp8).numpy()
        v8 = KC.quant_ref(v_new, cfg.scale_v, cfg.fp8).numpy()
        qmax_byte = KC.quant_ref(torch.full((1, 1, 1, 1), 1.0e9, dtype=cfg.dtype), torch.ones(1, 1), cfg.fp8).item()
        sat = 0
        for b in range(B):
            shadow.write(b, st.lens0[b], k8[b, :, :st.T[b]], v8[b, :, :st.T[b]])
            sat += int(((k8[b, :, :st.T[b]] & 0x7F) == qmax_byte).sum())
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
                    kj = shadow.kd(b, j, j + 1)[:, 0]                              # [HKV, D]
                    c = 6.0 * math.sqrt(D) / np.maximum((kj ** 2).sum(-1), 1e-6)
                    q[st.cu[b] + p] = torch.from_numpy(np.repeat(kj * c[:, None], G, 0)).float()
        yield StepData(i=i, step=st, k_new=k_new, v_new=v_new, q=q.to(cfg.dtype), saturated=sat)


# ---- the reference of a step and the state check ----------------------------------------------------------------------------------------------
def reference(shadow, st, qd, left):
    """[(out [HQ, Sq_b, D], lse [HQ, Sq_b]) or None per slot]: fp64 attention of the de-quantised queries qd [total, HQ, D] over the shadow's
    de-quantised keys of every slot, causal at the bottom right (window (left, 0) on a windowed trace)"""
    D = qd.shape[-1]
    sm = 1.0 / math.sqrt(D)
    res = []
    for b in range(B):
        n, L = st.T[b], st.lens1[b]
        if n == 0:
            res.append(None)
            continue
        q = np.ascontiguousarray(qd[st.cu[b]:st.cu[b + 1]].transpose(1, 0, 2))
        if left is None:
            o, l = S.softmax64(q[None], shadow.kd(b, 0, L)[None], shadow.vd(b, 0, L)[None], [L], True, sm)
            res.append((o[0], l[0]))
        else:
            # the keys below the window never enter: the evicted pages' keys are still in the shadow and still not attended
            res.append(W.reference(q, shadow.kd(b, 0, L), shadow.vd(b, 0, L), L, (left, 0), 1, sm)[:2])
    return res


def grade_step(st, out, lse, ref):
    """(worst |err| / bound over the step's rows, worst LSE error); NaN anywhere counts as infinite"""
    from tests import gpu_utils                                                     # (imports the product's binding: no device call)
    worst = worst_lse = 0.0
    for b in range(B):
        if ref[b] is None:
            continue
        o = np.asarray(out[st.cu[b]:st.cu[b + 1]], np.float64).transpose(1, 0, 2)
        l = np.asarray(lse[:, st.cu[b]:st.cu[b + 1]], np.float64)
        if np.isnan(o).any() or not np.isfinite(l).all():
            return math.inf, math.inf
        worst = max(worst, gpu_utils.grade(o, ref[b][0])[2])
        worst_lse = max(worst_lse, float(np.abs(l - ref[b][1]).max()))
    return worst, worst_lse


def state_failures(trace, st, shadow, lens, pool_rows, gathered=None, product_dead=None, k_rule=None):
    """what is wrong with the cache after a step, as a list of strings (empty: nothing).  lens: the cache's seqlens; pool_rows: (K, V)
    row-major uint8 numpy [P, HKV, page_size, D] of the pools, looked up key by key through the shadow's table (paged_cases.gather_rows) --
    or `gathered`, (K, V) [B, HKV, >= L, D], for the contiguous cache; product_dead: the product's dead-page counts on a windowed trace.
    k_rule (tests/serving_trace_rope_sinks.py): what the live K bytes are held to in place of equality, k_rule(got, want, [(lo_b, hi_b)])
    -> strings; V and everything else stay exact."""
    bad = []
    ps = trace.page_size
    if list(lens) != list(st.lens1):
        bad.append(f"seqlens {list(lens)} != {st.lens1}")
    nan = PC.NAN_BYTE[shadow.cfg.fmt]
    for name, want, rows in (("K", shadow.k8, 0), ("V", shadow.v8, 1)):
        got = gathered[rows] if gathered is not None else PC.gather_rows(pool_rows[rows], st.table, ps)
        spans = [(st.evicted[b] * ps, st.lens1[b]) for b in range(B)]
        if name == "K" and k_rule is not None:
            bad += k_rule(got, want, spans)
            spans = []
        for b, (lo, hi) in enumerate(spans):
            if not np.array_equal(got[b][:, lo:hi], want[b][:, lo:hi]):
                keys = np.nonzero((got[b][:, lo:hi] != want[b][:, lo:hi]).any((0, 2)))[0] + lo
                bad.append(f"{name} bytes of slot {b}: {len(keys)} live keys differ, first {int(keys[0])}")
        if gathered is None and not (pool_rows[rows][st.nan_pages] == nan).all():
            pages = [p for p in st.nan_pages if not (pool_rows[rows][p] == nan).all()]
            bad.append(f"{name}: free / poison pages {pages} are no longer all NaN")
    if product_dead is not None:
        want = [W.dead_pages(L, trace.left, ps) for L in st.lens1]
        if list(product_dead) != want:
            bad.append(f"dead pages {list(product_dead)} != {want}")
    return bad


class Result:
    def __init__(self):
        self.worst, self.worst_lse, self.state, self.refs, self.saturated, self.steps = 0.0, 0.0, [], [], 0, 0

    def __repr__(self):
        return f"worst |err| / bound {self.worst:.3f}, worst LSE error {self.worst_lse:.2e}, {len(self.state)} state failures, {self.saturated} saturated K bytes"


def run(trace, cfg, ops, refs=None, steps=None, splits_every=5, extra_splits=3):
    """Drive `ops` through the trace.  ops (duck-typed, see the two test files):
        start(trace, cfg)                               make the cache, fill the pool with NaN bytes
        host(step)                                      NaN-fill step.poison, write step.table, write step.lens0 into seqlens
        append(sd)                                      one padded append with new_lens = step.T
        attend(sd, num_splits) -> out fp32 [total, HQ, D], lse [HQ, total], qd fp64 [total, HQ, D] (the call's own q8 * scale_q)
        lens(), pool_rows() or gathered(), dead_pages(left)
    refs: the references of an earlier run of the same (trace, cfg), reused (the mutant runs).  Returns a Result; nothing is asserted here."""
    shadow = Shadow(cfg)
    res = Result()
    ops.start(trace, cfg)
    for sd in materialise(trace, cfg, shadow):
        if steps is not None and sd.i >= steps:
            break
        st = sd.step
        ops.host(st)
        ops.append(sd)
        out, lse, qd = ops.attend(sd, 0)
        ref = refs[sd.i] if refs is not None else reference(shadow, st, qd, trace.left)
        res.refs.append(ref)
        w, wl = grade_step(st, out, lse, ref)
        if sd.i % splits_every == 0 and extra_splits:
            out3, lse3, _ = ops.attend(sd, extra_splits)
            w3, wl3 = grade_step(st, out3, lse3, ref)
            w, wl = max(w, w3), max(wl, wl3)
        res.worst, res.worst_lse = max(res.worst, w), max(res.worst_lse, wl)
        pool = ops.pool_rows() if trace.paged else None
        bad = state_failures(trace, st, shadow, ops.lens(), pool, None if trace.paged else ops.gathered(),
                             ops.dead_pages(trace.left) if trace.left is not None else None)
        res.state += [(sd.i, st.events, m) for m in bad]
        res.saturated += sd.saturated
        res.steps += 1
    return res

"""The RoPE + sinks serving trace (tests/serving_trace_rope_sinks.py) on the CPU: every one of the nine traces of serving_trace.SEEDS
through the product's EAGER definitions (apply_rope_paged_varlen, paged_kv_cache_append_varlen_rope_fp8, fp8_attn_paged_varlen_sink_func
and, on equal counts, fp8_attn_paged_sink_func) under the grading the GPU file uses -- with the share of K bytes that land one code beside
the fp64 shadow's (printed; within 2^-14) and the condition that every head's sink takes a real share of the denominator on a real share
of its rows --, and the harness's TEETH: ten named mutants wrapped around the eager path.  A mutant that changes cache bytes must fail
the state check (for K: break the one-code rule or the 2^-14 cap); every mutant must push the worst |err| / bound above 1 or the LSE error
above LSE_TOL on every trace whose flags say the trace can see it.  The smallest ratio per mutant is printed (DESIGN.md section 4.26
records it); no margin is fixed in advance."""
import contextlib
import math
from unittest import mock

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import paged_varlen
from tests import paged_cases as PC
from tests import serving_trace as ST
from tests import serving_trace_rope_sinks as RS
from tests import splitkv_cases as S
from tests.test_cpu_serving_trace import IDS, TRACES, _deq_q

B, HKV, G, HQ = ST.B, ST.HKV, ST.G, ST.HQ
CFG = dict(D=64, dtype=torch.bfloat16, fmt="e4m3")       # the eager definitions do not depend on D: the smallest keeps the file quick
# mutant -> the flag that says a trace can see it (None: every trace; "window": the windowed traces)
MUTANTS = {
    "K rotated at the token's index in the step": None,
    "K positions from a count that ignores the rollback": "rollback_over_page_edge",
    "K positions counted from the first live page": "window",
    "the other pairing for K": None,
    "V rotated too": None,
    "q rotated at the lengths after the append": None,
    "sink dropped": None,
    "sink read at the kv-head index": None,
    "sink multiplied by sm_scale": None,
    "sink added once per split": None,
}
STATELESS = tuple(MUTANTS)[5:]                              # mutants of q and of the attention call: no byte of the cache changes
POSITION_MUTANTS = tuple(MUTANTS)[:3]
SMALLEST = {}                                               # mutant -> [(trace id, worst ratio, worst LSE error / LSE_TOL)]
SHARES = {}                                                 # trace id -> the largest share of K bytes beside the shadow's


class EagerOps:
    """the product's eager definitions on CPU tensors, optionally wrapped in ONE named mutant"""

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant

    def start(self, trace, cfg):
        self.trace, self.cfg = trace, cfg
        self.c = qa.alloc_paged_kv_cache_fp8(trace.num_pages, HKV, trace.page_size, cfg.D, batch_size=B, max_pages_per_seq=trace.M,
                                             scale_k=cfg.scale_k, scale_v=cfg.scale_v, dtype=cfg.dtype, device="cpu", fp8_format=cfg.fmt)
        assert self.c.layout == "rowmajor"
        self.nan = PC.NAN_BYTE[cfg.fmt]
        self.c.k.view(torch.uint8).fill_(self.nan)
        self.c.v.view(torch.uint8).fill_(self.nan)
        self.c.block_table.fill_(ST.POISON)

    def _pools(self):
        return self.c.k.view(torch.uint8), self.c.v.view(torch.uint8)

    def host(self, st):
        self.before = self.c.seqlens.tolist()                                          # what a count that no host edit reaches would hold
        for pool in self._pools():
            pool[st.poison] = self.nan
        self.c.block_table.copy_(torch.from_numpy(st.table))
        self.c.seqlens.copy_(torch.tensor(st.lens0, dtype=torch.int32))

    # -- rotate q, then the fused append ---------------------------------------------------------------------------------------------------
    def _wrong_positions(self, st):
        """paged_varlen._rope_positions_host under the position mutants: the base of every slot replaced"""
        real, ps = paged_varlen._rope_positions_host, self.trace.page_size

        def positions(cache, cu_seqlens, total, T, appended):
            rows, pos = real(cache, cu_seqlens, total, T, appended)
            wrong = []
            for b in range(B):
                base = {"K rotated at the token's index in the step": 0,
                        "K positions from a count that ignores the rollback": self.before[b] if st.events[b].startswith("rollback") else st.lens0[b],
                        "K positions counted from the first live page": st.lens0[b] - st.evicted[b] * ps}[self.mutant]
                wrong += [min(base + t, T - 1) for t in range(st.T[b])]
            assert len(wrong) == len(pos)
            return rows, wrong
        return positions

    def step(self, sd):
        st, cfg, c = sd.step, self.cfg, self.c
        cu = torch.tensor(st.cu, dtype=torch.int32)
        rope = dict(interleaved=cfg.il)
        late = self.mutant == "q rotated at the lengths after the append"
        if not late:
            self.q_rot = qa.apply_rope_paged_varlen(sd.q, c, cu, cfg.cos, cfg.sin, **rope)
        v_new = sd.v_new
        if self.mutant == "V rotated too":
            v_new = qa.apply_rope_paged_varlen(sd.v_new, c, cu, cfg.cos, cfg.sin, **rope)
        with contextlib.ExitStack() as stack:
            if self.mutant in POSITION_MUTANTS:
                stack.enter_context(mock.patch.object(paged_varlen, "_rope_positions_host", self._wrong_positions(st)))
            il = not cfg.il if self.mutant == "the other pairing for K" else cfg.il
            qa.paged_kv_cache_append_varlen_rope_fp8(c, sd.k_new, v_new, cu, cfg.cos, cfg.sin, interleaved=il)
        if late:
            self.q_rot = qa.apply_rope_paged_varlen(sd.q, c, cu, cfg.cos, cfg.sin, **rope)       # (appended=True would be right)
        return self.q_rot.double().numpy()

    # -- the attention calls ---------------------------------------------------------------------------------------------------------------
    def _sinks(self):
        s = self.cfg.sinks
        if self.mutant == "sink dropped":
            return torch.full_like(s, -math.inf)
        if self.mutant == "sink read at the kv-head index":
            return s[torch.arange(HQ) // G].clone()
        if self.mutant == "sink multiplied by sm_scale":
            return s / math.sqrt(self.cfg.D)
        return s

    def attend(self, sd, num_splits):
        st, left, cfg = sd.step, self.trace.left, self.cfg
        window = (-1, 0) if left is None else (left, 0)
        cu = torch.tensor(st.cu, dtype=torch.int32)
        kw = dict(max_seqlen_k=max(st.lens1), num_splits=num_splits, return_lse=True)
        q, sinks = self.q_rot, self._sinks()
        per_split = self.mutant == "sink added once per split" and num_splits > 1
        res = qa.fp8_attn_paged_varlen_sink_func(q, self.c, cu, max(st.T), sinks, window, return_partials=per_split, **kw)
        out, lse = res[0].float().numpy().astype(np.float64), res[1].numpy().astype(np.float64)
        if per_split:
            # the sink enters every split that holds a key of the row, not the merge once: n exp(sink_h) in the denominator
            pl = res[3].numpy().astype(np.float64)                                     # [ns, HQ, total], sink-free; -inf: no key
            n = np.isfinite(pl).sum(0)
            assert n.min() >= 1
            keys = np.logaddexp.reduce(pl, axis=0)
            wrong = np.logaddexp(keys, cfg.sinks64[:, None] + np.log(n))
            out, lse = out * np.exp(lse - wrong).T[..., None], wrong
        live = [t for t in st.T if t]
        if len(set(live)) == 1 and self.mutant is None:
            # every slot with queries has the same count: the dense paged sink entry gives the same rows, bit for bit
            n = live[0]
            qd = torch.zeros((B, HQ, n, cfg.D), dtype=cfg.dtype)
            for b in range(B):
                if st.T[b]:
                    qd[b] = q[st.cu[b]:st.cu[b + 1]].transpose(0, 1)
            do, dl = qa.fp8_attn_paged_sink_func(qd, self.c, sinks, window, **kw)
            for b in range(B):
                if st.T[b]:
                    assert torch.equal(do[b].transpose(0, 1), res[0][st.cu[b]:st.cu[b + 1]]) and torch.equal(dl[b], res[1][:, st.cu[b]:st.cu[b + 1]]), (sd.i, b)
        qd = np.zeros((sum(st.T), HQ, cfg.D))
        for b in range(B):
            if st.T[b]:
                qd[st.cu[b]:st.cu[b + 1]] = _deq_q(q[st.cu[b]:st.cu[b + 1]].transpose(0, 1)[None], cfg.fp8)[0].transpose(0, 1).numpy()
        return out, lse, qd

    # -- the state -------------------------------------------------------------------------------------------------------------------------
    def lens(self):
        return self.c.seqlens.tolist()

    def pool_rows(self):
        return tuple(p.numpy() for p in self._pools())

    def dead_pages(self, left):
        return qa.paged_window_dead_pages(self.c.seqlens, left, self.trace.page_size).tolist()


# ---- 1. the pieces of the shadow ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_round_once_is_the_nearest_16_bit_value_and_the_half_step_bound_is_the_least_a_correct_rounding_meets(dtype):
    g = torch.Generator().manual_seed(5)
    y = (torch.randn(1 << 20, generator=g, dtype=torch.float64) * torch.logspace(-3, 3, 1 << 20, base=2.0, dtype=torch.float64)).numpy()
    r = RS.round_once(y, dtype)
    # nearest: no neighbour in the format is closer
    bits = r.view(torch.int16).to(torch.int32)
    for step in (-1, 1):
        other = np.nan_to_num((bits + step).to(torch.int16).view(dtype).double().numpy(), nan=math.inf)     # (the code below zero is a NaN)
        assert (np.abs(r.double().numpy() - y) <= np.abs(other - y)).all()
    err = np.abs(r.double().numpy() - y)
    assert (err <= RS.halfstep(y, dtype)).all()
    normal = np.abs(y) >= 2.0 ** -13
    rel = float((err / np.abs(y))[normal].max())
    u = 2.0 ** -RS.SIG_BITS[dtype]
    print(f"{dtype}: worst relative error of the correct rounding {rel:.3e} = {rel / u:.3f} of 2^-{RS.SIG_BITS[dtype]}")
    assert u / 2 < 0.98 * u < rel <= u, "the correct rounding reaches the format's half step: no relative bound below it can hold"
    # torch's own cast rounds twice and is not always the nearest
    twice = torch.from_numpy(y).to(dtype)
    print(f"{dtype}: torch's fp64 cast is not the nearest value in {int((twice != r).sum())} of {y.size}")
    assert (twice != r).any() and (np.abs(twice.double().numpy() - y) >= err).all()


def test_the_one_code_rule():
    e4 = lambda *b: np.array(b, np.uint8)
    ok = RS.one_code(e4(0x00, 0x80, 0x10, 0x10, 0x90, 0x7E, 0x01), e4(0x80, 0x00, 0x11, 0x0F, 0x91, 0x7D, 0x00), "e4m3")
    assert ok.all()
    bad = RS.one_code(e4(0x10, 0x10, 0x01, 0x7E, 0x7F, 0x00), e4(0x12, 0x91, 0x81, 0x7F, 0x7F ^ 0x01, 0x82), "e4m3")
    assert not bad.any()
    assert RS.one_code(e4(0x7B), e4(0x7A), "e5m2").all() and not RS.one_code(e4(0x7B), e4(0x7C), "e5m2").any()
    seen = []
    rule = RS.k_rule("e4m3", seen)
    want = np.full((1, 2, 1 << 13, 4), 0x30, np.uint8)                                  # 2^16 live bytes: the cap is four of them
    got = want.copy()
    got[0, 0, :4, 0] = 0x31
    assert rule([got], [want], [(0, 1 << 13)]) == [] and seen == [(4, 1 << 16)]
    got[0, 1, 9, 0] = 0x2F
    assert len(rule([got], [want], [(0, 1 << 13)])) == 1
    got[0, 1, 9, 0] = 0x33
    assert len(rule([got], [want], [(0, 1 << 13)])) == 2
    assert rule([got], [want], [(10, 1 << 13)]) == []                                   # keys below the span (evicted pages) are not compared


# ---- 2. the eager definitions and the mutants ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,left", TRACES, ids=IDS)
def test_the_eager_definitions_pass_every_step_and_every_mutant_is_caught(ps, left):
    torch.set_num_threads(4)
    trace, cfg = ST.trace_of(ps, left), RS.Cfg(**CFG)
    clean = RS.run(trace, cfg, EagerOps())
    print(f"eager ps {ps} left {left}: {clean}")
    assert clean.steps == ST.STEPS and clean.worst < 1.0 and clean.worst_lse < S.LSE_TOL and not clean.state, (clean, clean.state[:3])
    assert clean.q_worst <= 1.0, clean.q_worst
    assert clean.saturated > 0, "saturation is part of the model"
    assert clean.k_share <= RS.K_SHARE_CAP
    SHARES[f"ps{ps}-{left}"] = clean.k_share
    # every head's sink takes more than a tenth of the denominator on a quarter of its rows and less than nine tenths on a quarter
    share = clean.sink_shares(cfg.sinks64)
    above, below = (share > 0.1).mean(1), (share < 0.9).mean(1)
    print("  sink share > 0.1 on " + " ".join(f"{x:.2f}" for x in above) + " of the rows per head, < 0.9 on " + " ".join(f"{x:.2f}" for x in below))
    assert (above >= 0.25).all() and (below >= 0.25).all(), (above, below)
    for name, flag in MUTANTS.items():
        if flag == "window":
            if left is None:
                continue
        elif flag is not None:
            assert trace.flags[flag]
        res = RS.run(trace, cfg, EagerOps(name), refs=clean.refs)
        SMALLEST.setdefault(name, []).append((f"ps{ps}-{left}", res.worst, res.worst_lse / S.LSE_TOL))
        print(f"  mutant {name!r}: worst |err| / bound {res.worst:.2f}, worst LSE error / LSE_TOL {res.worst_lse / S.LSE_TOL:.2f}, "
              f"q error / bound {res.q_worst:.2f}, {len(res.state)} state failures"
              + (f", first at step {res.state[0][0]}: {res.state[0][2]}" if res.state else ""))
        assert res.worst > 1.0 or res.worst_lse > S.LSE_TOL, (name, res.worst, res.worst_lse)
        if name in STATELESS:
            assert not res.state, (name, res.state[:3])
        else:
            assert res.state, name
        if name == "q rotated at the lengths after the append":
            assert res.q_worst > 1.0, "the bound on q_rot sees it too"


def test_the_smallest_ratio_of_every_mutant_and_the_k_byte_shares_are_printed():
    """(after the traces above, in file order) the figures DESIGN.md section 4.26 records"""
    assert len(SHARES) == len(TRACES) and set(SMALLEST) == set(MUTANTS), "run with the parametrised traces above: this test only reports them"
    for tid, share in SHARES.items():
        print(f"trace {tid}: largest share of live K bytes one code beside the shadow's {share:.2e} (cap {RS.K_SHARE_CAP:.2e})")
    for name, seen in SMALLEST.items():
        tid, r, l = min(seen, key=lambda x: x[1])
        print(f"mutant {name!r}: smallest worst |err| / bound {r:.2f} (trace {tid}, LSE error / LSE_TOL {l:.2f} there) over {len(seen)} traces")
        assert all(max(x[1], x[2]) > 1.0 for x in seen)


def test_the_fast_trace_passes_through_the_eager_definition():
    """the FAST trace of the GPU file (unit-variance queries, no pointer rows): the eager definition knows one numerics, so this pins the data"""
    torch.set_num_threads(4)
    res = RS.run(ST.trace_of(128), RS.Cfg(pointers=False, q_std=1.0, **CFG), EagerOps(), splits_every=10)
    assert res.worst < 1.0 and res.worst_lse < S.LSE_TOL and not res.state and res.q_worst <= 1.0, res


# ---- 3. the teeth of the K rule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("il", [False, True])
def test_a_k_position_shifted_by_one_breaks_the_one_code_rule_in_every_appended_row(il):
    """a shadow whose keys are rotated one position further, against the bytes the eager append leaves: every appended key of every slot
    holds a byte more than one code away (no attention call is made: the appends of the whole trace)"""
    trace, cfg = ST.trace_of(64), RS.Cfg(interleaved=il, **CFG)
    ops, shadow = EagerOps(), RS.Shadow(cfg)
    ops.start(trace, cfg)
    rows = 0
    for sd in RS.materialise(trace, cfg, shadow, k_shift=1):
        st = sd.step
        ops.host(st)
        ops.step(sd)
        got = PC.gather_rows(ops.pool_rows()[0], st.table, trace.page_size)
        for b in range(B):
            lo, hi = st.lens0[b], st.lens1[b]
            broken = ~RS.one_code(got[b][:, lo:hi], shadow.k8[b][:, lo:hi], cfg.fmt)
            assert broken.any((0, 2)).all(), (sd.i, b)
            rows += hi - lo
    assert rows > 1024

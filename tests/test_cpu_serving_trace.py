"""The serving-trace harness (tests/serving_trace.py) on the CPU: the coverage flags of every trace the GPU file runs, every trace through
the product's EAGER definitions (CPU tensors: paged_kv_cache_append_fp8, fp8_attn_paged_varlen_func, fp8_attn_paged_func and their window
and contiguous siblings) under the grading the GPU file uses, and the harness's TEETH: six named mutants wrapped around the eager path,
each of which must push the worst |err| / bound above 1 on some step AND fail the state check on every trace whose flags say the trace
can see it.  (The packed-query mutant changes no byte of the cache: it is asked for the ratio only, and the state check must stay clean
under it.)  The smallest ratio per mutant is printed; DESIGN.md section 4.22 records it.  No margin is fixed in advance."""
import contextlib
import math
from unittest import mock

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import nn, paged, paged_varlen
from tests import paged_cases as PC
from tests import serving_trace as ST
from tests import splitkv_cases as S
from tests import splitkv_window_cases as W

B, HKV, HQ = ST.B, ST.HKV, ST.HQ
CFG = dict(D=64, dtype=torch.bfloat16, fmt="e4m3")       # the eager definitions do not depend on D: the smallest keeps the file quick
TRACES = [(ps, left) for left in (None,) + ST.LEFTS for ps in ST.PAGE_SIZES]
IDS = [f"ps{ps}-{'causal' if left is None else f'left{left}'}" for ps, left in TRACES]
# mutant -> the flag that says a trace can see it (None: every trace; "window": the windowed traces)
MUTANTS = {
    "append ignores a rollback": "rollback_over_page_edge",
    "append zeroes the rest of a partly covered chunk": "start_mid_chunk",
    "stale table after reuse": "reused_by_other_slot_partly",
    "page index off by one at a page edge": "straddle_page",
    "one dead page too many": "window",
    "packed queries of the idle neighbour": "idle_before_active",
}
STATELESS = ("packed queries of the idle neighbour",)       # mutants of the attention call alone: no byte of the cache changes
SMALLEST = {}                                               # mutant -> [(trace id, worst ratio)]


def _deq_q(q, fp8):
    q8, sq = nn._dynamically_quantize_fp8(q, reduction_dim=[2, 3], fp8_dtype=fp8)
    return (q8.float() * sq[..., None, None]).double()


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
        for pool in self._pools():
            pool[st.poison] = self.nan
        table = torch.from_numpy(st.table)
        if self.mutant == "stale table after reuse":
            old = self.c.block_table
            table = torch.where((old != ST.POISON) & (table != ST.POISON), old, table)     # a reassigned entry keeps the slot's previous page
        self.c.block_table.copy_(table)
        lens0 = list(st.lens0)
        if self.mutant == "append ignores a rollback":
            cur = self.c.seqlens.tolist()
            lens0 = [cur[b] if st.events[b].startswith("rollback") else lens0[b] for b in range(B)]
        self.c.seqlens.copy_(torch.tensor(lens0, dtype=torch.int32))

    # -- the append ------------------------------------------------------------------------------------------------------------------------
    def append(self, sd):
        st, ps = sd.step, self.trace.page_size
        table = self.c.block_table.tolist()
        edge = []
        if self.mutant == "page index off by one at a page edge":
            # the first key of a page is looked up one page early: remember what the right place held, append, move the bytes
            for b in range(B):
                for j in range(st.lens0[b], st.lens1[b]):
                    if j % ps == 0 and j > 0:
                        edge.append((table[b][j // ps], table[b][j // ps - 1], [pool[table[b][j // ps], :, 0].clone() for pool in self._pools()]))
        qa.paged_kv_cache_append_fp8(self.c, sd.k_new, sd.v_new, new_lens=torch.tensor(st.T, dtype=torch.int32))
        for right, wrong, kept in edge:
            for pool, old in zip(self._pools(), kept):
                pool[wrong, :, 0] = pool[right, :, 0]
                pool[right, :, 0] = old
        if self.mutant == "append zeroes the rest of a partly covered chunk":
            for b in range(B):
                if st.T[b]:
                    lo, hi = st.lens0[b], st.lens1[b]
                    for j in list(range(lo // 64 * 64, lo)) + list(range(hi, -(-hi // 64) * 64)):
                        for pool in self._pools():
                            pool[table[b][j // ps], :, j % ps] = 0

    # -- the attention calls ---------------------------------------------------------------------------------------------------------------
    def _gather(self, real):
        """gather_paged_eager under the lookup mutants"""
        ps, left = self.trace.page_size, self.trace.left

        def gather(cache, Skv=None):
            kv = real(cache, Skv)
            table = cache.block_table.tolist()
            if self.mutant == "page index off by one at a page edge":
                for b in range(kv.k.shape[0]):
                    for j in range(ps, kv.k.shape[2], ps):
                        for img, pool in zip((kv.k, kv.v), (cache.k, cache.v)):
                            img.view(torch.uint8)[b, :, j] = pool.view(torch.uint8)[table[b][j // ps - 1], :, 0]
            if self.mutant == "one dead page too many":
                for b in range(kv.k.shape[0]):
                    dead = W.dead_pages(self.lens1[b], left, ps, max(self.sq[b], 1)) + 1
                    kv.k.view(torch.uint8)[b, :, :dead * ps] = self.nan
                    kv.v.view(torch.uint8)[b, :, :dead * ps] = self.nan
            return kv
        return gather

    def attend(self, sd, num_splits):
        st, left = sd.step, self.trace.left
        self.lens1, self.sq = st.lens1, st.T
        cu = torch.tensor(st.cu, dtype=torch.int32)
        kw = dict(max_seqlen_k=max(st.lens1), num_splits=num_splits, return_lse=True)
        with contextlib.ExitStack() as stack:
            if self.mutant in ("page index off by one at a page edge", "one dead page too many"):
                g = self._gather(paged.gather_paged_eager)
                stack.enter_context(mock.patch.object(paged, "gather_paged_eager", g))
                stack.enter_context(mock.patch.object(paged_varlen, "gather_paged_eager", g))
            if left is None:
                out, lse = qa.fp8_attn_paged_varlen_func(sd.q, self.c, cu, max(st.T), causal=True, **kw)
            else:
                out, lse = qa.fp8_attn_paged_varlen_window_func(sd.q, self.c, cu, max(st.T), (left, 0), **kw)
            live = [t for t in st.T if t]
            if len(set(live)) == 1 and self.mutant is None:
                # every slot with queries has the same count: the dense paged entry gives the same rows (idle slots get zero queries' worth
                # of zeros as their rows; they are not compared)
                n = live[0]
                qd = torch.zeros((B, HQ, n, self.cfg.D), dtype=self.cfg.dtype)
                for b in range(B):
                    if st.T[b]:
                        qd[b] = sd.q[st.cu[b]:st.cu[b + 1]].transpose(0, 1)
                if left is None:
                    do, dl = qa.fp8_attn_paged_func(qd, self.c, causal=True, **kw)
                else:
                    do, dl = qa.fp8_attn_paged_window_func(qd, self.c, (left, 0), **kw)
                for b in range(B):
                    if st.T[b]:
                        assert torch.equal(do[b].transpose(0, 1), out[st.cu[b]:st.cu[b + 1]]) and torch.equal(dl[b], lse[:, st.cu[b]:st.cu[b + 1]]), (sd.i, b)
        out, lse = out.float().numpy().copy(), lse.numpy().copy()
        if self.mutant == "packed queries of the idle neighbour":
            for b in range(1, B):
                if st.T[b - 1] == 0 and st.T[b]:          # slot b - 1 has no queries, and slot b is given those: its rows are never computed
                    out[st.cu[b]:st.cu[b + 1]] = 0
                    lse[:, st.cu[b]:st.cu[b + 1]] = 0
        qd = np.zeros((sum(st.T), HQ, self.cfg.D))
        for b in range(B):
            if st.T[b]:
                qd[st.cu[b]:st.cu[b + 1]] = _deq_q(sd.q[st.cu[b]:st.cu[b + 1]].transpose(0, 1)[None], self.cfg.fp8)[0].transpose(0, 1).numpy()
        return out, lse, qd

    # -- the state -------------------------------------------------------------------------------------------------------------------------
    def lens(self):
        return self.c.seqlens.tolist()

    def pool_rows(self):
        return tuple(p.numpy() for p in self._pools())

    def dead_pages(self, left):
        dead = qa.paged_window_dead_pages(self.c.seqlens, left, self.trace.page_size).tolist()
        return [d + 1 for d in dead] if self.mutant == "one dead page too many" else dead


class ContiguousEagerOps:
    """the contiguous KVCacheFP8 through kv_cache_append_fp8 and fp8_attn_splitkv_func: one batch element per shadow slot; the dense entry
    takes one query count, so a slot's queries are the LAST rows of a block padded in front with zero rows (causal is bottom-right: the
    last Sq_b rows of Sq_max attend what Sq_b rows alone attend)"""

    def start(self, trace, cfg):
        self.trace, self.cfg = trace, cfg
        self.c = qa.alloc_kv_cache_fp8(B, HKV, ST.CAP, cfg.D, scale_k=cfg.scale_k, scale_v=cfg.scale_v, dtype=cfg.dtype, device="cpu", fp8_format=cfg.fmt)
        self.c.k.view(torch.uint8).fill_(PC.NAN_BYTE[cfg.fmt])
        self.c.v.view(torch.uint8).fill_(PC.NAN_BYTE[cfg.fmt])

    def host(self, st):
        self.c.seqlens.copy_(torch.tensor(st.lens0, dtype=torch.int32))

    def append(self, sd):
        qa.kv_cache_append_fp8(self.c, sd.k_new, sd.v_new, new_lens=torch.tensor(sd.step.T, dtype=torch.int32))

    def attend(self, sd, num_splits):
        st, n = sd.step, max(sd.step.T)
        q = torch.zeros((B, HQ, n, self.cfg.D), dtype=self.cfg.dtype)
        for b in range(B):
            if st.T[b]:
                q[b, :, n - st.T[b]:] = sd.q[st.cu[b]:st.cu[b + 1]].transpose(0, 1)
        do, dl = qa.fp8_attn_splitkv_func(q, self.c, causal=True, seqused_k=self.c.seqlens, num_splits=num_splits, return_lse=True)
        dq = _deq_q(q, self.cfg.fp8)
        out, lse, qd = np.zeros((sum(st.T), HQ, self.cfg.D), np.float32), np.zeros((HQ, sum(st.T)), np.float32), np.zeros((sum(st.T), HQ, self.cfg.D))
        for b in range(B):
            if st.T[b]:
                rows = slice(st.cu[b], st.cu[b + 1])
                out[rows], lse[:, rows] = do[b, :, n - st.T[b]:].transpose(0, 1).float().numpy(), dl[b, :, n - st.T[b]:].numpy()
                qd[rows] = dq[b, :, n - st.T[b]:].transpose(0, 1).numpy()
        return out, lse, qd

    def lens(self):
        return self.c.seqlens.tolist()

    def gathered(self):
        return self.c.k.view(torch.uint8).numpy(), self.c.v.view(torch.uint8).numpy()


# ---- 1. the flags -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,left", TRACES, ids=IDS)
def test_every_trace_the_gpu_file_runs_sets_every_coverage_flag(ps, left):
    t = ST.trace_of(ps, left)
    assert len(t.steps) == ST.STEPS and all(v for v in t.flags.values()), {f: v for f, v in t.flags.items() if not v}
    assert set(t.flags) == set(ST.FLAGS + (ST.WINDOW_FLAGS if left is not None else ()))
    assert max(max(s.lens1) for s in t.steps) <= ST.MAX_LEN
    for st in t.steps:                                     # what the trace promises the kernels: entries in range, POISON never handed out
        assert 0 <= st.table.min() and st.table.max() < t.num_pages and ST.POISON in st.nan_pages and any(st.T)
        for b in range(B):
            need = -(-st.lens1[b] // ps)
            assert (st.table[b, st.evicted[b]:need] != ST.POISON).all() and (st.table[b, need:] == ST.POISON).all() and (st.table[b, :st.evicted[b]] == ST.POISON).all()
    assert all(set(st.T) <= {0, 1} for st in t.steps[-ST.TAIL:]), "the graph stretch is decode / idle only"
    assert ST.Trace(ST.SEEDS[(ps, left)], ps, left).steps[-1].lens1 == t.steps[-1].lens1, "the generator is deterministic"


def test_the_dead_page_count_of_the_traces_is_the_products():
    """splitkv_window_cases.dead_pages counts the evictions; paged_window_dead_pages must agree, over every length of every windowed trace"""
    for ps, left in TRACES:
        if left is not None:
            lens = sorted({L for st in ST.trace_of(ps, left).steps for L in st.lens0 + st.lens1})
            for nq in (1, 7, 130):
                got = qa.paged_window_dead_pages(torch.tensor(lens, dtype=torch.int32), left, ps, num_queries=nq).tolist()
                assert got == [W.dead_pages(L, left, ps, nq) for L in lens]


# ---- 2. the eager definitions and the mutants -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,left", TRACES, ids=IDS)
def test_the_eager_definitions_pass_every_step_and_every_mutant_is_caught(ps, left):
    torch.set_num_threads(4)
    trace, cfg = ST.trace_of(ps, left), ST.Cfg(**CFG)
    clean = ST.run(trace, cfg, EagerOps())
    print(f"eager ps {ps} left {left}: {clean}")
    assert clean.steps == ST.STEPS and clean.worst < 1.0 and clean.worst_lse < S.LSE_TOL and not clean.state, (clean, clean.state[:3])
    assert clean.saturated > 0, "saturation is part of the model"
    for name, flag in MUTANTS.items():
        if flag == "window":
            if left is None:
                continue
        else:
            assert trace.flags[flag]
        res = ST.run(trace, cfg, EagerOps(name), refs=clean.refs)
        SMALLEST.setdefault(name, []).append((f"ps{ps}-{left}", res.worst))
        print(f"  mutant {name!r}: worst |err| / bound {res.worst:.2f}, {len(res.state)} state failures"
              + (f", first at step {res.state[0][0]}: {res.state[0][2]}" if res.state else ""))
        assert res.worst > 1.0, (name, res.worst)
        if name in STATELESS:
            assert not res.state, (name, res.state[:3])
        else:
            assert res.state, name


def test_the_smallest_ratio_of_every_mutant_is_printed():
    """(after the traces above, in file order) the figure DESIGN.md section 4.22 records"""
    for name, seen in SMALLEST.items():
        tid, r = min(seen, key=lambda x: x[1])
        print(f"mutant {name!r}: smallest worst |err| / bound {r:.2f} (trace {tid}) over {len(seen)} traces")
        assert r > 1.0


def test_the_contiguous_cache_runs_the_same_trace_without_paging_events():
    torch.set_num_threads(4)
    trace = ST.Trace(ST.CONTIGUOUS_SEED, 128, None, paged=False)
    assert all(not e.startswith(("finish", "evict")) for st in trace.steps for e in st.events)
    assert any(e.startswith("rollback") for st in trace.steps for e in st.events)
    res = ST.run(trace, ST.Cfg(**CFG), ContiguousEagerOps())
    print(f"eager contiguous: {res}")
    assert res.steps == ST.STEPS and res.worst < 1.0 and res.worst_lse < S.LSE_TOL and not res.state, (res, res.state[:3])


def test_the_fast_trace_passes_through_the_eager_definition():
    """the FAST trace of the GPU file (unit-variance queries, no pointer rows): the eager definition knows one numerics, so this pins the
    data, not the precision"""
    torch.set_num_threads(4)
    res = ST.run(ST.trace_of(128), ST.Cfg(pointers=False, q_std=1.0, **CFG), EagerOps(), splits_every=10)
    assert res.worst < 1.0 and res.worst_lse < S.LSE_TOL and not res.state, res

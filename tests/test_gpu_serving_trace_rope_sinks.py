"""-m gpu: the serving traces of tests/serving_trace.py through the step a gpt-oss layer is made of (tests/serving_trace_rope_sinks.py):
apply_rope_paged_varlen on the step's packed q BEFORE the append, paged_kv_cache_append_varlen_rope_fp8 on the step's UNROTATED packed K,
fp8_attn_paged_varlen_sink_func under (-1, 0) or (left, 0) with num_splits 0; every fifth step a second call with nine splits (the chained
merge); on steps whose busy slots have one query count also fp8_attn_paged_sink_func, bit-equal row for row.

After every step: q_rot against the fp64 rotation by value, out and the LSE against the fp64 reference with the sink column on the
shadow's de-quantised keys and the call's own q8 / scale_q (gpu_utils.grade, LSE_TOL), cache.seqlens, the V bytes of every live key
exactly, the K bytes under the one-code rule and the 2^-14 cap, the NaN of every free page, the dead-page counts.  The shadow rotates in
fp64 and imports no rule of the product.  tests/test_cpu_serving_trace_rope_sinks.py shows that this grading catches ten named mutants.
The pool starts as NaN bytes and every unread table entry points at a NaN page: no entry is ever out of range."""
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import serving_trace as ST
from tests import serving_trace_rope_sinks as RS
from tests import splitkv_cases as S
from tests.test_gpu_serving_trace import DEV, DeviceOps, _cus, _same_bits, _su

pytestmark = pytest.mark.gpu

B, HKV, HQ = ST.B, ST.HKV, ST.HQ
# D, dtype, format, interleaved; the first is gpt-oss's own layout
CONFIGS = [(64, torch.bfloat16, "e4m3", False), (128, torch.float16, "e5m2", True), (256, torch.bfloat16, "e4m3", False)]
CAUSAL = [(ps,) + CONFIGS[i] for i, ps in enumerate(ST.PAGE_SIZES)]
# every configuration meets every window_left once; the last case is given bf16 sinks
WINDOWED = [(ps, left) + CONFIGS[(i + j) % 3] + (torch.bfloat16 if (i, j) == (2, 1) else torch.float32,)
            for j, left in enumerate(ST.LEFTS) for i, ps in enumerate(ST.PAGE_SIZES)]


def _id(case):
    return "-".join(str(x)[6:] if isinstance(x, torch.dtype) else f"il{int(x)}" if isinstance(x, bool) else str(x) for x in case)


class RopeSinkOps(DeviceOps):
    """the HIP entries of the RoPE + sinks step on the paged cache of test_gpu_serving_trace.DeviceOps"""

    def start(self, trace, cfg):
        super().start(trace, cfg)
        self.cos, self.sin, self.sinks = cfg.cos.to(DEV), cfg.sin.to(DEV), cfg.sinks.to(DEV)
        self.window = (-1, 0) if trace.left is None else (trace.left, 0)

    def step(self, sd):
        cfg, cu = self.cfg, _su(sd.step.cu)
        self.q_rot = qa.apply_rope_paged_varlen(sd.q.to(DEV), self.c, cu, self.cos, self.sin, interleaved=cfg.il)
        qa.paged_kv_cache_append_varlen_rope_fp8(self.c, sd.k_new.to(DEV), sd.v_new.to(DEV), cu, self.cos, self.sin, interleaved=cfg.il)
        return self.q_rot.double().cpu().numpy()

    def _native_call(self, q, cu, st, ns, Skv):
        c = self.c
        return _native.fp8_attention_paged_varlen(q, c.k, c.v, c.scale_k, c.scale_v, c.block_table, c.seqlens, cu, max_seqlen_q=max(st.T), Skv=Skv,
                                                  num_pages=c.num_pages, page_size=c.page_size, fp8_dtype=self.cfg.fp8, numerics=c.numerics,
                                                  precision=self.precision, num_splits=ns, return_lse=True, return_quant=True, window=self.window,
                                                  sinks=self.sinks.float())

    def attend(self, sd, num_splits):
        st, c, window = sd.step, self.c, self.window
        q, cu, Skv = self.q_rot[:sum(st.T)], _su(st.cu), max(st.lens1)
        kw = dict(max_seqlen_k=Skv, num_splits=num_splits, precision=self.precision, return_lse=True)
        out, lse = qa.fp8_attn_paged_varlen_sink_func(q, c, cu, max(st.T), self.sinks, window, **kw)
        raw = self._native_call(q, cu, st, num_splits, Skv)
        assert _same_bits(raw[0], out) and _same_bits(raw[1], lse), (sd.i, "the public function is the C call")
        live = [t for t in st.T if t]
        if len(set(live)) == 1:
            # one query count among the busy slots: the dense paged sink entry gives their rows bit for bit, with the split count this call ran
            n, total = live[0], sum(st.T)
            ns = num_splits or _native.paged_varlen_window_auto_splits(B, HQ, HKV, total, n, Skv, self.cfg.D, window[0], _cus())
            qd = torch.zeros((B, HQ, n, self.cfg.D), dtype=self.cfg.dtype, device=DEV)
            for b in range(B):
                if st.T[b]:
                    qd[b] = q[st.cu[b]:st.cu[b + 1]].transpose(0, 1)
            do, dl = qa.fp8_attn_paged_sink_func(qd, c, self.sinks, window, **dict(kw, num_splits=ns))
            for b in range(B):
                if st.T[b]:
                    rows = slice(st.cu[b], st.cu[b + 1])
                    assert _same_bits(do[b].transpose(0, 1), out[rows]) and _same_bits(dl[b], lse[:, rows]), (sd.i, b, "dense paged != packed")
        return out.float().cpu().numpy(), lse.cpu().numpy(), self._deq_q(raw[2], raw[3], st)


class GraphOps(RopeSinkOps):
    """... with the last ST.TAIL steps (decode / idle only) as replays of ONE captured "rotate q, RoPE-append, attend with sinks" graph:
    between replays the host writes the table, the lengths of a rollback and cu_seqlens, and copies the step's tokens into the captured
    token bucket of B rows (K / V rows behind cu[B]: NaN; q rows behind it: zeros, as is q_rot's buffer)"""

    def start(self, trace, cfg):
        super().start(trace, cfg)
        self.first, self.graph = len(trace.steps) - ST.TAIL, None
        self.qs, self.qr = (torch.zeros((B, HQ, cfg.D), dtype=cfg.dtype, device=DEV) for _ in range(2))
        self.ks, self.vs = (torch.zeros((B, HKV, cfg.D), dtype=cfg.dtype, device=DEV) for _ in range(2))
        self.cus = _su([0] * (B + 1))

    def _step(self, c):
        rope = dict(interleaved=self.cfg.il)
        qa.apply_rope_paged_varlen(self.qs, c, self.cus, self.cos, self.sin, out=self.qr, **rope)
        qa.paged_kv_cache_append_varlen_rope_fp8(c, self.ks, self.vs, self.cus, self.cos, self.sin, **rope)
        return qa.fp8_attn_paged_varlen_sink_func(self.qr, c, self.cus, 1, self.sinks, self.window, num_splits=0, return_lse=True)

    def _capture(self):
        warm = self._alloc()                                                               # (appends nothing: cu_seqlens = 0 at this point)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._step(warm)
        torch.cuda.current_stream().wait_stream(side)
        before = self.c.seqlens.tolist()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out_s, self.lse_s = self._step(self.c)
        assert self.c.seqlens.tolist() == before, "capture ran nothing"

    def step(self, sd):
        if sd.i < self.first:
            return super().step(sd)
        if self.graph is None:
            self._capture()
        st, total = sd.step, sum(sd.step.T)
        assert set(st.T) <= {0, 1} and total <= B
        for dst, src in ((self.ks, sd.k_new), (self.vs, sd.v_new)):
            dst.fill_(float("nan"))
            dst[:total] = src.to(DEV)
        self.qs.zero_()
        self.qs[:total] = sd.q.to(DEV)
        self.qr.zero_()
        self.cus.copy_(_su(st.cu))
        self.graph.replay()
        torch.cuda.synchronize()
        self.q_rot = self.qr
        assert not self.qr[total:].any(), "rows behind cu[B] are not written"
        return self.qr[:total].double().cpu().numpy()

    def attend(self, sd, num_splits):
        if sd.i < self.first or num_splits:
            return super().attend(sd, num_splits)
        st, total = sd.step, sum(sd.step.T)
        # the same calls outside the graph on the cache the replay left: q at the positions BEFORE the append (appended=True), then the sink
        # entry -- the same bits, and the q8 / scale_q the reference de-quantises
        again = qa.apply_rope_paged_varlen(self.qs, self.c, self.cus, self.cos, self.sin, interleaved=self.cfg.il, appended=True)
        assert _same_bits(again[:total], self.qr[:total]), (sd.i, "replayed q_rot != eager")
        raw = self._native_call(self.qr, self.cus, st, 0, ST.CAP)
        assert _same_bits(raw[0][:total], self.out_s[:total]) and _same_bits(raw[1][:, :total], self.lse_s[:, :total]), (sd.i, "replay != eager")
        return self.out_s[:total].float().cpu().numpy(), self.lse_s[:, :total].cpu().numpy(), self._deq_q(raw[2], raw[3], st)


def _passes(res, what):
    print(f"{what}: {res}")
    assert res.steps == ST.STEPS and not res.state, (what, res.state[:3])
    assert res.worst < 1.0, (what, res.worst)
    assert res.worst_lse < S.LSE_TOL, (what, res.worst_lse)
    assert res.q_worst <= 1.0, (what, res.q_worst)


@pytest.mark.parametrize("page_size,D,dtype,fmt,il", CAUSAL, ids=[_id(c) for c in CAUSAL])
def test_a_causal_schedule_through_rope_append_and_sinks_stays_within_the_bounds_of_the_shadow_model(page_size, D, dtype, fmt, il):
    res = RS.run(ST.trace_of(page_size), RS.Cfg(D, dtype, fmt, il), RopeSinkOps())
    _passes(res, f"rope + sinks trace ps{page_size} d{D} {fmt} il{int(il)}")
    assert res.saturated > 0


@pytest.mark.parametrize("page_size,left,D,dtype,fmt,il,sink_dtype", WINDOWED, ids=[_id(c) for c in WINDOWED])
def test_a_windowed_schedule_with_evictions_through_rope_append_and_sinks_stays_within_the_bounds(page_size, left, D, dtype, fmt, il, sink_dtype):
    """window (left, 0): the leading dead pages are freed, NaN-filled and handed to other slots, their table entries point at the NaN page,
    and a slot appends -- at positions that still count the evicted keys -- after its page went to another slot"""
    res = RS.run(ST.trace_of(page_size, left), RS.Cfg(D, dtype, fmt, il, sink_dtype), RopeSinkOps())
    _passes(res, f"rope + sinks window trace ps{page_size} left{left} d{D} {fmt} il{int(il)} sinks {str(sink_dtype)[6:]}")


def test_a_fast_schedule_on_unit_variance_queries_stays_within_the_bounds():
    """precision="fast" on the data FAST is stated for (unit-variance queries, no pointer rows): the sink entries take the exact one-term
    sweep, and the bounds are unchanged"""
    res = RS.run(ST.trace_of(128), RS.Cfg(128, torch.bfloat16, "e4m3", pointers=False, q_std=1.0), RopeSinkOps("fast"))
    _passes(res, "FAST rope + sinks trace ps128 d128 e4m3")


def test_the_last_decode_steps_as_replays_of_one_captured_rope_append_sink_graph_stay_within_the_bounds():
    ops = GraphOps()
    res = RS.run(ST.trace_of(64, 63), RS.Cfg(64, torch.bfloat16, "e4m3"), ops)
    _passes(res, "rope + sinks graph stretch ps64 left63 d64 e4m3")
    assert ops.graph is not None

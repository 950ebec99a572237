"""-m gpu: the serving traces of tests/serving_trace.py with the device side appending through paged_kv_cache_append_varlen_fp8 -- each
step's tokens PACKED by its counts ([total, Hkv, D] under the step's cu_seqlens, the tensor the attention call takes as cu_seqlens_q)
instead of padded to the longest chunk.  The shadow model and its per-step checks (pool bytes of every live key looked up through the
table, seqlens, the NaN of every free page, the outputs against the fp64 reference) are tests/serving_trace.py's, unchanged; the attention
side is tests/test_gpu_serving_trace.py's DeviceOps.  One trace per page size at one (D, dtype, format) each; in each the last ST.TAIL
steps (decode / idle only) run as replays of ONE captured packed-append-then-attend graph."""
import pytest
import torch

import quantumattention_amd as qa
from tests import serving_trace as ST
from tests.test_gpu_serving_trace import DEV, DeviceOps, _passes, _same_bits, _su

pytestmark = pytest.mark.gpu

B, HKV, HQ = ST.B, ST.HKV, ST.HQ
CASES = [(64, 128, torch.bfloat16, "e4m3"), (128, 64, torch.float16, "e5m2"), (256, 256, torch.bfloat16, "e4m3")]     # page size, D, dtype, format
IDS = [f"ps{p}-d{d}-{str(t)[6:]}-{f}" for p, d, t, f in CASES]


def _packed(x, T):
    """[total, HKV, D] of a step's padded tokens x [B, HKV, Tmax, D]: slot b's first T_b rows, in slot order"""
    return torch.cat([x[b, :, :T[b]].transpose(0, 1) for b in range(B)])


class PackedAppendOps(DeviceOps):
    """DeviceOps with the packed append, and the last ST.TAIL steps as replays of one captured graph: between replays the host writes the
    table, the lengths of a rollback and cu_seqlens, and copies the step's tokens into the captured token bucket (rows behind cu[B]: NaN)"""

    def start(self, trace, cfg):
        super().start(trace, cfg)
        self.first, self.graph = len(trace.steps) - ST.TAIL, None
        self.qs = torch.zeros((B, HQ, cfg.D), dtype=cfg.dtype, device=DEV)                 # a token bucket of B rows: cu[B] <= B
        self.ks, self.vs = (torch.zeros((B, HKV, cfg.D), dtype=cfg.dtype, device=DEV) for _ in range(2))
        self.cus = _su([0] * (B + 1))

    def _step(self, c):
        qa.paged_kv_cache_append_varlen_fp8(c, self.ks, self.vs, self.cus)
        return qa.fp8_attn_paged_varlen_func(self.qs, c, self.cus, 1, causal=True, num_splits=0, return_lse=True)

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

    def append(self, sd):
        T = sd.step.T
        k, v = _packed(sd.k_new, T).to(DEV), _packed(sd.v_new, T).to(DEV)
        if sd.i < self.first:
            qa.paged_kv_cache_append_varlen_fp8(self.c, k, v, _su(sd.step.cu))
            return
        if self.graph is None:
            self._capture()
        total = sum(T)
        assert set(T) <= {0, 1} and total <= B
        for dst, src in ((self.ks, k), (self.vs, v)):
            dst.fill_(float("nan"))
            dst[:total] = src
        self.qs.zero_()
        self.qs[:total] = sd.q.to(DEV)
        self.cus.copy_(_su(sd.step.cu))

    def attend(self, sd, num_splits):
        if sd.i < self.first or num_splits:
            return super().attend(sd, num_splits)
        st, total = sd.step, sum(sd.step.T)
        self.graph.replay()
        torch.cuda.synchronize()
        # the same call outside the graph on the cache the replay left: the same bits, and the q8 / scale_q the reference de-quantises
        raw = self._native_call(self.qs, self.cus, st, 0, ST.CAP)
        assert _same_bits(raw[0][:total], self.out_s[:total]) and _same_bits(raw[1][:, :total], self.lse_s[:, :total]), (sd.i, "replay != eager")
        return self.out_s[:total].float().cpu().numpy(), self.lse_s[:, :total].cpu().numpy(), self._deq_q(raw[2], raw[3], st)


@pytest.mark.parametrize("page_size,D,dtype,fmt", CASES, ids=IDS)
def test_a_long_mixed_schedule_through_the_packed_append_stays_within_the_bound_of_the_shadow_model(page_size, D, dtype, fmt):
    ops = PackedAppendOps()
    res = ST.run(ST.trace_of(page_size), ST.Cfg(D, dtype, fmt), ops)
    _passes(res, f"packed-append trace ps{page_size} d{D} {fmt}")
    assert res.saturated > 0 and ops.graph is not None

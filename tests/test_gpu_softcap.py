"""Logit soft-capping on the MI355X (quantumattention_amd/softcap.py, include/qattn_softcap.h) through the three entries -- contiguous,
paged, packed over paged -- on the problems of tests/softcap_cases.py (every input exact in e4m3, so the fp64 oracle needs no quantiser):

  the fp64 oracle with the cap applied in fp64, over the cap ladder (0.5 / 2 / 50 at scale g / sqrt(D), g 1 / 4), the windows and the
  splits: out within the fp8-V bound of tests/gpu_utils.py, the LSE -- of the CAPPED scores -- within the siblings' LSE_TOL (|dy/dx| <= 1:
  the cap shrinks score errors and leaves the P.V arithmetic alone; no new tolerance), rows without a key exactly zero with lse -inf.
  ACCURATE on every rung; FAST's one-term sweep where the sibling's bound is stated for it (tests/softcap_cases.graded_heads), its LSE
  and its empty rows on every rung;
  the closed-form cap probe whose teeth tests/test_cpu_softcap.py shows on these very inputs;
  the bit identities: paged = contiguous on the gathered cache; packed = paged on each slot alone, idle slots included;
  merge_attn_states(partials) = out, lse; precision "fast" = itself called with an LSE; softcap 0.0 = the window sibling;
  NaN bytes in keys outside the window and behind seqused_k influence no bit; one captured graph follows rewritten seqlens, table and
  cu_seqlens_q; torch.compile(fullgraph=True) of "append, then attend with softcap" gives the eager bits."""
import functools
import gc
import math

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from tests import gpu_utils
from tests import paged_cases as P
from tests import paged_varlen_cases as V
from tests import softcap_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """This module's device memory goes back to the driver when its last test is done: tests later in the suite measure a call's
    peak allocation against the caching allocator's state (tests/test_gpu_window.py), and cached blocks of this module's sizes would be
    handed out whole to their smaller requests."""
    yield
    _dev.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

DEV = "cuda"
ENTRIES = ("contig", "paged", "packed")


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class Dev:
    """a problem's objects on the device: the paged cache, the contiguous PreparedKV the table selects from it, q dense and packed"""

    def __init__(self, p, **cache_kw):
        self.p = p
        self.c, self.table = p.cache(DEV, **cache_kw)
        self.kv = qa.PreparedKV(P.gather(self.c.k, self.table, C.HKV, C.PAGE, p.D), P.gather(self.c.v, self.table, C.HKV, C.PAGE, p.D),
                                self.c.scale_k, self.c.scale_v, (C.B, C.HKV, C.CAP, p.D), self.c.fp8_format, self.c.dtype, self.c.numerics, "frag")
        self.q = p.q.to(DEV)
        self.qp, self.cu, _ = p.packed_q(DEV)

    def call(self, entry, cap, window, **kw):
        """(out [B, HQ, Sq, D], lse [B, HQ, Sq], ...the partials as the entry returns them) through the public function; cap None: the
        window sibling"""
        p, c = self.p, self.c
        kw.setdefault("return_lse", True)
        if entry == "contig":
            if cap is None:
                return qa.fp8_attn_splitkv_window_func(self.q, self.kv, window, seqused_k=c.seqlens, **kw)
            return qa.fp8_attn_splitkv_softcap_func(self.q, self.kv, cap, window, seqused_k=c.seqlens, **kw)
        if entry == "paged":
            if cap is None:
                return qa.fp8_attn_paged_window_func(self.q, c, window, **kw)
            return qa.fp8_attn_paged_softcap_func(self.q, c, cap, window, **kw)
        if cap is None:
            res = qa.fp8_attn_paged_varlen_window_func(self.qp, c, self.cu, p.Sq, window, **kw)
        else:
            res = qa.fp8_attn_paged_varlen_softcap_func(self.qp, c, self.cu, p.Sq, cap, window, **kw)
        if not isinstance(res, tuple):
            return res.view(C.B, p.Sq, C.HQ, p.D).transpose(1, 2)
        return (res[0].view(C.B, p.Sq, C.HQ, p.D).transpose(1, 2), res[1].view(C.HQ, C.B, p.Sq).transpose(0, 1)) + tuple(res[2:])


@functools.lru_cache(maxsize=None)
def _dev(D, Sq):
    return Dev(C.Problem(D, Sq))


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Sq", C.CASES)
def test_the_three_entries_are_within_the_siblings_bounds_of_the_fp64_oracle_over_the_cap_ladder(D, Sq):
    d = _dev(D, Sq)
    worst = [0.0, 0.0]
    for window in C.WINDOWS:
        empty = d.p.empty(window)
        for cap in C.CAPS:
            for gain in C.GAINS:
                ro, rl = d.p.reference(window, cap, gain)
                rung = [0.0, 0.0]
                for ns in C.SPLITS:
                    for precision in ("accurate", "fast"):
                        for entry in ENTRIES:
                            out, lse = d.call(entry, cap, window, scale=d.p.scale(gain), num_splits=ns, precision=precision)
                            what = (entry, D, Sq, window, cap, gain, ns, precision)
                            o, l = gpu_utils.out_to_f32(out), lse.float().cpu().numpy()
                            with np.errstate(invalid="ignore"):
                                err = float(np.abs(l - rl)[~empty].max())
                            heads = C.graded_heads(precision, cap, gain)
                            if heads:
                                rung[0] = max(rung[0], float((np.abs(o - ro) / C.bound(ro))[:, heads].max()))
                                gpu_utils.assert_within_bound(o[:, heads], ro[:, heads], what=what)
                            rung[1] = max(rung[1], err / C.LSE_TOL)
                            assert err <= C.LSE_TOL, (what, "lse", err)
                            assert (o[empty] == 0).all() and np.isneginf(l[empty]).all(), (what, "a row without a key: zeros, lse -inf")
                print(f"softcap D{D} Sq{Sq} {window} cap {cap} g {gain}: worst |err| / bound {rung[0]:.3f}, LSE error / {C.LSE_TOL} {rung[1]:.3f}")
                worst = [max(a, b) for a, b in zip(worst, rung)]
    print(f"softcap D{D} Sq{Sq}: worst |err| / bound {worst[0]:.3f}, worst LSE error / {C.LSE_TOL} {worst[1]:.3f}")


@pytest.mark.parametrize("D", (64, 128, 256))
def test_the_cap_probe_through_every_entry_is_its_closed_form(D):
    worst = 0.0
    for Sq in C.PROBE_SQS:
        d = Dev(C.Probe(D, Sq))
        for window in C.WINDOWS:
            for cap in C.PROBE_CAPS:
                ro, rl = d.p.expected(window, cap)
                for ns in C.SPLITS:
                    for precision in ("accurate", "fast"):
                        bnd = C.probe_bound(ro, precision)
                        for entry in ENTRIES:
                            out, lse = d.call(entry, cap, window, scale=C.PROBE_SCALE, num_splits=ns, precision=precision)
                            o, l = gpu_utils.out_to_f32(out), lse.float().cpu().numpy()
                            what = (entry, D, Sq, window, cap, ns, precision)
                            live = ro != 0
                            worst = max(worst, float((np.abs(o - ro)[live] / bnd[live]).max()))
                            assert np.all(np.abs(o - ro) <= bnd), (what, float((np.abs(o - ro)[live] / bnd[live]).max()))
                            assert (o[~live] == 0).all(), what
                            assert float(np.abs(l - rl).max()) <= C.LSE_TOL, (what, "lse")
    print(f"cap probe D{D}: worst |err| / bound {worst:.3f} (tests/test_cpu_softcap.py: the dropped and the misplaced cap move it by >= {C.TEETH})")


# ---- the bit identities -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Sq", [(64, 5), (128, 5), (256, 5)])
def test_paged_is_contiguous_on_the_gathered_cache_and_packed_is_paged_on_each_slot_alone_idle_slots_included(D, Sq):
    d = _dev(D, Sq)
    sq = [5, 0, 3, 1]
    qp, cud, cu = d.p.packed_q(DEV, sq)
    for window in C.WINDOWS:
        for cap, gain in ((2.0, 4.0), (50.0, 1.0)):
            for ns in C.SPLITS:
                for precision in ("accurate", "fast"):
                    kw = dict(num_splits=ns, precision=precision, scale=d.p.scale(gain), return_lse=True, return_partials=True)
                    a = qa.fp8_attn_paged_softcap_func(d.q, d.c, cap, window, **kw)
                    b = qa.fp8_attn_splitkv_softcap_func(d.q, d.kv, cap, window, seqused_k=d.c.seqlens, **kw)
                    assert len(a) == len(b) == 5 and all(_same_bits(x, y) for x, y in zip(a, b)), (D, window, cap, ns, precision)
                    got = qa.fp8_attn_paged_varlen_softcap_func(qp, d.c, cud, max(sq), cap, window, **kw)
                    for s in range(C.B):
                        if sq[s]:
                            want = qa.fp8_attn_paged_softcap_func(V.alone(qp, cu, s), V.one_slot(d.c, s), cap, window, **kw)
                            what = (D, window, cap, ns, precision, s)
                            assert _same_bits(V.rows_of(got[0], "o", cu, s), want[0]) and _same_bits(V.rows_of(got[1], "l", cu, s), want[1]), what
                            if ns > 1:
                                assert _same_bits(V.rows_of(got[2], "po", cu, s), want[2]) and _same_bits(V.rows_of(got[3], "pl", cu, s), want[3]), what


@pytest.mark.parametrize("D,Sq", [(64, 1), (64, 130), (128, 5), (256, 5)])
def test_the_partials_merge_to_out_and_lse_fast_is_itself_with_an_lse_and_softcap_zero_is_the_window_sibling(D, Sq):
    d = _dev(D, Sq)
    for window in C.WINDOWS:
        for precision in ("accurate", "fast"):
            for entry in ENTRIES:
                for ns in C.SPLITS:
                    what = (entry, D, Sq, window, ns, precision)
                    kw = dict(num_splits=ns, precision=precision, scale=d.p.scale(4.0))
                    # softcap 0.0: the sibling, bit for bit (out, lse, the partials)
                    z = d.call(entry, 0.0, window, return_partials=True, **kw)
                    s = d.call(entry, None, window, return_partials=True, **kw)
                    assert len(z) == len(s) == 5 and all(_same_bits(x, y) for x, y in zip(z, s)), (what, "softcap 0.0")
                    got = d.call(entry, 2.0, window, return_partials=True, **kw)
                    assert not _same_bits(got[0], s[0]) and not _same_bits(got[1], s[1]), (what, "the cap is felt")
                    # no LSE request: the bits of the call with one (the exact sweep, never the byte-exponential one)
                    alone = d.call(entry, 2.0, window, return_lse=False, **kw)
                    assert _same_bits(alone, got[0]), (what, "without an LSE request")
                    if ns > 1:
                        if entry == "packed":
                            po, pl = list(got[2].unbind(0)), list(got[3].unbind(0))
                            mo, ml = qa.merge_attn_states(po, pl, out_dtype=d.q.dtype)
                            mo, ml = mo.view(C.B, Sq, C.HQ, D).transpose(1, 2), ml.view(C.HQ, C.B, Sq).transpose(0, 1)
                        else:
                            mo, ml = qa.merge_attn_states(list(got[2].unbind(0)), list(got[3].unbind(0)), out_dtype=d.q.dtype)
                        assert _same_bits(mo, got[0]) and _same_bits(ml, got[1]), (what, "merge_attn_states(partials)")
                    else:
                        assert got[2].numel() == got[3].numel() == 0, what


@pytest.mark.parametrize("D", (64, 256))
def test_nan_bytes_in_keys_outside_the_window_and_behind_seqused_k_influence_no_bit(D):
    """K and V of every key below lo_b = L_b - Sq - left and behind L_b hold NaN bytes (hot) or zeros (cold): the same bits, all finite.
    (-1, 0) has dead keys behind L_b only; under (127, 0) and (63, 0) the window's first chunk holds dead keys beside live ones."""
    p = C.Problem(D, 5)
    for window in ((127, 0), (63, 0), (-1, 0)):
        hot, cold = Dev(p, dead=0x7F, window=window), Dev(p, dead=0, window=window)
        for cap, gain in ((2.0, 4.0), (50.0, 1.0)):
            for ns in (1, 2):
                for precision in ("accurate", "fast"):
                    for entry in ENTRIES:
                        kw = dict(num_splits=ns, precision=precision, scale=p.scale(gain), return_partials=True)
                        a = hot.call(entry, cap, window, **kw)
                        b = cold.call(entry, cap, window, **kw)
                        what = (entry, D, window, cap, ns, precision)
                        assert torch.isfinite(a[0].float()).all() and torch.isfinite(a[1]).all(), what
                        assert all(_same_bits(x, y) for x, y in zip(a, b)), what


# ---- graphs and torch.compile ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 2, 9])
def test_a_graph_captured_once_follows_rewritten_seqlens_table_and_cu_seqlens_q(ns):
    p = C.Problem(64, 5)
    d = Dev(p)
    window, cap, scale = (127, 0), 2.0, p.scale(4.0)
    qp, cud, _ = p.packed_q(DEV, [5, 5, 5, 5])
    attend = lambda: (qa.fp8_attn_paged_softcap_func(d.q, d.c, cap, window, scale=scale, num_splits=ns, return_lse=True)
                      + qa.fp8_attn_paged_varlen_softcap_func(qp, d.c, cud, 5, cap, window, scale=scale, num_splits=ns, return_lse=True))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        attend()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = attend()
    table0 = d.c.block_table.clone()
    swapped = table0.clone()
    swapped[[0, 3]] = table0[[3, 0]]                                  # slots 0 and 3 read each other's pages
    steps = (([60, 300, 1100, 1270], table0, [0, 5, 10, 15, 20]), ([65, 128, 129, 1280], swapped, [0, 5, 5, 8, 9]),
             (list(C.LENS), table0, [0, 5, 10, 15, 20]))
    for lens, table, cu in steps:
        d.c.seqlens.copy_(torch.tensor(lens, dtype=torch.int32))
        d.c.block_table.copy_(table)
        cud.copy_(torch.tensor(cu, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        want = attend()
        torch.cuda.synchronize()
        n_used = cu[-1]
        assert _same_bits(res[0], want[0]) and _same_bits(res[1], want[1]), (ns, lens, "paged")
        assert _same_bits(res[2][:n_used], want[2][:n_used]) and _same_bits(res[3][:, :n_used], want[3][:, :n_used]), (ns, lens, "packed")


def test_torch_compile_fullgraph_of_append_then_attend_with_softcap_gives_the_eager_bits():
    D = 64
    p = C.Problem(D, 1)
    kn, vn = (torch.randn(C.B, C.HKV, 1, D, generator=torch.Generator().manual_seed(s)).bfloat16().to(DEV) for s in (1, 2))
    q = p.q.to(DEV)
    qp, cud, _ = p.packed_q(DEV)
    scale = p.scale(4.0)

    def dense(cache):
        def f(q, kn, vn):
            qa.paged_kv_cache_append_fp8(cache, kn, vn)
            return qa.fp8_attn_paged_softcap_func(q * 2, cache, 50.0, (127, 0), scale=scale, num_splits=2, return_lse=True)
        return f

    def packed(cache):
        def f(q, kn, vn):
            qa.paged_kv_cache_append_fp8(cache, kn, vn)
            return qa.fp8_attn_paged_varlen_softcap_func(q * 2, cache, cud, 1, 2.0, scale=scale, num_splits=1, return_lse=True)
        return f

    def fresh():
        c, _ = p.cache(DEV)
        c.seqlens.copy_(torch.tensor([60, 300, 1100, 1270], dtype=torch.int32))
        return c

    for step, query in ((dense, q), (packed, qp)):
        ca, cb = fresh(), fresh()
        torch._dynamo.reset()
        got = torch.compile(step(ca), fullgraph=True)(query, kn, vn)
        want = step(cb)(query, kn, vn)
        assert ca.seqlens.tolist() == cb.seqlens.tolist() == [61, 301, 1101, 1271] and torch.equal(ca.k, cb.k) and torch.equal(ca.v, cb.v)
        for name, x, y in zip(("out", "lse"), got, want):
            assert _same_bits(x, y), (step.__name__, name, x.dtype, y.dtype, x.shape, y.shape, float((x.float() - y.float()).abs().max()))
        assert not math.isnan(float(got[0].float().sum()))

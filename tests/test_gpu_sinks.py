"""Learned attention sinks on the MI355X (quantumattention_amd/sinks.py, include/qattn_sinks.h) through the three entries -- contiguous,
paged, packed over paged -- on the problems of tests/sinks_cases.py (every input exact in e4m3, so the fp64 oracle needs no quantiser):

  the oracle with the sink column: out within the fp8-V bound of tests/gpu_utils.py (the sink only scales a row by 1 - p_sink <= 1), the
  LSE -- sink included -- within the siblings' LSE_TOL (logaddexp is 1-Lipschitz in the key LSE), rows without a key exactly zero with
  lse == sink_h exactly; ACCURATE and FAST, 1 / 2 / 9 splits;
  the constant-V probe whose teeth tests/test_cpu_sinks.py shows on these very inputs;
  the bit identities: -inf sinks = the window sibling (out, lse, row_path, partials); the partials under finite sinks = the sibling's;
  merge_attn_states_with_sinks(partials) = out, lse; paged = contiguous on the gathered cache; packed = paged on each slot alone;
  a NaN or +inf sink poisons exactly its head; NaN bytes in keys outside the window influence no bit; one captured graph follows a
  rewritten sinks tensor; torch.compile(fullgraph=True) of "append, then attend with sinks" gives the eager bits."""
import functools
import math

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import gpu_utils
from tests import paged_cases as P
from tests import paged_varlen_cases as V
from tests import sinks_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
NINF = [-math.inf] * S.HQ
ENTRIES = ("contig", "paged", "packed")


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _t(x):
    return torch.tensor(np.asarray(x, np.float32), device=DEV)


class Dev:
    """a problem's objects on the device: the paged cache, the contiguous PreparedKV the table selects from it, q dense and packed"""

    def __init__(self, p, **cache_kw):
        self.p = p
        self.c, self.table = p.cache(DEV, **cache_kw)
        self.kv = qa.PreparedKV(P.gather(self.c.k, self.table, S.HKV, S.PAGE, p.D), P.gather(self.c.v, self.table, S.HKV, S.PAGE, p.D),
                                self.c.scale_k, self.c.scale_v, (S.B, S.HKV, S.CAP, p.D), self.c.fp8_format, self.c.dtype, self.c.numerics, "frag")
        self.q = p.q.to(DEV)
        self.qp, self.cu, _ = p.packed_q(DEV)

    def call(self, entry, sinks, window, **kw):
        """(out [B, HQ, Sq, D], lse [B, HQ, Sq], ...the partials as the entry returns them) through the public function; sinks None: the
        window sibling"""
        p, c = self.p, self.c
        kw.setdefault("return_lse", True)
        if entry == "contig":
            if sinks is None:
                return qa.fp8_attn_splitkv_window_func(self.q, self.kv, window, seqused_k=c.seqlens, **kw)
            return qa.fp8_attn_splitkv_sink_func(self.q, self.kv, sinks, window, seqused_k=c.seqlens, **kw)
        if entry == "paged":
            if sinks is None:
                return qa.fp8_attn_paged_window_func(self.q, c, window, **kw)
            return qa.fp8_attn_paged_sink_func(self.q, c, sinks, window, **kw)
        if sinks is None:
            res = qa.fp8_attn_paged_varlen_window_func(self.qp, c, self.cu, p.Sq, window, **kw)
        else:
            res = qa.fp8_attn_paged_varlen_sink_func(self.qp, c, self.cu, p.Sq, sinks, window, **kw)
        if not isinstance(res, tuple):
            return res.view(S.B, p.Sq, S.HQ, p.D).transpose(1, 2)
        return (res[0].view(S.B, p.Sq, S.HQ, p.D).transpose(1, 2), res[1].view(S.HQ, S.B, p.Sq).transpose(0, 1)) + tuple(res[2:])


@functools.lru_cache(maxsize=None)
def _dev(D, Sq, const_v=False):
    return Dev(S.Problem(D, Sq, const_v=const_v))


def _grade(out, lse, ro, rl, empty, snk, what):
    o, l = gpu_utils.out_to_f32(out), lse.float().cpu().numpy()
    gpu_utils.assert_within_bound(o, ro, what=what)
    err = float(np.abs(l - rl).max())
    assert err <= S.LSE_TOL, (what, "lse", err)
    assert (o[empty] == 0).all(), (what, "a row without a key is exactly zero")
    assert np.array_equal(l[empty], np.broadcast_to(snk[None, :, None], l.shape)[empty]), (what, "... and its lse is sink_h exactly")
    return float((np.abs(o - ro) / S.bound(ro)).max()), err / S.LSE_TOL


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sq", S.SQS)
@pytest.mark.parametrize("D", S.DS)
def test_the_three_entries_are_within_the_siblings_bounds_of_the_fp64_oracle_with_the_sink_column(D, Sq):
    d = _dev(D, Sq)
    worst = [0.0, 0.0]
    for window in S.WINDOWS:
        snk = d.p.ladder(window)
        st = _t(snk)
        empty = np.isneginf(d.p.keys_state(window)[1])
        ro, rl = d.p.reference(window, snk)
        for ns in S.SPLITS:
            for precision in ("accurate", "fast"):
                for entry in ENTRIES:
                    out, lse = d.call(entry, st, window, num_splits=ns, precision=precision)
                    r = _grade(out, lse, ro, rl, empty, snk, (entry, D, Sq, window, ns, precision))
                    worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"sinks D{D} Sq{Sq}: worst |err| / bound {worst[0]:.3f}, worst LSE error / {S.LSE_TOL} {worst[1]:.3f}")


@pytest.mark.parametrize("Sq", S.SQS)
@pytest.mark.parametrize("D", S.DS)
def test_the_constant_v_probe_through_every_entry_is_v_times_one_minus_the_sinks_share(D, Sq):
    d = _dev(D, Sq, True)
    worst = 0.0
    for window in S.WINDOWS:
        snk = d.p.ladder(window)
        st = _t(snk)
        lse_k = d.p.keys_state(window)[1]
        share = 1.0 / (1.0 + np.exp(lse_k - snk[None, :, None].astype(np.float64)))
        v0 = d.p.v.double().numpy()[:, :, 0].repeat(S.G, axis=1)[:, :, None, :]
        ref = np.where(np.isneginf(lse_k)[..., None], 0.0, v0 * (1.0 - share)[..., None])
        for ns in S.SPLITS:
            for entry in ENTRIES:
                out, _ = d.call(entry, st, window, num_splits=ns)
                o = gpu_utils.out_to_f32(out)
                gpu_utils.assert_within_bound(o, ref, what=(entry, D, Sq, window, ns))
                worst = max(worst, float((np.abs(o - ref) / S.bound(ref)).max()))
    print(f"constant-V probe D{D} Sq{Sq}: worst |err| / bound {worst:.3f} (tests/test_cpu_sinks.py: every mutant moves a row by >= {S.TEETH})")


@pytest.mark.parametrize("D", S.DS)
def test_a_sink_far_above_every_score_neither_overflows_nor_loses_the_lse(D):
    """sink_h = lse_keys + 30 / 60 / 200: the sink's term is 2^43 / 2^87 / 2^289 times the keys' sum -- the last two beyond what the sweep's
    own shift can hold in fp32 (the kernel sums under the sink's shift from 2^64 on).  Same bounds: out is v times a share of e^-30 or
    less, the LSE is the sink's to 2e-3."""
    d = _dev(D, 5)
    for window in ((-1, 0), (127, 0)):
        base = d.p.ladder(window) - np.log(np.array(S.LADDER, np.float32))
        empty = np.isneginf(d.p.keys_state(window)[1])
        for above in (30.0, 60.0, 200.0):
            snk = (base + np.float32(above)).astype(np.float32)
            ro, rl = d.p.reference(window, snk)
            for ns in (1, 2):
                for entry in ENTRIES:
                    out, lse = d.call(entry, _t(snk), window, num_splits=ns)
                    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all(), (entry, D, window, above, ns)
                    _grade(out, lse, ro, rl, empty, snk, (entry, D, window, above, ns))


# ---- the bit identities -------------------------------------------------------------------------------------------------------------------------
def _native_call(d, entry, window, sinks, **kw):
    """the _native functions: row_path comes back too"""
    c = d.c
    kw = dict(window=window, sinks=sinks, return_lse=True, return_partials=True, return_path=True, **kw)
    if entry == "contig":
        return _native.fp8_attention_splitkv(d.q, d.kv.k, d.kv.v, d.kv.scale_k, d.kv.scale_v, Skv=S.CAP, seqused_k=c.seqlens, **kw)
    if entry == "paged":
        return _native.fp8_attention_paged_splitkv(d.q, c.k, c.v, c.scale_k, c.scale_v, c.block_table, c.seqlens, Skv=S.CAP, num_pages=c.num_pages,
                                                   page_size=S.PAGE, **kw)
    return _native.fp8_attention_paged_varlen(d.qp, c.k, c.v, c.scale_k, c.scale_v, c.block_table, c.seqlens, d.cu, max_seqlen_q=d.p.Sq, Skv=S.CAP,
                                              num_pages=c.num_pages, page_size=S.PAGE, **kw)


@pytest.mark.parametrize("D,Sq", [(64, 1), (64, 130), (128, 5), (128, 130)])
def test_minus_inf_sinks_are_the_window_sibling_and_finite_sinks_leave_its_partials_alone(D, Sq):
    """out, lse, partial_o, partial_lse, partial_path, row_path.  Under FAST the sibling is called with its LSE, as here: the sink entries
    run the exact one-term sweep where the sibling without an LSE request would take the byte-exponential one."""
    d = _dev(D, Sq)
    ninf = _t(NINF)
    for window in S.WINDOWS:
        st = _t(d.p.ladder(window))
        for ns in S.SPLITS:
            for precision in ("accurate", "fast"):
                for entry in ENTRIES:
                    what = (entry, D, Sq, window, ns, precision)
                    sib = _native_call(d, entry, window, None, num_splits=ns, precision=precision)
                    got = _native_call(d, entry, window, ninf, num_splits=ns, precision=precision)
                    assert len(got) == len(sib) == 6 and all(_same_bits(x, y) for x, y in zip(got, sib)), what
                    fin = _native_call(d, entry, window, st, num_splits=ns, precision=precision)
                    assert all(_same_bits(x, y) for x, y in zip(fin[2:], sib[2:])), (what, "partials and row_path")
                    assert not _same_bits(fin[0], sib[0]) and not _same_bits(fin[1], sib[1]), (what, "the sink is felt")
                    if ns > 1:
                        parts_o, parts_l = list(fin[2].unbind(0)), list(fin[3].unbind(0))
                        mo, ml = qa.merge_attn_states_with_sinks(parts_o, parts_l, st, out_dtype=d.q.dtype)
                        assert _same_bits(mo, fin[0]) and _same_bits(ml, fin[1]), (what, "merge_attn_states_with_sinks(partials)")
    # FAST without an LSE request: the bits of the call with one
    st = _t(d.p.ladder((-1, 0)))
    for entry in ENTRIES:
        a = d.call(entry, st, (-1, 0), num_splits=1, precision="fast", return_lse=False)
        b = d.call(entry, st, (-1, 0), num_splits=1, precision="fast")[0]
        assert _same_bits(a, b), entry


@pytest.mark.parametrize("D", S.DS)
def test_paged_is_contiguous_on_the_gathered_cache_and_packed_is_paged_on_each_slot_alone_idle_slots_included(D):
    d = _dev(D, 5)
    sq = [5, 0, 3, 1]
    qp, cud, cu = d.p.packed_q(DEV, sq)
    for window in S.WINDOWS:
        st = _t(d.p.ladder(window))
        for ns in S.SPLITS:
            for precision in ("accurate", "fast"):
                kw = dict(num_splits=ns, precision=precision, return_lse=True, return_partials=True)
                a = qa.fp8_attn_paged_sink_func(d.q, d.c, st, window, **kw)
                b = qa.fp8_attn_splitkv_sink_func(d.q, d.kv, st, window, seqused_k=d.c.seqlens, **kw)
                assert len(a) == len(b) == 5 and all(_same_bits(x, y) for x, y in zip(a, b)), (D, window, ns, precision)
                got = qa.fp8_attn_paged_varlen_sink_func(qp, d.c, cud, max(sq), st, window, **kw)
                for s in range(S.B):
                    if sq[s]:
                        want = qa.fp8_attn_paged_sink_func(V.alone(qp, cu, s), V.one_slot(d.c, s), st, window, **kw)
                        what = (D, window, ns, precision, s)
                        assert _same_bits(V.rows_of(got[0], "o", cu, s), want[0]) and _same_bits(V.rows_of(got[1], "l", cu, s), want[1]), what
                        if ns > 1:
                            assert _same_bits(V.rows_of(got[2], "po", cu, s), want[2]) and _same_bits(V.rows_of(got[3], "pl", cu, s), want[3]), what


@pytest.mark.parametrize("D", S.DS)
def test_a_nan_or_plus_inf_sink_makes_exactly_its_heads_rows_nan(D):
    d = _dev(D, 130)                                               # (rows without a key included)
    keep = [0, 1, 3]
    for window in ((127, 0), (0, 0)):
        snk = d.p.ladder(window)
        for poison in (math.nan, math.inf):
            bad = snk.copy()
            bad[2] = poison
            for ns in S.SPLITS:
                for entry in ENTRIES:
                    out, lse = d.call(entry, _t(bad), window, num_splits=ns)
                    ref = d.call(entry, _t(snk), window, num_splits=ns)
                    what = (entry, D, window, poison, ns)
                    assert torch.isnan(out[:, 2].float()).all() and torch.isnan(lse[:, 2]).all(), what
                    assert _same_bits(out[:, keep], ref[0][:, keep]) and _same_bits(lse[:, keep], ref[1][:, keep]), what


@pytest.mark.parametrize("D", S.DS)
def test_nan_bytes_in_keys_outside_the_window_still_influence_no_bit(D):
    """K and V of every key below lo_b = L_b - Sq - left and behind L_b hold NaN bytes (hot) or zeros (cold): the same bits, all finite"""
    p = S.Problem(D, 5)
    for window in ((127, 0), (63, 0)):
        hot, cold = Dev(p, dead=0x7F, window=window), Dev(p, dead=0, window=window)
        st = _t(p.ladder(window))
        for ns in (1, 2):
            for precision in ("accurate", "fast"):
                for entry in ENTRIES:
                    a = hot.call(entry, st, window, num_splits=ns, precision=precision, return_partials=True)
                    b = cold.call(entry, st, window, num_splits=ns, precision=precision, return_partials=True)
                    assert torch.isfinite(a[0].float()).all() and torch.isfinite(a[1]).all(), (entry, D, window, ns, precision)
                    assert all(_same_bits(x, y) for x, y in zip(a, b)), (entry, D, window, ns, precision)


# ---- graphs and torch.compile ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 2, 9])
def test_a_graph_captured_once_follows_a_rewritten_sinks_tensor(ns):
    d = _dev(64, 5)
    window = (127, 0)
    snk = d.p.ladder(window)
    st = _t(snk)
    attend = lambda s: (qa.fp8_attn_paged_sink_func(d.q, d.c, s, window, num_splits=ns, return_lse=True)
                        + qa.fp8_attn_paged_varlen_sink_func(d.qp, d.c, d.cu, 5, s, window, num_splits=ns, return_lse=True))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        attend(st)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = attend(st)
    for new in (snk + 1.5, snk[::-1].copy(), np.array(NINF, np.float32), snk):
        st.copy_(_t(new))
        graph.replay()
        torch.cuda.synchronize()
        want = attend(_t(new))
        assert all(_same_bits(x, y) for x, y in zip(res, want)), (ns, new)


def test_torch_compile_fullgraph_of_append_then_attend_with_sinks_gives_the_eager_bits():
    D = 64
    p = S.Problem(D, 1)
    st = _t(p.ladder((127, 0)))
    kn, vn = (torch.randn(S.B, S.HKV, 1, D, generator=torch.Generator().manual_seed(s)).bfloat16().to(DEV) for s in (1, 2))
    q = p.q.to(DEV)
    qp, cud, _ = p.packed_q(DEV)

    def dense(cache):
        def f(q, kn, vn, s):
            qa.paged_kv_cache_append_fp8(cache, kn, vn)
            return qa.fp8_attn_paged_sink_func(q * 2, cache, s, (127, 0), num_splits=2, return_lse=True)
        return f

    def packed(cache):
        def f(q, kn, vn, s):
            qa.paged_kv_cache_append_fp8(cache, kn, vn)
            return qa.fp8_attn_paged_varlen_sink_func(q * 2, cache, cud, 1, s, num_splits=1, return_lse=True)
        return f

    def fresh():
        c, _ = p.cache(DEV)
        c.seqlens.copy_(torch.tensor([60, 300, 1100, 1270], dtype=torch.int32))
        return c

    for step, query, snk in ((dense, q, st), (packed, qp, st.bfloat16())):      # (16-bit sinks: up-cast inside the traced function)
        ca, cb = fresh(), fresh()
        torch._dynamo.reset()
        got = torch.compile(step(ca), fullgraph=True)(query, kn, vn, snk)
        want = step(cb)(query, kn, vn, snk)
        assert ca.seqlens.tolist() == cb.seqlens.tolist() == [61, 301, 1101, 1271] and torch.equal(ca.k, cb.k) and torch.equal(ca.v, cb.v)
        for name, x, y in zip(("out", "lse"), got, want):
            assert _same_bits(x, y), (step.__name__, name, x.dtype, y.dtype, x.shape, y.shape, float((x.float() - y.float()).abs().max()))
        assert not math.isnan(float(got[0].float().sum()))

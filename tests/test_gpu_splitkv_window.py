"""Sliding windows for the split-KV, paged and packed-paged entries on the MI355X (quantumattention_amd/splitkv_window.py,
include/qattn_splitkv_window.h), contract point by contract point:

  1  (-1, 0) / (-1, -1) give the bits of the sibling with causal=True / False: out, lse, row_path, q8, scale_q and all partials;
  2  one split, Hq = Hkv, contiguous prepared K / V: out and lse are the bits of fp8_window_attn_pv_func(pv_precision="fp8");
  3  paged = the contiguous window entry on the gathered cache; packed = the paged window entry on each slot alone;
  4  out, lse = merge_attn_states(partials);
  5  bytes of keys outside [lo_i, L_i) -- NaN patterns, keys that share lo_i's chunk -- and table entries outside the window's pages
     influence no output bit;
then the membership probes of tests/probes.py through all three entries, the fp64 oracle within the fp8-V bound with the lower edge
inside a chunk / on a chunk, page and split boundary, one captured graph that follows the moved window over freed pages, the ops called
directly and torch.compile(fullgraph=True) of "append, then attend".  Tables, pools and query counts are the shared ones of
tests/paged_cases.py / tests/paged_varlen_cases.py; the window rules are restated in tests/splitkv_window_cases.py."""
import math

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import gpu_utils
from tests import paged_cases as P
from tests import paged_varlen_cases as V
from tests import probes as PR
from tests import splitkv_window_cases as W
from tests.gpu_utils import bits8
from tests.test_gpu_paged import CFG_IDS, CFGS, GS, SCALE_K, _cache, _contig, _gathered, _pack, _paged, _rand, _rows, _same_bits, _su
from tests.test_gpu_paged_varlen import _dense_alone, _rows_equal, _varlen
from tests.test_gpu_probes import T, count_ratio, deq_q, lse_ratio

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HKV, CAP = P.B, P.HKV, P.CAP
ALL = dict(return_lse=True, return_partials=True, return_quant=True, return_path=True)
NAMES = ("out", "lse", "partial_o", "partial_lse", "partial_path", "q8", "scale_q", "row_path")
# a window per shared table: the lower edge inside a chunk / on a chunk / page / split boundary for the 1100- and 1280-key sequences
REAL_WINDOWS = [(1000, 0), (63, 0), (1024, 37), (253, 0), (200, 0), (300, -1), (0, 0), (5, 1100)]


def _all_same(got, want, what):
    assert len(got) == len(want)
    for name, x, y in zip(NAMES, got, want):
        assert _same_bits(x, y), (what, name)


# ---- 1 and 3 on the packed entry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
@pytest.mark.parametrize("D,dtype,fmt", CFGS, ids=CFG_IDS)
def test_packed_no_window_is_the_sibling_and_a_window_is_the_paged_window_entry_on_each_slot_alone(D, dtype, fmt, page_size):
    for i, t in enumerate(P.shared_tables(page_size)):
        G, sq = V.qcase(page_size, i)
        Hq, cu, total = HKV * G, V.cu_of(sq), sum(sq)
        c = _cache(t, D, dtype, fmt, _pack(*_rows(t, D, fmt, 11 * D + i), fmt))
        q = _rand((total, Hq, D), dtype, 7 * D + i, mul=1.5)
        cud = _su(cu)
        real = REAL_WINDOWS[(i + page_size // 64) % len(REAL_WINDOWS)], REAL_WINDOWS[(i + 4 + page_size // 64 + D // 64) % len(REAL_WINDOWS)]
        for ns in (1, 3, 9):
            for precision in ("accurate", "fast"):
                kw = dict(precision=precision, num_splits=ns, **ALL)
                for causal, window in ((True, (-1, 0)), (False, (-1, -1))):
                    _all_same(_varlen(q, c, cud, max(sq), window=window, **kw), _varlen(q, c, cud, max(sq), is_causal=causal, **kw),
                              (t.lens, sq, ns, precision, window))
                for window in real:
                    got = _varlen(q, c, cud, max(sq), window=window, **kw)
                    for x in got[:4]:
                        assert not torch.isnan(x.float()).any(), (t.lens, sq, ns, precision, window)
                    for b in range(B):
                        if sq[b]:
                            _rows_equal(got, _dense_alone(q, c, cu, b, window=window, **kw), cu, b, Hq, D, (t.lens, G, sq, ns, precision, window))
                    if ns == 1 and precision == "fast":     # no LSE: the byte-exponential sweep
                        bare = _varlen(q, c, cud, max(sq), window=window, precision="fast", num_splits=1)
                        for b in range(B):
                            if sq[b]:
                                want = _dense_alone(q, c, cu, b, window=window, precision="fast", num_splits=1)
                                assert _same_bits(V.rows_of(bare, "o", cu, b), want), (t.lens, sq, b, window)
        # the public function is that call
        pub = qa.fp8_attn_paged_varlen_window_func(q, c, cud, max(sq), real[0], num_splits=3, return_lse=True, return_partials=True)
        raw = _varlen(q, c, cud, max(sq), window=real[0], num_splits=3, return_lse=True, return_partials=True)
        assert len(pub) == len(raw) == 5 and all(_same_bits(x, y) for x, y in zip(pub, raw))


# ---- 1 and 3 on the dense entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
@pytest.mark.parametrize("D,dtype,fmt", CFGS, ids=CFG_IDS)
def test_dense_no_window_is_the_sibling_and_paged_is_the_contiguous_window_entry_on_the_gathered_cache(D, dtype, fmt, page_size):
    names = ("out", "lse", "partial_o", "partial_lse", "partial_path", "row_path")
    for i, t in enumerate(P.shared_tables(page_size)):
        G, Sq = GS[(i + page_size // 64) % 4]
        c = _cache(t, D, dtype, fmt, _pack(*_rows(t, D, fmt, 11 * D + i), fmt))
        kv = _gathered(c, t.table, D)
        q = _rand((B, HKV * G, Sq, D), dtype, 7 * D + i, mul=1.5)
        su = c.seqlens
        real = REAL_WINDOWS[(i + page_size // 64) % len(REAL_WINDOWS)], REAL_WINDOWS[(i + 4 + page_size // 64 + D // 64) % len(REAL_WINDOWS)]
        for ns in (1, 3, 9):
            for precision in ("accurate", "fast"):
                kw = dict(precision=precision, num_splits=ns, return_lse=True, return_partials=True, return_path=True)
                for causal, window in ((True, (-1, 0)), (False, (-1, -1))):
                    for call in (lambda **k2: _paged(q, c, su, **k2), lambda **k2: _contig(q, kv, su, **k2)):
                        for name, x, y in zip(names, call(window=window, **kw), call(is_causal=causal, **kw)):
                            assert _same_bits(x, y), (t.lens, G, Sq, ns, precision, window, name)
                for window in real:
                    got, want = _paged(q, c, su, window=window, **kw), _contig(q, kv, su, window=window, **kw)
                    for name, x, y in zip(names, got, want):
                        assert _same_bits(x, y), (t.lens, G, Sq, ns, precision, window, name)
                    assert not torch.isnan(got[0].float()).any() and not torch.isnan(got[2]).any()
        # the public functions are those calls; num_splits = 0 picks the window rule's count on both
        for ns in (3, 0):
            pub = qa.fp8_attn_paged_window_func(q, c, real[0], num_splits=ns, return_lse=True, return_partials=True)
            ref = qa.fp8_attn_splitkv_window_func(q, kv, real[0], seqused_k=su, num_splits=ns, return_lse=True, return_partials=True)
            assert len(pub) == len(ref) == 5 and all(_same_bits(x, y) for x, y in zip(pub, ref))


# ---- 2: one split on contiguous prepared K / V = the FP8-PV window kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.bfloat16), (128, torch.float16), (256, torch.bfloat16)])
def test_one_split_with_hq_equal_hkv_gives_the_bits_of_the_fp8_pv_window_function(D, dtype):
    """every key used, so the prepared head-wise scales are that function's per-(sequence, head) scales; Sq 1 / 5 / 40 / 130 / 300 over
    1100 keys (a decode, part of a tile, more than two tiles) and Sq > Skv"""
    H = 2
    for Sq, Skv in ((1, 1100), (5, 1100), (40, 1100), (130, 1100), (300, 1100), (130, 65)):
        q = _rand((2, H, Sq, D), dtype, 3 * D + Sq, mul=1.5)
        k, v = _rand((2, H, Skv, D), dtype, 5 * D + Sq, mul=1.5), _rand((2, H, Skv, D), dtype, 7 * D + Sq)
        kv = qa.prepare_kv_fp8(k, v)
        for window in W.PROBE_WINDOWS + [(-1, -1), (5, 1100), (1000, 0)]:
            for precision in ("accurate", "fast"):
                out, lse = qa.fp8_attn_splitkv_window_func(q, kv, window, num_splits=1, precision=precision, return_lse=True)
                wo, wl = qa.fp8_window_attn_pv_func(q, k, v, window, pv_precision="fp8", precision=precision, return_lse=True)
                assert _same_bits(out, wo.contiguous()) and _same_bits(lse, wl.contiguous()), (D, Sq, Skv, window, precision)


# ---- 4: the merge ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [3, 9])
def test_out_and_lse_are_merge_attn_states_of_the_partials(ns):
    D, dtype, fmt, ps = 128, torch.bfloat16, "e4m3", 64
    t = P.shared_tables(ps)[3]
    G, sq = V.QCASES[2]
    c = _cache(t, D, dtype, fmt, _pack(*_rows(t, D, fmt, 41), fmt))
    qp = _rand((sum(sq), HKV * G, D), dtype, 42, mul=1.5)
    qd = _rand((B, HKV * G, 5, D), dtype, 43, mul=1.5)
    kv = _gathered(c, t.table, D)

    def merged(po, plse):
        parts_o, parts_l = list(po.unbind(0)), list(plse.unbind(0))
        if ns <= _native.MERGE_MAX_PARTIALS:
            return qa.merge_attn_states(parts_o, parts_l, out_dtype=dtype)
        mo, ml = qa.merge_attn_states(parts_o[:8], parts_l[:8], out_dtype=torch.float32)     # the entry's chain: 8, then 7 more through fp32
        return qa.merge_attn_states([mo] + parts_o[8:], [ml] + parts_l[8:], out_dtype=dtype)

    for window in ((1000, 0), (200, 0), (1024, 37)):
        for precision in ("accurate", "fast"):
            kw = dict(num_splits=ns, precision=precision, return_lse=True, return_partials=True)
            for res in (qa.fp8_attn_paged_varlen_window_func(qp, c, _su(V.cu_of(sq)), max(sq), window, **kw),
                        qa.fp8_attn_paged_window_func(qd, c, window, **kw),
                        qa.fp8_attn_splitkv_window_func(qd, kv, window, seqused_k=c.seqlens, **kw)):
                out, lse, po, plse, _ = res
                mo, ml = merged(po, plse)
                assert _same_bits(mo, out) and _same_bits(ml, lse), (window, precision)


# ---- the membership probes through all three entries ----------------------------------------------------------------------------------------------------
PROBE_PS, PROBE_SCALE = 128, 2.0 ** -8          # +-1, 0.5 and 0 over 2^-8 are exact in e4m3


def _probe_cache(case, D, dtype):
    """the case's keys and values appended to a paged cache behind a shuffled table (fixed power-of-two scales: every probe value exact)"""
    nB, M = len(case.alloc), CAP // PROBE_PS
    c = qa.alloc_paged_kv_cache_fp8(nB * M + 1, PR_HKV, PROBE_PS, D, batch_size=nB, max_pages_per_seq=M, scale_k=PROBE_SCALE, scale_v=PROBE_SCALE,
                                    dtype=dtype, device=DEV, fp8_format="e4m3")
    c.block_table.copy_(_su(np.random.RandomState(5).permutation(nB * M).reshape(nB, M) + 1))
    kn, vn = (torch.zeros(nB, PR_HKV, max(case.alloc), D, dtype=dtype, device=DEV) for _ in range(2))
    at = 0
    for b, a in enumerate(case.alloc):
        kn[b, :, :a], vn[b, :, :a] = T(case.k[at:at + a], dtype).transpose(0, 1), T(case.v[at:at + a], dtype).transpose(0, 1)
        at += a
    qa.paged_kv_cache_append_fp8(c, kn, vn, new_lens=_su(case.alloc))
    assert c.seqlens.tolist() == case.alloc
    return c, kn, vn


PR_HQ, PR_HKV = W.PROBE_HQ, W.PROBE_HKV


def _grade_probe(case, out, lse, dtype, what):
    """out [total_q, Hq, D], lse [Hq, total_q] against the case's fp64 reference: the count probe to REL ref, the others to the fp8-V bound"""
    ref, ref_lse = case.reference()
    if case.probe == "count":
        ls = []
        for s in case.seqs:
            Hq, _, n, _, D = s.dims
            tot = np.broadcast_to(PR.count_expected(s.mask, D)[1], (Hq, n))
            ls.append(PR.count_lse(deq_q(s.q[None], dtype, "e4m3", "head")[0], s.k[:, 0], tot) if n and s.m else np.full((Hq, n), -np.inf))
        ref_lse = np.concatenate(ls, 1)
    o = gpu_utils.out_to_f32(out)
    dead = np.isneginf(ref_lse).T
    assert (o[dead] == 0).all(), (what, "rows without a key must be exactly 0")
    r = count_ratio(o, ref, dtype, what) if case.probe == "count" else float((np.abs(o - ref) / PR.project_bound(ref, False)).max())
    return r, lse_ratio(lse.cpu().numpy(), ref_lse, W.LSE_TOL, what)


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("window", W.PROBE_WINDOWS, ids=[f"w{a}_{b}" for a, b in W.PROBE_WINDOWS])
def test_membership_probes_through_the_three_window_entries(D, window):
    """count / decoy / pointer probes (tests/test_cpu_splitkv_window.py shows their teeth on exactly these inputs): the packed entry on all
    four sequences at once, the paged and the contiguous entry on each sequence alone, three splits, precision accurate"""
    res = {}
    for probe in ("count", "decoy", "pointer"):
        dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[PR.WINDOW_COUNT_DTYPE[D]] if probe == "count" else torch.bfloat16
        case = W.probe_case(probe, D, window)
        c, kn, vn = _probe_cache(case, D, dtype)
        q = T(case.q, dtype)
        cu = V.cu_of(case.lq)
        kw = dict(num_splits=3, return_lse=True)
        out, lse = qa.fp8_attn_paged_varlen_window_func(q, c, _su(cu), max(case.lq), window, **kw)
        res[f"{probe} packed"], res[f"{probe} packed lse"] = _grade_probe(case, out, lse, dtype, f"{probe} packed")
        outs, lses, outs_c, lses_c = [], [], [], []
        for b, (n, m) in enumerate(zip(case.lq, case.alloc)):
            qb = V.alone(q, cu, b)
            o, l = qa.fp8_attn_paged_window_func(qb, V.one_slot(c, b), window, **kw)
            outs.append(o[0].transpose(0, 1))
            lses.append(l[0])
            o, l = qa.fp8_attn_splitkv_window_func(qb, (kn[b:b + 1, :, :m].contiguous(), vn[b:b + 1, :, :m].contiguous()), window, **kw)
            outs_c.append(o[0].transpose(0, 1))
            lses_c.append(l[0])
        res[f"{probe} paged"], res[f"{probe} paged lse"] = _grade_probe(case, torch.cat(outs), torch.cat(lses, 1), dtype, f"{probe} paged")
        res[f"{probe} contig"], res[f"{probe} contig lse"] = _grade_probe(case, torch.cat(outs_c), torch.cat(lses_c, 1), dtype, f"{probe} contig")
    print(f"window {window} D {D}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert all(v <= 1.0 for v in res.values()), res


# ---- the fp64 oracle ---------------------------------------------------------------------------------------------------------------------------------------
def _fp8_f64(bytes_u8, fmt):
    return torch.from_numpy(np.ascontiguousarray(bytes_u8)).view(P.FP8[fmt]).double()


@pytest.mark.parametrize("D,fmt", [(64, "e4m3"), (128, "e4m3"), (256, "e4m3"), (128, "e5m2")])
def test_gqa_three_splits_is_within_the_fp8_v_bound_of_the_fp64_windowed_softmax(D, fmt):
    """tests/splitkv_window_cases.ORACLE_CASES at GQA 4, page size 128: the lower edge inside a chunk, on a chunk, a page and a split
    boundary; per case the fp64 reference on the call's own q8 rows and on the pool's bytes looked up key by key through the table;
    bound gpu_utils.grade's, |got - ref| < 2^-6 max(1, |ref| / 2), LSE to 2e-3.  The window with more than 1024 keys (L = 1280, left 1100)
    cannot hold 1024 keys per split with three splits over 1280 keys, so it also runs with ONE split under precision="fast": the one-term
    sweep, asserted by its path bytes.  That run takes queries of unit variance: FAST is stated for score variance sm_scale^2 D <= 1
    (include/qattn_window.h; it has no rescue pass), and the keys here de-quantise to a standard deviation of scale_k <= 1 -- the 1.5x
    queries of the two-term runs would put the one-term sweep outside the domain it is stated for."""
    dtype, ps, G = torch.bfloat16, 128, 4
    Hq = HKV * G
    worst = worst_lse = 0.0
    for Sq, L, window, _ in W.ORACLE_CASES:
        t = P.Tables(ps, (L, L - 1, 0), seed=7)
        rk, rv = _rows(t, D, fmt, 5 + Sq)
        c = _cache(t, D, dtype, fmt, _pack(rk, rv, fmt), scale_k=torch.tensor([[0.5, 1.0], [0.75, 0.6], [1.0, 0.4]]))
        q, q_unit = _rand((B, Hq, Sq, D), dtype, 6 + Sq, mul=1.5), _rand((B, Hq, Sq, D), dtype, 6 + Sq)
        k8n, v8n = (P.gather_rows(r.cpu().numpy(), t.table, ps) for r in (rk, rv))            # [B, HKV, CAP, D] by the key-level lookup
        runs = [(3, "accurate"), (3, "fast")] + ([(1, "fast")] if window[0] >= 1024 else [])
        for ns, precision in runs:
            out, lse, q8, sqs, path = _paged(q if ns == 3 else q_unit, c, c.seqlens, window=window, precision=precision, num_splits=ns, return_lse=True, return_quant=True,
                                             return_path=True)
            if ns == 1:
                assert (path[0] == gpu_utils.PATH_ONE_TERM).all() and (path[1] == gpu_utils.PATH_ONE_TERM).all(), "the one-term sweep is reached"
            sk, sv = c.scale_k.double().cpu(), c.scale_v.double().cpu()
            dq = _fp8_f64(bits8(q8), fmt) * sqs.double().cpu()[..., None, None]
            for b, Lb in enumerate(t.lens):
                if Lb == 0:
                    assert (out[b] == 0).all() and torch.isneginf(lse[b]).all()
                    continue
                dk = _fp8_f64(k8n[b], fmt) * sk[b][:, None, None]
                dv = _fp8_f64(v8n[b], fmt) * sv[b][:, None, None]
                ro, rl, _, _, _, rpath = W.reference(dq[b].numpy(), dk.numpy(), dv.numpy(), Lb, window, ns, 1.0 / math.sqrt(D), precision)
                r_out = gpu_utils.grade(gpu_utils.out_to_f32(out[b])[None], ro[None])[2]
                r_lse = lse_ratio(lse[b].cpu().numpy(), rl, W.LSE_TOL, (Sq, L, window))
                worst, worst_lse = max(worst, r_out), max(worst_lse, r_lse)
                assert np.array_equal(path[b].cpu().numpy(), rpath), (Sq, Lb, window, ns, precision)
    print(f"window GQA 4 D{D} {fmt}: worst |err| / bound {worst:.3f}, worst LSE error / 2e-3 {worst_lse:.3f}")
    assert worst < 1.0 and worst_lse <= 1.0, (worst, worst_lse)


# ---- 5: dead bytes ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_size", P.PAGE_SIZES)
@pytest.mark.parametrize("D,fmt", [(64, "e4m3"), (128, "e4m3"), (256, "e4m3"), (128, "e5m2")])
def test_keys_below_the_window_and_table_entries_outside_its_pages_influence_no_bit(D, fmt, page_size):
    """hot: NaN bytes in K and V of EVERY key below lo_i = L_i - Sq_i - left (those in lo_i's own chunk and page included) and behind L_i,
    the table entries below lo_i // page_size and behind ceil(L_i / page_size) POISON or far out of range (they are never read: no address
    is formed from them).  cold: zeros there, and entry 0.  Every output bit is the same, and finite."""
    dtype, ps = torch.bfloat16, page_size
    for i, t in enumerate(P.shared_tables(ps)):
        G, sq = V.qcase(ps, i)
        Hq, cu, total = HKV * G, V.cu_of(sq), sum(sq)
        for window in ((1000, 0), (200, 37), (63, 0)):
            rk, rv = _rows(t, D, fmt, 13 * D + i)
            zk, zv = rk.clone(), rv.clone()
            hot_table, cold_table = t.table.copy(), t.zeroed.copy()
            shared_page = int(t.table[t.sharers[0], 0]) if t.shared else -1
            for b, L in enumerate(t.lens):
                lo = W.interval_lo(L, sq[b], window[0]) if sq[b] else L            # (an idle slot reads nothing)
                for j0, j1 in ((0, lo), (L, t.need[b] * ps)):
                    for pg in range(j0 // ps, -(-j1 // ps)):
                        page = int(t.table[b, pg])
                        if page == shared_page:
                            continue
                        a, e = max(j0 - pg * ps, 0), min(j1 - pg * ps, ps)
                        for r, z in ((rk, zk), (rv, zv)):
                            r[page, :, a:e] = P.NAN_BYTE[fmt]
                            z[page, :, a:e] = 0
                for pg in range(lo // ps):
                    hot_table[b, pg] = P.POISON if pg % 2 else 2 ** 30 + pg
                    cold_table[b, pg] = 0
                hot_table[b, t.need[b]:] = [P.POISON if pg % 2 else -(2 ** 30) - pg for pg in range(t.need[b], t.M)]
            hot = _cache(t, D, dtype, fmt, _pack(rk, rv, fmt), table=hot_table)
            cold = _cache(t, D, dtype, fmt, _pack(zk, zv, fmt), table=cold_table)
            q = _rand((total, Hq, D), dtype, 17 * D + i, mul=1.5)
            cud = _su(cu)
            for ns in (1, 3):
                for precision in ("accurate", "fast"):
                    kw = dict(num_splits=ns, precision=precision, return_lse=True, return_partials=True)
                    got = qa.fp8_attn_paged_varlen_window_func(q, hot, cud, max(sq), window, **kw)
                    want = qa.fp8_attn_paged_varlen_window_func(q, cold, cud, max(sq), window, **kw)
                    assert torch.isfinite(got[0].float()).all() and not torch.isnan(got[1]).any() and not torch.isnan(got[2]).any()
                    assert all(_same_bits(x, y) for x, y in zip(got, want)), (t.lens, sq, window, ns, precision)
                    for b in range(B):                        # ... and through the dense paged entry on each slot alone
                        if sq[b]:
                            a = qa.fp8_attn_paged_window_func(V.alone(q, cu, b), V.one_slot(hot, b), window, **kw)
                            z = qa.fp8_attn_paged_window_func(V.alone(q, cu, b), V.one_slot(cold, b), window, **kw)
                            assert all(_same_bits(x, y) for x, y in zip(a, z)), (t.lens, sq, b, window, ns, precision)


@pytest.mark.parametrize("D", [64, 128, 256])
def test_contiguous_keys_below_the_window_influence_no_bit(D):
    """the prepared row-major bytes below lo_b and behind L_b replaced by NaN bytes, then re-laid into the images: lo_b = 95 and 1003 leave
    dead keys inside lo_b's chunk (their V bytes must not reach the matrix pipe) and whole chunks below it (never read)"""
    Bn, Hq, Hkv, Sq, Skv = 2, 4, 2, 5, 1100
    used, window = [1100, 1036], (1000, 28)
    q, k, v = _rand((Bn, Hq, Sq, D), torch.bfloat16, D), _rand((Bn, Hkv, Skv, D), torch.bfloat16, D + 1), _rand((Bn, Hkv, Skv, D), torch.bfloat16, D + 2)
    k8, sk = _native.quant_fp8(k, scaling="head-wise")
    v8, sv = _native.quant_fp8(v, scaling="head-wise")
    su = _su(used)

    def run(fill, ns, precision):
        kb, vb = k8.clone().view(torch.uint8), v8.clone().view(torch.uint8)
        for b, L in enumerate(used):
            lo = W.interval_lo(L, Sq, window[0])
            for x in (kb, vb):
                x[b, :, :lo] = fill
                x[b, :, L:] = fill
        kf, vf = _native.pack_fp8(kb.view(k8.dtype), _native.LAYOUT_KFRAG), _native.pack_fp8(vb.view(v8.dtype), _native.LAYOUT_VFRAG)
        return _native.fp8_attention_splitkv(q, kf, vf, sk, sv, Skv=Skv, window=window, precision=precision, num_splits=ns, seqused_k=su,
                                             return_lse=True, return_partials=True)

    for ns in (1, 3):
        for precision in ("accurate", "fast"):
            hot, cold = run(0x7F, ns, precision), run(0, ns, precision)
            assert torch.isfinite(hot[0].float()).all()
            assert all(_same_bits(x, y) for x, y in zip(hot, cold)), (D, ns, precision)


# ---- one captured graph follows the moved window over freed pages -----------------------------------------------------------------------------------------
def test_one_captured_step_follows_the_window_after_seqlens_advanced_and_dead_pages_were_overwritten():
    """append 1 + attend under (127, 0), captured once; before every replay the pages paged_window_dead_pages names are overwritten with
    NaN bytes and their table entries with out-of-range values -- the allocator took them back -- in the graphed cache only"""
    D, dtype, fmt, ps, left = 128, torch.bfloat16, "e4m3", 64, 127
    lens0 = [ps - 3, 5, 1100]
    t = P.Tables(ps, lens0, seed=4, need=[4, 3, 20])
    pools = _pack(*_rows(t, D, fmt, 31, poison=False), fmt)
    mk = lambda: _cache(t, D, dtype, fmt, pools, lens=lens0)
    graphed, eager, warm = mk(), mk(), mk()
    attend = lambda q, c: qa.fp8_attn_paged_window_func(q, c, (left, 0), num_splits=2, max_seqlen_k=1280, return_lse=True)
    inputs = lambda s: (_rand((B, 8, 1, D), dtype, 700 + s), _rand((B, HKV, 1, D), dtype, 800 + s, mul=1.5), _rand((B, HKV, 1, D), dtype, 900 + s, mul=1.5))
    qs, ks, vs = (x.clone() for x in inputs(0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        qa.paged_kv_cache_append_fp8(warm, ks, vs)
        attend(qs, warm)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        qa.paged_kv_cache_append_fp8(graphed, ks, vs)
        out_s, lse_s = attend(qs, graphed)
    assert graphed.seqlens.tolist() == lens0                       # capture ran nothing
    freed = 0
    for s in range(70):                                            # the window moves across a page boundary of every slot that is long enough
        q, k, v = inputs(s)
        for dst, src in zip((qs, ks, vs), (q, k, v)):
            dst.copy_(src)
        # the allocator's view BEFORE the step: after the append the slot holds seqlens + 1 keys and attends with one query
        dead = qa.paged_window_dead_pages(graphed.seqlens + 1, left, ps, num_queries=1).tolist()
        for b in range(B):
            for pg in range(dead[b]):
                page = int(t.table[b, pg])
                graphed.k.view(graphed.num_pages, -1)[page] = P.NAN_BYTE[fmt]
                graphed.v.view(graphed.num_pages, -1)[page] = P.NAN_BYTE[fmt]
                graphed.block_table[b, pg] = 2 ** 30 + pg
                freed += 1
        graph.replay()
        torch.cuda.synchronize()
        qa.paged_kv_cache_append_fp8(eager, k, v)
        out, lse = attend(q, eager)
        assert graphed.seqlens.tolist() == eager.seqlens.tolist() == [n + s + 1 for n in lens0], s
        assert _same_bits(out_s, out) and _same_bits(lse_s, lse), s
        assert torch.isfinite(out_s.float()).all(), s
    assert dead == [(lens0[b] + 70 - 1 - left) // ps if lens0[b] + 70 - 1 - left > 0 else 0 for b in range(B)] and dead[2] == 16 and freed > 16 * 60


# ---- the library ops and torch.compile ---------------------------------------------------------------------------------------------------------------------
def test_the_library_ops_called_directly_are_the_functions():
    D, dtype, fmt, ps, window = 128, torch.bfloat16, "e4m3", 128, (200, 3)
    t = P.shared_tables(ps)[1]
    G, sq = V.QCASES[2]
    c = _cache(t, D, dtype, fmt, _pack(*_rows(t, D, fmt, 95), fmt))
    kv = _gathered(c, t.table, D)
    qp, qd = _rand((sum(sq), HKV * G, D), dtype, 98), _rand((B, HKV * G, 5, D), dtype, 99)
    cud = _su(V.cu_of(sq))
    kw = dict(num_splits=2, return_lse=True, return_partials=True)
    got = qa.ops.fp8_paged_varlen_splitkv_window_attention_forward(qp, c.k, c.v, c.scale_k, c.scale_v, c.block_table, c.seqlens, cud, max(sq), CAP,
                                                                   c.num_pages, ps, 2, 200, 3, fmt, "compiled", "accurate", True, True)
    want = qa.fp8_attn_paged_varlen_window_func(qp, c, cud, max(sq), window, **kw)
    assert len(got) == len(want) == 5 and all(_same_bits(x, y) for x, y in zip(got, want))
    got = qa.ops.fp8_paged_splitkv_window_attention_forward(qd, c.k, c.v, c.scale_k, c.scale_v, c.block_table, c.seqlens, CAP, c.num_pages, ps, 2, 200, 3,
                                                            fmt, "compiled", "accurate", True, True)
    want = qa.fp8_attn_paged_window_func(qd, c, window, **kw)
    assert len(got) == len(want) == 5 and all(_same_bits(x, y) for x, y in zip(got, want))
    got = qa.ops.fp8_splitkv_window_attention_forward(qd, kv.k, kv.v, kv.scale_k, kv.scale_v, c.seqlens, CAP, 2, 200, 3, fmt, "compiled", "accurate",
                                                      True, True)
    assert all(_same_bits(x, y) for x, y in zip(got, want))        # (paged = contiguous on the gathered cache)


def test_torch_compile_fullgraph_of_append_then_attend_under_a_window_gives_the_eager_bits():
    D, dtype, fmt, ps, T_ = 64, torch.float16, "e4m3", 64, 4
    t = P.Tables(ps, (CAP,) * B, seed=90, need=[CAP // ps] * B)
    pools = _pack(*_rows(t, D, fmt, 90), fmt)
    counts = (4, 1, 2)
    q, kn, vn = _rand((sum(counts), 4, D), dtype, 92), _rand((B, HKV, T_, D), dtype, 93), _rand((B, HKV, T_, D), dtype, 94)
    qd = _rand((B, 4, 2, D), dtype, 95)
    cud, nl = _su(V.cu_of(counts)), _su(counts)

    def packed(cache):
        def f(q, kn, vn, cu, nl):
            qa.paged_kv_cache_append_fp8(cache, kn, vn, new_lens=nl)
            return qa.fp8_attn_paged_varlen_window_func(q * 2, cache, cu, T_, (70, 0), num_splits=2, max_seqlen_k=256, return_lse=True)
        return f

    def dense(cache):
        def f(q, kn, vn, cu, nl):
            qa.paged_kv_cache_append_fp8(cache, kn, vn, new_lens=nl)
            return qa.fp8_attn_paged_window_func(q * 2, cache, (70, 0), num_splits=0, max_seqlen_k=256, return_lse=True)
        return f

    for step, query in ((packed, q), (dense, qd)):
        ca, cb = (_cache(t, D, dtype, fmt, pools, lens=[130, 63, 0]) for _ in range(2))
        torch._dynamo.reset()
        got = torch.compile(step(ca), fullgraph=True)(query, kn, vn, cud, nl)
        want = step(cb)(query, kn, vn, cud, nl)
        assert all(_same_bits(x, y) for x, y in zip(got, want))
        assert ca.seqlens.tolist() == cb.seqlens.tolist() == [134, 64, 2] and torch.equal(ca.k, cb.k) and torch.equal(ca.v, cb.v)
        assert not math.isnan(float(got[0].float().sum()))
    # the contiguous cache: append, then attend under a window
    k0, v0 = _rand((B, HKV, 130, D), dtype, 96), _rand((B, HKV, 130, D), dtype, 97)

    def contig(cache):
        def f(q, kn, vn):
            qa.kv_cache_append_fp8(cache, kn, vn)
            return qa.fp8_attn_splitkv_window_func(q * 2, cache, (70, 0), seqused_k=cache.seqlens, num_splits=2, return_lse=True)
        return f

    ca, cb = (qa.kv_cache_from_prefill_fp8(k0, v0, capacity=256) for _ in range(2))
    torch._dynamo.reset()
    got = torch.compile(contig(ca), fullgraph=True)(qd, kn, vn)
    want = contig(cb)(qd, kn, vn)
    assert all(_same_bits(x, y) for x, y in zip(got, want)) and ca.seqlens.tolist() == cb.seqlens.tolist() == [134] * B

"""Buffer contract of the lightning indexer's entries -- qattn_paged_mla_index_cache_append_fp8, qattn_fp8_mla_index_scores,
qattn_mla_index_select, qattn_fp8_mla_index_topk (include/qattn_mla_index.h), qattn_mla_index_select_split, qattn_fp8_mla_index_topk_split
(include/qattn_mla_index_split.h), qattn_fp8_mla_index_scores_varlen and qattn_fp8_mla_index_topk_varlen (include/qattn_mla_index_prefill.h)
-- held the way tests/test_gpu_mla_buffer_contract.py holds the latent-cache entries: ctypes calls on guarded arenas (tests/arena.py) of
EXACTLY the stated sizes at the stated alignments (pool, q16, k16, q8, workspace: 16 bytes; table, weights, logits, indices, kend, lengths,
scales: 4), and the five assertions of tests/test_gpu_buffer_contract.py's Plan.  The int32 outputs (indices, kend) are pre-filled with a
value no entry produces; logits behind wider strides keep their pads, and with fill_tail = 0 their tails.  The workspaces hold logits rows,
kend and histograms: 0xFF bytes there are NaN logits and huge counts, and change no bit."""
import numpy as np
import pytest
import torch

from quantumattention_amd import _native
from tests.test_gpu_buffer_contract import ALIGN4, _kind, _stream
from tests.test_gpu_mla_buffer_contract import (APPEND_NAMES, B, DEV, FP8, P0, MPlan, _caller, _gen, _i32, _ll, filled_pool, hold_append,
                                                padded_q)

pytestmark = pytest.mark.gpu

N = 700                                           # max_seqlen_k: no multiple of the 512-key range, the last range is partial
LENS = (0, 1, 300, N)
SQ = 2


@pytest.mark.parametrize("ps,dtype,fmt,with_new_lens,advance",
                         [(1, torch.bfloat16, "e4m3", True, 1), (16, torch.float16, "e5m2", False, 1), (64, torch.bfloat16, "e4m3", True, 0)],
                         ids=["ps1-new_lens", "ps16-fp16-e5m2-null", "ps64-no-advance"])
def test_paged_mla_index_cache_append_fp8(ps, dtype, fmt, with_new_lens, advance):
    hold_append("index", ps, dtype, fmt, with_new_lens, advance)


def _problem(ps, Hi, dtype, fmt, n=N, lens=LENS):
    """an index cache whose slot 3 owns the pool's last page (ps 1 and 70: its keys end in the pool's last row), q and weights"""
    pool, table, num_pages, scale = filled_pool("index", ps, lens, dtype, fmt, 9 * ps + Hi, owner=3, cap=n)
    g = _gen(ps + Hi)
    q = torch.randn(B, Hi, SQ, 128, generator=g).to(dtype).to(DEV)
    w = torch.randn(B, SQ, Hi, generator=g).to(DEV)
    return pool, table, num_pages, scale, q, w


def _inputs(p, ps, pool, table, scale, q, w, su):
    """carves the inputs every scoring entry shares; returns the leading arguments up to max_seqlen_k"""
    Hi, M = q.shape[1], table.shape[1]
    qs, wstr = padded_q(q.shape), (SQ * (Hi + 3) + 1, Hi + 3, 1)
    pq = p.inp_view("q16", q, qs, row_bytes=2 * 128)
    pw = p.inp_view("weights", w, wstr, row_bytes=4 * (Hi + 3), align=ALIGN4)
    pp = p.inp("pool", pool.view(-1), row_bytes=128)
    ptab, psc, psu = p.inp("block_table", table, align=ALIGN4), p.inp("scale", scale, align=ALIGN4), p.inp("seqused_k", su, align=ALIGN4)
    return (pq, _native.fmt_of(q.dtype), _ll(*qs[:3]), pw, _ll(*wstr[:2]), pp, ptab, M, table.shape[0] * M + 3, ps, M, psc, psu, B, Hi, SQ, N)


SCORE_CASES = [(1, 1, torch.bfloat16, "e4m3", True), (64, 4, torch.float16, "e5m2", False), (70, 64, torch.bfloat16, "e4m3", True)]
SCORE_IDS = ["ps1-h1-causal", "ps64-h4-fp16-e5m2", "ps70-h64-causal"]


@pytest.mark.parametrize("fill_tail", [1, 0], ids=["fill-tail", "leave-tail"])
@pytest.mark.parametrize("ps,Hi,dtype,fmt,causal", SCORE_CASES, ids=SCORE_IDS)
def test_fp8_mla_index_scores(ps, Hi, dtype, fmt, causal, fill_tail):
    L = _native.lib()
    pool, table, num_pages, scale, q, w = _problem(ps, Hi, dtype, fmt)
    su = _i32(LENS)
    _, wlog, wq8, wsq = _native.fp8_mla_index_topk(q, w, pool, scale, table, su, Skv=N, topk=8, num_pages=num_pages, page_size=ps,
                                                   fp8_dtype=FP8[fmt], is_causal=causal, return_q8=True, select=False)
    kend = torch.tensor([[max(Lb - SQ + i + 1, 0) if causal else Lb for i in range(SQ)] for Lb in LENS], device=DEV)
    below = torch.arange(N, device=DEV)[None, None, :] < kend[..., None]
    assert torch.isneginf(wlog[~below]).all() and torch.isfinite(wlog[below]).all()
    lstr = (SQ * (N + 9) + 5, N + 9, 1)
    view = lambda b: torch.as_strided(b.view(torch.float32), (B, SQ, N), lstr)
    if fill_tail:   # every logical element is written; the pads between the rows keep the pre-fill
        logical, want = (lambda b: view(b).contiguous().view(-1).view(torch.uint8)), wlog
    else:           # ... and so do the elements kend <= j < max_seqlen_k
        logical, want = (lambda b: view(b)[below].contiguous().view(torch.uint8)), wlog[below]
    p = MPlan()
    head = _inputs(p, ps, pool, table, scale, q, w, su)
    plog = p.out("logits", 4 * ((B - 1) * lstr[0] + (SQ - 1) * lstr[1] + N), "fp32", align=ALIGN4, row_bytes=4 * lstr[1], logical=logical)
    pq8 = p.out("q8", B * Hi * SQ * 128, "fp8", row_bytes=128)
    psq = p.out("scale_q", 4 * B * Hi * SQ, "fp32", align=ALIGN4)
    p.check(lambda: L.qattn_fp8_mla_index_scores(*head, _native.fmt_of(FP8[fmt]), int(causal), plog, _ll(*lstr[:2]), fill_tail, pq8, psq, _stream()),
            {"logits": want, "q8": wq8, "scale_q": wsq})


def _rows(n):
    """logits fp32 [2, SQ, n]: random rows with ties, and ONE all-equal row -- at n above QATTN_MLA_INDEX_LDS_CANDIDATES its threshold
    bin holds the whole row"""
    x = torch.randn(2, SQ, n, generator=_gen(n)).mul(4).round().div(4)
    x[0, 1] = 0.5
    return x.to(DEV)


SELECT_CASES = [(700, 70, (700, 700)), (700, 800, (700, 650)), (9000, 70, (9000, 50))]     # N, topk, seqused_k (kend <= topk: no logit is read)
SELECT_IDS = ["n700-k70", "n700-k800-above-kend", "n9000-k70-all-equal-row"]


@pytest.mark.parametrize("ns", [1, 2, 5], ids=["select", "split2", "split5"])
@pytest.mark.parametrize("n,topk,used", SELECT_CASES, ids=SELECT_IDS)
def test_mla_index_select_and_select_split(n, topk, used, ns):
    """ns = 1: qattn_mla_index_select; else qattn_mla_index_select_split, bit-equal to it whatever the workspace held"""
    L = _native.lib()
    assert n <= _native.MLA_INDEX_LDS_CANDIDATES or n == 9000
    x, su = _rows(n), _i32(used)
    want = _native.mla_index_select(x, su, topk, is_causal=True)
    assert (want[0, SQ - 1, :min(topk, n)] >= 0).all() and (want[..., min(topk, n):] == -1).all()
    lstr = (SQ * (n + 3) + 1, n + 3, 1)
    p = MPlan()
    plog = p.inp_view("logits", x, lstr, row_bytes=4 * lstr[1], align=ALIGN4)            # NaN in the pads and the guards
    psu = p.inp("seqused_k", su, align=ALIGN4)
    pidx = p.out("indices", 4 * 2 * SQ * topk, "int32", align=ALIGN4, row_bytes=4 * topk)
    if ns == 1:
        call = lambda: L.qattn_mla_index_select(plog, _ll(*lstr[:2]), psu, 2, SQ, n, topk, 1, pidx, _stream())
    else:
        wb = L.qattn_mla_index_select_split_workspace_bytes(2, SQ, n, ns)
        assert wb > 0
        pw = p.scratch("workspace", wb)
        call = lambda: L.qattn_mla_index_select_split(plog, _ll(*lstr[:2]), psu, 2, SQ, n, topk, 1, ns, pidx, pw, wb, _stream())
    p.check(call, {"indices": want})


@pytest.mark.parametrize("own_logits", [False, True], ids=["rows-in-workspace", "callers-logits"])
@pytest.mark.parametrize("ns", [1, 3], ids=["topk", "topk-split3"])
@pytest.mark.parametrize("ps,Hi,dtype,fmt,causal", SCORE_CASES[1:], ids=SCORE_IDS[1:])
def test_fp8_mla_index_topk_and_topk_split(ps, Hi, dtype, fmt, causal, ns, own_logits):
    """assertion d is the point: 0xFF bytes in the workspace are NaN logits behind every row's kend and counts nobody cleared"""
    L = _native.lib()
    topk = 70
    pool, table, num_pages, scale, q, w = _problem(ps, Hi, dtype, fmt)
    su = _i32(LENS)
    widx, wlog, wq8, wsq = _native.fp8_mla_index_topk(q, w, pool, scale, table, su, Skv=N, topk=topk, num_pages=num_pages, page_size=ps,
                                                      fp8_dtype=FP8[fmt], is_causal=causal, return_logits=True, return_q8=True, select_splits=1)
    p = MPlan()
    head = _inputs(p, ps, pool, table, scale, q, w, su)
    pidx = p.out("indices", 4 * B * SQ * topk, "int32", align=ALIGN4, row_bytes=4 * topk)
    pq8 = p.out("q8", B * Hi * SQ * 128, "fp8", row_bytes=128)
    psq = p.out("scale_q", 4 * B * Hi * SQ, "fp32", align=ALIGN4)
    expected = {"indices": widx, "q8": wq8, "scale_q": wsq}
    plog = None
    if own_logits:
        plog = p.out("logits", 4 * B * SQ * N, "fp32", align=ALIGN4, row_bytes=4 * N)
        expected["logits"] = wlog
    if ns == 1:
        wb = 0 if own_logits else L.qattn_fp8_mla_index_workspace_bytes(B, SQ, N)
        assert own_logits or wb >= 4 * B * SQ * N
    else:
        wb = L.qattn_fp8_mla_index_topk_split_workspace_bytes(B, SQ, N, ns, int(own_logits))
        assert wb == L.qattn_mla_index_select_split_workspace_bytes(B, SQ, N, ns) + (0 if own_logits else L.qattn_fp8_mla_index_workspace_bytes(B, SQ, N))
    pw = p.scratch("workspace", wb)
    tail = (pidx, plog, pq8, psq, pw, wb, _stream())
    if ns == 1:
        call = lambda: L.qattn_fp8_mla_index_topk(*head, topk, _native.fmt_of(FP8[fmt]), int(causal), *tail)
    else:
        call = lambda: L.qattn_fp8_mla_index_topk_split(*head, topk, _native.fmt_of(FP8[fmt]), int(causal), ns, *tail)
    p.check(call, expected)


# ------------------------------------------------------------------------------------------------------------- the packed entries
V_COUNTS = (11, 0, 5, 3)                          # no multiple of the 8-token tile; slot 1 idle; four more rows pad the bucket
V_TOTAL = sum(V_COUNTS) + 4
VARLEN_CASES = [(200, 8, 4, torch.bfloat16, "e4m3", True), (2200, 8, 64, torch.bfloat16, "e4m3", True), (2200, 64, 4, torch.float16, "e5m2", False)]
VARLEN_IDS = ["n200-ps8-h4-causal", "n2200-ps8-h64-causal", "n2200-ps64-h4-fp16-e5m2"]


def _packed(n, ps, Hi, dtype, fmt):
    lens = (n, 7, 2, min(n, 150))                 # slot 0 full: its keys end in the pool's last row (ps 8); slot 2: L_b = 2 < n_b = 5
    pool, table, num_pages, scale = filled_pool("index", ps, lens, dtype, fmt, 13 * ps + Hi, owner=0, cap=n)
    g = _gen(n + Hi)
    q = torch.randn(V_TOTAL, Hi, 128, generator=g).to(dtype).to(DEV)
    w = torch.randn(V_TOTAL, Hi, generator=g).to(DEV)
    return pool, table, num_pages, scale, q, w, _i32(lens), _i32(np.concatenate([[0], np.cumsum(V_COUNTS)]))


def _packed_inputs(p, n, ps, pool, table, scale, q, w, su, cu):
    Hi, M = q.shape[1], table.shape[1]
    qs, ws = padded_q(q.shape), Hi + 5
    pq = p.inp_view("q16", q, qs, row_bytes=2 * 128)
    pw = p.inp_view("weights", w, (ws, 1), row_bytes=4 * ws, align=ALIGN4)
    p.never_read(q, slice(sum(V_COUNTS), None))                                              # rows at or behind cu[B] are NOT read
    p.never_read(w, slice(sum(V_COUNTS), None))
    pp = p.inp("pool", pool.view(-1), row_bytes=128)
    ptab, psc, psu = p.inp("block_table", table, align=ALIGN4), p.inp("scale", scale, align=ALIGN4), p.inp("seqused_k", su, align=ALIGN4)
    pcu = p.inp("cu_seqlens_q", cu, align=ALIGN4)
    return (pq, _native.fmt_of(q.dtype), _ll(*qs[:2]), pw, ws, pp, ptab, M, B * M + 3, ps, M, psc, pcu, psu, B, Hi, V_TOTAL, n)


@pytest.mark.parametrize("fill_tail", [1, 0], ids=["fill-tail", "leave-tail"])
@pytest.mark.parametrize("n,ps,Hi,dtype,fmt,causal", VARLEN_CASES, ids=VARLEN_IDS)
def test_fp8_mla_index_scores_varlen(n, ps, Hi, dtype, fmt, causal, fill_tail):
    L = _native.lib()
    pool, table, num_pages, scale, q, w, su, cu = _packed(n, ps, Hi, dtype, fmt)
    _, wlog, wq8, wsq, wkend = _native.fp8_mla_index_topk_varlen(q, w, pool, scale, table, cu, su, Skv=n, topk=8, num_pages=num_pages, page_size=ps,
                                                                 fp8_dtype=FP8[fmt], is_causal=causal, return_q8=True, select=False)
    live = sum(V_COUNTS)
    assert not wkend[live:].any() and int(wkend[live - 1]) == min(n, 150) and (wkend[11:16] == _i32([0, 0, 0, 1, 2] if causal else [2] * 5)).all()
    ls = n + 11
    p = MPlan()
    head = _packed_inputs(p, n, ps, pool, table, scale, q, w, su, cu)
    view = lambda b: torch.as_strided(b.view(torch.float32), (V_TOTAL, n), (ls, 1))
    below = torch.arange(n, device=DEV)[None, :] < wkend[:, None]
    if fill_tail:
        logical, want = (lambda b: view(b).contiguous().view(-1).view(torch.uint8)), wlog
    else:           # the elements at and behind kend -- every element of a padded row -- keep the pre-fill
        logical, want = (lambda b: view(b)[below].contiguous().view(torch.uint8)), wlog[below]
    plog = p.out("logits", 4 * ((V_TOTAL - 1) * ls + n), "fp32", align=ALIGN4, row_bytes=4 * ls, logical=logical)
    pkend = p.out("kend", 4 * V_TOTAL, "int32", align=ALIGN4)                               # written for EVERY row, the padded ones included
    pq8 = p.out("q8", V_TOTAL * Hi * 128, "fp8", row_bytes=128)
    psq = p.out("scale_q", 4 * V_TOTAL * Hi, "fp32", align=ALIGN4)
    first = p.check(lambda: L.qattn_fp8_mla_index_scores_varlen(*head, _native.fmt_of(FP8[fmt]), int(causal), plog, ls, fill_tail, pkend, pq8, psq,
                                                                _stream()), {"logits": want, "kend": wkend, "q8": wq8, "scale_q": wsq})
    # the padded bucket: logits -inf (when filled), q8 and scale_q rows 0
    assert not fill_tail or torch.isneginf(first["logits"].view(torch.float32).view(V_TOTAL, n)[live:]).all()
    assert not first["q8"].view(V_TOTAL, -1)[live:].any() and not first["scale_q"].view(V_TOTAL, -1)[live:].any()


@pytest.mark.parametrize("own_logits", [False, True], ids=["rows-in-workspace", "callers-logits"])
@pytest.mark.parametrize("n,ps,Hi,dtype,fmt,causal", VARLEN_CASES, ids=VARLEN_IDS)
def test_fp8_mla_index_topk_varlen(n, ps, Hi, dtype, fmt, causal, own_logits):
    L = _native.lib()
    topk = 70
    pool, table, num_pages, scale, q, w, su, cu = _packed(n, ps, Hi, dtype, fmt)
    widx, wlog, wq8, wsq, wkend = _native.fp8_mla_index_topk_varlen(q, w, pool, scale, table, cu, su, Skv=n, topk=topk, num_pages=num_pages,
                                                                    page_size=ps, fp8_dtype=FP8[fmt], is_causal=causal, return_logits=True,
                                                                    return_q8=True)
    assert (widx[sum(V_COUNTS):] == -1).all() and (widx[0, :min(topk, int(wkend[0]))] >= 0).all()
    p = MPlan()
    head = _packed_inputs(p, n, ps, pool, table, scale, q, w, su, cu)
    pidx = p.out("indices", 4 * V_TOTAL * topk, "int32", align=ALIGN4, row_bytes=4 * topk)
    pq8 = p.out("q8", V_TOTAL * Hi * 128, "fp8", row_bytes=128)
    psq = p.out("scale_q", 4 * V_TOTAL * Hi, "fp32", align=ALIGN4)
    expected = {"indices": widx, "q8": wq8, "scale_q": wsq}
    plog = None
    kend_bytes = (4 * V_TOTAL + 255) // 256 * 256                                            # the header: kend rounded up to 256 bytes, then the rows
    if own_logits:
        plog = p.out("logits", 4 * V_TOTAL * n, "fp32", align=ALIGN4, row_bytes=4 * n)
        expected["logits"] = wlog
        wb = kend_bytes
    else:
        wb = L.qattn_fp8_mla_index_varlen_workspace_bytes(V_TOTAL, n)
        assert wb == kend_bytes + (4 * V_TOTAL * n + 255) // 256 * 256
    pw = p.scratch("workspace", wb)
    p.check(lambda: L.qattn_fp8_mla_index_topk_varlen(*head, topk, _native.fmt_of(FP8[fmt]), int(causal), pidx, plog, pq8, psq, pw, wb, _stream()),
            expected)
    ws = p.ar["workspace"].interior
    assert torch.equal(ws[:4 * V_TOTAL].view(torch.int32), wkend), "kend is the workspace's first section"
    if not own_logits:   # (the rows in the workspace get no tail fill: the selection reads no element at or behind kend)
        below = torch.arange(n, device=DEV)[None, :] < wkend[:, None]
        rows = ws[kend_bytes:kend_bytes + 4 * V_TOTAL * n].view(torch.int32).view(V_TOTAL, n)
        assert torch.equal(rows[below], wlog.view(torch.int32)[below]), "the logits rows follow kend's 256-byte section"


# --------------------------------------------------------------------------------------------------------------- the argument checks
SCORE_HEAD = ("q", "in_fmt", "qs", "w", "ws", "pool", "table", "tstride", "num_pages", "page", "max_pages", "scale", "used", "B", "Hi", "Sq", "N")
GOOD = dict(q=P0, in_fmt=_native.FMT_BF16, w=P0, pool=P0, table=P0, tstride=4, num_pages=9, page=16, max_pages=4, scale=P0, used=P0, B=2, Hi=4, Sq=1,
            N=64, fmt=_native.FMT_E4M3, causal=1)
SELECT_BAD = (dict(logits=None), dict(logits=P0 + 2), dict(idx=P0 + 2), dict(idx=None), dict(used=None), dict(ls=_ll(-64, 64)), dict(topk=0),
              dict(topk=2048 * 64 + 1), dict(N=0), dict(N=(1 << 30) + 1), dict(B=1 << 16, Sq=1 << 15), dict(Sq=0))


def test_the_argument_checks_of_qattn_mla_index_h_return_their_codes_before_any_launch():
    """what tests/test_cpu_mla_index.py leaves out.  Four of these entries take no workspace that could be withheld: EVERY call below
    breaks a documented rule."""
    L = _native.lib()
    app = _caller(L.qattn_paged_mla_index_cache_append_fp8, (APPEND_NAMES[0],) + APPEND_NAMES[2:4] + APPEND_NAMES[5:],
                  dict(ckv=P0, in_fmt=_native.FMT_BF16, cs=_ll(192, 192), pool=P0, scale=P0, table=P0, tstride=4, seqlens=P0, advance=1, B=2, T=3,
                       num_pages=9, page=16, max_pages=4, fmt=_native.FMT_E4M3))
    for kw in (dict(ckv=None), dict(ckv=P0 + 8), dict(pool=P0 + 8), dict(table=P0 + 2), dict(cs=_ll(196, 196)), dict(cs=_ll(192, -192)), dict(tstride=3),
               dict(page=0), dict(T=0), dict(num_pages=1 << 28, page=8), dict(max_pages=1 << 27, tstride=1 << 27)):
        assert app(**kw) == -1, kw
    assert app(fmt=_native.FMT_BF16) == -3
    scores = _caller(L.qattn_fp8_mla_index_scores, SCORE_HEAD + ("fmt", "causal", "logits", "ls", "fill", "q8", "sq", "stream"),
                     GOOD | dict(logits=P0, fill=1))
    for kw in (dict(q=None), dict(q=P0 + 8), dict(pool=P0 + 8), dict(q8=P0 + 8, sq=P0), dict(table=P0 + 2), dict(w=P0 + 2), dict(logits=P0 + 2),
               dict(logits=None), dict(qs=_ll(516, 132, 132)), dict(ws=_ll(-4, 4)), dict(ls=_ll(-64, 64)), dict(tstride=3), dict(Hi=65), dict(Hi=0),
               dict(N=65), dict(B=65536), dict(Sq=0)):
        assert scores(**kw) == -1, kw
    assert scores(fmt=_native.FMT_BF16) == -3
    select = _caller(L.qattn_mla_index_select, ("logits", "ls", "used", "B", "Sq", "N", "topk", "causal", "idx", "stream"),
                     dict(logits=P0, used=P0, B=2, Sq=1, N=64, topk=8, causal=1, idx=P0))
    for kw in SELECT_BAD:
        assert select(**kw) == -1, kw
    topk = _caller(L.qattn_fp8_mla_index_topk, SCORE_HEAD + ("topk", "fmt", "causal", "idx", "logits", "q8", "sq", "wsp", "wsb", "stream"),
                   GOOD | dict(topk=8, idx=P0, wsb=0))
    short = L.qattn_fp8_mla_index_workspace_bytes(2, 1, 64) - 1
    for kw in (dict(), dict(wsp=P0, wsb=short), dict(wsp=P0 + 8, wsb=short + 1), dict(idx=P0 + 2, logits=P0), dict(idx=None, logits=P0),
               dict(topk=2048 * 64 + 1), dict(topk=0), dict(logits=P0 + 2), dict(w=P0 + 2, logits=P0)):
        assert topk(**kw) == -1, kw


def test_the_argument_checks_of_qattn_mla_index_split_h_return_their_codes_before_any_launch():
    L = _native.lib()
    split = _caller(L.qattn_mla_index_select_split, ("logits", "ls", "used", "B", "Sq", "N", "topk", "causal", "ns", "idx", "wsp", "wsb", "stream"),
                    dict(logits=P0, used=P0, B=2, Sq=1, N=64, topk=8, causal=1, ns=2, idx=P0, wsb=0))
    short = L.qattn_mla_index_select_split_workspace_bytes(2, 1, 64, 2) - 1
    assert short > 0
    for kw in SELECT_BAD + (dict(), dict(wsp=P0, wsb=short), dict(wsp=P0 + 8, wsb=short + 1), dict(ns=0), dict(ns=257), dict(ns=1, N=0), dict(B=65536), dict(Sq=65536)):
        assert split(**kw) == -1, kw
    topk = _caller(L.qattn_fp8_mla_index_topk_split,
                   SCORE_HEAD + ("topk", "fmt", "causal", "ns", "idx", "logits", "q8", "sq", "wsp", "wsb", "stream"), GOOD | dict(topk=8, ns=2, idx=P0, wsb=0))
    own = L.qattn_fp8_mla_index_topk_split_workspace_bytes(2, 1, 64, 2, 1)
    assert 0 < own < L.qattn_fp8_mla_index_topk_split_workspace_bytes(2, 1, 64, 2, 0)
    for kw in (dict(), dict(logits=P0), dict(logits=P0, wsp=P0, wsb=own - 1), dict(wsp=P0, wsb=own), dict(logits=P0, wsp=P0 + 8, wsb=own),
               dict(ns=0, logits=P0), dict(ns=257, logits=P0), dict(idx=P0 + 2, logits=P0)):
        assert topk(**kw) == -1, kw


def test_the_argument_checks_of_qattn_mla_index_prefill_h_return_their_codes_before_any_launch():
    """beyond tests/test_cpu_mla_index_prefill.py: the 16-byte classes it leaves out (pool, q8), every 4-byte class, the stride rule"""
    L = _native.lib()
    names = ("q", "in_fmt", "qs", "w", "ws", "pool", "table", "tstride", "num_pages", "page", "max_pages", "scale", "cu", "used", "B", "Hi", "tq", "N")
    good = dict(q=P0, in_fmt=_native.FMT_BF16, w=P0, ws=0, pool=P0, table=P0, tstride=4, num_pages=9, page=16, max_pages=4, scale=P0, cu=P0, used=P0,
                B=2, Hi=4, tq=9, N=64, fmt=_native.FMT_E4M3, causal=1)
    scores = _caller(L.qattn_fp8_mla_index_scores_varlen, names + ("fmt", "causal", "logits", "ls", "fill", "kend", "q8", "sq", "stream"),
                     good | dict(logits=P0, ls=0, fill=1, kend=P0))
    for kw in (dict(pool=P0 + 8), dict(q8=P0 + 8, sq=P0), dict(table=P0 + 2), dict(w=P0 + 2), dict(logits=P0 + 2), dict(used=P0 + 2),
               dict(kend=P0 + 2), dict(q8=P0, sq=P0 + 2), dict(qs=_ll(516, 132)), dict(qs=_ll(-512, 128)), dict(tstride=3), dict(N=65),
               dict(tq=(1 << 31) - 65535)):
        assert scores(**kw) == -1, kw
    topk = _caller(L.qattn_fp8_mla_index_topk_varlen, names + ("topk", "fmt", "causal", "idx", "logits", "q8", "sq", "wsp", "wsb", "stream"),
                   good | dict(topk=8, idx=P0, wsb=0))
    full = L.qattn_fp8_mla_index_varlen_workspace_bytes(9, 64)
    for kw in (dict(wsp=P0, wsb=full - 1), dict(wsp=None, wsb=full), dict(pool=P0 + 8, wsp=P0, wsb=full), dict(idx=P0 + 2, wsp=P0, wsb=full),
               dict(logits=P0 + 2, wsp=P0, wsb=full)):
        assert topk(**kw) == -1, kw

"""Buffer contract of the latent-cache MLA entries -- qattn_paged_mla_cache_append_fp8, qattn_fp8_mla_paged_forward (include/qattn_mla.h),
qattn_paged_mla_row_cache_append_fp8, qattn_fp8_mla_paged_sparse_forward (include/qattn_mla_sparse.h) and
qattn_fp8_mla_paged_sparse_varlen_forward (include/qattn_mla_sparse_prefill.h) -- held the way tests/test_gpu_buffer_contract.py holds the
dense entries: the C entry through ctypes, every caller-provided buffer carved from a guarded arena (tests/arena.py) of EXACTLY the size the
header states at the alignment it states (pools, q16, ckv16, kpe16, out, q8, workspace: 16 bytes; tables, indices, lengths, scales, lse,
scale_q: 4).  After the call every guard is intact, every output is bit-equal to the ordinary `_native` call, nothing the contract says is
written is left unwritten, and no bit depends on what the workspace held or on bytes outside the inputs -- the pads of a strided q or index
view and the never-written (NaN) bytes of the pool included.  The appends: exactly the appended keys' bytes leave the pool's marker.
The helpers here also serve tests/test_gpu_mla_index_buffer_contract.py.  Every table entry, index and length is in range of the pool."""
import ctypes

import numpy as np
import pytest
import torch

from quantumattention_amd import _native
from tests import arena as A
from tests.test_gpu_buffer_contract import ALIGN4, ALIGN16, Plan, _kind, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, CAP = 4, 256
FP8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
NAN_BYTE = 0x7F                                   # NaN in both fp8 formats: what a never-written pool byte holds here
WIDTH = {"dense": 576, "row": 576, "index": 128}
SM_SCALE = 192.0 ** -0.5
COUNTS = (0, 1, 5, 3)                             # the packed tokens of the four slots; four more rows pad the bucket
TOTAL_Q = sum(COUNTS) + 4


class MPlan(Plan):
    """Plan with a strided input view at a chosen alignment (indices, weights: 4 bytes) and rows that are never read."""

    def __init__(self):
        super().__init__()
        self.dead = []

    def inp_view(self, name, t, strides, span=None, row_bytes=0, align=ALIGN16):
        span = _span(t.shape, strides) if span is None else span
        r = self.ar.carve(name, span * t.element_size(), align=align, row_bytes=row_bytes, role="in", kind=_kind(t.dtype))
        self.views.append((r, t, strides))
        r.load_view(t, strides, hostile=True)
        return r.ptr

    def never_read(self, t, rows):
        """rows of an input tensor INSIDE its interior that the contract says are not read: NaN (an int tensor: INT32_MIN) in the hostile
        runs, zero in the benign one"""
        self.dead.append((t, rows))

    def run(self, call, hostile, fill):
        for t, rows in self.dead:
            t[rows] = 0 if not hostile else float("nan") if t.is_floating_point() else torch.iinfo(t.dtype).min
        return super().run(call, hostile, fill)


def _i32(x):
    return torch.tensor(np.asarray(x), dtype=torch.int32, device=DEV)


def _ll(*v):
    return (ctypes.c_longlong * len(v))(*v)


def _span(shape, strides):
    """elements from the first to the last element of a view: the last row's last element ends the buffer"""
    return sum((n - 1) * s for n, s in zip(shape, strides)) + 1


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _table(M, num_pages, seed, owner, entry):
    """private shuffled pages [B, M]; table[owner][entry] is the pool's LAST page"""
    t = torch.randperm(num_pages - 1, generator=_gen(seed))[:B * M].view(B, M).to(torch.int32)
    t[owner, entry] = num_pages - 1
    return t


def _pool_bytes(kind, num_pages, ps):
    L = _native.lib()
    return {"dense": L.qattn_mla_pool_bytes, "row": L.qattn_mla_row_pool_bytes, "index": L.qattn_mla_index_pool_bytes}[kind](num_pages, ps)


def _new_pool(kind, num_pages, ps, fill):
    nb = _pool_bytes(kind, num_pages, ps)
    assert nb == num_pages * ps * WIDTH[kind]
    pool = torch.full((nb,), fill, dtype=torch.uint8, device=DEV)
    return pool if kind == "dense" else pool.view(num_pages, ps, WIDTH[kind])


def _append(kind, pool, scale, table, seqlens, x, **kw):
    """the ordinary append of x [B, T, W] (W = 576: the latent and the rotary slice of one projection)"""
    if kind == "index":
        return _native.paged_mla_index_cache_append_fp8(pool, scale, table, seqlens, x, **kw)
    f = _native.paged_mla_cache_append_fp8 if kind == "dense" else _native.paged_mla_row_cache_append_fp8
    return f(pool, scale, table, seqlens, x[..., :512], x[..., 512:], **kw)


def filled_pool(kind, ps, lens, dtype, fmt, seed, owner, cap=CAP):
    """(pool, table, num_pages, scale): slot b holds lens[b] random keys behind a shuffled table, every other byte is NaN; the last used
    page of slot `owner` is the pool's last page"""
    M = -(-cap // ps)
    num_pages = B * M + 3
    table = _table(M, num_pages, seed, owner, (max(lens[owner], 1) - 1) // ps).to(DEV)
    g = _gen(seed + 1)
    x = (torch.randn(B, max(max(lens), 1), WIDTH[kind], generator=g) * 1.5).to(dtype).to(DEV)
    scale = (torch.rand(B, generator=g) * 0.02 + 0.01).to(DEV)
    pool = _new_pool(kind, num_pages, ps, NAN_BYTE)
    _append(kind, pool, scale, table, torch.zeros(B, dtype=torch.int32, device=DEV), x, num_pages=num_pages, page_size=ps, fp8_dtype=FP8[fmt],
            new_lens=_i32(lens))
    return pool, table, num_pages, scale


def _chunk_index():
    """[64, 576] byte offsets of (key, channel) inside a 36 864-byte chunk: the formula of include/qattn_mla.h"""
    k, d = torch.arange(64).view(64, 1), torch.arange(576).view(1, 576)
    return ((((k >> 5) * 9 + (d >> 6)) << 11) + (((d >> 5) & 1) << 10) + (((d >> 4) & 1) << 9) + ((k & 31) << 4) + (d & 15)).to(DEV)


def pool_rows(kind, flat, num_pages, ps):
    """uint8 [num_pages ps, W]: row p ps + k = key k of page p, whatever the pool's layout"""
    if kind != "dense":
        return flat.view(num_pages * ps, WIDTH[kind])
    return flat.view(num_pages * (ps // 64), 36864)[:, _chunk_index()].reshape(num_pages * ps, 576)


# ---------------------------------------------------------------------------------------------------------------- the three appends
T_APPEND = 70
APPEND_LENS = [CAP - T_APPEND, 37, CAP - 26, 0]   # fills the pool's last page to its last row / starts mid-page / overflows: 26 of 70 stored
APPEND_NEW = [T_APPEND, 33, T_APPEND, 5]


def hold_append(kind, ps, dtype, fmt, with_new_lens, advance):
    L = _native.lib()
    W, M = WIDTH[kind], CAP // ps
    num_pages = B * M + 3
    table = _table(M, num_pages, 11 + ps, 0, M - 1)
    g = _gen(100 * ps + W)
    x = (torch.randn(B, T_APPEND, W, generator=g) * 3).to(dtype).to(DEV)
    scale = (torch.rand(B, generator=g) * 0.02 + 0.01).to(DEV)
    new = APPEND_NEW if with_new_lens else [T_APPEND] * B
    end = [min(p + n, CAP) for p, n in zip(APPEND_LENS, new)]
    assert end[0] == CAP and APPEND_LENS[2] + new[2] > CAP and (ps == 1 or APPEND_LENS[1] % ps != 0)
    # the inputs: slices of ONE wider projection [B, T, W + 64], rows and batches padded; its last row's last used element ends the buffer
    ts = W + 64
    strides = (T_APPEND * ts + 16, ts, 1)
    ar = A.Arena(DEV)
    rx = ar.carve("x16", 2 * _span(x.shape, strides), align=16, row_bytes=2 * ts, role="in", kind=_kind(dtype))
    rsc = ar.carve("scale", 4 * B, align=4, role="in", kind="fp32")
    rsc.load(scale)
    rtab = ar.carve("block_table", 4 * B * M, align=4, role="in", kind="int32")
    rtab.load(table.to(DEV))
    rnew = ar.carve("new_lens", 4 * B, align=4, role="in", kind="int32")
    rnew.load(_i32(new))
    rsl = ar.carve("seqlens", 4 * B, align=4, role="scratch")
    rpool = ar.carve("pool", _pool_bytes(kind, num_pages, ps), align=16, row_bytes=W, role="scratch")
    s2 = _ll(*strides[:2])
    mine = torch.zeros(num_pages * ps, dtype=torch.bool, device=DEV)
    for b in range(B):
        js = torch.arange(APPEND_LENS[b], end[b])
        mine[(table[b].long()[js // ps] * ps + js % ps).to(DEV)] = True
    assert mine[num_pages * ps - 1], "the append fills the pool's last row"
    tail = (rtab.ptr, M, rsl.ptr, rnew.ptr if with_new_lens else None, advance, B, T_APPEND, num_pages, ps, M, _native.fmt_of(FP8[fmt]), _stream())
    runs = []
    for hostile, fill in ((True, 0xA5), (False, NAN_BYTE)):
        ar.set_input_guards(hostile)
        rx.load_view(x, strides, hostile=hostile)
        rpool.fill(fill)
        rsl.interior.view(torch.int32).copy_(_i32(APPEND_LENS))
        if kind == "index":
            rc = L.qattn_paged_mla_index_cache_append_fp8(rx.ptr, _native.fmt_of(dtype), s2, rpool.ptr, rsc.ptr, *tail)
        else:
            f = L.qattn_paged_mla_cache_append_fp8 if kind == "dense" else L.qattn_paged_mla_row_cache_append_fp8
            rc = f(rx.ptr, rx.ptr + 2 * 512, _native.fmt_of(dtype), s2, s2, rpool.ptr, rsc.ptr, *tail)
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.qattn_strerror(rc))
        A.assert_guards_intact(ar)
        assert rsl.interior.view(torch.int32).tolist() == (end if advance else APPEND_LENS)
        rows = pool_rows(kind, rpool.interior, num_pages, ps)
        other = rows[~mine]
        assert (other == fill).all(), f"pool: {(other != fill).any(-1).sum().item()} keys the call does not append lost their pre-fill 0x{fill:02x}"
        runs.append(rows[mine].clone())
        # ... and the whole pool holds the bytes of the ordinary call (the binding on torch tensors) from the same starting state
        want = _new_pool(kind, num_pages, ps, fill)
        sl = _i32(APPEND_LENS)
        _append(kind, want, scale, table.to(DEV), sl, x, num_pages=num_pages, page_size=ps, fp8_dtype=FP8[fmt],
                new_lens=_i32(new) if with_new_lens else None, advance=bool(advance))
        assert torch.equal(want.view(-1), rpool.interior) and sl.tolist() == (end if advance else APPEND_LENS)
    assert torch.equal(runs[0], runs[1]), "an appended byte depends on what the pool, the guards or the pads held"
    assert (runs[0] != 0xA5).any(-1).all(), "every appended key left the marker"


APPEND_CASES = [(64, torch.bfloat16, "e4m3", True, 1), (64, torch.float16, "e5m2", False, 1), (128, torch.bfloat16, "e4m3", True, 0)]
APPEND_IDS = ["ps64-new_lens", "ps64-fp16-e5m2-null", "ps128-no-advance"]
ROW_APPEND_CASES = [(1, torch.bfloat16, "e4m3", True, 1), (16, torch.float16, "e5m2", False, 1), (64, torch.bfloat16, "e4m3", True, 0),
                    (64, torch.bfloat16, "e4m3", False, 1)]
ROW_APPEND_IDS = ["ps1-new_lens", "ps16-fp16-e5m2-null", "ps64-no-advance", "ps64-null"]


@pytest.mark.parametrize("ps,dtype,fmt,with_new_lens,advance", APPEND_CASES, ids=APPEND_IDS)
def test_paged_mla_cache_append_fp8(ps, dtype, fmt, with_new_lens, advance):
    hold_append("dense", ps, dtype, fmt, with_new_lens, advance)


@pytest.mark.parametrize("ps,dtype,fmt,with_new_lens,advance", ROW_APPEND_CASES, ids=ROW_APPEND_IDS)
def test_paged_mla_row_cache_append_fp8(ps, dtype, fmt, with_new_lens, advance):
    hold_append("row", ps, dtype, fmt, with_new_lens, advance)


# ------------------------------------------------------------------------------------------------------ qattn_fp8_mla_paged_forward
def padded_q(shape):
    """element strides of a [.., rows, W] view with 8 pad elements behind every row and 16 more behind every block of rows"""
    strides = [1]
    for i in range(len(shape) - 1, 0, -1):
        strides.insert(0, shape[i] * strides[0] + 8 * (len(shape) - i))
    return tuple(strides)


DENSE_LENS = (0, 1, 100, 200)                     # an empty slot; slot 3 ends mid-chunk in the pool's last page


@pytest.mark.parametrize("mode,ns", [("one", 1), ("workspace", 3), ("partials", 3)], ids=["ns1", "ns3-workspace", "ns3-partials"])
@pytest.mark.parametrize("Hq,Sq", [(20, 3), (128, 1)], ids=["h20-s3", "h128-s1"])
@pytest.mark.parametrize("ps,dtype,fmt,causal", [(64, torch.bfloat16, "e4m3", True), (128, torch.float16, "e5m2", False)],
                         ids=["ps64-bf16-e4m3-causal", "ps128-fp16-e5m2"])
def test_fp8_mla_paged_forward(ps, dtype, fmt, causal, Hq, Sq, mode, ns):
    L = _native.lib()
    pool, table, num_pages, scale = filled_pool("dense", ps, DENSE_LENS, dtype, fmt, 3 * ps + Hq, owner=3)
    M = table.shape[1]
    q = (torch.randn(B, Hq, Sq, 576, generator=_gen(Hq + Sq)) * 1.5).to(dtype).to(DEV)
    su = _i32(DENSE_LENS)
    parts = mode == "partials"
    wo, wl, wpo, wpl, wq8, wsq = _native.fp8_mla_paged_attention(q, pool, scale, table, su, Skv=CAP, num_pages=num_pages, page_size=ps,
                                                                 fp8_dtype=FP8[fmt], is_causal=causal, sm_scale=SM_SCALE, num_splits=ns,
                                                                 return_partials=parts, return_q8=True)
    rows = B * Hq * Sq
    p = MPlan()
    qs = padded_q(q.shape)
    pq = p.inp_view("q16", q, qs, row_bytes=2 * 576)
    pp = p.inp("pool", pool, row_bytes=576)
    ptab, psc, psu = p.inp("block_table", table, align=ALIGN4), p.inp("scale", scale, align=ALIGN4), p.inp("seqused_k", su, align=ALIGN4)
    po = p.out("out", 2 * rows * 512, _kind(dtype), row_bytes=2 * 512)
    pl = p.out("lse", 4 * rows, "fp32", align=ALIGN4)
    pq8 = p.out("q8", rows * 576, "fp8", row_bytes=576)
    psq = p.out("scale_q", 4 * rows, "fp32", align=ALIGN4)
    expected = {"out": wo, "lse": wl, "q8": wq8, "scale_q": wsq}
    ppo = ppl = None
    if parts:
        ppo = p.out("partial_o", 4 * ns * rows * 512, "fp32", row_bytes=4 * 512)
        ppl = p.out("partial_lse", 4 * ns * rows, "fp32", align=ALIGN4)
        expected.update(partial_o=wpo, partial_lse=wpl)
    wb = 0 if parts else L.qattn_fp8_mla_paged_workspace_bytes(B, Hq, Sq, ns)
    assert (wb == 0) == (mode != "workspace")
    pw = p.scratch("workspace", wb)
    p.check(lambda: L.qattn_fp8_mla_paged_forward(pq, _native.fmt_of(dtype), _ll(*qs[:3]), pp, ptab, M, num_pages, ps, M, psc, po, pl, psu, B, Hq, Sq,
                                                  CAP, _native.fmt_of(FP8[fmt]), int(causal), SM_SCALE, ns, pq8, psq, ppo, ppl, pw, wb, _stream()),
            expected)


# ----------------------------------------------------------------------------------------------- qattn_fp8_mla_paged_sparse_forward
SPARSE_LENS = (0, 1, 100, CAP)                    # slot 3 is full: its last key is the last row of the pool's last page


def draw_lists(shape, seed):
    """int32 lists over [-1, CAP): every row holds a -1, a duplicate, a position at or behind every limit but slot 3's, and CAP - 1"""
    idx = torch.randint(-1, CAP, shape, generator=_gen(seed), dtype=torch.int32)
    idx[..., 1], idx[..., 2], idx[..., 3], idx[..., -1] = -1, idx[..., 0], CAP - 1, CAP - 1
    return idx.to(DEV)


SPARSE_CASES = [   # page size, Hq, topk, ns, partials caller-provided, causal, dtype, format
    (1, 16, 70, 1, False, True, torch.bfloat16, "e4m3"),
    (16, 72, 70, 2, False, False, torch.bfloat16, "e4m3"),
    (64, 128, 70, 2, True, True, torch.float16, "e5m2"),
    (16, 128, 70, 1, False, False, torch.bfloat16, "e4m3"),
    (64, 16, 2112, 2, False, True, torch.bfloat16, "e4m3"),
    (1, 72, 2112, 2, True, False, torch.bfloat16, "e4m3"),
]
SPARSE_IDS = ["ps1-h16-k70-ns1-causal", "ps16-h72-k70-ns2", "ps64-h128-k70-ns2-partials-fp16-e5m2-causal", "ps16-h128-k70-ns1",
              "ps64-h16-k2112-ns2-causal", "ps1-h72-k2112-ns2-partials"]


@pytest.mark.parametrize("ps,Hq,topk,ns,parts,causal,dtype,fmt", SPARSE_CASES, ids=SPARSE_IDS)
def test_fp8_mla_paged_sparse_forward(ps, Hq, topk, ns, parts, causal, dtype, fmt):
    L = _native.lib()
    Sq = 2
    pool, table, num_pages, scale = filled_pool("row", ps, SPARSE_LENS, dtype, fmt, 5 * ps + Hq, owner=3)
    M = table.shape[1]
    q = (torch.randn(B, Hq, Sq, 576, generator=_gen(Hq + topk)) * 1.5).to(dtype).to(DEV)
    idx = draw_lists((B, Sq, topk), topk + ps)
    su = _i32(SPARSE_LENS)
    wo, wl, wpo, wpl, wq8, wsq = _native.fp8_mla_paged_sparse_attention(q, pool, scale, table, su, idx, num_pages=num_pages, page_size=ps,
                                                                        fp8_dtype=FP8[fmt], is_causal=causal, sm_scale=SM_SCALE, num_splits=ns,
                                                                        return_partials=parts, return_q8=True)
    rows = B * Hq * Sq
    p = MPlan()
    qs, istr = padded_q(q.shape), (Sq * (topk + 5) + 3, topk + 5, 1)
    pq = p.inp_view("q16", q, qs, row_bytes=2 * 576)
    pi = p.inp_view("indices", idx, istr, row_bytes=4 * (topk + 5), align=ALIGN4)           # INT32_MIN / INT32_MAX in the pads and guards
    pp = p.inp("pool", pool.view(-1), row_bytes=576)
    ptab, psc, psu = p.inp("block_table", table, align=ALIGN4), p.inp("scale", scale, align=ALIGN4), p.inp("seqused_k", su, align=ALIGN4)
    po = p.out("out", 2 * rows * 512, _kind(dtype), row_bytes=2 * 512)
    pl = p.out("lse", 4 * rows, "fp32", align=ALIGN4)
    pq8 = p.out("q8", rows * 576, "fp8", row_bytes=576)
    psq = p.out("scale_q", 4 * rows, "fp32", align=ALIGN4)
    expected = {"out": wo, "lse": wl, "q8": wq8, "scale_q": wsq}
    ppo = ppl = None
    if parts:
        ppo = p.out("partial_o", 4 * ns * rows * 512, "fp32", row_bytes=4 * 512)
        ppl = p.out("partial_lse", 4 * ns * rows, "fp32", align=ALIGN4)
        expected.update(partial_o=wpo, partial_lse=wpl)
    wb = 0 if parts else L.qattn_fp8_mla_paged_sparse_workspace_bytes(B, Hq, Sq, ns)
    assert (wb == 0) == (parts or ns == 1)
    pw = p.scratch("workspace", wb)
    first = p.check(lambda: L.qattn_fp8_mla_paged_sparse_forward(pq, _native.fmt_of(dtype), _ll(*qs[:3]), pp, ptab, M, num_pages, ps, M, psc, pi,
                                                                 _ll(*istr[:2]), topk, po, pl, psu, B, Hq, Sq, _native.fmt_of(FP8[fmt]), int(causal),
                                                                 SM_SCALE, ns, pq8, psq, ppo, ppl, pw, wb, _stream()), expected)
    lse = first["lse"].view(torch.float32).view(B, Hq, Sq)
    assert torch.isneginf(lse[0]).all() and torch.isfinite(lse[3, :, Sq - 1]).all()       # the empty slot; the full slot's last position


# ---------------------------------------------------------------------------------------- qattn_fp8_mla_paged_sparse_varlen_forward
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("ps,Hq,dtype,fmt", [(16, 16, torch.bfloat16, "e4m3"), (64, 128, torch.float16, "e5m2"), (1, 160, torch.bfloat16, "e4m3")],
                         ids=["ps16-h16", "ps64-h128-fp16-e5m2", "ps1-h160"])
def test_fp8_mla_paged_sparse_varlen_forward(ps, Hq, dtype, fmt, causal):
    """this entry takes NO workspace (its argument list has none): out, lse, q8 and scale_q are all it writes, the padded rows included"""
    L = _native.lib()
    topk, live = 70, sum(COUNTS)
    pool, table, num_pages, scale = filled_pool("row", ps, SPARSE_LENS, dtype, fmt, 7 * ps + Hq, owner=3)
    M = table.shape[1]
    q = (torch.randn(TOTAL_Q, Hq, 576, generator=_gen(Hq + 1)) * 1.5).to(dtype).to(DEV)
    idx = draw_lists((TOTAL_Q, topk), Hq + ps)
    su, cu = _i32(SPARSE_LENS), _i32(np.concatenate([[0], np.cumsum(COUNTS)]))
    wo, wl, wq8, wsq = _native.fp8_mla_paged_sparse_varlen_attention(q, pool, scale, table, su, idx, cu, num_pages=num_pages, page_size=ps,
                                                                     fp8_dtype=FP8[fmt], is_causal=causal, sm_scale=SM_SCALE, return_q8=True)
    p = MPlan()
    qs, istr = padded_q(q.shape), (topk + 7, 1)
    pq = p.inp_view("q16", q, qs, row_bytes=2 * 576)
    pi = p.inp_view("indices", idx, istr, row_bytes=4 * istr[0], align=ALIGN4)
    p.never_read(q, slice(live, None))                                                       # the padded bucket: neither q nor its list is read
    p.never_read(idx, slice(live, None))
    pp = p.inp("pool", pool.view(-1), row_bytes=576)
    ptab, psc, psu = p.inp("block_table", table, align=ALIGN4), p.inp("scale", scale, align=ALIGN4), p.inp("seqused_k", su, align=ALIGN4)
    pcu = p.inp("cu_seqlens_q", cu, align=ALIGN4)
    po = p.out("out", 2 * TOTAL_Q * Hq * 512, _kind(dtype), row_bytes=2 * 512)
    pl = p.out("lse", 4 * Hq * TOTAL_Q, "fp32", align=ALIGN4)
    pq8 = p.out("q8", TOTAL_Q * Hq * 576, "fp8", row_bytes=576)
    psq = p.out("scale_q", 4 * TOTAL_Q * Hq, "fp32", align=ALIGN4)
    first = p.check(lambda: L.qattn_fp8_mla_paged_sparse_varlen_forward(pq, _native.fmt_of(dtype), _ll(*qs[:2]), pp, ptab, M, num_pages, ps, M, psc, pi,
                                                                        istr[0], topk, pcu, po, pl, psu, B, TOTAL_Q, Hq, _native.fmt_of(FP8[fmt]),
                                                                        int(causal), SM_SCALE, pq8, psq, _stream()),
                    {"out": wo, "lse": wl, "q8": wq8, "scale_q": wsq})
    # the padded bucket: zero rows, LSE -inf, q8 and scale_q zero
    assert not first["out"].view(TOTAL_Q, -1)[live:].any() and not first["q8"].view(TOTAL_Q, -1)[live:].any()
    assert not first["scale_q"].view(TOTAL_Q, -1)[live:].any()
    assert torch.isneginf(first["lse"].view(torch.float32).view(Hq, TOTAL_Q)[:, live:]).all()
    assert torch.isfinite(first["lse"].view(torch.float32).view(Hq, TOTAL_Q)[:, live - 1]).all()   # slot 3's last token sees all its keys


# --------------------------------------------------------------------------------------------------------------- the argument checks
def _caller(f, names, good):
    assert len(names) == len(f.argtypes), (len(names), len(f.argtypes))
    base = dict.fromkeys(names) | good
    return lambda **kw: f(*(base | kw).values())


P0 = 0x1000   # a 16-byte-aligned address that is never dereferenced: every call below fails a check first

APPEND_NAMES = ("ckv", "kpe", "in_fmt", "cs", "ks", "pool", "scale", "table", "tstride", "seqlens", "new_lens", "advance", "B", "T", "num_pages",
                "page", "max_pages", "fmt", "stream")
FWD_NAMES = ("q", "in_fmt", "qs", "pool", "table", "tstride", "num_pages", "page", "max_pages", "scale", "out", "lse", "used", "B", "Hq", "Sq", "Skv",
             "fmt", "causal", "sm", "ns", "q8", "sq", "po", "pl", "ws", "wsb", "stream")
SPARSE_NAMES = FWD_NAMES[:10] + ("idx", "istr", "topk") + FWD_NAMES[10:16] + FWD_NAMES[17:]
VARLEN_NAMES = ("q", "in_fmt", "qs", "pool", "table", "tstride", "num_pages", "page", "max_pages", "scale", "idx", "istride", "topk", "cu", "out",
                "lse", "used", "B", "tq", "Hq", "fmt", "causal", "sm", "q8", "sq", "stream")


def test_the_argument_checks_of_qattn_mla_h_return_their_codes_before_any_launch():
    """what tests/test_cpu_mla.py leaves out: the alignment of every pointer class, the stride rule, table_stride, a short workspace.  The
    forward calls carry no workspace, so a call that passed every other check would still return before any device call."""
    L = _native.lib()
    app = _caller(L.qattn_paged_mla_cache_append_fp8, APPEND_NAMES,
                  dict(ckv=P0, kpe=P0, in_fmt=_native.FMT_BF16, cs=_ll(640, 640), ks=_ll(640, 640), pool=P0, scale=P0, table=P0, tstride=4, seqlens=P0,
                       advance=1, B=2, T=3, num_pages=9, page=64, max_pages=4, fmt=_native.FMT_E4M3))
    INVALID = app(ckv=None)
    assert INVALID == -1
    for kw in (dict(ckv=P0 + 8), dict(kpe=P0 + 8), dict(pool=P0 + 8), dict(table=P0 + 2), dict(cs=_ll(644, 644)), dict(ks=_ll(640, 68)), dict(cs=_ll(-640, 640)), dict(tstride=3), dict(page=96),
               dict(T=0), dict(pool=None), dict(seqlens=None)):
        assert app(**kw) == INVALID, kw
    assert app(fmt=_native.FMT_BF16) == -3 and app(in_fmt=_native.FMT_E4M3) == -3
    fwd = _caller(L.qattn_fp8_mla_paged_forward, FWD_NAMES,
                  dict(q=P0, in_fmt=_native.FMT_BF16, pool=P0, table=P0, tstride=4, num_pages=9, page=64, max_pages=4, scale=P0, out=P0, lse=P0, used=P0,
                       B=2, Hq=16, Sq=1, Skv=256, fmt=_native.FMT_E4M3, causal=1, sm=0.07, ns=2, wsb=0))
    short = L.qattn_fp8_mla_paged_workspace_bytes(2, 16, 1, 2) - 1
    for kw in (dict(q=P0 + 8), dict(pool=P0 + 8), dict(out=P0 + 8), dict(q8=P0 + 8, sq=P0), dict(table=P0 + 2),
               dict(qs=_ll(16 * 580, 580, 580)), dict(qs=_ll(-9216, 576, 576)),
               dict(tstride=3), dict(ns=65), dict(sm=0.0), dict(Skv=257), dict(page=32),
               dict(), dict(ws=P0, wsb=short), dict(ws=P0 + 8, wsb=short + 1)):
        assert fwd(**kw) == INVALID, kw
    assert fwd(fmt=_native.FMT_FP16) == -3


def test_the_argument_checks_of_qattn_mla_sparse_h_return_their_codes_before_any_launch():
    """beyond tests/test_cpu_mla_sparse.py: alignment classes, the stride rule, table_stride, topk above QATTN_MLA_SPARSE_MAX_TOPK,
    num_splits below ceil(topk / 2048), a short workspace"""
    L = _native.lib()
    app = _caller(L.qattn_paged_mla_row_cache_append_fp8, APPEND_NAMES,
                  dict(ckv=P0, kpe=P0, in_fmt=_native.FMT_BF16, cs=_ll(640, 640), ks=_ll(640, 640), pool=P0, scale=P0, table=P0, tstride=4, seqlens=P0,
                       advance=1, B=2, T=3, num_pages=9, page=16, max_pages=4, fmt=_native.FMT_E4M3))
    INVALID = app(ckv=None)
    assert INVALID == -1
    for kw in (dict(ckv=P0 + 8), dict(kpe=P0 + 8), dict(pool=P0 + 8), dict(table=P0 + 2), dict(cs=_ll(644, 644)), dict(ks=_ll(640, 68)),
               dict(tstride=3), dict(page=0), dict(num_pages=1 << 28, page=8), dict(max_pages=1 << 27, tstride=1 << 27)):
        assert app(**kw) == INVALID, kw
    fwd = _caller(L.qattn_fp8_mla_paged_sparse_forward, SPARSE_NAMES,
                  dict(q=P0, in_fmt=_native.FMT_BF16, pool=P0, table=P0, tstride=4, num_pages=9, page=16, max_pages=4, scale=P0, idx=P0, topk=70,
                       out=P0, lse=P0, used=P0, B=2, Hq=16, Sq=1, fmt=_native.FMT_E4M3, causal=1, sm=0.07, ns=2, wsb=0))
    short = L.qattn_fp8_mla_paged_sparse_workspace_bytes(2, 16, 1, 2) - 1
    for kw in (dict(q=P0 + 8), dict(pool=P0 + 8), dict(out=P0 + 8), dict(q8=P0 + 8, sq=P0), dict(table=P0 + 2), dict(idx=P0 + 2), dict(idx=None),
               dict(qs=_ll(16 * 580, 580, 580)), dict(istr=_ll(-70, 70)), dict(tstride=3), dict(topk=2048 * 64 + 1), dict(topk=0),
               dict(topk=2049, ns=1), dict(topk=4097, ns=2), dict(ns=65), dict(sm=float("inf")),
               dict(), dict(ws=P0, wsb=short), dict(ws=P0 + 8, wsb=short + 1)):
        assert fwd(**kw) == INVALID, kw
    assert fwd(fmt=_native.FMT_FP16) == -3


def test_the_argument_checks_of_qattn_mla_sparse_prefill_h_return_their_codes_before_any_launch():
    """this entry has no workspace to withhold: EVERY call here breaks a documented rule (tests/test_cpu_mla_sparse_prefill.py holds the
    Python-side reasons)"""
    L = _native.lib()
    call = _caller(L.qattn_fp8_mla_paged_sparse_varlen_forward, VARLEN_NAMES,
                   dict(q=P0, in_fmt=_native.FMT_BF16, pool=P0, table=P0, tstride=4, num_pages=9, page=16, max_pages=4, scale=P0, idx=P0, istride=70,
                        topk=70, cu=P0, out=P0, lse=P0, used=P0, B=2, tq=5, Hq=16, fmt=_native.FMT_E4M3, causal=1, sm=0.07))
    for kw in (dict(q=None), dict(q=P0 + 8), dict(pool=P0 + 8), dict(out=P0 + 8), dict(q8=P0 + 8, sq=P0), dict(table=P0 + 2), dict(idx=P0 + 2),
               dict(cu=P0 + 2), dict(cu=None), dict(qs=_ll(16 * 580, 580)), dict(qs=_ll(-9216, 576)), dict(istride=-1), dict(tstride=3),
               dict(topk=2048 * 64 + 1), dict(topk=0), dict(Hq=0), dict(tq=0), dict(B=0), dict(sm=0.0), dict(page=0),
               dict(num_pages=1 << 28, page=8)):
        assert call(**kw) == -1, kw
    assert call(fmt=_native.FMT_FP16) == -3 and call(in_fmt=_native.FMT_E4M3) == -3

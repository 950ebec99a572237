"""-m gpu: the scale ladder of tests/scale_ladder.py through the FP8-PV family on the MI355X ("Scale ladder for the FP8-PV and
split-KV entries"): the three FP8-P.V siblings (block-sparse, packed, window), split-KV over prepared K / V, the fixed-scale cache, the paged
cache and packed queries over the paged cache -- WHICH scale_q, scale_k and scale_v, of which batch entry / sequence slot, kv head and
query head of a GQA group, each of them applies to each row.

tests/test_cpu_scale_ladder_fp8pv.py shows, on the very cases and used lengths below, that every named mis-indexing moves the reference
by >= 4 x the bound applied here -- among them the two the per-lane `g` of the split-KV kernels invites (a 128-row tile packs the rows of
the G query heads of a kv head), which only `group_ladder` reaches.  The checks are those of tests/test_gpu_scale_ladder.py, none loosened:
1. oracle grading: every row against the fp64 masked softmax on the CPU quantiser's output (never on a scale a GPU call returned), with
   tests/gpu_utils.grade at the fp8-V bound; the LSE within LSE_TOL of tests/splitkv_cases.py; row_path the literal table of that file;
2. quantiser echo: the bytes an entry returns / prepares are the CPU quantiser's and those of the call without gains, every scale
   exactly 2^e times the plain one;
3. exact equivariance, no oracle: e only (f = 0) -- every output is the plain call's bit for bit; V head ladder -- out = 2^e x the plain out
   bit for bit, lse and paths equal;
4. the bit-for-bit chain on ladder inputs with G = 2: cache = paged cache = prepared K / V; a packed sequence = the dense paged call on it.
Each test prints worst |err| / bound."""
import functools

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import paged_cases as PC
from tests import paged_varlen_cases as V
from tests import scale_ladder as L
from tests import splitkv_cases as S
from tests.gpu_utils import TDT, bits8, out_to_f32, unpack_frag
from tests.scale_ladder import B, HKV, HQ
from tests.test_gpu_scale_ladder import G, Log, pack
from tests.test_gpu_varlen_fp8 import _image

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = ("accurate", "fast")
LSE_TOL = S.LSE_TOL
IDS = [L.case_id(c) for c in L.FP8PV_CASES]
PACKED_IDS = [f"D{c[0]}_S{c[1]}_{L.NAME[c[2]]}_{c[3]}" for c in L.PACKED_CASES]
KINDS = ("head", "vhead", "group")
PAGE_SIZES = (64, 128)
LADDERS = {
    "head": L.head_ladder_plain_v,                                   # e and f on q and k, the plain V
    "vhead": lambda *a: L.head_ladder(*a, v_head=True),              # ... with V x 2^E_VHEAD
    "group": L.group_ladder,                                         # sparse / dense heads inside a GQA group, e on q and k
    "plain": lambda *a: L.head_ladder(*a, gains=False),              # the head ladder's codes without any gain
    "e only": lambda *a: L.head_ladder(*a, f=False),                 # e on q and k, the plain V
    "plain + V head": lambda *a: L.head_ladder(*a, gains=False, v_head=True),
    "group, plain": lambda *a: L.group_ladder(*a, gains=False),      # the group ladder's codes with e = 0
}
GAIN_V = np.exp2(L.E_VHEAD)[:, L.kv_of(), None, None]               # [B, HQ, 1, 1]


def tensors(kind, D, Sq, Skv, dtype):
    return G(*LADDERS[kind](D, Sq, Skv).tensors(dtype))


@functools.lru_cache(maxsize=None)
def reference(kind, D, Sq, Skv, causal, dtype, fp8, sq=None):
    """(ladder, the CPU quantiser's output, ref out [B, HQ, Sq, D], ref lse [B, HQ, Sq]) at the used lengths -- computed once per case, shared,
    left unchanged.  sq: queries per batch entry (packed queries; default Sq)"""
    lad = LADDERS[kind](D, Sq, Skv)
    qz = L.quantise(lad, dtype, fp8, "head", v_block=False)
    out, lse = L.UsedScores(qz, L.used_mask(Sq, Skv, L.used_lengths(Skv), causal, sq)).softmax()
    return lad, qz, out, lse


def same_bits(x, y):
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(view[x.element_size()]), y.contiguous().view(view[y.element_size()]))


def all_same(got, want, what, names=None):
    assert len(got) == len(want), what
    for i, (x, y) in enumerate(zip(got, want)):
        assert same_bits(x, y), (what, names[i] if names else i, "must be equal bit for bit")


def scaled_by_the_v_gain(out, base, dtype, what, gain=GAIN_V):
    """out = 2^e x base bit for bit; fp16 elements whose plain or scaled value lies below the smallest normal number were rounded on the
    subnormal grid once before the gain and once after it: held to that grid (tests/test_gpu_scale_ladder.py)"""
    out, base = (x if isinstance(x, np.ndarray) else out_to_f32(x) for x in (out, base))
    tiny = float(torch.finfo(dtype).tiny)
    sub = tiny * float(torch.finfo(dtype).eps)
    want = base * gain
    normal = (np.abs(want) >= tiny) & (np.abs(base) >= tiny)
    assert np.array_equal(out[normal], want[normal]), (what, "V head ladder: out = 2^e x the plain output")
    assert (np.abs(out - want) <= np.maximum(1.0, gain) * sub).all(), (what, "V head ladder: subnormal elements")


def same_outputs(got, want, idx, what):
    """the outputs idx of two eight-output calls (NAMES), bit for bit; an output neither call returned is None in both"""
    for i in idx:
        if got[i] is None or want[i] is None:
            assert got[i] is None and want[i] is None, (what, NAMES[i])
        else:
            assert same_bits(got[i], want[i]), (what, NAMES[i], "must be equal bit for bit")


NAMES = ("out", "lse", "partial_o", "partial_lse", "partial_path", "q8", "scale_q", "row_path")
E_ONLY_SAME = (0, 1, 2, 3, 4, 5, 7)      # e only: everything but scale_q
V_HEAD_SAME = (1, 3, 4, 5, 6, 7)         # V head ladder: everything but out and partial_o, which are 2^e x the plain ones


def su(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def heads_of(lad, which):
    """indices of the sparse / dense query heads of the group ladder"""
    return np.nonzero(lad.sparse if which == "sparse" else ~lad.sparse)[0]


# ---- (b) split-KV over prepare_kv_fp8 -------------------------------------------------------------------------------------------------------------
def splitkv(q, kv, used, causal, ns, precision, lse=True):
    """(out, lse | None, partial_o, partial_lse, partial_path, q8, scale_q, row_path) through the C entry"""
    res = _native.fp8_attention_splitkv(q, kv.k, kv.v, kv.scale_k, kv.scale_v, Skv=kv.shape[2], fp8_dtype=TDT[kv.fp8_format], numerics=kv.numerics,
                                        is_causal=causal, precision=precision, num_splits=ns, seqused_k=su(used), return_lse=lse, return_partials=True,
                                        return_quant=True, return_path=True)
    return res if lse else (res[0], None) + tuple(res[1:])


def check_prepared(kv, qz, what):
    """the prepared images and scales are the CPU quantiser's"""
    Bk, Hkv, Skv, D = kv.shape
    for img, s, layout, b8, sc in ((kv.k, kv.scale_k, _native.LAYOUT_KFRAG, qz.k8, qz.sk), (kv.v, kv.scale_v, _native.LAYOUT_VFRAG, qz.v8, qz.sv)):
        got = unpack_frag(img.cpu().numpy(), layout, Bk, Hkv, Skv, D)
        assert np.array_equal(got[:, :, :Skv], b8) and not got[:, :, Skv:].any(), (what, "prepared image")
        assert np.array_equal(s.cpu().numpy(), sc), (what, "prepared scale")


def grade_splitkv(log, res, qz, ref, ref_lse, used, Sq, causal, ns, precision):
    out, lse, q8, sq, path = res[0], res[1], res[5], res[6], res[7]
    assert np.array_equal(bits8(q8), qz.q8) and np.array_equal(sq.cpu().numpy(), qz.sq), (log.what, "q8 / scale_q: the CPU quantiser's")
    assert np.array_equal(path.cpu().numpy(), S.expected_row_path(used, HQ, HKV, Sq, ns, causal, precision)), (log.what, ns, precision, "row_path")
    log.out(out_to_f32(out), ref)
    if lse is not None:
        log.lse_err(lse.cpu().numpy(), ref_lse, LSE_TOL)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", L.FP8PV_CASES, ids=IDS)
def test_split_kv_on_the_ladders(case, kind):
    """every head under both precisions.  The group ladder's sparse heads put their scores on a lattice of a few values, the input the
    one-term sweep is least exact on (docs/ISSUE_one_term_sweep_on_lattice_scores.md): their FAST figure is printed on its own"""
    D, Sq, Skv, causal, dtype, fp8 = case
    lad, qz, ref, ref_lse = reference(kind, *case)
    used = L.used_lengths(Skv)
    tq, tk, tv = G(*lad.tensors(dtype))
    kv = qa.prepare_kv_fp8(tk, tv, fp8_format=fp8)
    log = Log(f"split-KV, {kind} ladder {L.case_id(case)}")
    check_prepared(kv, qz, log.what)
    fast = {"sparse": Log(log.what + ", FAST, sparse heads"), "dense": Log(log.what + ", FAST, dense heads")}
    accurate = Log(log.what + ", ACCURATE, all heads")
    for ns in L.SPLITS:
        for precision in PRECISIONS:
            for lse in (True, False) if (ns == 1 and precision == "fast") else (True,):      # without the LSE: the byte-exponential sweep
                res = splitkv(tq, kv, used, causal, ns, precision, lse=lse)
                grade_splitkv(log, res, qz, ref, ref_lse, used, Sq, causal, ns, precision)
                if kind == "group" and precision == "fast":
                    for which, lg in fast.items():
                        h = heads_of(lad, which)
                        lg.out(out_to_f32(res[0])[:, h], ref[:, h])
                elif kind == "group":
                    accurate.out(out_to_f32(res[0]), ref)
    if kind == "group":
        for lg in (accurate,) + tuple(fast.values()):
            lg.done()
    log.done()


# ---- (c) exact equivariance of the split-KV entry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.FP8PV_CASES, ids=IDS)
def test_split_kv_exact_equivariance(case):
    """no oracle.  sm_log2e scale_q scale_k sees only exact power-of-two moves, scale_v / l is applied once in the epilogue, the merge is
    linear in fp32: e only -- out, lse, row_path, the partials and their paths are the plain call's; V head ladder -- out and the fp32 partial
    outputs are 2^e x the plain ones, every LSE and path byte equal"""
    D, Sq, Skv, causal, dtype, fp8 = case
    used = L.used_lengths(Skv)
    prep = lambda t: (t[0], qa.prepare_kv_fp8(t[1], t[2], fp8_format=fp8))
    plain, e_only, vhead = (prep(tensors(k, D, Sq, Skv, dtype)) for k in ("plain", "e only", "plain + V head"))
    group, group_plain = (prep(tensors(k, D, Sq, Skv, dtype)) for k in ("group", "group, plain"))
    gain = torch.from_numpy(GAIN_V.astype(np.float32)).to(DEV)
    n = 0
    for ns in L.SPLITS:
        for precision in PRECISIONS:
            for lse in (True, False) if (ns == 1 and precision == "fast") else (True,):
                what = f"split-KV {L.case_id(case)} ns {ns} {precision} lse {lse}"
                call = lambda t: splitkv(*t, used, causal, ns, precision, lse=lse)
                base = call(plain)
                same_outputs(call(e_only), base, E_ONLY_SAME, what + ", e only")
                same_outputs(call(group), call(group_plain), E_ONLY_SAME, what + ", group ladder against its e = 0 twin")
                got = call(vhead)
                same_outputs(got, base, V_HEAD_SAME, what + ", V head ladder")
                scaled_by_the_v_gain(got[0], base[0], dtype, what)
                if got[2].numel():
                    assert torch.equal(got[2], base[2] * gain), (what, "V head ladder: partial_o = 2^e x plain")
                n += 1
    print(f"exact equivariance, split-KV {L.case_id(case)}: {n} (splits, precision) pairs bit for bit: e only, the group ladder, the V head ladder")


# ---- (d) the fixed-scale caches -----------------------------------------------------------------------------------------------------------------
def paged_from(tk, tv, scale_k, scale_v, ps, dtype, fp8, T, slots=None):
    """a PagedKVCacheFP8 whose slot slots[b] holds batch entry b of tk / tv (the other slots stay empty): a shuffled table of distinct
    in-range pages, the given scales per slot, the first Skv - T keys appended in one call and the last T in another.  (cache, table)"""
    Bk, Hkv, Skv, D = tk.shape
    slots = list(range(Bk)) if slots is None else list(slots)
    n = max(slots) + 1
    M = -(-Skv // ps)
    num_pages = n * M + 2
    table = np.random.RandomState(ps + Skv).permutation(num_pages)[:n * M].reshape(n, M).astype(np.int32)
    sk, sv = (torch.ones(n, Hkv, dtype=torch.float32, device=DEV) for _ in range(2))
    sk[slots], sv[slots] = scale_k, scale_v
    c = qa.alloc_paged_kv_cache_fp8(num_pages, Hkv, ps, D, batch_size=n, max_pages_per_seq=M, scale_k=sk, scale_v=sv, dtype=dtype, device=DEV,
                                    fp8_format=fp8)
    c.block_table.copy_(torch.from_numpy(table))
    kk, vv = (torch.zeros(n, Hkv, Skv, D, dtype=dtype, device=DEV) for _ in range(2))
    kk[slots], vv[slots] = tk, tv
    live = torch.zeros(n, dtype=torch.int32, device=DEV)
    live[slots] = 1
    qa.paged_kv_cache_append_fp8(c, kk[:, :, :Skv - T].contiguous(), vv[:, :, :Skv - T].contiguous(), new_lens=live * (Skv - T))
    if T:
        qa.paged_kv_cache_append_fp8(c, kk[:, :, Skv - T:].contiguous(), vv[:, :, Skv - T:].contiguous(), new_lens=live * T)
    assert c.seqlens.tolist() == [Skv if b in slots else 0 for b in range(n)]
    return c, table


@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("case", L.FP8PV_CASES, ids=IDS)
def test_fixed_scale_caches_hold_the_prepared_bits_and_give_the_split_kv_bits(case, T):
    """KVCacheFP8 from a prefill of Skv - T keys (headroom 1) + an append of T, PagedKVCacheFP8 filled the same way through a shuffled table
    with the ladder's own scales per slot: the images (gathered through the table) are prepare_kv_fp8's, and every output of
    fp8_attn_splitkv_func on the cache and of fp8_attn_paged_func is (b)'s bit for bit"""
    D, Sq, Skv, causal, dtype, fp8 = case
    used = su(L.used_lengths(Skv))
    for kind in KINDS:
        tq, tk, tv = tensors(kind, D, Sq, Skv, dtype)
        kv = qa.prepare_kv_fp8(tk, tv, fp8_format=fp8)
        what = f"{kind} ladder {L.case_id(case)} T {T}"
        cache = qa.kv_cache_from_prefill_fp8(tk[:, :, :Skv - T].contiguous(), tv[:, :, :Skv - T].contiguous(), Skv, headroom=1.0, fp8_format=fp8)
        qa.kv_cache_append_fp8(cache, tk[:, :, Skv - T:].contiguous(), tv[:, :, Skv - T:].contiguous())
        assert cache.seqlens.tolist() == [Skv] * B and same_bits(cache.scale_k, kv.scale_k) and same_bits(cache.scale_v, kv.scale_v), what
        assert torch.equal(cache.k, kv.k) and torch.equal(cache.v, kv.v), (what, "the cache's images are prepare_kv_fp8's")
        paged = []
        for ps in PAGE_SIZES:
            c, table = paged_from(tk, tv, kv.scale_k, kv.scale_v, ps, dtype, fp8, T)
            assert torch.equal(PC.gather(c.k, table, HKV, ps, D), kv.k) and torch.equal(PC.gather(c.v, table, HKV, ps, D), kv.v), (what, ps, "gathered pool")
            paged.append((ps, c))
        for ns in L.SPLITS:
            for precision in PRECISIONS:
                kw = dict(causal=causal, seqused_k=used, num_splits=ns, precision=precision, return_lse=True, return_partials=True)
                want = qa.fp8_attn_splitkv_func(tq, kv, **kw)
                all_same(qa.fp8_attn_splitkv_func(tq, cache, **kw), want, (what, ns, precision, "KVCacheFP8"), NAMES)
                for ps, c in paged:
                    all_same(qa.fp8_attn_paged_func(tq, c, max_seqlen_k=Skv, **kw), want, (what, ns, precision, "paged", ps), NAMES)


def half_codes(b8, fp8):
    """the bytes of half the value of bytes that are 0 or +- the largest code: one exponent step down (224, 28672: representable)"""
    step = {"e4m3": 8, "e5m2": 4}[fp8]
    return np.where(b8 & 0x7F, b8 - step, b8).astype(np.uint8)


@pytest.mark.parametrize("case", L.FP8PV_CASES[:3], ids=IDS[:3])
def test_caches_with_headroom_2_hold_the_half_codes_at_twice_the_scales(case):
    """one case per head dim.  headroom 2: scale_k, scale_v exactly 2 x the quantiser's, every non-zero byte exactly the code of half the
    format's largest number -- the de-quantised K and V are the ladder's, so the reference is (b)'s.  The paged cache gets the same scales"""
    D, Sq, Skv, causal, dtype, fp8 = case
    T = 7
    used = L.used_lengths(Skv)
    for kind in KINDS:
        lad, qz, ref, ref_lse = reference(kind, *case)
        tq, tk, tv = G(*lad.tensors(dtype))
        log = Log(f"caches with headroom 2, {kind} ladder {L.case_id(case)}")
        cache = qa.kv_cache_from_prefill_fp8(tk[:, :, :Skv - T].contiguous(), tv[:, :, :Skv - T].contiguous(), Skv, headroom=2.0, fp8_format=fp8)
        qa.kv_cache_append_fp8(cache, tk[:, :, Skv - T:].contiguous(), tv[:, :, Skv - T:].contiguous())
        assert np.array_equal(cache.scale_k.cpu().numpy(), 2 * qz.sk) and np.array_equal(cache.scale_v.cpu().numpy(), 2 * qz.sv), (log.what, "scales exactly 2 x")
        for img, layout, b8 in ((cache.k, _native.LAYOUT_KFRAG, qz.k8), (cache.v, _native.LAYOUT_VFRAG, qz.v8)):
            got = unpack_frag(img.cpu().numpy(), layout, B, HKV, Skv, D)
            assert np.array_equal(got[:, :, :Skv], half_codes(b8, fp8)) and not got[:, :, Skv:].any(), (log.what, "the half codes")
        c, table = paged_from(tk, tv, cache.scale_k, cache.scale_v, 128, dtype, fp8, T)
        assert torch.equal(PC.gather(c.k, table, HKV, 128, D), cache.k) and torch.equal(PC.gather(c.v, table, HKV, 128, D), cache.v), log.what
        for ns in L.SPLITS:
            for precision in PRECISIONS:
                kw = dict(causal=causal, seqused_k=su(used), num_splits=ns, precision=precision, return_lse=True)
                out, lse = qa.fp8_attn_splitkv_func(tq, cache, **kw)
                log.out(out_to_f32(out), ref)
                log.lse_err(lse.cpu().numpy(), ref_lse, LSE_TOL)
                all_same(qa.fp8_attn_paged_func(tq, c, max_seqlen_k=Skv, **kw), (out, lse), (log.what, ns, precision, "paged"), NAMES)
        log.done()


# ---- (e) packed queries over the paged cache ---------------------------------------------------------------------------------------------------
SLOTS, CU = (0, 2), [0, L.PACKED_SQ[0], L.PACKED_SQ[0], sum(L.PACKED_SQ)]     # slot 1 is idle: no query, no key


def packed_q(tq):
    """[B, HQ, 130, D] -> [135, HQ, D]: the 130 rows of batch entry 0, then the first 5 rows of batch entry 1"""
    return torch.cat([tq[b, :, :n].transpose(0, 1) for b, n in enumerate(L.PACKED_SQ)]).contiguous()


def paged_varlen(q, c, used3, Skv, causal, ns, precision):
    return _native.fp8_attention_paged_varlen(q, c.k, c.v, c.scale_k, c.scale_v, c.block_table, used3, su(CU), max_seqlen_q=max(L.PACKED_SQ), Skv=Skv,
                                              num_pages=c.num_pages, page_size=c.page_size, fp8_dtype=TDT[c.fp8_format], is_causal=causal,
                                              precision=precision, num_splits=ns, return_lse=True, return_partials=True, return_quant=True, return_path=True)


def paged_alone(q, c, used3, Skv, causal, ns, precision, b):
    """the dense paged entry on slot b alone: its queries, row b of the table, of the scales and of the lengths, the same pools"""
    one = lambda t: t[b:b + 1].contiguous()
    return _native.fp8_attention_paged_splitkv(V.alone(q, CU, b), c.k, c.v, one(c.scale_k), one(c.scale_v), one(c.block_table), one(used3), Skv=Skv,
                                               num_pages=c.num_pages, page_size=c.page_size, fp8_dtype=TDT[c.fp8_format], is_causal=causal,
                                               precision=precision, num_splits=ns, return_lse=True, return_partials=True, return_quant=True, return_path=True)


def rows_equal(got, want, b, D, what):
    """slot b's rows of the eight outputs of a packed call against the dense call on it alone (tests/test_gpu_paged_varlen.py)"""
    for name, kind, x, y in zip(NAMES, ("o", "l", "po", "pl", "pl", None, None, "l"), got, want):
        if name == "q8":       # the slab [Hq, Sq_b, D] at byte Hq D start_b
            x = x.view(torch.uint8)[HQ * D * CU[b]:HQ * D * CU[b + 1]].view(1, HQ, CU[b + 1] - CU[b], D).view(y.dtype)
        elif name == "scale_q":
            x = x[b:b + 1]
        elif x.numel() == 0:
            assert y.numel() == 0, (what, name)
            continue
        else:
            x = V.rows_of(x, kind, CU, b)
        assert same_bits(x, y), (what, "slot", b, name, "the dense paged call on the slot alone, bit for bit")


PACKED_PAGED = [c for c in L.FP8PV_CASES if c[1] == L.PACKED_SQ[0]]


@pytest.mark.parametrize("page_size", PAGE_SIZES)
@pytest.mark.parametrize("case", PACKED_PAGED, ids=[L.case_id(c) for c in PACKED_PAGED])
def test_packed_queries_over_the_paged_cache(case, page_size):
    """three slots, slot 1 idle; slots 0 and 2 hold the ladder's two batch entries with 130 and 5 queries: `g` must come from the sequence's
    own query count, scale_q / scale_k / scale_v from (slot, head).  Every row of slots 0 and 2 against the oracle; each slot's rows = the
    dense paged call on it alone; e only and V head ladder exactly"""
    D, Sq, Skv, causal, dtype, fp8 = case
    used3 = su([L.used_lengths(Skv)[0], 0, L.used_lengths(Skv)[1]])

    def cache_of(kind):
        tq, tk, tv = tensors(kind, D, Sq, Skv, dtype)
        kv = qa.prepare_kv_fp8(tk, tv, fp8_format=fp8)
        return packed_q(tq), paged_from(tk, tv, kv.scale_k, kv.scale_v, page_size, dtype, fp8, 7, SLOTS)[0]

    unpacked = lambda x, b: out_to_f32(V.rows_of(x, "o", CU, b))[0]
    for kind in KINDS:
        lad, qz, ref, ref_lse = reference(kind, *case, sq=L.PACKED_SQ)
        q, c = cache_of(kind)
        log = Log(f"packed queries over the paged cache (page size {page_size}), {kind} ladder {L.case_id(case)}")
        for ns in L.SPLITS:
            for precision in PRECISIONS:
                got = paged_varlen(q, c, used3, Skv, causal, ns, precision)
                for b, (slot, n) in enumerate(zip(SLOTS, L.PACKED_SQ)):
                    q8 = bits8(got[5])[HQ * D * CU[slot]:HQ * D * CU[slot + 1]].reshape(HQ, n, D)
                    assert np.array_equal(q8, qz.q8[b, :, :n]) and np.array_equal(got[6][slot].cpu().numpy(), qz.sq[b]), (log.what, "q8 / scale_q: the CPU quantiser's")
                    log.out(unpacked(got[0], slot), ref[b, :, :n])
                    log.lse_err(V.rows_of(got[1], "l", CU, slot)[0].cpu().numpy(), ref_lse[b, :, :n], LSE_TOL)
                    rows_equal(got, paged_alone(q, c, used3, Skv, causal, ns, precision, slot), slot, D, (log.what, ns, precision))
        log.done()
    # exact equivariance
    (qp, cp), (qe, ce), (qv, cv) = (cache_of(k) for k in ("plain", "e only", "plain + V head"))
    (qg, cg), (qg0, cg0) = (cache_of(k) for k in ("group", "group, plain"))
    for ns in L.SPLITS:
        for precision in PRECISIONS:
            what = f"packed paged {L.case_id(case)} page size {page_size} ns {ns} {precision}"
            call = lambda q, c: paged_varlen(q, c, used3, Skv, causal, ns, precision)
            base = call(qp, cp)
            same_outputs(call(qe, ce), base, E_ONLY_SAME, what + ", e only")
            same_outputs(call(qg, cg), call(qg0, cg0), E_ONLY_SAME, what + ", group ladder against its e = 0 twin")
            got = call(qv, cv)
            same_outputs(got, base, V_HEAD_SAME, what + ", V head ladder")
            for b, slot in enumerate(SLOTS):
                scaled_by_the_v_gain(V.rows_of(got[0], "o", CU, slot)[0], V.rows_of(base[0], "o", CU, slot)[0], dtype, what, GAIN_V[b])
                if got[2].numel():
                    gain = torch.from_numpy(GAIN_V[b].astype(np.float32)).to(DEV)
                    assert torch.equal(V.rows_of(got[2], "po", CU, slot), V.rows_of(base[2], "po", CU, slot) * gain), (what, "V head ladder: partial_o = 2^e x plain")


# ---- (a) the three FP8-P.V siblings ------------------------------------------------------------------------------------------------------------
def sibling_masks(S):
    """{entry: mask [B, 1 or HQ, S, S]}: what each call below attends (tests/test_cpu_scale_ladder_fp8pv.packed_masks: the teeth)"""
    used = L.used_lengths(S)
    rep = lambda m: np.broadcast_to(m, (B,) + m.shape).copy()
    return {"packed, seqused_k": L.used_mask(S, S, used, False), "packed causal, seqused_k": L.used_mask(S, S, used, True, top_left=True),
            "window": rep(L.mask_of(S, S, window=L.WINDOW)), "window (-1, 0)": L.used_mask(S, S, [S, S], True),
            "block-sparse, all tiles": rep(L.mask_of(S, S)), "block-sparse, sparse tiles": rep(L.mask_of(S, S, tiles=L.sparse_tiles(S)))}


@functools.lru_cache(maxsize=None)
def sibling_references(kind, D, S, dtype, fp8):
    """(ladder, the CPU quantiser's output, {entry: (ref out, ref lse)})"""
    lad = LADDERS[kind](D, S, S)
    qz = L.quantise(lad, dtype, fp8, "head", v_block=False)
    return lad, qz, {name: L.UsedScores(qz, m).softmax() for name, m in sibling_masks(S).items()}


def siblings(tq, tk, tv, S, fp8, precision):
    """{entry: (out, lse, path as torch tensors in the entry's own layout; (q8, k8, v8 bytes [B, H, S, D] -- k8 / v8 zero behind the used keys --,
    scale_q, scale_k, scale_v) as numpy)} of every FP8-PV sibling on one problem"""
    D = tq.shape[3]
    used = L.used_lengths(S)
    pq, pk, pv = pack(tq), pack(tk), pack(tv)
    cu = torch.tensor([0, S, 2 * S], dtype=torch.int32, device=DEV)
    kw = dict(fp8_dtype=TDT[fp8], precision=precision, return_lse=True, return_quant=True, return_path=True)

    def packed_quant(r, lens):
        q8, k8, v8 = bits8(r[2]), bits8(r[3]), bits8(r[4])
        rows = lambda buf, layout: np.stack([np.pad(_image(buf, layout, S * i, i, m, HKV, D)[0, :, :m], ((0, 0), (0, S - m), (0, 0))) for i, m in enumerate(lens)])
        return (q8[:B * HQ * S * D].reshape(B, HQ, S, D), rows(k8, _native.LAYOUT_KFRAG), rows(v8, _native.LAYOUT_VFRAG)) + tuple(x.cpu().numpy() for x in r[5:8])

    res = {}
    for causal in (False, True):
        r = _native.fp8_quant_attention_varlen_fp8pv(pq, pk, pv, cu, cu, su(used), is_causal=causal, **kw)
        res["packed causal, seqused_k" if causal else "packed, seqused_k"] = (r[0], r[1], r[8], packed_quant(r, used))
    for name, (left, right) in (("window", L.WINDOW), ("window (-1, 0)", (-1, 0))):
        r = _native.fp8_quant_attention_varlen_window_fp8pv(pq, pk, pv, cu, cu, None, window_left=left, window_right=right, **kw)
        res[name] = (r[0], r[1], r[8], packed_quant(r, [S, S]))
    nb = -(-S // 128)
    for name, tiles in (("block-sparse, all tiles", np.ones((HQ, nb, nb), bool)), ("block-sparse, sparse tiles", L.sparse_tiles(S))):
        r = _native.fp8_block_sparse_attention_fp8pv(tq, tk, tv, torch.from_numpy(tiles[None]).to(DEV), **kw)
        res[name] = (r[0], r[1], r[8], tuple(bits8(x) for x in r[2:5]) + tuple(x.cpu().numpy() for x in r[5:8]))
    return res


def dense_out(name, out, lse, S):
    """(out fp32 [B, HQ, S, D], lse [B, HQ, S]) numpy of an entry's own layout"""
    if name.startswith("block-sparse"):
        return out_to_f32(out), lse.cpu().numpy()
    return out_to_f32(out).reshape(B, S, HQ, -1).transpose(0, 2, 1, 3), lse.cpu().numpy().reshape(HQ, B, S).transpose(1, 0, 2)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", L.PACKED_CASES, ids=PACKED_IDS)
def test_fp8pv_siblings_on_the_head_ladder(case, precision):
    """block-sparse (the all-true mask and sparse_tiles), packed (causal and not, a batch entry a sequence, with seqused_k) and window (at WINDOW
    and at (-1, 0)) with FP8 P.V, on the plain-V head ladder and on the V head ladder: oracle grading, the quantiser echo, the exact equivariance"""
    D, S, dtype, fp8 = case
    used = L.used_lengths(S)
    plain = siblings(*tensors("plain", D, S, S, dtype), S, fp8, precision)
    e_only = siblings(*tensors("e only", D, S, S, dtype), S, fp8, precision)
    plain_vhead = siblings(*tensors("plain + V head", D, S, S, dtype), S, fp8, precision)
    for kind in ("head", "vhead"):
        lad, qz, refs = sibling_references(kind, D, S, dtype, fp8)
        got = siblings(*G(*lad.tensors(dtype)), S, fp8, precision)
        log = Log(f"FP8-PV siblings {precision}, {kind} ladder D {D} S {S} {L.NAME[dtype]} {fp8}")
        for name, (out, lse, path, quant) in got.items():
            ref, ref_lse = refs[name]
            o, l = dense_out(name, out, lse, S)
            assert (o[np.isneginf(ref_lse)] == 0).all(), (name, "rows without a key must be exactly 0")
            w, wl = log.out(o, ref), log.lse_err(l, ref_lse, LSE_TOL)
            assert w < 1.0 and wl < 1.0, (log.what, name, w, wl)
            # echo: the bytes of the plain call and the CPU quantiser's (K and V: on the used keys), the scales exactly 2^e times the plain ones
            lens = used if "seqused_k" in name else [S, S]
            cut = lambda b8: np.stack([np.where(np.arange(S)[None, :, None] < m, b8[i], 0) for i, m in enumerate(lens)])
            for i, cpu in ((0, qz.q8), (1, cut(qz.k8)), (2, cut(qz.v8))):
                assert np.array_equal(quant[i], plain[name][3][i]) and np.array_equal(quant[i], cpu), (log.what, name, "q8 / k8 / v8", i)
            for i, e, cpu in ((3, lad.e_q, qz.sq), (4, lad.e_k, qz.sk), (5, lad.e_v, qz.sv)):
                assert np.array_equal(quant[i], plain[name][3][i] * np.exp2(e).astype(np.float32)) and np.array_equal(quant[i], cpu), (log.what, name, "scale", i)
        log.done()
    for name in plain:      # exact equivariance
        all_same(e_only[name][:3], plain[name][:3], (precision, name, "e only"), ("out", "lse", "row_path"))
        all_same(plain_vhead[name][1:3], plain[name][1:3], (precision, name, "V head ladder"), ("lse", "row_path"))
        scaled_by_the_v_gain(dense_out(name, *plain_vhead[name][:2], S)[0], dense_out(name, *plain[name][:2], S)[0], dtype, (precision, name))

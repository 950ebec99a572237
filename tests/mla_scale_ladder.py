"""The scale ladder of the MLA entries: inputs on which a quantisation scale read at the WRONG INDEX shows, the mutants
that name those wrong indices, and the checks tests/test_cpu_mla_scale_ladder.py (the teeth, the eager definitions) and
tests/test_gpu_mla_scale_ladder.py (the kernels) share.  tests/scale_ladder.py is the same idea for the attention entries.

Everything starts from the exact grid data of tests/mla_cases.py and carries gains that are POWERS OF TWO, so the fp8 bytes of the cache and
of q8 are those of the plain (no-gain) inputs -- the quantiser echo -- while the scales differ by x4 and more:

slot ladder     cache.scale[b] = S0 2^E_SLOT[b], the latent of slot b is grid x that scale, the slot's queries carry 2^-E_SLOT[b]: scale_q x
                scale[b], and with it every score, is the plain call's, the output is 2^E_SLOT[b] times the plain one.
q ladder        on top of it query row (h, i) carries 2^F[h, i] (F_ROWS: neighbouring heads, neighbouring rows of a head and the two sides
                of a head boundary of the packed 64-row tile are all a factor >= 4 apart); packed tokens: F[t, h] = -2 (t mod 2 + h mod 2).
index ladder    icache.scale[b] = 2^-2 2^E_SLOT[b] with the keys scaled to match, q_idx of (h, i) x 2^F[h, i]; weights x 2^-F (w scale_q is the
                plain call's: exact equivariance) or plain (the logits change: the fp64 formula judges).
prefill ladder  v[i, h] x 2^EV[i, h], k_pe[i] x 2^EK[i], k_nope[i, h] x 2^(EK[i] + GH[h]) with the abs-max of every (i, h) planted in k_nope,
                q x 2^-(EK[i] + GH[h]).

The reference is the entry's fp64 oracle (mla_cases.reference, mla_sparse_cases.reference, mla_index_cases.ref_logits,
mla_prefill_cases.reference) on the inputs themselves and on scales computed HERE -- never a scale a device call returned.  A MUTANT is that
reference with one scale table re-indexed, given as the ratio wrong / right of the score scale and of the output scale of every row.  Grading
is the project's (gpu_utils.grade: 2^-6 max(1, |ref| / 2); mla_cases.LSE_TOL) on out / 2^e against ref / 2^e, 2^e the gain of the row's slot
or (sequence, head): the bound bites as on the plain data whatever the gain."""
import functools

import numpy as np
import torch

import quantumattention_amd as qa
from quantumattention_amd import mla
from quantumattention_amd import mla_prefill as MP
from quantumattention_amd.mla import PagedMLACacheFP8
from tests import mla_cases as C
from tests import mla_index_cases as X
from tests import mla_index_prefill_cases as XP
from tests import mla_prefill_cases as PF
from tests import mla_sparse_cases as S
from tests.gpu_utils import TOL, grade

B = C.B
S0 = 0.5                                          # the base scale of the latent: grid x 0.5 has rms 0.76 <= 1 (the suite's plain data: 0.25)
E_SLOT = np.array([-2, -6, 0, -4])                # distinct, >= 2 apart, the largest gain 1 (scale_ladder.E_VHEAD's rule); not monotone: slot b+1,
                                                  # slot b-1 and slot 0 each make the scales of slots 1 AND 3 too large
LAT_SEED = 100                                    # of the latent (mla_cases.make_latent's)
F_ROWS = {1: ((0,), (-2,)), 3: ((0, -2, -4), (-2, 0, -2)), 4: ((0, -2, -4, -2), (-4, 0, -2, -4))}      # F[h % 2][i] per Sq
LARGE, TEETH = 4.0, 4.0                           # tests/scale_ladder.py's: a mutant must show where it makes a scale >= LARGE x too large
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}

# ---- the case tables: ONE place, so that the CPU teeth are shown on the very inputs the GPU tests run -------------------------------------
DECODE_CASES = [(16, 4, "e4m3", torch.bfloat16), (20, 3, "e4m3", torch.bfloat16), (128, 1, "e4m3", torch.bfloat16), (16, 4, "e5m2", torch.float16)]
DENSE_PAGES, DENSE_SPLITS = (64, 128), (1, 3, 0)
SPARSE_TOPKS, SPARSE_PAGES, SPARSE_SPLITS = (65, 200), (1, 16, 64), (1, 2)
COUNTS, VARLEN_LENS, VARLEN_TOPK = (0, 1, 5, 3), (64, 1, 3, 200), 130      # tests/test_gpu_mla_sparse_prefill.py's
VARLEN_TOTAL = sum(COUNTS) + 4
VARLEN_HEADS = (16, 72, 160)
INDEX_CASES = [(64, 3, 16, "e4m3", torch.bfloat16), (20, 3, 64, "e4m3", torch.bfloat16), (20, 3, 1, "e5m2", torch.float16)]   # (Hi, Sq, page, ..)
INDEX_VARLEN_CASES = [("a", 64, 16, "e4m3", torch.bfloat16), ("b", 33, 1, "e4m3", torch.bfloat16), ("b", 20, 64, "e5m2", torch.float16)]
INDEX_TILE = XP.TQ                                # packed tokens per workgroup of the prefill indexer
PREFILL_CASES = [("e4m3", torch.bfloat16), ("e5m2", torch.float16)]
PREFILL_H = 3
EK = np.array([0, -4, -2, -4, -6, -2, 0])         # per sequence of mla_prefill_cases.LENS; sequence 4 reads a LARGER scale at i + 1 and at i - 1
GH = np.array([0, 2, 0])
EV = np.array([-2, 0, -4, -2, -6, 0, -4])[:, None] + np.array([0, -2, 0])[None, :]
# (mutant, where) pairs that are NOT in the table, by name, with the reason
NOT_LISTED = {
    ("scale_q of row i+1 / i-1 / read as [B, Sq, H]", "Sq = 1"): "one row per head: the three re-indexings are the identity",
    ("slot scale at the packed row / tile index", "the decode entries"): "their slot is a grid coordinate; the packed entries search it",
    ("slot scale at the token-tile index", "the packed sparse entry"): "one token per workgroup: it is the packed row index, which is listed",
}


def decode_id(c):
    return f"Hq{c[0]}_Sq{c[1]}_{c[2]}_{NAME[c[3]]}"


def f_rows(H, Sq):
    """int [H, Sq]"""
    return np.array([F_ROWS[Sq][h % 2] for h in range(H)])


def f_tokens(T, H):
    """int [T, H]"""
    return -2 * (np.arange(T)[:, None] % 2 + np.arange(H)[None, :] % 2)


def exact(x, dtype):
    """a float32 tensor as `dtype`; every value must be exact in it"""
    y = x.to(dtype)
    assert torch.equal(y.float(), x.float())
    return y


def t2(e):
    """2^e as a float32 tensor"""
    return torch.from_numpy(np.exp2(np.asarray(e, np.float64))).float()


def slot_of_tokens(counts, total):
    """int [total]: the slot of every packed token, -1 behind cu[B]"""
    s = np.full(total, -1)
    s[:sum(counts)] = np.repeat(np.arange(len(counts)), counts)
    return s


# ---- grading ----------------------------------------------------------------------------------------------------------------------------------
def grade_rows(out, lse, ref_o, ref_l, e, what):
    """out, ref_o [rows.., Dv], lse, ref_l [rows..] numpy; e [rows..]: log2 of the row's gain.  Asserts the project's bounds on out / 2^e and the
    -inf / zero-row rules; returns (worst |err| / bound, worst lse error)"""
    g, fin = np.exp2(np.asarray(e, np.float64))[..., None], np.isfinite(ref_l)
    worst = grade(np.asarray(out, np.float64) / g, ref_o / g)[2]
    lerr = float(np.abs(lse[fin] - ref_l[fin]).max()) if fin.any() else 0.0
    assert worst < 1.0, (what, "worst |err| / bound", worst)
    assert np.array_equal(np.isneginf(lse), ~fin), what                  # a row without a key: LSE -inf exactly ...
    assert (np.asarray(out)[~fin] == 0).all(), what                      # ... and a zero row
    assert lerr <= C.LSE_TOL, (what, "lse", lerr)
    return worst, lerr


def shown(ref_o, ref_l, mut_o, mut_l, e):
    """bool [rows..]: the mutant moves an element of the row by >= TEETH x its bound, or the row's LSE by >= TEETH x LSE_TOL"""
    g = np.exp2(np.asarray(e, np.float64))[..., None]
    bound = TOL * np.maximum(1.0, np.abs(ref_o / g) / 2.0)
    both = np.isfinite(ref_l) & np.isfinite(mut_l)
    dl = np.where(both, np.abs(np.where(both, mut_l, 0.0) - np.where(both, ref_l, 0.0)), 0.0)
    return ((np.abs(mut_o - ref_o) / g / bound).max(-1) >= TEETH) | (dl >= TEETH * C.LSE_TOL)


LONE_SHARE = 0.05


def lone_rows(ref, probe):
    """bool [rows..]: rows that attend ONE distinct key -- their output under a probe that halves every score scale is the reference's bit
    for bit (p = 1 whatever the scale).  Such a row can show a score mutant in its LSE alone, by (ratio - 1) |s|, s its one score"""
    return np.isfinite(ref[1]) & (probe[0] == ref[0]).all(-1)


def teeth(name, ref, mut, score_ratio, out_ratio, e, lone):
    """The rule of the teeth for one mutant: EVERY row with a key where it makes the score scale or the output scale >= LARGE x too large is
    shown (`shown`), but for lone rows whose one score is too near 0 to move the LSE by TEETH x LSE_TOL -- at most LONE_SHARE of the judged
    rows.  Returns (rows judged, lone rows not shown)."""
    rows = np.isfinite(ref[1]) & ((score_ratio >= LARGE) | (out_ratio >= LARGE))
    assert rows.any(), (name, "no row gets a scale >= LARGE x too large: the ladder does not reach this mutant")
    miss = rows & ~shown(ref[0], ref[1], mut[0], mut[1], e)
    assert not (miss & ~lone).any(), (name, "rows not shown", int((miss & ~lone).sum()), "of", int(rows.sum()))
    assert miss.sum() <= LONE_SHARE * rows.sum(), (name, "lone rows not shown", int(miss.sum()), "of", int(rows.sum()))
    return int(rows.sum()), int(miss.sum())


def stays_normal(ref_plain, e, dtype):
    """bool: the elements whose 2^e-fold cannot leave the normal range of `dtype` -- decided from the plain REFERENCE: a kernel inside its
    bound is at least |ref| - bound there (bf16 has fp32's exponent range: every element)"""
    if dtype == torch.bfloat16:
        return np.ones(ref_plain.shape, bool)
    bound = TOL * np.maximum(1.0, np.abs(ref_plain) / 2.0)
    return (np.abs(ref_plain) - bound) * np.exp2(np.asarray(e, np.float64))[..., None] >= 2.0 ** -14


def assert_scaled_bits(got, plain, e, keep, what):
    """got == 2^e plain bit for bit on the elements `keep` (torch 16-bit tensors; e numpy [rows..])"""
    want = (plain.float().cpu() * t2(e)[..., None]).to(plain.dtype)
    diff = (got.cpu().view(torch.int16).int() - want.view(torch.int16).int()).abs()[torch.from_numpy(np.ascontiguousarray(keep))]
    assert diff.numel() > 0 and int(diff.max()) == 0, (what, "elements off", int((diff != 0).sum()), "largest ulp distance", int(diff.max()))


def assert_echo(q8, sq, q8_plain, sq_plain, e, what):
    """the quantiser echo: the bytes of q8 are the plain call's and scale_q is exactly 2^e times the plain one"""
    assert torch.equal(q8.view(torch.uint8).cpu(), q8_plain.view(torch.uint8).cpu()), what
    assert torch.equal(sq.cpu(), sq_plain.cpu() * t2(e)), what


# ---- the decode entries: fp8_mla_paged_func, fp8_mla_paged_sparse_func ------------------------------------------------------------------------
class Decode:
    """q [B, Hq, Sq, 576], lat [B, CAP, 576] in `dtype` (CPU), scale fp32 [B], e [B] and f [Hq, Sq]: the exponents they were built with"""

    def __init__(self, q, lat, scale, e, f, dtype):
        self.q, self.lat, self.scale, self.e, self.f, self.dtype = q, lat, scale, e, f, dtype
        self.e_rows = np.broadcast_to(e[:, None, None], q.shape[:3])                      # log2 of the output's gain per row
        self.e_q = f[None] - e[:, None, None]                                             # log2 of scale_q / the plain scale_q


@functools.lru_cache(maxsize=None)
def decode_inputs(Hq, Sq, dtype, slot=True, rows=True):
    """slot: the slot ladder; rows: the q ladder on top.  Neither: the plain inputs (the grid data at the base scale S0)."""
    e = E_SLOT if slot else np.zeros(B, int)
    f = f_rows(Hq, Sq) if rows else np.zeros((Hq, Sq), int)
    q = C.make_q(Hq, Sq, torch.float32) * t2(f[None] - e[:, None, None])[..., None]
    lat = C.draw((B, C.CAP, C.D), LAT_SEED) * S0 * t2(e)[:, None, None]
    return Decode(exact(q, dtype), exact(lat, dtype), (S0 * t2(e)).contiguous(), e, f, dtype)


def make_cache(kind, page, lens, inp, fmt, device, table_seed=7):
    """kind "dense": the chunk-image cache of fp8_mla_paged_func; "row": the row-major cache of the sparse entries.  Zero-filled, slot b
    holds the first lens[b] rows of inp.lat under inp.scale behind a shuffled table"""
    table, num_pages = C.make_table(page, table_seed)
    alloc, append = ((qa.alloc_paged_mla_cache_fp8, qa.paged_mla_cache_append_fp8) if kind == "dense" else
                     (qa.alloc_paged_mla_row_cache_fp8, qa.paged_mla_row_cache_append_fp8))
    cache = alloc(num_pages, page, batch_size=B, max_pages_per_seq=table.shape[1], scale=inp.scale, dtype=inp.dtype, device=device, fp8_format=fmt)
    cache.block_table.copy_(table)
    lat = inp.lat.to(device)
    append(cache, lat[..., :C.DV], lat[..., C.DV:], new_lens=torch.tensor(lens, dtype=torch.int32, device=device))
    assert cache.seqlens.tolist() == list(lens) and torch.equal(cache.scale.cpu(), inp.scale)
    return cache


def pool_bytes(cache):
    """uint8 [num_pages, page_size, channels] on the CPU, whatever the layout"""
    if cache.layout == "frag":
        return mla.pool_rowmajor(cache.pool, cache.num_pages, cache.page_size).cpu()
    return cache.pool.view(torch.uint8).cpu()


def decode_reference(inp, lens, causal=True, idx=None, score_ratio=None, out_ratio=None):
    """the fp64 oracle on the inputs themselves (idx: the sparse one); a mutant's ratios [B, Hq, Sq] multiply the score scale (folded into q: the
    oracle has one latent for scores and values) and the output"""
    q = inp.q.double().numpy() * (1.0 if score_ratio is None else score_ratio[..., None])
    lat = inp.lat.double().numpy()
    out, lse = C.reference(q, lat, lens, C.SM_SCALE, causal) if idx is None else S.reference(q, lat, idx, lens, C.SM_SCALE, causal)
    return out * (1.0 if out_ratio is None else out_ratio[..., None]), lse


def slot_tables(scale):
    """{name: the slot scales a mis-indexing reads} for scale float64 [B]"""
    return {"slot b+1": np.roll(scale, -1), "slot b-1": np.roll(scale, 1), "slot 0 for every slot": np.repeat(scale[:1], len(scale))}


def slot_mutants(ratio_rows):
    """{name: (score_ratio, out_ratio)} from {name: ratio per row}: each table in the scores only, in the output only, and in both"""
    res = {}
    for name, r in ratio_rows.items():
        one = np.ones_like(r)
        res.update({f"{name}, scores": (r, one), f"{name}, output": (one, r), f"{name}, both": (r, r)})
    return res


def transposed_read(sq):
    """sq [.., H, R] read as if it were [.., R, H]: element (h, i) comes from flat address i H + h"""
    H, R = sq.shape[-2:]
    flat = sq.reshape(sq.shape[:-2] + (H * R,))
    return flat[..., (np.arange(R)[None, :] * H + np.arange(H)[:, None])]


def decode_mutants(inp):
    """{name: (score_ratio, out_ratio) [B, Hq, Sq]}: the slot scale and scale_q read at a wrong index"""
    s, Sq = inp.scale.double().numpy(), inp.q.shape[2]
    res = slot_mutants({n: np.broadcast_to((t / s)[:, None, None], inp.q.shape[:3]).copy() for n, t in slot_tables(s).items()})
    sq, one = np.exp2(inp.e_q.astype(np.float64)), np.ones(inp.q.shape[:3])
    q_tables = {"scale_q of head h+1": np.roll(sq, -1, 1), "scale_q of head h-1": np.roll(sq, 1, 1)}
    if Sq > 1:                                    # NOT_LISTED: Sq = 1
        q_tables.update({"scale_q of row i+1": np.roll(sq, -1, 2), "scale_q of row i-1": np.roll(sq, 1, 2), "scale_q read as [B, Sq, H]": transposed_read(sq)})
    res.update({n: (t / sq, one) for n, t in q_tables.items()})
    return res


def decode_teeth(inp, lens, idx=None, causal=True):
    """{mutant: rows judged}; asserts the rule on every mutant"""
    ref = decode_reference(inp, lens, causal, idx)
    lone = lone_rows(ref, decode_reference(inp, lens, causal, idx, np.full(inp.q.shape[:3], 0.5)))
    return {n: teeth(n, ref, decode_reference(inp, lens, causal, idx, sr, orr), sr, orr, inp.e_rows, lone) for n, (sr, orr) in decode_mutants(inp).items()}


def check_decode(kind, Hq, Sq, fmt, dtype, device, pages, splits, topk=None, lens_sets=C.LENS):
    """One case of the dense (kind "dense") or the sparse (kind "row") decode entry over lens_sets x pages x splits, causal: the ladder
    (slot + q) against the fp64 oracle, the quantiser echo, and the slot ladder alone against the plain call bit for bit.  Returns the worst
    |err| / bound."""
    lad, slot, plain = decode_inputs(Hq, Sq, dtype), decode_inputs(Hq, Sq, dtype, rows=False), decode_inputs(Hq, Sq, dtype, False, False)
    idx = None if kind == "dense" else S.draw_indices(Sq, topk, seed=1000 * topk + Sq)
    didx, worst = None if idx is None else idx.to(device), 0.0
    def call(inp, cache, ns):
        if kind == "dense":
            return qa.fp8_mla_paged_func(inp.q.to(device), cache, scale=C.SM_SCALE, causal=True, num_splits=ns, max_seqlen_k=C.CAP, return_lse=True, return_q8=True)
        return qa.fp8_mla_paged_sparse_func(inp.q.to(device), cache, didx, scale=C.SM_SCALE, causal=True, num_splits=ns, return_lse=True, return_q8=True)
    for lens in lens_sets:
        ref, ref_p = decode_reference(lad, lens, True, idx), decode_reference(plain, lens, True, idx)
        keep = stays_normal(ref_p[0], slot.e_rows, dtype)
        for page in pages:
            c_l, c_p = make_cache(kind, page, lens, lad, fmt, device), make_cache(kind, page, lens, plain, fmt, device)
            assert torch.equal(pool_bytes(c_l), pool_bytes(c_p)), (lens, page)                      # echo: the cache bytes
            for ns in splits:
                what = (kind, Hq, Sq, fmt, topk, lens, page, ns)
                (o, l, q8, sq), (o_s, l_s, q8_s, sq_s), (o_p, l_p, q8_p, sq_p) = call(lad, c_l, ns), call(slot, c_l, ns), call(plain, c_p, ns)
                assert torch.equal(q8_p.float().cpu() * sq_p.cpu()[..., None], plain.q.float()), what   # exact inputs: the plain q8 is q itself
                assert_echo(q8, sq, q8_p, sq_p, lad.e_q, what)
                assert_echo(q8_s, sq_s, q8_p, sq_p, slot.e_q, what)
                worst = max(worst, grade_rows(o.float().cpu().numpy(), l.cpu().numpy(), ref[0], ref[1], lad.e_rows, what)[0])
                assert torch.equal(l_s.view(torch.int32), l_p.view(torch.int32)), what              # slot ladder alone: the scores are the plain call's
                assert_scaled_bits(o_s, o_p, slot.e_rows, keep, what)
    return worst


# ---- sparse MLA on packed tokens: fp8_mla_paged_sparse_varlen_func ----------------------------------------------------------------------------
class Packed:
    """q [TOTAL, Hq, 576] (CPU), idx [TOTAL, topk], cu, slot [TOTAL] (-1: padding), e_rows / e_q [TOTAL, Hq]"""


@functools.lru_cache(maxsize=None)
def varlen_inputs(Hq, dtype, slot=True, rows=True):
    p = Packed()
    p.slot = slot_of_tokens(COUNTS, VARLEN_TOTAL)
    live = p.slot >= 0
    e = np.where(live, (E_SLOT if slot else np.zeros(B, int))[np.maximum(p.slot, 0)], 0)
    f = np.where(live[:, None], f_tokens(VARLEN_TOTAL, Hq), 0) if rows else np.zeros((VARLEN_TOTAL, Hq), int)
    q = C.make_q(Hq, 4, torch.float32).permute(0, 2, 1, 3).reshape(16, Hq, C.D)[:VARLEN_TOTAL]
    p.e_rows, p.e_q = np.broadcast_to(e[:, None], (VARLEN_TOTAL, Hq)), f - e[:, None]
    p.q = exact(q * t2(p.e_q)[..., None], dtype).contiguous()
    p.idx = S.draw_indices(4, VARLEN_TOPK, seed=1000 * VARLEN_TOPK).reshape(16, VARLEN_TOPK)[:VARLEN_TOTAL].contiguous()
    p.cu = torch.tensor(np.concatenate([[0], np.cumsum(COUNTS)]), dtype=torch.int32)
    p.lat = decode_inputs(16, 1, dtype, slot, False)                                   # (the latent and the slot scales)
    return p


def varlen_reference(p, causal, score_ratio=None, out_ratio=None):
    """(out [TOTAL, Hq, 512], lse [TOTAL, Hq]) fp64: mla_sparse_cases.reference per slot on the slot's tokens; padding: zero rows, -inf"""
    T, Hq = p.q.shape[:2]
    out, lse, lo = np.zeros((T, Hq, C.DV)), np.full((T, Hq), -np.inf), 0
    q = p.q.double().numpy() * (1.0 if score_ratio is None else score_ratio[..., None])
    lat = p.lat.lat.double().numpy()
    for b, n in enumerate(COUNTS):
        if n:
            o, l = S.reference(q[lo:lo + n].transpose(1, 0, 2)[None], lat[b:b + 1], p.idx[lo:lo + n][None].numpy(), (VARLEN_LENS[b],), C.SM_SCALE, causal)
            out[lo:lo + n], lse[lo:lo + n] = o[0].transpose(1, 0, 2), l[0].T
        lo += n
    return out * (1.0 if out_ratio is None else out_ratio[..., None]), lse


def packed_slot_tables(scale, slot, tile):
    """{name: the scale every live packed token reads [n]}: slot_tables at the token's slot, and the table indexed by the packed row / by the
    token tile (wrapped into the table: a model of an index that was never searched)"""
    live = slot[slot >= 0]
    t = np.arange(len(live))
    res = {n: tab[live] for n, tab in slot_tables(scale).items()}
    res.update({"slot scale at the packed row index": scale[t % len(scale)], "slot scale at the token-tile index": scale[(t // tile) % len(scale)]})
    return res


def varlen_mutants(p):
    """{name: (score_ratio, out_ratio) [TOTAL, Hq]}"""
    s, n, Hq = p.lat.scale.double().numpy(), sum(COUNTS), p.q.shape[1]
    def rows(r):                                  # a ratio per live token -> [TOTAL, Hq]
        full = np.ones((VARLEN_TOTAL, Hq))
        full[:n] = r[:, None]
        return full
    tables = packed_slot_tables(s, p.slot, 1)
    del tables["slot scale at the token-tile index"]          # (one token per workgroup: the packed row index)
    res = slot_mutants({name: rows(t / s[p.slot[:n]]) for name, t in tables.items()})
    sq, one = np.exp2(p.e_q[:n].astype(np.float64)), np.ones((VARLEN_TOTAL, Hq))
    q_tables = {"scale_q of head h+1": np.roll(sq, -1, 1), "scale_q of head h-1": np.roll(sq, 1, 1), "scale_q of token t+1": np.roll(sq, -1, 0),
                "scale_q of token t-1": np.roll(sq, 1, 0), "scale_q read as [Hq, total]": transposed_read(sq)}
    for name, t in q_tables.items():
        r = one.copy()
        r[:n] = t / sq
        res[name] = (r, one)
    return res


def varlen_teeth(p, causal):
    ref = varlen_reference(p, causal)
    lone = lone_rows(ref, varlen_reference(p, causal, np.full(p.q.shape[:2], 0.5)))
    return {n: teeth(n, ref, varlen_reference(p, causal, sr, orr), sr, orr, p.e_rows, lone) for n, (sr, orr) in varlen_mutants(p).items()}


def one_slot(cache, b):
    return PagedMLACacheFP8(cache.pool, cache.scale[b:b + 1], cache.block_table[b:b + 1], cache.seqlens[b:b + 1], cache.num_pages,
                            cache.page_size, cache.fp8_format, cache.dtype, cache.layout)


def check_varlen(Hq, fmt, dtype, page, device, chain=True):
    """The packed sparse entry, causal and not: the ladder against the fp64 oracle, the echo, the slot ladder alone against the plain call
    bit for bit, and (chain) the ladder against fp8_mla_paged_sparse_func(num_splits=1) per slot bit for bit.  Returns the worst |err| / bound."""
    lad, slot, plain = varlen_inputs(Hq, dtype), varlen_inputs(Hq, dtype, rows=False), varlen_inputs(Hq, dtype, False, False)
    c_l, c_p = make_cache("row", page, VARLEN_LENS, lad.lat, fmt, device), make_cache("row", page, VARLEN_LENS, plain.lat, fmt, device)
    assert torch.equal(pool_bytes(c_l), pool_bytes(c_p))
    idx, cu, worst, n = lad.idx.to(device), lad.cu.to(device), 0.0, sum(COUNTS)
    call = lambda p, cache, causal: qa.fp8_mla_paged_sparse_varlen_func(p.q.to(device), cache, idx, cu, scale=C.SM_SCALE, causal=causal, return_lse=True, return_q8=True)
    for causal in (True, False):
        what = ("packed sparse", Hq, fmt, page, causal)
        (o, l, q8, sq), (o_s, l_s, q8_s, sq_s), (o_p, l_p, q8_p, sq_p) = call(lad, c_l, causal), call(slot, c_l, causal), call(plain, c_p, causal)
        assert torch.equal(q8_p[:n].float().cpu() * sq_p[:n].cpu()[..., None], plain.q[:n].float()), what
        assert_echo(q8, sq, q8_p, sq_p, lad.e_q, what)
        assert_echo(q8_s, sq_s, q8_p, sq_p, slot.e_q, what)
        ref, ref_p = varlen_reference(lad, causal), varlen_reference(plain, causal)
        worst = max(worst, grade_rows(o.float().cpu().numpy(), l.cpu().numpy().T, ref[0], ref[1], lad.e_rows, what)[0])
        assert torch.equal(l_s.view(torch.int32), l_p.view(torch.int32)), what
        assert_scaled_bits(o_s, o_p, slot.e_rows, stays_normal(ref_p[0], slot.e_rows, dtype), what)
        lo = 0
        for b, cnt in enumerate(COUNTS if chain else ()):
            rows = slice(lo, lo + cnt)
            lo += cnt
            if cnt:
                w_o, w_l, w_q8, w_sq = qa.fp8_mla_paged_sparse_func(lad.q[rows].to(device).transpose(0, 1)[None], one_slot(c_l, b), idx[rows][None], scale=C.SM_SCALE,
                                                                    causal=causal, num_splits=1, return_lse=True, return_q8=True)
                assert torch.equal(o[rows].view(torch.int16), w_o[0].transpose(0, 1).view(torch.int16)), (what, b)
                assert torch.equal(l[:, rows].view(torch.int32), w_l[0].view(torch.int32)), (what, b)
                assert torch.equal(q8[rows].view(torch.uint8), w_q8[0].transpose(0, 1).view(torch.uint8)) and torch.equal(sq[rows], w_sq[0].transpose(0, 1)), (what, b)
    return worst


# ---- the indexer: fp8_mla_index_topk_func, fp8_mla_index_topk_varlen_func ----------------------------------------------------------------------
ROUNDING = 256 * 2.0 ** -24                       # tests/test_gpu_mla_index.py's bound on random data: x the magnitude sum of a logit
JUDGED_KEYS = 16                                  # index teeth: rows with fewer live keys are not judged -- a logit moves by the sum over the
                                                  # TOUCHED heads of relu(q.k) w (wrong - right scale), and half the ReLU terms and 1 / 15 of
                                                  # the grid weights are zero: on a one-key row that sum can be 0 (it is, X.LENS[0] slot 1)


class Index:
    """q [B, Hi, Sq, 128] or [T, Hi, 128], w fp32 [B, Sq, Hi] or [T, Hi], keys [B, cap, 128] (CPU), scale fp32 [B], e [B], f [Hi, Sq] / [T, Hi]"""


def _index_keys(p, e, cap, dtype, seed=7):
    p.e, p.dtype, p.cap = e, dtype, cap
    p.keys = exact(C.draw((B, cap, X.D), seed + 100) * X.SCALE_K * t2(e)[:, None, None], dtype)
    p.scale = (X.SCALE_K * t2(e)).contiguous()


@functools.lru_cache(maxsize=None)
def index_inputs(Hi, Sq, dtype, ladder=True, weights="plain"):
    """weights "inverse": w x 2^-F (w scale_q is the plain call's); "plain": the logits change"""
    p = Index()
    _index_keys(p, E_SLOT if ladder else np.zeros(B, int), X.CAP, dtype)
    p.f = f_rows(Hi, Sq) if ladder else np.zeros((Hi, Sq), int)
    p.q = exact(X.make_q(Hi, Sq, torch.float32) * t2(p.f)[None, :, :, None], dtype)
    p.w = C.draw((B, Sq, Hi), 50) * (t2(-p.f.T)[None] if weights == "inverse" else 1.0)
    p.sq = (2.0 ** -7 * t2(p.f))[None].expand(B, -1, -1).contiguous()                   # scale_q by the kernel's rule: amax 3.5 2^F over 448
    p.q8 = (p.q.float() / p.sq[..., None]).to(torch.float8_e4m3fn)
    assert torch.equal(p.q8.float() * p.sq[..., None], p.q.float())
    return p


@functools.lru_cache(maxsize=None)
def index_varlen_inputs(shape, Hi, dtype, ladder=True, weights="plain"):
    p = Index()
    p.counts, p.lens = XP.SHAPES[shape]
    _index_keys(p, E_SLOT if ladder else np.zeros(B, int), XP.CAP, dtype)
    p.slot = slot_of_tokens(p.counts, XP.TOTAL)
    p.f = np.where((p.slot >= 0)[:, None], f_tokens(XP.TOTAL, Hi), 0) if ladder else np.zeros((XP.TOTAL, Hi), int)
    p.q = exact(X.make_q(Hi, XP.TOTAL, torch.float32)[0].transpose(0, 1) * t2(p.f)[..., None], dtype).contiguous()
    p.w = (C.draw((XP.TOTAL, Hi), 50) * (t2(-p.f) if weights == "inverse" else 1.0)).contiguous()
    p.sq = (2.0 ** -7 * t2(p.f)).contiguous()
    p.q8 = (p.q.float() / p.sq[..., None]).to(torch.float8_e4m3fn)
    p.cu = torch.tensor(np.concatenate([[0], np.cumsum(p.counts)]), dtype=torch.int32)
    return p


def make_icache(p, page, lens, fmt, device, seed=7):
    """mla_index_cases.make_icache with the ladder's keys and per-slot scales"""
    M = -(-p.cap // page)
    num_pages = B * M + 3
    g = torch.Generator().manual_seed(seed)
    icache = qa.alloc_paged_mla_index_cache_fp8(num_pages, page, batch_size=B, max_pages_per_seq=M, scale=p.scale, dtype=p.dtype, device=device, fp8_format=fmt)
    icache.pool.view(torch.uint8).fill_(0x7f)
    icache.block_table.copy_(torch.randperm(num_pages, generator=g)[: B * M].reshape(B, M).to(torch.int32))
    qa.paged_mla_index_cache_append_fp8(icache, p.keys.to(device), new_lens=torch.tensor(lens, dtype=torch.int32, device=device))
    assert icache.seqlens.tolist() == list(lens)
    return icache


def with_scale(icache, scale):
    return type(icache)(icache.pool, torch.as_tensor(scale, dtype=torch.float64), icache.block_table, icache.seqlens, icache.num_pages, icache.page_size,
                        icache.fp8_format, icache.dtype, icache.layout)


def index_reference(p, icache, lens, causal, sq=None, scale=None):
    """fp64 (logits [B, Sq, cap], magnitude sums) by mla_index_cases.ref_logits on the CPU cache's bytes and the scales of the construction"""
    return X.ref_logits(p.q8, p.sq if sq is None else sq, p.w, icache if scale is None else with_scale(icache, scale), lens, causal, p.cap)


def index_varlen_reference(p, icache, causal, sq=None, scale=None):
    """fp64 (logits [TOTAL, cap], magnitude sums): the dense reference per slot on the slot's tokens; padding rows: -inf"""
    sq = p.sq if sq is None else sq
    ic = icache if scale is None else with_scale(icache, scale)
    logits, mag, lo = np.full((XP.TOTAL, p.cap), -np.inf), np.zeros((XP.TOTAL, p.cap)), 0
    for b, n in enumerate(p.counts):
        if n:
            rows = slice(lo, lo + n)
            ex = lambda t: t[None].expand((B,) + tuple(t.shape))
            r, m = X.ref_logits(ex(p.q8[rows].transpose(0, 1)), ex(torch.as_tensor(sq[rows]).t()), ex(p.w[rows]), ic, p.lens, causal, p.cap)
            logits[rows], mag[rows] = r[b], m[b]
        lo += n
    return logits, mag


def fp32_exact(logits):
    """every live fp64 logit is an fp32 number"""
    live = np.isfinite(logits)
    return bool((logits[live].astype(np.float32).astype(np.float64) == logits[live]).all())


def index_teeth(ref, mag, mutants):
    """every row a mutant touches, with >= JUDGED_KEYS live keys, has a logit moved by >= TEETH x the rounding bound of the random-data tests;
    {mutant: rows judged}"""
    live, res = np.isfinite(ref), {}
    for name, (mut, touched) in mutants.items():
        rows = touched & (live.sum(-1) >= JUDGED_KEYS)
        assert rows.any(), (name, "touches no judged row")
        moved = np.where(live, np.abs(np.where(live, mut, 0.0) - np.where(live, ref, 0.0)) / np.maximum(ROUNDING * mag, 1e-300), 0.0).max(-1)
        assert (moved[rows] >= TEETH).all(), (name, "rows not shown", int((moved[rows] < TEETH).sum()))
        res[name] = int(rows.sum())
    return res


def index_mutants(p, icache, lens, causal):
    """{name: (logits, rows touched [B, Sq])} of the dense indexer"""
    s, sq = p.scale.double().numpy(), p.sq.double().numpy()
    res = {n: (index_reference(p, icache, lens, causal, scale=t)[0], np.broadcast_to((t != s)[:, None], sq[:, 0].shape)) for n, t in slot_tables(s).items()}
    q_tables = {"scale_q of head h+1": np.roll(sq, -1, 1), "scale_q of head h-1": np.roll(sq, 1, 1), "scale_q of row i+1": np.roll(sq, -1, 2),
                "scale_q of row i-1": np.roll(sq, 1, 2), "scale_q read as [B, Sq, H] (the layout of the weights)": transposed_read(sq)}
    res.update({n: (index_reference(p, icache, lens, causal, sq=torch.from_numpy(t))[0], (t != sq).any(1)) for n, t in q_tables.items()})
    return res


def index_varlen_mutants(p, icache, causal):
    """{name: (logits, rows touched [TOTAL])} of the packed indexer"""
    s, sq, n = p.scale.double().numpy(), p.sq.double().numpy(), sum(p.counts)
    own = s[p.slot[:n]]
    res, base = {}, index_varlen_reference(p, icache, causal)[0]
    for name, t in packed_slot_tables(s, p.slot, INDEX_TILE).items():
        ref = base.copy()
        ref[:n] *= (t / own)[:, None]
        res[name] = (ref, np.concatenate([t != own, np.zeros(XP.TOTAL - n, bool)]))
    q_tables = {"scale_q of head h+1": np.roll(sq[:n], -1, 1), "scale_q of head h-1": np.roll(sq[:n], 1, 1), "scale_q of token t+1": np.roll(sq[:n], -1, 0),
                "scale_q of token t-1": np.roll(sq[:n], 1, 0), "scale_q read as [Hi, total]": transposed_read(sq[:n])}
    for name, t in q_tables.items():
        full = sq.copy()
        full[:n] = t
        res[name] = (index_varlen_reference(p, icache, causal, sq=full)[0], (full != sq).any(1))
    return res


def _grade_logits(got, ref, mag, what):
    """the logits against fp64: bit for bit where every fp32 partial sum is exact (the sum of the magnitudes stays below 2^24 units), else the
    rounding bound of the random-data tests.  Returns the worst |err| / that bound."""
    live = np.isfinite(ref)
    assert np.array_equal(np.isneginf(got), ~live), what
    if not live.any():
        return 0.0
    if fp32_exact(ref):
        assert np.array_equal(got[live], ref[live]), what
    worst = float((np.abs(got[live] - ref[live]) / np.maximum(ROUNDING * mag[live], 1e-300)).max())
    assert worst < 1.0, (what, worst)
    return worst


def check_index(Hi, Sq, page, fmt, dtype, device, topk=64, lens_sets=X.LENS):
    """The dense indexer, causal and not: the plain-weights ladder against fp64, the echo, and the inverse-weights ladder against the plain call
    (logits 2^E_SLOT[b] x plain bit for bit, equal indices).  Returns the worst |err| / rounding bound (0: bit for bit)."""
    lad, inv, plain = index_inputs(Hi, Sq, dtype), index_inputs(Hi, Sq, dtype, weights="inverse"), index_inputs(Hi, Sq, dtype, False)
    worst = 0.0
    call = lambda p, ic, causal: qa.fp8_mla_index_topk_func(p.q.to(device), p.w.to(device), ic, topk, causal=causal, max_seqlen_k=p.cap, return_logits=True, return_q8=True)
    for lens in lens_sets:
        ic_l, ic_p, ic_ref = make_icache(lad, page, lens, fmt, device), make_icache(plain, page, lens, fmt, device), make_icache(lad, page, lens, fmt, "cpu")
        assert torch.equal(pool_bytes(ic_l), pool_bytes(ic_p)) and torch.equal(pool_bytes(ic_l), pool_bytes(ic_ref)), lens
        for causal in (True, False):
            what = ("index", Hi, Sq, page, fmt, lens, causal)
            (i_l, g_l, q8, sq), (i_i, g_i, q8_i, sq_i), (i_p, g_p, q8_p, sq_p) = call(lad, ic_l, causal), call(inv, ic_l, causal), call(plain, ic_p, causal)
            assert_echo(q8, sq, q8_p, sq_p, lad.f[None], what)
            assert torch.equal(q8.view(torch.uint8).cpu(), lad.q8.view(torch.uint8)) and torch.equal(sq.cpu(), lad.sq), what
            ref, mag = index_reference(lad, ic_ref, lens, causal)
            worst = max(worst, _grade_logits(g_l.double().cpu().numpy(), ref, mag, what))
            assert torch.equal(i_l.cpu(), X.ref_select(g_l, lens, topk, causal)), what
            assert torch.equal(g_i.cpu().view(torch.int32), (g_p.cpu() * t2(lad.e)[:, None, None]).view(torch.int32)), what
            assert torch.equal(i_i, i_p), what
    return worst


def check_index_varlen(shape, Hi, page, fmt, dtype, device, topk=24, chain=True):
    """The packed indexer: as check_index, and (chain) the ladder against the dense entry on every slot's tokens bit for bit."""
    lad, inv, plain = (index_varlen_inputs(shape, Hi, dtype, *a) for a in ((True, "plain"), (True, "inverse"), (False, "plain")))
    ic_l, ic_p, ic_ref = make_icache(lad, page, lad.lens, fmt, device), make_icache(plain, page, lad.lens, fmt, device), make_icache(lad, page, lad.lens, fmt, "cpu")
    assert torch.equal(pool_bytes(ic_l), pool_bytes(ic_p)) and torch.equal(pool_bytes(ic_l), pool_bytes(ic_ref))
    cu, worst, e_tok = lad.cu.to(device), 0.0, np.where(lad.slot >= 0, E_SLOT[np.maximum(lad.slot, 0)], 0)
    call = lambda p, ic, causal: qa.fp8_mla_index_topk_varlen_func(p.q.to(device), p.w.to(device), ic, cu, topk, causal=causal, max_seqlen_k=p.cap, return_logits=True, return_q8=True)
    for causal in (True, False):
        what = ("packed index", shape, Hi, page, fmt, causal)
        (i_l, g_l, q8, sq), (i_i, g_i, q8_i, sq_i), (i_p, g_p, q8_p, sq_p) = call(lad, ic_l, causal), call(inv, ic_l, causal), call(plain, ic_p, causal)
        assert_echo(q8, sq, q8_p, sq_p, lad.f, what)
        n = sum(lad.counts)
        assert torch.equal(q8[:n].view(torch.uint8).cpu(), lad.q8[:n].view(torch.uint8)) and torch.equal(sq[:n].cpu(), lad.sq[:n]), what
        ref, mag = index_varlen_reference(lad, ic_ref, causal)
        worst = max(worst, _grade_logits(g_l.double().cpu().numpy(), ref, mag, what))
        assert torch.equal(g_i.cpu().view(torch.int32), (g_p.cpu() * t2(e_tok)[:, None]).view(torch.int32)), what
        assert torch.equal(i_i, i_p), what
        lo = 0
        for b, cnt in enumerate(lad.counts if chain else ()):
            rows = slice(lo, lo + cnt)
            lo += cnt
            if cnt:
                qd, wd = lad.q[rows].to(device).transpose(0, 1)[None].expand(B, -1, -1, -1), lad.w[rows].to(device)[None].expand(B, -1, -1)
                d_i, d_g = qa.fp8_mla_index_topk_func(qd, wd, ic_l, topk, causal=causal, max_seqlen_k=lad.cap, return_logits=True)
                assert torch.equal(g_l[rows].view(torch.int32), d_g[b].view(torch.int32)) and torch.equal(i_l[rows], d_i[b]), (what, b)
    return worst


# ---- prefill: fp8_mla_prefill_varlen_func ------------------------------------------------------------------------------------------------------
class Prefill:
    """q [tq, H, 192], kv [tk, H, 256] = k_nope | v, k_pe [tk, 64] (CPU), seq_q / seq_k: the sequence of every row, e_k [7, H], e_v [7, H]"""


@functools.lru_cache(maxsize=None)
def prefill_inputs(dtype, gains=True, gh=True):
    """grid data with the abs-max of every (sequence, head) planted in row 0 of the sequence: 3.5 in k_nope (k_pe stays <= 3) and 1.75 in V
    = grid x 0.5 (rms 0.76), q's channel 0 = +-3.5.  gains: the ladder; gh: with the per-head gain GH of k_nope (off: K and q carry EK alone,
    every score is the plain call's)"""
    p, H, lens = Prefill(), PREFILL_H, PF.LENS
    p.seq_q, p.seq_k = (np.repeat(np.arange(len(lens)), [l[j] for l in lens]) for j in (0, 1))
    tq, tk = len(p.seq_q), len(p.seq_k)
    q, kn, v, kp = C.draw((tq, H, MP.D_QK), 300), C.draw((tk, H, MP.D_NOPE), 301), C.draw((tk, H, MP.D_V), 302) * 0.5, C.draw((tk, MP.D_ROPE), 303)
    q[..., 0] = 3.5 * torch.where(C.draw((tq, H), 304) < 0, -1.0, 1.0)
    first = torch.tensor([k0 for k0, (_, lk) in zip(np.cumsum([0] + [b for _, b in lens]).tolist(), lens) if lk > 0])
    kn[first, :, 0], v[first, :, 0] = 3.5, 1.75
    ek = (EK if gains else np.zeros(len(lens), int))[:, None] + (GH if gains and gh else np.zeros(H, int))[None, :]
    p.e_pe = EK if gains else np.zeros(len(lens), int)
    p.e_k, p.e_v = ek, (EV if gains else np.zeros((len(lens), H), int))
    p.q = exact(q * t2(-ek[p.seq_q])[..., None], dtype)
    p.kv = exact(torch.cat([kn * t2(ek[p.seq_k])[..., None], v * t2(p.e_v[p.seq_k])[..., None]], dim=-1), dtype)
    p.k_pe = exact(kp * t2(p.e_pe[p.seq_k])[:, None], dtype)
    p.e_rows, p.dtype = p.e_v[p.seq_q], dtype
    return p


def prefill_scales(p, fmt):
    """(scale_k, scale_v) fp32 [7, H] by the header's rule: max(amax / fmax, 2^-23) over the sequence's k_nope of the head and its shared k_pe /
    over its v -- computed here from the inputs"""
    H, tdt = p.kv.shape[1], PF.TDT[fmt]
    ak, av, k0 = torch.zeros((len(PF.LENS), H)), torch.zeros((len(PF.LENS), H)), 0
    for i, (_, lk) in enumerate(PF.LENS):
        if lk:
            rows = slice(k0, k0 + lk)
            ak[i] = torch.maximum(p.kv[rows, :, :MP.D_NOPE].float().abs().amax(dim=(0, 2)), p.k_pe[rows].float().abs().amax())
            av[i] = p.kv[rows, :, MP.D_NOPE:].float().abs().amax(dim=(0, 2))
        k0 += lk
    return MP.kv_scale_eager(ak, tdt), MP.kv_scale_eager(av, tdt)


def prefill_reference(p, fmt, causal, sk_read=None, sv_read=None):
    """(out [tq, H, 128], lse [tq, H]) fp64: K and V quantised by the eager quantiser under prefill_scales; a mutant de-quantises the same bytes
    with the scales it reads"""
    sk, sv = prefill_scales(p, fmt)
    kd, vd = PF.dequantised_kv(p.kv, p.k_pe, sk, sv, fmt)
    if sk_read is not None:
        kd = kd * (sk_read / sk.double().numpy())[p.seq_k][..., None]
    if sv_read is not None:
        vd = vd * (sv_read / sv.double().numpy())[p.seq_k][..., None]
    out, lse = PF.reference(p.q.double().numpy(), kd, vd, causal)
    return out, lse.T


def prefill_mutants(p, fmt):
    """{name: (scale_k read, scale_v read, score_ratio [tq, H], out_ratio [tq, H])}"""
    sk, sv = (t.double().numpy() for t in prefill_scales(p, fmt))
    res = {}
    for name, ax, r in (("sequence i+1", 0, -1), ("sequence i-1", 0, 1), ("head h+1", 1, -1), ("head h-1", 1, 1)):
        res[f"scale_k of {name}"] = (np.roll(sk, r, ax), None)
        res[f"scale_v of {name}"] = (None, np.roll(sv, r, ax))
    res["scale_k used for V"] = (None, sk)
    one = np.ones(p.e_rows.shape)
    return {n: (a, b, one if a is None else (a / sk)[p.seq_q], one if b is None else (b / sv)[p.seq_q]) for n, (a, b) in res.items()}


def prefill_teeth(p, fmt, causal):
    ref = prefill_reference(p, fmt, causal)
    sk = prefill_scales(p, fmt)[0].double().numpy()
    lone = lone_rows(ref, prefill_reference(p, fmt, causal, 0.5 * sk))
    return {n: teeth(n, ref, prefill_reference(p, fmt, causal, a, b), sr, orr, p.e_rows, lone) for n, (a, b, sr, orr) in prefill_mutants(p, fmt).items()}


def check_prefill(fmt, dtype, causal, device):
    """The ladder against the fp64 reference, the echo (q8; scale_q, scale_k, scale_v exactly 2^e times the plain call's), and the ladder without
    GH against the plain call: lse bit for bit, out = 2^EV x plain.  Returns the worst |err| / bound."""
    lad, flat, plain = prefill_inputs(dtype), prefill_inputs(dtype, gh=False), prefill_inputs(dtype, False)
    cu_q, cu_k = (t.to(device) for t in PF.tables())
    def call(p):
        with qa.config.patch({"attention.fp8_format": fmt}):
            return qa.fp8_mla_prefill_varlen_func(p.q.to(device), p.kv.to(device)[..., :128], p.k_pe.to(device), p.kv.to(device)[..., 128:], cu_q, cu_k, 130, 200,
                                                  scale=PF.SM_SCALE, causal=causal, return_lse=True, return_quantized=True)
    what = ("prefill", fmt, dtype, causal)
    got, got_f, got_p = call(lad), call(flat), call(plain)
    has_keys = torch.tensor([lk > 0 for _, lk in PF.LENS])[:, None]
    for p, g in ((lad, got), (flat, got_f)):
        assert_echo(g[2], g[3], got_p[2], got_p[3], -p.e_k[p.seq_q], what)
        assert torch.equal(g[4].cpu(), torch.where(has_keys, got_p[4].cpu() * t2(p.e_k), got_p[4].cpu())), what          # (no key: the floor, no gain)
        assert torch.equal(g[5].cpu(), torch.where(has_keys, got_p[5].cpu() * t2(p.e_v), got_p[5].cpu())), what
        sk, sv = prefill_scales(p, fmt)
        assert torch.equal(g[4].cpu(), sk) and torch.equal(g[5].cpu(), sv), what
    assert torch.equal(got_p[2].float().cpu() * got_p[3].cpu()[..., None], plain.q.float()), what
    ref, ref_p = prefill_reference(lad, fmt, causal), prefill_reference(plain, fmt, causal)
    worst = grade_rows(got[0].float().cpu().numpy(), got[1].cpu().numpy().T, ref[0], ref[1], lad.e_rows, what)[0]
    assert torch.equal(got_f[1].view(torch.int32), got_p[1].view(torch.int32)), what
    assert_scaled_bits(got_f[0], got_p[0], flat.e_rows, stays_normal(ref_p[0], flat.e_rows, dtype), what)
    return worst

"""The rotary embedding at the CALLER's positions on the MI355X (quantumattention_amd/paged_varlen.py
`paged_kv_cache_append_varlen_rope_pos_fp8` / `apply_rope_positions`, quantumattention_amd/tree.py `tree_positions`,
include/qattn_paged_varlen_rope_pos.h).

THE RULES, byte for byte.  (1) From the same starting state the positions append leaves pools and seqlens as "rotate K in torch
(apply_rope_eager) at clamp(positions, 0, T - 1), then paged_kv_cache_append_varlen_fp8" leaves them -- for positions that repeat
(siblings), descend and lie outside [0, T); whole pools are compared, pre-filled with a sentinel byte, so a stray store shows.
(2) apply_rope_positions is apply_rope_eager at those positions.  (3) With positions[start_b + t] = seqlens[b] + t both give the bits of
the fused entries of include/qattn_paged_varlen_rope.h.  Then a gpt-oss-shaped tree step over two rounds -- tree_positions -> rotate q ->
positions append -> tree-window-sink attend -> compact -- against an fp64 shadow that rotates at base + depth."""
import math

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import gpu_utils
from tests import kvcache_cases as KC
from tests import paged_cases as PC
from tests import paged_varlen_rope_cases as RC
from tests import probes
from tests import serving_trace_rope_sinks as RS
from tests import tree_cases as TC
from tests import tree_window_cases as W
from tests.test_gpu_paged_varlen_rope import MATRIX, MATRIX_IDS, _cache, _clone, _pool_rows, _same_bits, _same_state, _su, _tokens

pytestmark = pytest.mark.gpu

DEV = "cuda"
HKV, CAP, T, SENTINEL = RC.HKV, RC.CAP, RC.T, RC.SENTINEL
COUNTS = [0, 1, 2, 17, 63, 64, 65, 130]
STARTS = [5, 0, 1, 40, 63, 64, 104, 127]        # p mod 64 in {0, 1, 40, 63} (and 5); the last slot drops its tail: 127 + 130 > 256
B = len(COUNTS)
TOTAL = sum(COUNTS)
HQ = 2 * HKV


def _positions(seed, total=TOTAL, rows=T):
    """per slot: siblings (runs of one value), a descending run, values below 0 and at or above T -- and a few honest ones"""
    rng = np.random.RandomState(seed)
    pos = rng.randint(0, rows, total).astype(np.int64)
    cu = RC.cu_list(COUNTS)
    for i, n in enumerate(COUNTS):
        if n >= 17:
            s = cu[i]
            pos[s + 2:s + 6] = pos[s + 1]                          # siblings
            pos[s + 6:s + 12] = np.arange(40, 34, -1)              # descending
            pos[s + 12], pos[s + 13], pos[s + 14] = -3, rows, rows + (1 << 40)
            pos[s + 15] = -(1 << 62)
    return pos


def _clamped(pos, rows=T):
    return np.clip(pos, 0, rows - 1).tolist()


def _rule(cache, k, v, cu, pos, cos, sin, il, advance):
    k_rot = RC.rotate_at(k, _clamped(pos, cos.shape[0]), cos, sin, il)
    return qa.paged_kv_cache_append_varlen_fp8(cache, k_rot, v, cu, advance=advance)


# ---- 1. the append's rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype,fmt,page_size,il", MATRIX, ids=MATRIX_IDS)
def test_the_positions_append_leaves_pools_and_seqlens_as_rotating_in_torch_then_the_plain_append_leaves_them(D, dtype, fmt, page_size, il):
    c0 = _cache(D, dtype, fmt, page_size, seed=D + page_size, starts=STARTS)
    k, v = _tokens(TOTAL, D, dtype, 3 * D + page_size)
    k[5, 0, 3], k[70, 1, 0], k[200, 0, 1] = float("inf"), float("nan"), -float("inf")      # inf x 0 = NaN in the rotation, as in the composition
    if dtype == torch.float16:
        k[150, 1, :4] = 60000.0                                                           # an fp16 product that overflows in the rotation
    cu = _su(RC.cu_list(COUNTS))
    cos, sin = RC.tables(D, device=DEV)
    pos = _positions(D + page_size)
    assert pos.min() < 0 and pos.max() >= T
    posd = torch.from_numpy(pos).to(DEV)
    mine = None
    for advance in (True, False):
        a, b, p = _clone(c0), _clone(c0), _clone(c0)
        assert qa.paged_kv_cache_append_varlen_rope_pos_fp8(a, k, v, cu, posd, cos, sin, interleaved=il, advance=advance) is a
        _rule(b, k, v, cu, pos, cos, sin, il, advance)
        assert torch.equal(a.k, b.k), "K pool"
        assert torch.equal(a.v, b.v), "V pool"
        assert torch.equal(a.seqlens, b.seqlens)
        assert a.seqlens.tolist() == ([min(s + n, CAP) for s, n in zip(STARTS, COUNTS)] if advance else STARTS)
        # these positions are not the keys' indices: the fused entry at the cache's positions leaves other K bytes, the same V bytes
        qa.paged_kv_cache_append_varlen_rope_fp8(p, k, v, cu, cos, sin, interleaved=il, advance=advance)
        assert torch.equal(a.v, p.v) and not torch.equal(a.k, p.k)
        mine = a
    # exactly the appended keys' bytes changed: every other byte is still the sentinel
    table = c0.block_table.cpu().numpy()
    for pool in _pool_rows(mine):
        own = np.zeros(pool.shape[:3], bool)
        for i in range(B):
            keys = np.arange(STARTS[i], min(STARTS[i] + COUNTS[i], CAP))
            own[table[i][keys // page_size], :, keys % page_size] = True
        assert (pool[~own] == SENTINEL).all(), "a byte of a key the call does not append changed"
    assert STARTS[7] + COUNTS[7] > CAP       # (the dropped tail is in the matrix)


# ---- 2. sequential positions: the fused entries' bits --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype,fmt,page_size,il", MATRIX, ids=MATRIX_IDS)
def test_sequential_positions_give_the_bits_of_the_entries_at_the_caches_positions(D, dtype, fmt, page_size, il):
    c0 = _cache(D, dtype, fmt, page_size, seed=7 + D, starts=STARTS)
    k, v = _tokens(TOTAL, D, dtype, 5 * D + page_size)
    cu = _su(RC.cu_list(COUNTS))
    cos, sin = RC.tables(D, device=DEV)
    seq = torch.tensor(RC.positions(COUNTS, STARTS, TOTAL), dtype=torch.int64, device=DEV)
    a, b = _clone(c0), _clone(c0)
    qa.paged_kv_cache_append_varlen_rope_pos_fp8(a, k, v, cu, seq, cos, sin, interleaved=il)
    qa.paged_kv_cache_append_varlen_rope_fp8(b, k, v, cu, cos, sin, interleaved=il)
    assert _same_state(a, b) and not torch.equal(a.k, c0.k)
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(TOTAL, HQ, D, generator=g) * 2).to(dtype).to(DEV)
    assert _same_bits(qa.apply_rope_positions(x, seq, cos, sin, interleaved=il), qa.apply_rope_paged_varlen(x, c0, cu, cos, sin, interleaved=il))


# ---- 3. apply_rope_positions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype,fmt,page_size,il", MATRIX[::2], ids=MATRIX_IDS[::2])
def test_apply_rope_positions_is_apply_rope_eager_at_the_clamped_positions_bit_for_bit(D, dtype, fmt, page_size, il):
    g = torch.Generator().manual_seed(D + 1)
    qkv = (torch.randn(TOTAL, HQ + 2 * HKV, D, generator=g) * 2).to(dtype).to(DEV)
    qkv[3, 1, 2], qkv[9, 0, 0] = float("inf"), float("nan")
    if dtype == torch.float16:
        qkv[20, 2, :4] = 60000.0
    x = qkv[:, :HQ]                                                 # a strided q slice of the packed projection
    assert not x.is_contiguous()
    cos, sin = RC.tables(D, device=DEV)
    pos = _positions(D + 3)
    posd = torch.from_numpy(pos).to(DEV)
    want = RC.rotate_at(x, _clamped(pos), cos, sin, il)
    got = qa.apply_rope_positions(x, posd, cos, sin, interleaved=il)
    assert got.is_contiguous() and _same_bits(got, want.contiguous())
    out = torch.full((TOTAL, HQ, D), 7.0, dtype=dtype, device=DEV)
    assert qa.apply_rope_positions(x, posd, cos, sin, interleaved=il, out=out) is out and _same_bits(out, got)
    assert _same_bits(qa.apply_rope_positions(x.contiguous(), posd, cos.bfloat16(), sin.bfloat16(), interleaved=il),
                      qa.apply_rope_positions(x, posd, cos.bfloat16().float(), sin.bfloat16().float(), interleaved=il))
    assert qa.apply_rope_positions(x[:0], posd[:0], cos, sin).shape == (0, HQ, D)


def test_tree_positions_on_the_device_is_the_plain_walk():
    for name, (G, sq, lens) in W.CASES.items():
        for kind in ("chain", "star", "binary", "random", "junk"):
            words = TC.words_of(kind, sq, 3)[0]
            cu = RC.cu_list(sq)
            for appended in (False, True):
                base = [max(L - n, 0) for n, L in zip(sq, lens)]
                lens_in = [b_ + n for b_, n in zip(base, sq)] if appended else base
                want = [base[b] + W.depth_of(words, cu[b], n, p) for b, n in enumerate(sq) for p in range(n)]
                got = qa.tree_positions(torch.from_numpy(TC.as_int64(words)).to(DEV), _su(cu), _su(lens_in), appended=appended)
                assert got.dtype == torch.int64 and got.tolist() == want, (name, kind, appended)


# ---- 4. a gpt-oss-shaped tree step over two rounds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("left", [127, -1])
def test_two_rounds_of_a_gpt_oss_shaped_tree_step_against_an_fp64_shadow_that_rotates_at_base_plus_depth(left):
    """D 64, Hq 8, Hkv 2, 3 slots.  Per round: tree_positions -> apply_rope_positions on q -> positions append -> tree-window-sink attend
    -> compact.  The shadow keeps, per slot, the fp64-rotated (base + depth), once-rounded, reference-quantised K bytes and the V bytes of
    its live keys.  The K-byte allowance is tests/serving_trace_rope_sinks.py's: a live K byte may sit ONE CODE beside the shadow's (the
    product rotates in fp32) on at most 2^-14 of the live bytes; V bytes and lengths are exact.  The attention is graded against the fp64
    reference on the bytes the cache holds (tests/gpu_utils.assert_within_bound, probes.LSE_TOL); the rotated q against the fp64
    rotation by serving_trace_rope_sinks.q_ratio <= 1."""
    D, dtype, fmt, ps, G = 64, torch.bfloat16, "e4m3", 128, 4
    Hq, fp8 = HKV * G, PC.FP8[fmt]
    nB, cap = 3, 1280
    M = cap // ps
    gen = torch.Generator().manual_seed(5)
    sk, sv = torch.rand(nB, HKV, generator=gen) * 0.02 + 0.03, torch.rand(nB, HKV, generator=gen) * 0.02 + 0.03
    c = qa.alloc_paged_kv_cache_fp8(nB * M + 2, HKV, ps, D, batch_size=nB, max_pages_per_seq=M, scale_k=sk.to(DEV), scale_v=sv.to(DEV), dtype=dtype,
                                    device=DEV, fp8_format=fmt)
    c.block_table.copy_(torch.randperm(nB * M + 2, generator=gen)[:nB * M].view(nB, M).to(torch.int32))
    cos, sin = RS.tables(D, rows=cap)
    cosd, sind = cos.to(DEV), sin.to(DEV)
    sinks = torch.tensor(RS.SINKS, dtype=torch.float32)[:Hq] - 4.0
    shadow_k = [np.zeros((HKV, 0, D), np.uint8) for _ in range(nB)]
    shadow_v = [np.zeros((HKV, 0, D), np.uint8) for _ in range(nB)]

    def quant(x16, scale):        # x16 [n, HKV, D] 16-bit -> uint8 [HKV, n, D]
        return KC.quant_ref(x16.transpose(0, 1)[None], scale[None], fp8)[0].numpy()

    def append_shadow(k16, v16, cu, pos):
        for b in range(nB):
            rows = slice(cu[b], cu[b + 1])
            y, _ = RS.rotate64(k16[rows].cpu(), pos[rows], cos, sin, False)
            shadow_k[b] = np.concatenate([shadow_k[b], quant(RS.round_once(y, dtype), sk[b])], 1)
            shadow_v[b] = np.concatenate([shadow_v[b], quant(v16[rows].cpu(), sv[b])], 1)

    # the committed keys: a plain prefill at sequential positions through the same positions append
    base = [700, 200, 64]
    cu0 = RC.cu_list(base)
    k0, v0 = ((torch.randn(sum(base), HKV, D, generator=gen) * 1.5).to(dtype).to(DEV) for _ in range(2))
    pos0 = [t for n in base for t in range(n)]
    qa.paged_kv_cache_append_varlen_rope_pos_fp8(c, k0, v0, _su(cu0), torch.tensor(pos0, dtype=torch.int64, device=DEV), cosd, sind)
    append_shadow(k0, v0, cu0, pos0)
    diff = live = 0
    for rnd, (sq, kind) in enumerate((((40, 17, 5), "binary"), ((33, 60, 2), "random"))):
        cu, total, mx = RC.cu_list(sq), sum(sq), max(sq)
        words, parents = TC.words_of(kind, sq, rnd)
        wd, cud = torch.from_numpy(TC.as_int64(words)).to(DEV), _su(cu)
        lens0 = c.seqlens.tolist()
        assert lens0 == [x.shape[1] for x in shadow_k]
        q, kd, vd = ((torch.randn(total, h, D, generator=gen) * 1.5).to(dtype).to(DEV) for h in (Hq, HKV, HKV))
        pos = qa.tree_positions(wd, cud, c.seqlens)
        want_pos = [lens0[b] + W.depth_of(words, cu[b], n, p) for b, n in enumerate(sq) for p in range(n)]
        assert pos.tolist() == want_pos
        q_rot = qa.apply_rope_positions(q, pos, cosd, sind)
        assert RS.q_ratio(q_rot.double().cpu().numpy(), RS.rotate64(q.cpu(), want_pos, cos, sin, False), dtype) <= 1.0
        qa.paged_kv_cache_append_varlen_rope_pos_fp8(c, kd, vd, cud, pos, cosd, sind)
        append_shadow(kd, vd, cu, want_pos)
        lens = c.seqlens.tolist()
        assert lens == [a + n for a, n in zip(lens0, sq)] == [x.shape[1] for x in shadow_k]
        # the state: V bytes exact, K bytes within one code on at most 2^-14 of the live bytes
        rk, rv = (KC.from_image(img, layout, c.num_pages, HKV, ps, D).cpu().numpy() for img, layout in ((c.k, KC.KFRAG), (c.v, KC.VFRAG)))
        table = c.block_table.cpu().numpy()
        held_k, held_v = [], []
        for b, L in enumerate(lens):
            keys = np.arange(L)
            gk, gv = rk[table[b][keys // ps], :, keys % ps].transpose(1, 0, 2), rv[table[b][keys // ps], :, keys % ps].transpose(1, 0, 2)
            assert np.array_equal(gv, shadow_v[b]), (rnd, b)
            assert RS.one_code(gk, shadow_k[b], fmt).all(), (rnd, b)
            diff, live = diff + int((gk != shadow_k[b]).sum()), live + gk.size
            held_k.append(gk)
            held_v.append(gv)
        # the attention, on the bytes the cache holds
        out, lse, q8, sqs, path = _native.fp8_attention_paged_varlen(
            q_rot, c.k, c.v, c.scale_k, c.scale_v, c.block_table, c.seqlens, cud, max_seqlen_q=mx, Skv=cap, num_pages=c.num_pages, page_size=ps,
            fp8_dtype=fp8, num_splits=(1, 3)[rnd], return_lse=True, return_quant=True, return_path=True, tree_mask=wd, window=(left, 0),
            sinks=sinks.to(DEV))
        pub = qa.fp8_attn_paged_varlen_tree_window_func(q_rot, c, cud, mx, wd, (left, 0), sinks=sinks.to(DEV), num_splits=(1, 3)[rnd], return_lse=True)
        assert _same_bits(pub[0], out) and _same_bits(pub[1], lse)
        q8f = q8.view(torch.uint8).view(fp8).float().cpu().numpy().astype(np.float64)
        qd = np.zeros((total, Hq, D))
        for b, n in enumerate(sq):
            qd[cu[b]:cu[b + 1]] = (q8f[Hq * D * cu[b]:Hq * D * cu[b + 1]].reshape(Hq, n, D) * sqs[b].cpu().numpy().astype(np.float64)[:, None, None]).transpose(1, 0, 2)
        deq = lambda held, s: np.stack([np.pad(torch.from_numpy(h).view(fp8).float().numpy().astype(np.float64) * s[b].double().numpy()[:, None, None],
                                               ((0, 0), (0, cap - h.shape[1]), (0, 0))) for b, h in enumerate(held)])
        ref, ref_lse = W.reference(qd, deq(held_k, sk), deq(held_v, sv), lens, sq, G, words, 1.0 / math.sqrt(D), left, sinks.double().numpy())
        o = gpu_utils.out_to_f32(out)
        gpu_utils.assert_within_bound(o.transpose(1, 0, 2), gpu_utils.PathRef(ref.transpose(1, 0, 2), ref.transpose(1, 0, 2)), path.cpu().numpy(),
                                      what=("tree step", left, rnd))
        assert float(np.abs(lse.cpu().numpy() - ref_lse).max()) < probes.LSE_TOL
        # verify: accept a root-to-leaf path (the chain of parents of the last draft), then compact
        idx, cnt = [], []
        for b, n in enumerate(sq):
            path_b, a = [], n - 1
            while a >= 0:
                path_b.append(a)
                a = parents[cu[b] + a]
            path_b = path_b[::-1]
            idx += path_b + [0] * (n - len(path_b))
            cnt.append(len(path_b))
            keep = [lens0[b] + i for i in path_b]
            shadow_k[b] = np.concatenate([shadow_k[b][:, :lens0[b]], shadow_k[b][:, keep]], 1)
            shadow_v[b] = np.concatenate([shadow_v[b][:, :lens0[b]], shadow_v[b][:, keep]], 1)
        qa.paged_kv_cache_compact_fp8(c, cud, _su(idx), _su(cnt))
        assert c.seqlens.tolist() == [a + n for a, n in zip(lens0, cnt)]
        # an accepted path sits at base + 0, 1, 2, ...: the next round's committed keys carry the positions of a plain decode
        for b, n in enumerate(cnt):
            assert [want_pos[cu[b] + i] for i in idx[cu[b]:cu[b] + n]] == list(range(lens0[b], lens0[b] + n))
    print(f"tree step left={left}: {diff} of {live} live K bytes one code beside the shadow's")
    assert diff <= RS.K_SHARE_CAP * live, (diff, live)

"""-m gpu: split-KV FP8 attention over prepared K / V (qa.fp8_attn_splitkv_func, qattn_fp8_attention_splitkv_forward,
include/qattn_splitkv.h) on the MI355X.

Grading: per batch element the fp64 oracle (oracle.attention_forward, causal with q_offset = L_b - Sq) on the entry's own q8 rows and on the
prepared bytes and scales cut to the used keys; bound gpu_utils.grade, |got - ref| < 2^-6 max(1, |ref| / 2); LSE within 2e-3.  q8 / scale_q
and the prepared images equal the CPU quantiser's bit for bit, row_path equals the literal table of tests/splitkv_cases.py.  Then the
contract of the header, bit for bit: (a) out, lse = the merge of the partials; (b) a partial = the block-sparse FP8-PV entry under the mask
of the split's key blocks; (c) causal, one split = the sliding-window FP8-PV entry at (-1, 0); (d) a (k, v) pair = prepared K / V; (e) a
batched call = its per-element calls; (f) graph replay = eager, also after seqused_k is rewritten.  Then the membership probes at the split
boundaries, the causal edge and seqused_k, and torch.compile."""
import functools
import math

import numpy as np
import pytest
import torch

import oracle
import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import gpu_utils
from tests import probes as P
from tests import splitkv_cases as S
from tests.gpu_utils import FMT, TDT, bits8, bits16, fmt16

pytestmark = pytest.mark.gpu
DEV = "cuda"
NB = 128
ONE, TWO = 0, 1   # include/qattn.h QATTN_PATH_ONE_TERM / _TWO_TERM (literal: the header is the contract)
LSE_TOL = 2e-3


def _rand(shape, dtype, g):
    return torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32).to(dtype)


def _same_bits(x, y):
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
    return torch.equal(x.contiguous().view(view[x.element_size()]), y.contiguous().view(view[y.element_size()]))


def _qkv(seed, dtype=torch.bfloat16, B=1, Hq=4, Hkv=4, Sq=130, Skv=1100, D=128):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return _rand((B, Hq, Sq, D), dtype, g), _rand((B, Hkv, Skv, D), dtype, g), _rand((B, Hkv, Skv, D), dtype, g)


def _su(used):
    return None if used is None else torch.tensor(used, dtype=torch.int32, device=DEV)


def _call(q, kv, *, causal=False, ns=1, precision="accurate", used=None, scale=None, lse=True):
    """(out, lse | None, partial_o, partial_lse, partial_path, q8, scale_q, row_path) through the C entry"""
    res = _native.fp8_attention_splitkv(q, kv.k, kv.v, kv.scale_k, kv.scale_v, Skv=kv.shape[2], fp8_dtype=TDT[kv.fp8_format], numerics=kv.numerics,
                                        is_causal=causal, sm_scale=0.0 if scale is None else scale, precision=precision, num_splits=ns,
                                        seqused_k=_su(used), return_lse=lse, return_partials=True, return_quant=True, return_path=True)
    return res if lse else (res[0], None) + tuple(res[1:])


def _check_quantisers(res, q, k, v, kv):
    """q8 / scale_q of the call and the prepared images and scales against the CPU quantiser, bit for bit"""
    fp8 = kv.fp8_format
    rb, rs = oracle.quantize_fp8(bits16(q), fmt16(q.dtype), "head", FMT[fp8], "compiled")
    assert np.array_equal(bits8(res[5]), rb) and np.array_equal(res[6].cpu().numpy().view(np.uint32), rs.view(np.uint32))
    B, Hkv, Skv, D = kv.shape
    for x, img, s, layout in ((k, kv.k, kv.scale_k, _native.LAYOUT_KFRAG), (v, kv.v, kv.scale_v, _native.LAYOUT_VFRAG)):
        rb, rs = oracle.quantize_fp8(bits16(x), fmt16(x.dtype), "head", FMT[fp8], "compiled")
        got = gpu_utils.unpack_frag(img.cpu().numpy(), layout, B, Hkv, Skv, D)
        assert np.array_equal(got[:, :, :Skv], rb) and (got[:, :, Skv:] == 0).all()
        assert np.array_equal(s.cpu().numpy().view(np.uint32), rs.view(np.uint32))


def _prepared_rows(kv):
    """row-major uint8 [B, Hkv, Skv, D] of the two images"""
    B, Hkv, Skv, D = kv.shape
    return (gpu_utils.unpack_frag(kv.k.cpu().numpy(), _native.LAYOUT_KFRAG, B, Hkv, Skv, D)[:, :, :Skv],
            gpu_utils.unpack_frag(kv.v.cpu().numpy(), _native.LAYOUT_VFRAG, B, Hkv, Skv, D)[:, :, :Skv])


def _grade(res, kv, rows8, used, causal, scale, what, want_lse=True):
    """every batch element against the fp64 oracle on the returned q8 rows and the prepared bytes cut to the used keys; prints and returns
    the worst |err| / bound"""
    out, lse, q8, sq = res[0], res[1], res[5], res[6]
    B, Hq, Sq, D = out.shape
    Skv = kv.shape[2]
    f = FMT[kv.fp8_format]
    o = gpu_utils.out_to_f32(out)
    l = None if lse is None else lse.cpu().numpy()
    q8n, sqn, skn, svn = bits8(q8), sq.cpu().numpy(), kv.scale_k.cpu().numpy(), kv.scale_v.cpu().numpy()
    k8n, v8n = rows8
    worst = worst_lse = 0.0
    for b in range(B):
        L = Skv if used is None else min(max(used[b], 0), Skv)
        dead = max(Sq - L, 0) if causal else (Sq if L == 0 else 0)     # leading rows without a key
        assert (o[b, :, :dead] == 0).all() and (l is None or (l[b, :, :dead] == -math.inf).all()), (what, b, "rows without a key")
        if dead == Sq:
            continue
        ref = oracle.attention_forward(q8n[b:b + 1, :, dead:], k8n[b:b + 1, :, :L], v8n[b:b + 1, :, :L], f, f, f, sqn[b:b + 1], skn[b:b + 1],
                                       svn[b:b + 1], causal=causal, q_offset=L - Sq + dead, sm_scale=0.0 if scale is None else scale,
                                       return_lse=True)
        worst = max(worst, gpu_utils.grade(o[b:b + 1, :, dead:], ref[0])[2])
        if l is not None:
            assert np.isfinite(l[b, :, dead:]).all(), (what, b)
            worst_lse = max(worst_lse, float(np.abs(l[b:b + 1, :, dead:] - ref[1]).max()))
    print(f"{what}: worst |err| / bound {worst:.3f}, worst LSE error {worst_lse:.2e}")
    assert worst < 1.0, (what, worst)
    assert worst_lse < LSE_TOL, (what, worst_lse)
    return worst


CASES = [   # D, dtype, fp8, B, Hq, Hkv, Sq, Skv, used, causal, splits, scale
    (128, torch.bfloat16, "e4m3", 2, 8, 2, 1, 1100, None, False, (1, 2, 3, 9, 64), None),        # decode: G Sq = 4 rows, less than a wave
    (128, torch.bfloat16, "e4m3", 1, 8, 1, 5, 2304, None, True, (1, 2, 3, 18), None),            # 40 rows; 1152-key (one-term) and 768-key splits
    (64, torch.float16, "e4m3", 2, 4, 4, 130, 1100, [1100, 65], True, (1, 3, 8), None),          # G = 1, two tiles, a short batch element
    (64, torch.bfloat16, "e5m2", 1, 8, 2, 128, 2304, None, False, (2, 3), 0.1),                  # G Sq = 512: four whole tiles
    (256, torch.bfloat16, "e4m3", 2, 8, 1, 130, 2304, [0, 2304], True, (1, 2, 9), None),         # G Sq = 1040: a ragged ninth tile; an empty element
    (128, torch.bfloat16, "e4m3", 2, 4, 1, 5, 130, [3, 130], True, (1, 2, 8, 64), None),         # L < Sq: rows without a key; fewer blocks than splits
    (256, torch.float16, "e4m3", 1, 2, 2, 5, 1100, None, False, (1, 9), None),
    (64, torch.bfloat16, "e4m3", 1, 8, 1, 130, 1100, [1036], False, (1, 3, 18), None),           # the cut falls into the last block
    (128, torch.bfloat16, "e4m3", 2, 16, 2, 1, 1100, [1100, 1036], True, (1, 3, 9), None),       # G Sq = 8: eight heads' single rows in one wave
    (128, torch.float16, "e4m3", 1, 8, 2, 130, 2304, [2200], True, (1, 2, 18), None),            # G Sq = 520: four tiles and 8 rows of a fifth
]


@pytest.mark.parametrize("D,dtype,fp8,B,Hq,Hkv,Sq,Skv,used,causal,splits,scale", CASES)
def test_every_case_is_within_the_fp8_v_bound_of_the_oracle(D, dtype, fp8, B, Hq, Hkv, Sq, Skv, used, causal, splits, scale):
    g = torch.Generator(device=DEV).manual_seed(D + Sq + Skv + Hq)
    q, k, v = _rand((B, Hq, Sq, D), dtype, g), _rand((B, Hkv, Skv, D), dtype, g), _rand((B, Hkv, Skv, D), dtype, g)
    kv = qa.prepare_kv_fp8(k, v, fp8_format=fp8)
    rows8 = _prepared_rows(kv)
    lens = [Skv] * B if used is None else [min(max(u, 0), Skv) for u in used]
    checked = False
    for ns in splits:
        for precision in ("accurate", "fast"):
            what = f"D{D} Sq{Sq} G{Hq // Hkv} keys {lens} causal {causal} ns {ns} {fp8} {precision}"
            res = _call(q, kv, causal=causal, ns=ns, precision=precision, used=used, scale=scale)
            if not checked:
                _check_quantisers(res, q, k, v, kv)
                checked = True
            assert np.array_equal(res[7].cpu().numpy(), S.expected_row_path(lens, Hq, Hkv, Sq, ns, causal, precision)), what
            _grade(res, kv, rows8, used, causal, scale, what)
            if ns > 1:   # (a): the merge of the partials, bit for bit -- and the partials' path bytes are the literal table
                mo, ml = qa.merge_attn_states(list(res[2]), list(res[3]), out_dtype=dtype)
                assert _same_bits(mo, res[0]) and _same_bits(ml, res[1]), what
                assert np.array_equal(res[4].cpu().numpy(), S.partial_paths(lens, Hq, Hkv, Sq, ns, causal, precision)), what
            else:
                assert res[2].numel() == 0 and res[3].numel() == 0
            # the public function: the same bits
            po, pl = qa.fp8_attn_splitkv_func(q, kv, causal=causal, scale=scale, seqused_k=_su(used), num_splits=ns, precision=precision, return_lse=True)
            assert _same_bits(po, res[0]) and _same_bits(pl, res[1]), what
            # without the LSE: ns > 1 and ACCURATE keep every bit; FAST with one split runs byte exponentials on its one-term workgroups
            out_n = qa.fp8_attn_splitkv_func(q, kv, causal=causal, scale=scale, seqused_k=_su(used), num_splits=ns, precision=precision)
            if ns > 1 or precision == "accurate":
                assert _same_bits(out_n, res[0]), what
            else:
                res_b = _call(q, kv, causal=causal, ns=1, precision="fast", used=used, scale=scale, lse=False)
                assert _same_bits(res_b[0], out_n) and np.array_equal(res_b[7].cpu().numpy(), res[7].cpu().numpy())
                _grade(res_b, kv, rows8, used, causal, scale, what + " (byte)")
                two = torch.from_numpy(res[7].cpu().numpy() == TWO).to(DEV)
                assert torch.equal(res_b[0][two], res[0][two])


# ---- (b) a partial is the block-sparse FP8-PV entry under the mask of the split's key blocks ---------------------------------------------------
@pytest.mark.parametrize("D,dtype,Skv,splits", [(128, torch.bfloat16, 1100, (1, 2, 3, 9, 64)), (64, torch.float16, 2304, (1, 2, 3, 18)),
                                               (256, torch.bfloat16, 1100, (1, 3, 8)), (128, torch.bfloat16, 130, (1, 2, 8))])
def test_a_partial_equals_the_block_sparse_entry_under_the_mask_of_its_key_blocks(D, dtype, Skv, splits):
    B, H, Sq = 2, 2, 130
    q, k, v = _qkv(31, dtype, B=B, Hq=H, Hkv=H, Sq=Sq, Skv=Skv, D=D)
    kv = qa.prepare_kv_fp8(k, v)
    nqb, nkb = -(-Sq // NB), -(-Skv // NB)
    for precision in ("accurate", "fast"):
        full = _native.fp8_block_sparse_attention_fp8pv(q, k, v, torch.ones(B, H, nqb, nkb, dtype=torch.bool, device=DEV), precision=precision,
                                                        return_lse=True, return_path=True)
        for ns in splits:
            res = _call(q, kv, ns=ns, precision=precision)
            what = f"D{D} Skv{Skv} ns{ns} {precision}"
            if ns == 1:
                assert _same_bits(res[0], full[0]) and _same_bits(res[1], full[1]) and torch.equal(res[7], full[2]), what
                # ... and without the LSE (FAST: the byte-exponential sweep)
                full_n = _native.fp8_block_sparse_attention_fp8pv(q, k, v, torch.ones(B, H, nqb, nkb, dtype=torch.bool, device=DEV), precision=precision)
                assert _same_bits(qa.fp8_attn_splitkv_func(q, kv, num_splits=1, precision=precision), full_n), what
                continue
            for s in range(ns):
                lo, hi = S.split_keys(Skv, ns, s)
                mask = torch.zeros(B, H, nqb, nkb, dtype=torch.bool, device=DEV)
                mask[..., lo // NB:-(-hi // NB)] = True
                bs = _native.fp8_block_sparse_attention_fp8pv(q, k, v, mask, precision=precision, return_lse=True, return_path=True)
                assert _same_bits(res[2][s].to(dtype), bs[0]), (what, s)
                assert _same_bits(res[3][s], bs[1]) and torch.equal(res[4][s], bs[2]), (what, s)


# ---- (c) causal, one split: the sliding-window FP8-PV entry at (-1, 0) ---------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype,Sq,Skv", [(128, torch.bfloat16, 130, 1100), (64, torch.float16, 300, 1300), (256, torch.bfloat16, 130, 1100),
                                            (128, torch.bfloat16, 300, 130), (64, torch.bfloat16, 5, 2304)])
def test_causal_with_one_split_equals_the_window_entry(D, dtype, Sq, Skv):
    H = 2
    q, k, v = _qkv(32, dtype, B=1, Hq=H, Hkv=H, Sq=Sq, Skv=Skv, D=D)
    kv = qa.prepare_kv_fp8(k, v)
    cu_q = torch.tensor([0, Sq], dtype=torch.int32, device=DEV)
    cu_k = torch.tensor([0, Skv], dtype=torch.int32, device=DEV)
    pk = lambda t: t[0].transpose(0, 1).contiguous()
    for precision in ("accurate", "fast"):
        for lse in (True, False):
            w = _native.fp8_quant_attention_varlen_window_fp8pv(pk(q), pk(k), pk(v), cu_q, cu_k, window_left=-1, window_right=0, precision=precision,
                                                                return_lse=lse, return_path=True)
            res = _call(q, kv, causal=True, ns=1, precision=precision, lse=lse)
            what = f"D{D} ({Sq}, {Skv}) {precision} lse {lse}"
            assert _same_bits(res[0][0], w[0].transpose(0, 1).contiguous()), what
            assert torch.equal(res[7][0], w[-1]), what
            if lse:
                assert _same_bits(res[1][0], w[1]), what
    # the public dense call shape, two batch elements
    q, k, v = _qkv(33, dtype, B=2, Hq=H, Hkv=H, Sq=Sq, Skv=Skv, D=D)
    wo, wl = qa.fp8_window_attn_pv_func(q, k, v, (-1, 0), pv_precision="fp8", precision="accurate", return_lse=True)
    so, sl = qa.fp8_attn_splitkv_func(q, (k, v), causal=True, num_splits=1, return_lse=True)
    assert _same_bits(so, wo.contiguous()) and _same_bits(sl, wl.contiguous())


# ---- (d), (e): a pair is prepared inside; a batched call is its per-element calls -----------------------------------------------------------------
def test_a_kv_pair_gives_the_prepared_bits_and_keys_beyond_seqused_k_influence_nothing():
    q, k, v = _qkv(34, torch.float16, B=2, Hq=8, Hkv=2, Sq=5, Skv=1100, D=128)
    used = [1100, 700]
    with qa.config.patch({"attention.fp8_format": "e5m2"}):
        kv = qa.prepare_kv_fp8(k, v)
        assert kv.fp8_format == "e5m2" and kv.layout == "frag" and kv.k.dtype == torch.uint8
        for ns in (1, 3, 0):
            for causal in (False, True):
                for precision in ("accurate", "fast"):
                    a = qa.fp8_attn_splitkv_func(q, kv, causal=causal, seqused_k=_su(used), num_splits=ns, precision=precision, return_lse=True)
                    b = qa.fp8_attn_splitkv_func(q, (k, v), causal=causal, seqused_k=_su(used), num_splits=ns, precision=precision, return_lse=True)
                    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]), (ns, causal, precision)
                    assert _same_bits(qa.fp8_attn_splitkv_func(q, kv, causal=causal, seqused_k=_su(used), num_splits=ns, precision=precision),
                                      qa.fp8_attn_splitkv_func(q, (k, v), causal=causal, seqused_k=_su(used), num_splits=ns, precision=precision))
    # the prepared format travels with the object, not with the config at call time
    assert _same_bits(qa.fp8_attn_splitkv_func(q, kv, num_splits=3), qa.fp8_attn_splitkv_func(q, qa.prepare_kv_fp8(k, v, fp8_format="e5m2"), num_splits=3))
    # keys beyond seqused_k: other finite values below the head's abs-max (pinned inside the used keys, so the scales stay) change no bit
    k1, v1 = k.clone(), v.clone()
    k1[:, :, 0, 0], v1[:, :, 0, 0] = 8.0, 8.0
    k2, v2 = k1.clone(), v1.clone()
    k2[1, :, 700:] *= -0.5
    v2[1, :, 700:] *= -0.5
    kva, kvb = qa.prepare_kv_fp8(k1, v1), qa.prepare_kv_fp8(k2, v2)
    assert torch.equal(kva.scale_k, kvb.scale_k) and torch.equal(kva.scale_v, kvb.scale_v) and not torch.equal(kva.k, kvb.k)
    for ns in (1, 3, 9):
        for precision in ("accurate", "fast"):
            a = qa.fp8_attn_splitkv_func(q, kva, causal=True, seqused_k=_su(used), num_splits=ns, precision=precision, return_lse=True)
            b = qa.fp8_attn_splitkv_func(q, kvb, causal=True, seqused_k=_su(used), num_splits=ns, precision=precision, return_lse=True)
            assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]), (ns, precision)


@pytest.mark.parametrize("G", [1, 4])
def test_batched_call_equals_per_batch_element_calls(G):
    B, Hkv, Sq, Skv, D = 2, 2, 5, 1100, 128
    q, k, v = _qkv(35, B=B, Hq=Hkv * G, Hkv=Hkv, Sq=Sq, Skv=Skv, D=D)
    used = [1100, 333]
    kv = qa.prepare_kv_fp8(k, v)
    for ns in (1, 3, 9):
        for precision in ("accurate", "fast"):
            for causal in (False, True):
                out, lse = qa.fp8_attn_splitkv_func(q, kv, causal=causal, seqused_k=_su(used), num_splits=ns, precision=precision, return_lse=True)
                for b in range(B):
                    o1, l1 = qa.fp8_attn_splitkv_func(q[b:b + 1], (k[b:b + 1], v[b:b + 1]), causal=causal, seqused_k=_su(used[b:b + 1]), num_splits=ns,
                                                      precision=precision, return_lse=True)
                    assert _same_bits(o1[0], out[b]) and _same_bits(l1[0], lse[b]), (ns, precision, causal, b)


# ---- (f) graph replay ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 3, 9])
def test_graph_replay_equals_eager_and_follows_a_rewritten_seqused_k(ns):
    q, k, v = _qkv(36, B=2, Hq=8, Hkv=2, Sq=5, Skv=2304, D=128)
    kv = qa.prepare_kv_fp8(k, v)
    su = _su([2304, 1100])
    for precision in ("accurate", "fast"):
        call = lambda: qa.fp8_attn_splitkv_func(q, kv, causal=True, seqused_k=su, num_splits=ns, precision=precision, return_lse=True)
        su.copy_(_su([2304, 1100]))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            call()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out, lse = call()
        graph.replay()
        torch.cuda.synchronize()
        want = call()
        assert _same_bits(out, want[0]) and _same_bits(lse, want[1])
        old = out.clone()
        su.copy_(_su([130, 0]))
        graph.replay()
        torch.cuda.synchronize()
        want = call()
        assert _same_bits(out, want[0]) and _same_bits(lse, want[1])
        assert not _same_bits(out, old) and (out[1] == 0).all() and (lse[1] == -math.inf).all()


def test_torch_compile_fullgraph_gives_the_eager_bits():
    q, k, v = _qkv(37, torch.float16, B=2, Hq=8, Hkv=2, Sq=5, Skv=1100, D=64)
    kv = qa.prepare_kv_fp8(k, v)
    su = _su([1100, 65])

    def f(q, su):   # (the PreparedKV is an object of the caller's: a decode loop holds it across steps)
        return qa.fp8_attn_splitkv_func(q * 2, kv, causal=True, scale=0.1, seqused_k=su, num_splits=3, return_lse=True, return_partials=True)

    torch._dynamo.reset()
    got = torch.compile(f, fullgraph=True)(q, su)
    want = f(q, su)
    assert len(got) == 5 and all(_same_bits(a, b) for a, b in zip(got, want))

    # num_splits = 0: the rule is resolved at trace time (a function of the shape and the CU count) and the partials get its shape
    q2, k2, v2 = _qkv(38, B=1, Hq=8, Hkv=2, Sq=1, Skv=4096, D=128)
    kv2 = qa.prepare_kv_fp8(k2, v2)
    ns = _native.splitkv_auto_splits(1, 8, 2, 1, 4096, 128, torch.cuda.get_device_properties(0).multi_processor_count)
    assert ns > 1

    def f0(q):
        return qa.fp8_attn_splitkv_func(q + 0, kv2, return_lse=True, return_partials=True)

    torch._dynamo.reset()
    got = torch.compile(f0, fullgraph=True)(q2)
    want = f0(q2)
    assert got[2].shape[0] == ns and all(_same_bits(a, b) for a, b in zip(got, want))
    assert all(_same_bits(a, b) for a, b in zip(want, qa.fp8_attn_splitkv_func(q2, kv2, num_splits=ns, return_lse=True, return_partials=True)))


# ---- membership probes (tests/probes.py; teeth: tests/test_cpu_splitkv.py) -----------------------------------------------------------------------
def _T(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _probe(probe, D, Sq, alloc, used, ns, causal):
    """(q, k, v float64 dense, ref [1, Hq, Sq, D], ref_lse [1, Hq, Sq], tot) -- computed once, shared.  tot (count probe; else None): the
    keys every row attends, int [Hq, Sq] -- its expected LSE is s_r + ln tot on the q the quantiser leaves (_count_lse)"""
    if probe == "pointer":
        seq, _ = S.boundary_pointer_seq(D, Sq, alloc, used, ns, causal)
        base = S.make_probe("pointer", D, Sq, alloc, used, causal)
        _, k, v = S.dense_tensors(base, Sq, alloc)
        o, l = seq.softmax()
        return seq.q[None], k, v, o[None], l[None], None
    case = S.make_probe(probe, D, Sq, alloc, used, causal)
    tot = None
    if probe == "count":
        seq = case.seqs[0]
        tot = np.broadcast_to(P.count_expected(seq.mask, D)[1], seq.q.shape[:2])
    return S.dense_tensors(case, Sq, alloc) + S.dense_reference(case, Sq) + (tot,)


def _count_lse(q, k, tot, dtype):
    """the count probe's expected LSE [1, Hq, Sq]: one score per row, on q and k as the head-wise quantiser leaves them (the g = 1.5 rows
    move: tests/probes.py), plus ln of the row's key count; -inf where the row has no key"""
    def deq(x):
        x8, s = oracle.quantize_fp8(bits16(_T(x, dtype).cpu()), fmt16(dtype), "head", FMT["e4m3"])
        return oracle.fp8_to_f32(x8, FMT["e4m3"]).astype(np.float64) * s.astype(np.float64)[..., None, None]
    return P.count_lse(deq(q)[0], deq(k)[0][:, 0], tot)[None]


@pytest.mark.parametrize("D", [64, 128, 256])
def test_count_decoy_and_pointer_probes_at_the_split_boundaries_the_causal_edge_and_seqused_k(D):
    """exact-answer inputs on which one misplaced key moves the output -- or, count probe at D = 64, where a 64-key chunk takes one key of
    every channel and n_c / n barely moves, the row's LSE -- by >= 4 bounds (tests/test_cpu_splitkv.py).  The count probe's rows are flat:
    both precisions, |got - ref| <= REL ref and the LSE s_r + ln n(r) within LSE_TOL; the decoy and pointer probes' rows are peaked:
    ACCURATE (FAST has no rescue), the project's fp8-V bound and LSE_TOL."""
    res = {}
    for Sq, alloc, used, ns, causal in S.PROBE_SHAPES:
        for probe in ("count", "decoy", "pointer"):
            q, k, v, ref, ref_lse, tot = _probe(probe, D, Sq, alloc, used, ns, causal)
            dead = np.isneginf(ref_lse)
            for dtype in (torch.float16, torch.bfloat16) if probe == "count" else (torch.bfloat16,):
                kv = qa.prepare_kv_fp8(_T(k, dtype), _T(v, dtype))
                for precision in ("accurate", "fast") if probe == "count" else ("accurate",):
                    for n in sorted({ns, 1}):
                        got, lse = qa.fp8_attn_splitkv_func(_T(q, dtype), kv, causal=causal, seqused_k=_su([used]), num_splits=n, precision=precision,
                                                            return_lse=True)
                        out = gpu_utils.out_to_f32(got)
                        name = f"{probe} Sq{Sq} {used}/{alloc} ns{n} causal {causal} {precision} {str(dtype)[6:]}"
                        assert (out[dead] == 0).all() and np.array_equal(np.isneginf(lse.cpu().numpy()), dead), name
                        if probe == "count":
                            assert (out[ref == 0] == 0).all(), (name, "an element no allowed key feeds must be exactly 0")
                            nz = ref > 0
                            res[name] = float((np.abs(out - ref)[nz] / P.count_bound(ref, dtype)[nz]).max())
                            want = _count_lse(q, k, tot, dtype)
                            assert np.array_equal(np.isneginf(want), dead), name
                            res[name + " lse"] = float(np.abs(lse.cpu().numpy()[~dead] - want[~dead]).max() / LSE_TOL) if (~dead).any() else 0.0
                        else:
                            res[name] = float((np.abs(out - ref) / P.project_bound(ref, False)).max())
                            live = ~dead
                            res[name + " lse"] = float(np.abs(lse.cpu().numpy()[live] - ref_lse[live]).max() / LSE_TOL)
    print(f"probes D {D}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert all(v <= 1.0 for v in res.values()), {k: v for k, v in res.items() if v > 1.0}

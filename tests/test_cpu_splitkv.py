"""Split-KV attention over prepared K / V (quantumattention_amd/splitkv.py, include/qattn_splitkv.h) without a GPU: argument validation,
the eager definition against an fp64 reference, the split plan and the FAST rule written out literally and held against the partials the
eager definition returns, the host-only auto rule, and the teeth of the membership probes tests/test_gpu_splitkv.py runs."""
import math

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, nn, splitkv
from tests import gpu_utils
from tests import probes as P
from tests import splitkv_cases as S

EAGER = {"attention.force_eager_fallback": True}


def _rand(shape, dtype, g):
    return torch.randn(*shape, generator=g, dtype=torch.float32).to(dtype)


def _qkv(seed, B=2, Hq=4, Hkv=2, Sq=5, Skv=300, D=64, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return _rand((B, Hq, Sq, D), dtype, g), _rand((B, Hkv, Skv, D), dtype, g), _rand((B, Hkv, Skv, D), dtype, g)


# ---- validation ----------------------------------------------------------------------------------------------------------------------------
def test_exports():
    assert qa.fp8_attn_splitkv_func is splitkv.fp8_attn_splitkv_func and qa.prepare_kv_fp8 is splitkv.prepare_kv_fp8
    assert qa.PreparedKV is splitkv.PreparedKV
    assert "fp8_attn_splitkv_func" not in qa.__all__ and "prepare_kv_fp8" not in qa.__all__
    assert hasattr(qa.ops, "fp8_splitkv_attention_forward")


def test_prepare_kv_on_cpu_keeps_the_eager_quantisers_row_major_bytes():
    q, k, v = _qkv(0)
    for fmt, dt in (("e4m3", torch.float8_e4m3fn), ("e5m2", torch.float8_e5m2)):
        kv = qa.prepare_kv_fp8(k, v, fp8_format=fmt)
        assert kv.shape == (2, 2, 300, 64) and kv.fp8_format == fmt and kv.dtype == torch.bfloat16 and kv.layout == "rowmajor"
        k8, sk = nn._dynamically_quantize_fp8(k, reduction_dim=[2, 3], fp8_dtype=dt)
        v8, sv = nn._dynamically_quantize_fp8(v, reduction_dim=[2, 3], fp8_dtype=dt)
        assert kv.k.dtype == dt and torch.equal(kv.k.view(torch.uint8), k8.view(torch.uint8)) and torch.equal(kv.v.view(torch.uint8), v8.view(torch.uint8))
        assert torch.equal(kv.scale_k, sk) and torch.equal(kv.scale_v, sv) and kv.scale_k.shape == (2, 2)
        assert kv.nbytes() == 2 * 2 * 2 * 300 * 64
    with qa.config.patch({"attention.fp8_format": "e5m2"}):
        assert qa.prepare_kv_fp8(k, v).fp8_format == "e5m2"
    with qa.config.patch({"attention.smooth_k": True}):   # not followed
        kv2 = qa.prepare_kv_fp8(k, v)
    assert torch.equal(kv2.k.view(torch.uint8), qa.prepare_kv_fp8(k, v).k.view(torch.uint8))


@pytest.mark.parametrize("bad", ["k3d", "kv_shape", "kv_dtype", "f32", "D", "fmt", "numerics"])
def test_prepare_kv_refuses(bad):
    q, k, v = _qkv(1)
    kw = {}
    if bad == "k3d":
        k = k[0]
    elif bad == "kv_shape":
        v = v[:, :, :-1]
    elif bad == "kv_dtype":
        v = v.to(torch.float16)
    elif bad == "f32":
        k, v = k.float(), v.float()
    elif bad == "D":
        k, v = k[..., :48], v[..., :48]
    elif bad == "fmt":
        kw["fp8_format"] = "e3m4"
    else:
        kw["numerics"] = "exact"
    with pytest.raises(ValueError):
        qa.prepare_kv_fp8(k, v, **kw)


@pytest.mark.parametrize("bad", ["auto", "precision", "ns_hi", "ns_neg", "ns_bool", "ns_float", "q3d", "q_f32", "q_dtype", "q_D", "q_B", "heads",
                                 "used_dtype", "used_shape", "used_2d", "scale", "kv_type", "kv_triple", "kv_format"])
def test_splitkv_func_refuses(bad):
    q, k, v = _qkv(2)
    kv = qa.prepare_kv_fp8(k, v)
    kw = {}
    if bad == "auto":
        kw["precision"] = "auto"
    elif bad == "precision":
        kw["precision"] = "exact"
    elif bad == "ns_hi":
        kw["num_splits"] = 65
    elif bad == "ns_neg":
        kw["num_splits"] = -1
    elif bad == "ns_bool":
        kw["num_splits"] = True
    elif bad == "ns_float":
        kw["num_splits"] = 2.0
    elif bad == "q3d":
        q = q[0]
    elif bad == "q_f32":
        q = q.float()
    elif bad == "q_dtype":
        q = q.to(torch.float16)        # the keys were prepared from bf16
    elif bad == "q_D":
        q = torch.cat([q, q], -1)
    elif bad == "q_B":
        q = q[:1]
    elif bad == "heads":
        q = q[:, :3]
    elif bad == "used_dtype":
        kw["seqused_k"] = torch.tensor([3, 4])
    elif bad == "used_shape":
        kw["seqused_k"] = torch.tensor([3, 4, 5], dtype=torch.int32)
    elif bad == "used_2d":
        kw["seqused_k"] = torch.tensor([[3, 4]], dtype=torch.int32)
    elif bad == "scale":
        kw["scale"] = -1.0
    elif bad == "kv_type":
        kv = k
    elif bad == "kv_triple":
        kv = (k, v, v)
    elif bad == "kv_format":            # bytes of one fp8 format under the other's name
        kv = splitkv.PreparedKV(kv.k, kv.v, kv.scale_k, kv.scale_v, kv.shape, "e5m2", kv.dtype, kv.numerics, kv.layout)
    with pytest.raises(ValueError):
        qa.fp8_attn_splitkv_func(q, kv, **kw)


def test_a_device_image_is_refused_by_the_eager_definition_and_a_row_major_one_is_named():
    q, k, v = _qkv(3)
    kv = qa.prepare_kv_fp8(k, v)
    frag = splitkv.PreparedKV(kv.k.view(torch.uint8).flatten(), kv.v.view(torch.uint8).flatten(), kv.scale_k, kv.scale_v, kv.shape, kv.fp8_format,
                              kv.dtype, kv.numerics, "frag")
    with pytest.raises(ValueError, match="eager definition"):
        qa.fp8_attn_splitkv_func(q, frag)


# ---- the eager definition against fp64 ----------------------------------------------------------------------------------------------------
def _deq(kv):
    return (kv.k.float() * kv.scale_k[..., None, None]).double().numpy(), (kv.v.float() * kv.scale_v[..., None, None]).double().numpy()


def _deq_q(q, fp8_dtype=torch.float8_e4m3fn):
    q8, sq = nn._dynamically_quantize_fp8(q, reduction_dim=[2, 3], fp8_dtype=fp8_dtype)
    return (q8.float() * sq[..., None, None]).double().numpy()


@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("used", [None, [300, 3], [0, 200]])
def test_eager_definition_is_within_the_bound_of_fp64(G, causal, used):
    torch.set_num_threads(4)
    Hkv, Sq, Skv, D = 2, 5, 300, 64
    q, k, v = _qkv(10 + G, Hq=Hkv * G, Hkv=Hkv, Sq=Sq, Skv=Skv, D=D)
    if used is not None:   # keys beyond seqused_k influence nothing -- they only counted toward the scales
        for b, L in enumerate(used):
            k[b, :, L:] = 2.5
            v[b, :, L:] = -3.0
    kv = qa.prepare_kv_fp8(k, v)
    su = None if used is None else torch.tensor(used, dtype=torch.int32)
    kd, vd = _deq(kv)
    ref, ref_lse = S.softmax64(_deq_q(q), kd, vd, used or [Skv, Skv], causal, 1.0 / math.sqrt(D))
    dead = np.isneginf(ref_lse)
    if used == [300, 3] and causal:
        assert dead[1, :, :2].all() and not dead[1, :, 2:].any() and not dead[0].any()   # L = 3 < Sq = 5: rows 0, 1 have no key
    if used == [0, 200]:
        assert dead[0].all() and not dead[1].any()
    outs = {}
    for ns in (1, 3, 9):
        out, lse, po, plse, ppath = qa.fp8_attn_splitkv_func(q, kv, causal=causal, seqused_k=su, num_splits=ns, return_lse=True, return_partials=True)
        assert out.shape == q.shape and out.dtype == q.dtype and lse.shape == q.shape[:3] and lse.dtype == torch.float32
        assert po.shape == ((ns,) + tuple(q.shape) if ns > 1 else (0,)) and plse.shape == ((ns,) + tuple(q.shape[:3]) if ns > 1 else (0,))
        assert np.array_equal(np.isneginf(lse.numpy()), dead) and not torch.isnan(lse).any()
        assert (out.float().numpy()[dead] == 0).all()
        gpu_utils.assert_within_bound(out.float().numpy(), ref, what=(G, causal, used, ns))
        assert np.abs(lse.numpy()[~dead] - ref_lse[~dead]).max() < S.LSE_TOL if (~dead).any() else True
        if ns > 1:   # the documented identity, and the partials themselves against fp64 over the split's keys
            mo, ml = qa.merge_attn_states(list(po), list(plse), out_dtype=q.dtype)
            assert torch.equal(mo, out) and torch.equal(ml, lse)
            for s in range(ns):
                pr, pl = S.softmax64(_deq_q(q), kd, vd, used or [Skv, Skv], causal, 1.0 / math.sqrt(D),
                                     key_range=lambda b: S.split_keys((used or [Skv, Skv])[b], ns, s))
                assert np.array_equal(np.isneginf(plse[s].numpy()), np.isneginf(pl))
                assert np.abs(po[s].numpy() - pr).max() < 1e-4
        outs[ns] = out
        # the public tuple shapes
        assert torch.equal(qa.fp8_attn_splitkv_func(q, kv, causal=causal, seqused_k=su, num_splits=ns), out)
    assert (outs[1].float() - outs[9].float()).abs().max() < 2.0 ** -6


def test_a_kv_pair_and_config_eager_fallback_give_the_prepared_bits():
    q, k, v = _qkv(20, dtype=torch.float16)
    kv = qa.prepare_kv_fp8(k, v)
    a = qa.fp8_attn_splitkv_func(q, kv, num_splits=3, return_lse=True)
    b = qa.fp8_attn_splitkv_func(q, (k, v), num_splits=3, return_lse=True)
    with qa.config.patch(EAGER):
        c = qa.fp8_attn_splitkv_func(q, [k, v], num_splits=3, return_lse=True)
    assert all(torch.equal(a[i], b[i]) and torch.equal(a[i], c[i]) for i in range(2))
    assert a[0].dtype == torch.float16
    # num_splits = 0 on CPU tensors: the rule at 256 CUs
    ns = _native.splitkv_auto_splits(2, 4, 2, 5, 300, 64, 256)
    d = qa.fp8_attn_splitkv_func(q, kv, return_lse=True, return_partials=True)
    assert d[2].shape[0] == (ns if ns > 1 else 0)


# ---- the split plan and the FAST rule, literally ------------------------------------------------------------------------------------------------
def test_the_written_out_split_plan():
    assert [S.split_keys(1100, 3, s) for s in range(3)] == [(0, 384), (384, 768), (768, 1100)]          # 9 blocks, 3 each
    assert [S.split_keys(1100, 9, s) for s in range(9)][-2:] == [(896, 1024), (1024, 1100)]             # one block each, the last 76 keys
    assert [S.split_keys(2304, 2, s) for s in range(2)] == [(0, 1152), (1152, 2304)]
    assert [S.split_keys(130, 8, s) for s in range(8)] == [(0, 128), (128, 130)] + [(0, 0)] * 6           # fewer blocks than splits
    assert [S.split_keys(1100, 64, s) for s in range(64)][9:] == [(0, 0)] * 55
    assert [S.split_keys(1100, 4, s) for s in range(4)] == [(0, 384), (384, 768), (768, 1100), (0, 0)]   # per = 3: the fourth split is empty
    assert S.split_keys(0, 3, 0) == (0, 0) and S.split_keys(1, 3, 0) == (0, 1)
    # the module's own helper says the same
    for L in (0, 1, 130, 1100, 2304):
        for ns in (1, 2, 3, 8, 9, 18, 64):
            mine = [S.split_keys(L, ns, s) for s in range(ns)]
            theirs = [(lo, hi) if hi > lo else (0, 0) for lo, hi in splitkv.split_plan(L, ns)]
            assert mine == theirs, (L, ns)


def test_the_written_out_fast_rule():
    # 2304 keys: ns = 2 gives 1152-key splits (one-term under FAST), ns = 3 gives 768 (two-term); ACCURATE is two-term everywhere
    assert S.workgroup_code(2304, 1, 1, 2, 0, 0, False, "fast") == S.ONE and S.workgroup_code(2304, 1, 1, 3, 0, 0, False, "fast") == S.TWO
    assert S.workgroup_code(2304, 1, 1, 2, 0, 0, False, "accurate") == S.TWO
    assert S.workgroup_code(2304, 1, 1, 1, 0, 0, False, "fast") == S.ONE
    # seqused_k cuts the count: 1100 of them in one split is one-term, 1000 is not
    assert S.keys_swept(1100, 5, 4, 1, 0, 0, False) == 1100 and S.keys_swept(1000, 5, 4, 1, 0, 0, False) == 1000
    # causal: Sq = 130, G = 1, L = 1100 -- tile 0's last row (position 127) attends keys <= 127 + 970, tile 1's (129) all 1100
    assert S.keys_swept(1100, 130, 1, 1, 0, 0, True) == 1098 and S.keys_swept(1100, 130, 1, 1, 0, 1, True) == 1100
    # ... G = 8: 1040 packed rows; tile 0 holds positions 0 .. 127 of head 0, every later tile some head's last position (rows 129, 259, ...)
    assert S.keys_swept(1100, 130, 8, 1, 0, 0, True) == 1098 and all(S.keys_swept(1100, 130, 8, 1, 0, t, True) == 1100 for t in range(1, 9))
    # causal with L < Sq: the split above every row's edge sweeps nothing and carries the one-term code
    assert S.keys_swept(3, 5, 1, 1, 0, 0, True) == 3 and S.workgroup_code(0, 5, 1, 1, 0, 0, True, "accurate") == S.ONE
    assert S.keys_swept(300, 5, 1, 3, 2, 0, True) == 300 - 256 and S.keys_swept(258, 5, 1, 3, 2, 0, False) == 2
    # merged row_path: a row takes ONE_TERM from a one-term split that gave it a key, never from an empty one
    p = S.expected_row_path([2304, 1100], 4, 1, 5, 2, False, "fast")     # b = 0: 1152 + 1152 (one-term); b = 1: 640 + 460 (two-term)
    assert (p[0] == S.ONE).all() and (p[1] == S.TWO).all()
    p = S.expected_row_path([0, 1100], 4, 1, 5, 3, False, "accurate")
    assert (p[0] == S.ONE).all() and (p[1] == S.TWO).all()


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("ns", [1, 3, 9, 64])
def test_partials_of_the_eager_definition_own_the_keys_the_written_out_plan_says(ns, causal):
    """zero keys (every score 0) and one-hot values: partial s of a row is n_c / n over exactly the keys the row attends in split s, and
    exp(lse_s) counts them.  Two value codes -- key j -> channel j mod 64 and (j div 64) mod 64 -- tell shifted ranges apart."""
    torch.set_num_threads(4)
    B, Hq, Hkv, Sq, Skv, D = 2, 4, 1, 5, 1100, 64
    used = [1100, 130]
    q = torch.ones(B, Hq, Sq, D, dtype=torch.bfloat16)
    k = torch.zeros(B, Hkv, Skv, D, dtype=torch.bfloat16)
    su = torch.tensor(used, dtype=torch.int32)
    for code in (lambda j: j % D, lambda j: (j // D) % D):
        v = torch.zeros(B, Hkv, Skv, D, dtype=torch.bfloat16)
        j = torch.arange(Skv)
        v[:, :, j, code(j)] = 1.0
        res = qa.fp8_attn_splitkv_func(q, (k, v), causal=causal, seqused_k=su, num_splits=ns, precision="fast", return_lse=True, return_partials=True)
        out, lse, po, plse, ppath = res
        if ns == 1:
            po, plse = out.float()[None], lse[None]
        else:
            assert np.array_equal(ppath.numpy(), S.partial_paths(used, Hq, Hkv, Sq, ns, causal, "fast"))
        for s in range(ns):
            for b in range(B):
                for p in range(Sq):
                    lo, hi = S.row_keys(used[b], Sq, ns, s, p, causal)
                    want = np.bincount(code(np.arange(lo, hi)), minlength=D) if hi > lo else np.zeros(D)
                    got_n = torch.exp(plse[s, b, :, p]).numpy()
                    assert np.allclose(got_n, hi - lo, rtol=1e-5, atol=0), (s, b, p, got_n, hi - lo)
                    if hi == lo:
                        assert (plse[s, b, :, p] == -math.inf).all() and (po[s, b, :, p] == 0).all()
                    else:
                        # (the eager quantiser rounds V's scale in bf16, and with ns = 1 out is bf16: within 2^-7 of the value, which
                        # still tells neighbouring integer counts <= 18 apart)
                        assert np.abs(po[s, b, :, p].numpy() * (hi - lo) - want[None]).max() <= 2.0 ** -7 * max(1.0, want.max()), (s, b, p)


# ---- the auto rule (host-only) ---------------------------------------------------------------------------------------------------------------
def test_auto_splits_is_a_pure_function_of_the_shape():
    auto = _native.splitkv_auto_splits
    cus = 256
    assert auto(4, 32, 32, 4096, 4096, 128, cus) == 1            # 4096 tiles: the grid already fills the chip
    assert auto(64, 32, 8, 1, 32768, 128, cus) == 1              # 512 tiles = 2 per CU
    assert auto(1, 32, 8, 1, 32768, 128, cus) > 1
    assert auto(1, 32, 8, 1, 130, 128, cus) == 1                 # two key blocks: nothing to split
    for shape in [(1, 32, 8, 1, 32768, 128), (4, 32, 8, 1, 8192, 128), (1, 32, 8, 8, 32768, 128), (1, 40, 40, 64, 32760, 128), (1, 8, 8, 1, 1100, 64),
                  (2, 16, 2, 16, 130, 256), (1, 1, 1, 1, 1, 64), (3, 6, 3, 130, 100000, 64)]:
        B, Hq, Hkv, Sq, Skv, D = shape
        nkb = -(-Skv // 128)
        ns = auto(*shape, cus)
        assert 1 <= ns <= min(64, nkb), (shape, ns)
        assert ns == auto(*shape, cus) == auto(*shape, cus), "stable for a fixed input"
        per = -(-nkb // ns)
        assert -(-nkb // per) == ns, "no split is empty when every key is used"
        prev = ns
        for b in range(B + 1, B + 200, 7):   # monotone non-increasing in B
            cur = auto(b, Hq, Hkv, Sq, Skv, D, cus)
            assert cur <= prev, (shape, b, cur, prev)
            prev = cur
        assert auto(B, Hq, Hkv, Sq, Skv, D, 32) <= ns            # fewer CUs never ask for more splits
    assert auto(1, 32, 8, 1, 32768, 100, cus) == 1 and auto(1, 32, 5, 1, 32768, 128, cus) == 1 and auto(1, 32, 8, 1, 32768, 128, 0) == 1   # invalid: 1
    assert _native.lib().qattn_fp8_attention_splitkv_workspace_bytes(1, 32, 8, 1, 32768, 128, 65) == 0
    ws = [_native.lib().qattn_fp8_attention_splitkv_workspace_bytes(1, 32, 8, 1, 32768, 128, n) for n in (1, 2, 8, 9, 64, 0)]
    assert 0 < ws[0] < ws[1] < ws[2] < ws[3] < ws[4] == ws[5]


# ---- teeth of the probe cases the GPU file runs ---------------------------------------------------------------------------------------------------
def _assert_teeth(res, what):
    assert res, (what, "no mutant touched a row")
    print(f"{what}: " + ", ".join(f"{k} {v:.1f}x" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not v >= P.TEETH}
    assert not bad, (what, bad)


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("Sq,alloc,used,ns,causal", S.PROBE_SHAPES)
def test_teeth_of_the_probe_cases(D, Sq, alloc, used, ns, causal):
    """a chunk dropped beside any split boundary, the causal edge moved by one, the padding admitted, seqused_k off by one: each moves an
    element (D = 64 count probe: or the row's LSE, where a 64-key chunk takes one key of every channel) by >= 4 bounds"""
    what = f"D {D} Sq {Sq} keys {used}/{alloc} ns {ns} causal {causal}"
    # count probe: against REL_COUNT of the value (fp16: one key in 1100 on a 0.5-gain row is below 4 bf16 bounds at D = 64)
    case = S.make_probe("count", D, Sq, alloc, used, causal)
    seq = case.seqs[0]
    mut = dict(case.mutants[0])
    mut.update(S.split_mutants(seq, used, ns))
    assert any(name.startswith("chunk") for name in mut) and "seqused_k - 1" in mut and (used == alloc or "seqused_k + 1" in mut)
    assert not causal or {"hi-1", "hi+1"} <= set(mut)
    _assert_teeth(P.count_teeth(seq, mut, "fp16", lse_tol=S.LSE_TOL), what + " count")
    # pointer probe: rows point at the keys beside the split boundaries; decoy probe: the forbidden key beside every edge
    seq, targets = S.boundary_pointer_seq(D, Sq, alloc, used, ns, causal)
    others = {"kv head off by one": (np.roll(seq.k, 1, 0), np.roll(seq.v, 1, 0))}
    _assert_teeth(P.pointer_teeth(seq, targets, False, others), what + " pointer")
    case = S.make_probe("decoy", D, Sq, alloc, used, causal)
    if (case.aux[0] >= 0).any():
        _assert_teeth(P.decoy_teeth(case.seqs[0], case.aux[0], False), what + " decoy")
    else:
        assert not causal and used == alloc   # (no edge, no unused key: nothing to admit)


def test_a_chunk_attended_by_two_splits_moves_the_merged_lse():
    """the count probe at 1100 keys, three splits, with the chunk below the second boundary attended by BOTH neighbours: the merged LSE
    moves by ln(1164 / 1100) = 0.057 against LSE_TOL = 2e-3 (the output's n_c / n moves as well)"""
    D, Sq, L, ns = 128, 5, 1100, 3
    case = S.make_probe("count", D, Sq, L, L, False)
    q, k, v = (torch.from_numpy(t).to(torch.bfloat16) for t in S.dense_tensors(case, Sq, L))
    kv = qa.prepare_kv_fp8(k, v)
    out, lse, po, plse, _ = qa.fp8_attn_splitkv_func(q, kv, num_splits=ns, return_lse=True, return_partials=True)
    ref, _ = S.dense_reference(case, Sq)
    assert np.abs(out.float().numpy() - ref).max() <= (P.count_bound(ref, "bf16") + 1e-12).max()
    # the faulty plan: split 1 starts one chunk early (on the operands the eager definition attends: the quantiser moves the g = 1.5 rows)
    kd, vd = _deq(kv)
    lo, hi = S.split_keys(L, ns, 1)
    bad_o, bad_l = S.softmax64(_deq_q(q), kd, vd, [L], False, 1.0 / math.sqrt(D), key_range=lambda b: (lo - 64, hi))
    outs = [po[0], torch.from_numpy(bad_o).float(), po[2]]
    lses = [plse[0], torch.from_numpy(bad_l).float(), plse[2]]
    mo, ml = qa.merge_attn_states(outs, lses, out_dtype=torch.float32)
    moved = (ml - lse).abs().min().item()
    assert abs(moved - math.log(1164 / 1100)) < 1e-3 and moved > 20 * S.LSE_TOL
    assert (np.abs(mo.numpy() - ref) / np.maximum(P.count_bound(ref, "bf16"), 1e-30)).max() > P.TEETH


# ---- the C entry's argument checks (they run before any device call: no GPU needed) ---------------------------------------------------------------
def test_the_c_entry_refuses_bad_arguments_with_the_documented_codes_before_any_device_call():
    INVALID, DIM, FMT, WORKSPACE = -1, -2, -3, -4     # include/qattn.h QATTN_ERR_* (literal: the header is the contract)
    L = _native.lib()
    P16 = 0x10000     # an aligned address nobody dereferences: every call below returns before a launch
    good = dict(q16=P16, in_fmt=_native.FMT_BF16, k8=P16, v8=P16, scale_k=P16, scale_v=P16, out=P16, lse=None, seqused_k=None, B=1, Hq=8, Hkv=2,
                Sq=5, Skv=1100, D=128, fp8_fmt=_native.FMT_E4M3, numerics=0, causal=0, sm=0.0, precision=_native.PRECISION["accurate"], ns=3, q8=None,
                scale_q=None, row_path=None, po=None, pl=None, pp=None, ws=P16, ws_bytes=0, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        if "ws_bytes" not in kw:   # one byte short of what the header asks for: the last check, reached only when every other one passed
            a["ws_bytes"] = L.qattn_fp8_attention_splitkv_workspace_bytes(a["B"], a["Hq"], a["Hkv"], a["Sq"], a["Skv"], a["D"], a["ns"]) - 1
        return L.qattn_fp8_attention_splitkv_forward(*a.values())

    assert call() == WORKSPACE                      # valid arguments, a workspace one byte short
    assert call(ws=None) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    assert call(ns=0) == WORKSPACE                  # num_splits = 0 is sized for the most splits, before the CU count is asked for
    for bad in (dict(q16=None), dict(k8=None), dict(v8=None), dict(scale_k=None), dict(scale_v=None), dict(out=None), dict(B=0), dict(Sq=0),
                dict(Skv=-1), dict(numerics=7), dict(precision=_native.PRECISION["auto"]), dict(precision=9), dict(ns=-1), dict(ns=65),
                dict(B=65536), dict(Hq=2 * 65536, Hkv=2), dict(q16=P16 + 8), dict(k8=P16 + 4), dict(out=P16 + 2), dict(q8=P16 + 1), dict(po=P16 + 4),
                dict(ws=P16 + 8), dict(ns=0, po=P16), dict(ns=0, pl=P16), dict(ns=0, pp=P16), dict(Skv=2 ** 31 - 1)):
        assert call(**bad) == INVALID, bad
    for bad in (dict(D=96), dict(D=512), dict(Hq=7), dict(Hkv=3)):
        assert call(**bad) == DIM, bad
    for bad in (dict(in_fmt=_native.FMT_E4M3), dict(in_fmt=_native.FMT_FP32), dict(fp8_fmt=_native.FMT_BF16), dict(fp8_fmt=5)):
        assert call(**bad) == FMT, bad

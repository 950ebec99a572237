"""CPU tests of multi-head latent attention (include/qattn_mla.h, quantumattention_amd/mla.py): the eager definitions -- the specification of
the kernels -- against fp64 on tests/mla_cases.py's problems, the header's byte map, the split rule and the argument rejection reasons."""
import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, mla
from tests import mla_cases as C
from tests.gpu_utils import assert_within_bound


def _cpu_cache(page, lens, dtype=torch.bfloat16, fmt="e4m3"):
    table, num_pages = C.make_table(page)
    cache = qa.alloc_paged_mla_cache_fp8(num_pages, page, batch_size=C.B, max_pages_per_seq=table.shape[1], scale=C.SCALE_KV, dtype=dtype,
                                         device="cpu", fp8_format=fmt)
    cache.block_table.copy_(table)
    lat = C.make_latent(dtype)
    qa.paged_mla_cache_append_fp8(cache, lat[..., :C.DV], lat[..., C.DV:], new_lens=torch.tensor(lens, dtype=torch.int32))
    assert cache.seqlens.tolist() == list(lens)
    return cache, lat


@pytest.mark.parametrize("Hq,Sq", C.SHAPES)
@pytest.mark.parametrize("page", C.PAGES)
@pytest.mark.parametrize("causal", [True, False])
def test_eager_definitions_against_fp64(Hq, Sq, page, causal):
    q = C.make_q(Hq, Sq, torch.bfloat16)
    q8, sq = mla.quantize_q_eager(q)
    assert torch.equal(q8.float() * sq[..., None], q.float()) and bool((sq == C.SCALE_Q).all())      # the inputs are exact: no quantiser in the oracle
    for lens in C.LENS:
        cache, lat = _cpu_cache(page, lens)
        ref_o, ref_l = C.reference(q.double(), lat.double(), lens, C.SM_SCALE, causal)
        for ns in C.SPLITS:
            out, lse = qa.fp8_mla_paged_func(q, cache, scale=C.SM_SCALE, causal=causal, num_splits=ns, max_seqlen_k=C.CAP, return_lse=True)
            assert_within_bound(out.float().numpy(), ref_o, what=(Hq, Sq, page, causal, lens, ns))
            fin = np.isfinite(ref_l)
            assert np.array_equal(np.isneginf(lse.numpy()), ~fin) and np.abs(lse.numpy()[fin] - ref_l[fin]).max() <= C.LSE_TOL
            assert bool((out.float().numpy()[~fin] == 0).all())


def test_byte_map_against_a_double_loop():
    ps, pages = 128, 2
    off = np.empty((64, C.D), np.int64)
    for k in range(64):
        for d in range(C.D):
            t, key, s, hh, half, j = k // 32, k % 32, d // 64, (d // 32) % 2, (d // 16) % 2, d % 16      # [t:2][s:9][hh:2][half:2][key:32][16 B]
            off[k, d] = ((((t * 9 + s) * 2 + hh) * 2 + half) * 32 + key) * 16 + j
            assert off[k, d] == mla.chunk_byte_offset(k, d)
    assert sorted(off.reshape(-1).tolist()) == list(range(64 * C.D))
    flat = (torch.arange(pages * ps * C.D) % 251).to(torch.uint8)
    rows = mla.pool_rowmajor(flat, pages, ps)
    for p, k, d in ((0, 0, 0), (0, 37, 515), (1, 64, 0), (1, 127, 575)):
        assert rows[p, k, d] == flat[(p * 2 + k // 64) * 64 * C.D + off[k % 64, d]]


def test_auto_splits_is_monotone_and_keeps_1024_keys_per_split():
    assert {"qattn_mla_auto_splits", "qattn_fp8_mla_paged_forward", "qattn_paged_mla_cache_append_fp8"} <= set(_native.EXPORTS)
    for B, Hq, Sq in ((1, 128, 1), (1, 16, 4), (32, 128, 1), (4, 20, 3)):
        last = 1
        for Skv in (1, 1023, 1024, 2048, 8192, 32768, 1 << 20):
            ns = _native.mla_auto_splits(B, Hq, Sq, Skv, 256)
            assert 1 <= last <= ns <= 64 and (ns == 1 or Skv // ns >= 1024) and B * -(-Hq * Sq // 64) * ns <= max(256, B * -(-Hq * Sq // 64))
            last = ns
    assert _native.mla_auto_splits(1, 128, 1, 32768, 256) == 32 and _native.mla_auto_splits(32, 128, 1, 8192, 256) == 4


def test_rejection_reasons():
    cache, _ = _cpu_cache(64, C.LENS[0])
    q = C.make_q(16, 1, torch.bfloat16)
    assert mla.mla_input_reason(q, cache, scale=C.SM_SCALE) is None
    assert "576" in mla.mla_input_reason(q[..., :512], cache, scale=C.SM_SCALE)
    assert "scale is required" in mla.mla_input_reason(q, cache)
    with pytest.raises(ValueError, match="scale is required"):
        qa.fp8_mla_paged_func(q, cache)
    assert "same device" in mla.mla_input_reason(q.to("meta"), cache, scale=C.SM_SCALE)
    with pytest.raises(ValueError, match="multiple of 64"):
        qa.alloc_paged_mla_cache_fp8(4, 96, batch_size=1, max_pages_per_seq=2, scale=1.0, dtype=torch.bfloat16, device="cpu")
    with pytest.raises(ValueError, match="scale is required"):
        qa.alloc_paged_mla_cache_fp8(4, 64, batch_size=1, max_pages_per_seq=2, scale=None, dtype=torch.bfloat16, device="cpu")
    assert "ckv_new" in mla.mla_input_reason(None, cache, ckv_new=torch.zeros(C.B, 1, 500, dtype=torch.bfloat16), kpe_new=torch.zeros(C.B, 1, 64, dtype=torch.bfloat16))

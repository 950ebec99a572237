"""CPU tests of sparse multi-head latent attention (include/qattn_mla_sparse.h, quantumattention_amd/mla.py): the eager definitions -- the
specification of the kernels -- against the fp64 oracle on tests/mla_sparse_cases.py's problems, the split rule and the rejection reasons."""
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, mla
from tests import mla_cases as C
from tests import mla_sparse_cases as S
from tests.gpu_utils import assert_within_bound


@pytest.mark.parametrize("Hq,Sq,topk,causal,fmt,dtype", S.CASES)
def test_eager_definitions_against_fp64(Hq, Sq, topk, causal, fmt, dtype):
    S.check_sweep(Hq, Sq, topk, causal, fmt, dtype, "cpu", assert_within_bound)


def test_auto_splits_is_monotone_keeps_its_floor_and_fits_the_cus():
    assert {"qattn_mla_sparse_auto_splits", "qattn_fp8_mla_paged_sparse_forward", "qattn_paged_mla_row_cache_append_fp8",
            "qattn_mla_row_pool_bytes", "qattn_fp8_mla_paged_sparse_workspace_bytes"} <= set(_native.EXPORTS)
    for B, Hq, Sq in ((1, 128, 1), (1, 16, 4), (32, 128, 1), (4, 20, 3), (300, 16, 1)):
        last, base = 1, B * Sq * -(-Hq // 64)
        for topk in (1, 511, 512, 1024, 2048, 2049, 8192, 2048 * 64):
            ns, floor = _native.mla_sparse_auto_splits(B, Hq, Sq, topk, 256), -(-topk // 2048)
            assert max(last, floor) <= ns <= 64, (B, Hq, Sq, topk, ns)                   # monotone in topk, never below ceil(topk / 2048)
            assert ns == max(1, floor) or (base * ns <= 256 and topk // ns >= 128), (B, Hq, Sq, topk, ns)   # above the floor: fits, >= 128 entries
            last = ns
    assert _native.mla_sparse_auto_splits(1, 128, 1, 2048, 256) == 16 and _native.mla_sparse_auto_splits(32, 16, 1, 2048, 256) == 8
    assert _native.mla_sparse_auto_splits(32, 128, 1, 2048, 256) == 4 and _native.mla_sparse_auto_splits(128, 128, 1, 2048, 256) == 1


def test_rejection_reasons():
    cache = S.make_cache(16, C.LENS[0])
    q, idx = C.make_q(16, 1, torch.bfloat16), S.draw_indices(1, 65, 0)
    ok = dict(scale=C.SM_SCALE)
    assert mla.mla_sparse_input_reason(q, cache, idx, **ok) is None
    assert "int32" in mla.mla_sparse_input_reason(q, cache, idx.long(), **ok)
    assert "int32" in mla.mla_sparse_input_reason(q, cache, idx[:, :, None], **ok)
    assert "dense last dimension" in mla.mla_sparse_input_reason(q, cache, idx[:, :, ::2], **ok)
    assert "scale is required" in mla.mla_sparse_input_reason(q, cache, idx)
    assert "num_splits" in mla.mla_sparse_input_reason(q, cache, idx, num_splits=65, **ok)
    big = torch.zeros((C.B, 1, 2049), dtype=torch.int32)
    assert "num_splits" in mla.mla_sparse_input_reason(q, cache, big, num_splits=1, **ok)
    assert mla.mla_sparse_input_reason(q, cache, big, num_splits=2, **ok) is None
    table, num_pages = C.make_table(64)
    chunk = qa.alloc_paged_mla_cache_fp8(num_pages, 64, batch_size=C.B, max_pages_per_seq=table.shape[1], scale=1.0, dtype=torch.bfloat16, device="cpu")
    chunk.layout = "frag"      # (what a device allocation of the chunk image says)
    with pytest.raises(ValueError, match="row-major cache"):
        qa.fp8_mla_paged_sparse_func(q, chunk, idx, **ok)
    with pytest.raises(ValueError, match="positive integer"):
        qa.alloc_paged_mla_row_cache_fp8(4, 0, batch_size=1, max_pages_per_seq=2, scale=1.0, dtype=torch.bfloat16, device="cpu")
    with pytest.raises(ValueError, match="below 2\\^31"):
        qa.alloc_paged_mla_row_cache_fp8(2 ** 20, 2 ** 11, batch_size=1, max_pages_per_seq=2, scale=1.0, dtype=torch.bfloat16, device="meta")
    assert "ckv_new" in mla.mla_sparse_input_reason(None, cache, ckv_new=torch.zeros(C.B, 1, 500, dtype=torch.bfloat16),
                                                    kpe_new=torch.zeros(C.B, 1, 64, dtype=torch.bfloat16))

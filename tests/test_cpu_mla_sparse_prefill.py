"""CPU tests of sparse MLA on packed variable-length queries (include/qattn_mla_sparse_prefill.h): the names, the argument rules, and the eager
packed definition against the per-slot eager `fp8_mla_paged_sparse_func(num_splits=1)`."""
import os

import numpy as np
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from quantumattention_amd.mla import PagedMLACacheFP8
from tests import mla_cases as C
from tests import mla_sparse_cases as S

COUNTS, PAD, LENS, HQ, TOPK = (0, 1, 5, 3), 4, (64, 1, 3, 200), 5, 70
TOTAL = sum(COUNTS) + PAD


def make():
    q = C.make_q(HQ, 4, torch.bfloat16).permute(0, 2, 1, 3).reshape(16, HQ, C.D)[:TOTAL].contiguous()
    idx = S.draw_indices(4, TOPK, seed=3).reshape(16, TOPK)[:TOTAL].contiguous()
    cu = torch.tensor(np.concatenate([[0], np.cumsum(COUNTS)]), dtype=torch.int32)
    return q, S.make_cache(16, LENS), idx, cu


def test_names_and_symbol():
    assert callable(qa.fp8_mla_paged_sparse_varlen_func) and callable(qa.mla_sparse_varlen_input_reason)
    assert not {"fp8_mla_paged_sparse_varlen_func", "mla_sparse_varlen_input_reason"} & set(qa.__all__)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qattn_mla_sparse_prefill.h")).read()
    assert "int qattn_fp8_mla_paged_sparse_varlen_forward(" in header and "qattn_fp8_mla_paged_sparse_varlen_forward" in _native.EXPORTS


def test_input_reasons():
    q, cache, idx, cu = make()
    reason = lambda q=q, idx=idx, cu=cu, scale=C.SM_SCALE: qa.mla_sparse_varlen_input_reason(q, cache, idx, cu, scale=scale)
    assert reason() is None
    assert "3-D" in reason(q=q[None])
    assert "int32" in reason(idx=idx.long())
    assert "cu_seqlens_q" in reason(cu=cu[:-1])
    assert "scale is required" in reason(scale=None)
    with pytest.raises(ValueError, match="scale is required"):
        qa.fp8_mla_paged_sparse_varlen_func(q, cache, idx, cu)


@pytest.mark.parametrize("causal", [True, False])
def test_eager_packed_equals_the_per_slot_eager_call(causal):
    q, cache, idx, cu = make()
    out, lse, q8, sq = qa.fp8_mla_paged_sparse_varlen_func(q, cache, idx, cu, scale=C.SM_SCALE, causal=causal, return_lse=True, return_q8=True)
    assert tuple(out.shape) == (TOTAL, HQ, C.DV) and tuple(lse.shape) == (HQ, TOTAL)
    lo = 0
    for b, n in enumerate(COUNTS):
        rows = slice(lo, lo + n)
        lo += n
        if n == 0:
            continue
        one = PagedMLACacheFP8(cache.pool, cache.scale[b:b + 1], cache.block_table[b:b + 1], cache.seqlens[b:b + 1], cache.num_pages,
                               cache.page_size, cache.fp8_format, cache.dtype, cache.layout)
        w_o, w_l, w_q8, w_sq = qa.fp8_mla_paged_sparse_func(q[rows].transpose(0, 1)[None], one, idx[rows][None], scale=C.SM_SCALE, causal=causal,
                                                            num_splits=1, return_lse=True, return_q8=True)
        assert torch.equal(out[rows], w_o[0].transpose(0, 1)) and torch.equal(lse[:, rows], w_l[0])
        assert torch.equal(q8[rows].view(torch.uint8), w_q8[0].transpose(0, 1).view(torch.uint8)) and torch.equal(sq[rows], w_sq[0].transpose(0, 1))
    assert (out[lo:].float() == 0).all() and torch.isneginf(lse[:, lo:]).all() and (sq[lo:] == 0).all()   # the padded bucket
    assert not causal or torch.isneginf(lse[:, 1:3]).all()                                                # slot 2, causal: L_b < n_b, kend <= 0

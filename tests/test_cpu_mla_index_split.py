"""CPU tests of the multi-workgroup selection of the lightning indexer (include/qattn_mla_index_split.h): the rules of num_splits /
select_splits, the eager path under any valid value, the new names and fake shapes, and the invariants of the auto rule."""
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, mla_index, ops
from tests import mla_index_cases as X

MAX = mla_index.MAX_SELECT_SPLITS


@pytest.mark.parametrize("bad", [-1, MAX + 1, 2.0])
def test_split_counts_out_of_range_or_not_integers_raise(bad):
    rows, used = X.make_rows("distinct", 63), torch.tensor([63], dtype=torch.int32)
    with pytest.raises(ValueError, match="num_splits"):
        qa.mla_index_select(rows, 8, seqused_k=used, num_splits=bad)
    icache = X.make_icache(16, (1, 2, 3, 4), cap=64)
    with pytest.raises(ValueError, match="select_splits"):
        qa.fp8_mla_index_topk_func(X.make_q(4, 2, torch.bfloat16), torch.ones((X.B, 2, 4)), icache, 8, select_splits=bad)


@pytest.mark.parametrize("s", [0, 1, 3, MAX])
def test_eager_path_accepts_any_valid_value(s):
    rows, used = X.make_rows("dup16", 2049), torch.tensor([2049], dtype=torch.int32)
    assert torch.equal(qa.mla_index_select(rows, 64, seqused_k=used, num_splits=s), X.ref_select(rows, [2049], 64, True))
    icache = X.make_icache(16, (1, 20, 33, 64), cap=64)
    q, w = X.make_q(4, 2, torch.bfloat16), torch.ones((X.B, 2, 4))
    idx, logits = qa.fp8_mla_index_topk_func(q, w, icache, 8, return_logits=True, select_splits=s)
    assert torch.equal(idx, X.ref_select(logits, (1, 20, 33, 64), 8, True))


def test_names_exports_and_fake_shapes():
    assert hasattr(qa, "select_splits_reason") and "select_splits_reason" not in qa.__all__
    assert {"qattn_mla_index_select_split_workspace_bytes", "qattn_mla_index_select_auto_splits", "qattn_mla_index_select_split",
            "qattn_fp8_mla_index_topk_split_workspace_bytes", "qattn_fp8_mla_index_topk_split"} <= set(_native.EXPORTS)
    assert callable(ops.mla_index_select_split_forward) and callable(ops.fp8_mla_index_topk_split_forward)
    with torch.device("meta"):
        logits, used = torch.empty((2, 3, 100)), torch.empty((2,), dtype=torch.int32)
        q, w, pool = torch.empty((2, 4, 3, 128), dtype=torch.bfloat16), torch.empty((2, 3, 4)), torch.empty((5, 16, 128), dtype=torch.uint8)
        table, scale = torch.empty((2, 7), dtype=torch.int32), torch.empty((2,))
        got = torch.ops.quantumattention_amd.mla_index_select_split_forward(logits, used, 9, 4)
        assert tuple(got.shape) == (2, 3, 9) and got.dtype == torch.int32
        res = torch.ops.quantumattention_amd.fp8_mla_index_topk_split_forward(q, w, pool, scale, table, used, 100, 9, 5, 16, 4, "e4m3", True, True, True)
        assert [tuple(t.shape) for t in res] == [(2, 3, 9), (2, 3, 100), (2, 4, 3, 128), (2, 4, 3)] and res[0].dtype == torch.int32


def test_auto_rule_invariants():
    rule, seg, keys = _native.mla_index_select_auto_splits, _native.MLA_INDEX_AUTO_MIN_SEG, _native.MLA_INDEX_AUTO_MIN_KEYS
    least = _native.MLA_INDEX_AUTO_MIN_SPLITS
    for cus in (64, 256, 304):
        for rows in (1, 3, 4, 8, 9, 32, 33, 64, 128, cus // least, cus // least + 1, cus - 1, cus, cus + 1, 4096):
            for N in (1, 2048, keys - 1, keys, 32768, 131072, 2 ** 30):
                for topk in (1, 2048, 131072):
                    s = rule(rows, N, topk, cus)
                    assert 1 <= s <= MAX and (s == 1 or (rows * s <= cus and -(-N // s) >= seg and N >= keys and N > topk)), (cus, rows, N, topk, s)
                    assert s == rule(rows, N, topk, cus) and (rows < cus or s == 1)
                    # the measured table: under 8 splits a row was slower than on one workgroup, or no faster
                    assert s == 1 or s >= least, (cus, rows, N, topk, s)
                    assert rows * least <= cus or s == 1, (cus, rows, N, topk, s)
    assert rule(1, 131072, 2048, 256) == min(MAX, 256, 131072 // seg) and rule(0, 8192, 1, 256) == 1
    # the table's rows at 256 CUs, topk 2048: (B, N) -> the count measured faster than one workgroup beyond its spread, 1 where none was
    table = {(1, 8192): 1, (4, 8192): 1, (32, 8192): 1, (1, 16384): 8, (4, 16384): 8, (32, 16384): 8, (1, 32768): 16, (4, 32768): 16,
             (32, 32768): 8, (1, 131072): 64, (4, 131072): 64, (32, 131072): 8}
    assert {k: rule(k[0], k[1], 2048, 256) for k in table} == table
    assert [rule(rows, 16384, 2048, 256) for rows in (33, 64, 85, 128)] == [1, 1, 1, 1] and rule(32, 16384, 2048, 64) == 1

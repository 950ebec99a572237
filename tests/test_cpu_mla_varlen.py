"""CPU tests of dense MLA on packed variable-length queries (include/qattn_mla_varlen.h): the names, the argument rules, the split rule, the
fake op, and the eager packed definition against the fp64 oracle (bounds: tests/test_gpu_mla.py's)."""
import os

import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import mla_cases as C
from tests import mla_varlen_cases as V


def test_names_and_symbols():
    assert callable(qa.fp8_mla_paged_varlen_func) and callable(qa.mla_varlen_input_reason)
    assert not {"fp8_mla_paged_varlen_func", "mla_varlen_input_reason"} & set(qa.__all__)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qattn_mla_varlen.h")).read()
    for name in ("qattn_mla_varlen_auto_splits", "qattn_fp8_mla_paged_varlen_workspace_bytes", "qattn_fp8_mla_paged_varlen_forward"):
        assert name + "(" in header and name in _native.EXPORTS


def test_input_reasons():
    Hq, counts, lens = V.CASES[0]
    q, cu, total = V.make_q(Hq, counts), V.cu_of(counts), sum(counts) + V.PAD
    cache, _ = V.make_cache("cpu", len(counts), 64, lens)
    reason = lambda q=q, cache=cache, cu=cu, mq=9, scale=C.SM_SCALE: qa.mla_varlen_input_reason(q, cache, cu, mq, scale=scale)
    assert reason() is None
    assert "3-D" in reason(q=q[None])
    assert "cu_seqlens_q" in reason(cu=cu[:-1]) and "int32" in reason(cu=cu.long())
    assert "max_seqlen_q" in reason(mq=total + 1)
    row = qa.alloc_paged_mla_row_cache_fp8(8, 48, batch_size=len(counts), max_pages_per_seq=2, scale=1.0, dtype=torch.bfloat16, device="cpu")
    assert "multiple of 64" in reason(cache=row)      # a row-major cache: its pages need not hold whole chunks
    assert "scale is required" in reason(scale=None)
    with pytest.raises(ValueError, match="scale is required"):
        qa.fp8_mla_paged_varlen_func(q, cache, cu, 9)


@pytest.mark.parametrize("slots,Skv,cus,want", [(1, 32768, 256, 32), (36, 8192, 256, 7), (4, 8192, 256, 8), (300, 8192, 256, 1), (1, 1023, 256, 1),
                                                (2, 1 << 20, 256, 64), (0, 8192, 256, 1)])
def test_auto_splits(slots, Skv, cus, want):
    assert _native.mla_varlen_auto_splits(slots, Skv, cus) == want
    assert _native.mla_varlen_tile_slots(32, 543, 128) == 543 + 32 and _native.mla_varlen_tile_slots(4, 15, 16) == 2 + 4


def test_fake_op_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from quantumattention_amd import ops  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        e = lambda *s, dtype=torch.int32: torch.empty(*s, dtype=dtype, device="cuda")
        q = e(18, 16, 576, dtype=torch.bfloat16)
        out, lse, po, pl, q8, sq = torch.ops.quantumattention_amd.fp8_mla_paged_varlen_attention_forward(
            q, e(4 * 36864, dtype=torch.uint8), e(4, dtype=torch.float32), e(4, 1), e(4), e(5), 9, 64, 4, 64, 3, 0.07, "e4m3", True, True, True)
        assert out.shape == (18, 16, 512) and out.dtype == torch.bfloat16 and lse.shape == (16, 18) and lse.dtype == torch.float32
        assert po.shape == (3, 18, 16, 512) and pl.shape == (3, 18, 16) and q8.shape == (18, 16, 576) and q8.dtype == torch.float8_e4m3fn
        assert sq.shape == (18, 16)


@pytest.mark.parametrize("case", [V.CASES[0], V.CASES[3]])
@pytest.mark.parametrize("causal", [True, False])
def test_eager_definition_against_fp64(case, causal):
    Hq, counts, lens = case
    q, cu, total = V.make_q(Hq, counts), V.cu_of(counts), sum(counts)
    cache, _ = V.make_cache("cpu", len(counts), 64, lens)
    for ns in (1, 3):
        out, lse, po, pl, q8, sq = qa.fp8_mla_paged_varlen_func(q, cache, cu, max(counts), scale=C.SM_SCALE, causal=causal, num_splits=ns,
                                                                max_seqlen_k=C.CAP, return_lse=True, return_partials=True, return_q8=True)
        assert tuple(po.shape) == ((ns, total + V.PAD, Hq, C.DV) if ns > 1 else (0,)) and torch.equal((q8.float() * sq[..., None])[:total], q.float()[:total])
        ref = V.reference(q8.double() * sq.double()[..., None], V.dequant(cache), counts, lens, causal)
        V.check_against_reference(out, lse, ref, (case, causal, ns))

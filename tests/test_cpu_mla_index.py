"""CPU tests of the lightning indexer (include/qattn_mla_index.h): the input rules, the eager definitions against the fp64 logits and the
selection's reference (tests/mla_index_cases.py), the public names, and the eager append's bytes against the CPU quantiser."""
import pytest
import torch

import quantumattention_amd as qa
from tests import mla_index_cases as X

NAMES = ("PagedMLAIndexCacheFP8", "alloc_paged_mla_index_cache_fp8", "paged_mla_index_cache_append_fp8", "fp8_mla_index_topk_func",
         "mla_index_select", "mla_index_input_reason")


def test_the_names_are_package_attributes_outside_all():
    assert all(hasattr(qa, n) and n not in qa.__all__ for n in NAMES)


def _args():
    icache = X.make_icache(16, (1, 2, 3, 4), cap=64)
    return dict(q=X.make_q(4, 2, torch.bfloat16), weights=torch.ones((X.B, 2, 4)), icache=icache, topk=8)


RULES = [
    (lambda a: a.update(topk=0), "topk"),
    (lambda a: a.update(topk=2 ** 17 + 1), "topk"),
    (lambda a: a.update(q=a["q"].half()), "dtype"),
    (lambda a: a.update(q=a["q"][..., :64]), "head dimension"),
    (lambda a: a.update(q=torch.zeros((X.B, 65, 2, 128), dtype=torch.bfloat16), weights=torch.ones((X.B, 2, 65))), "Hi <= 64"),
    (lambda a: a.update(weights=a["weights"].double()), "weights"),
    (lambda a: a.update(weights=torch.ones((X.B, 4, 2))), "weights"),
    (lambda a: a.update(weights=torch.ones((X.B, 2, 8))[..., ::2]), "dense heads"),
    (lambda a: a.update(max_seqlen_k=65), "max_seqlen_k"),
    (lambda a: a.update(seqused_k=torch.zeros(X.B, dtype=torch.int64)), "seqused_k"),
    (lambda a: a.update(icache=object()), "PagedMLAIndexCacheFP8"),
]


@pytest.mark.parametrize("i", range(len(RULES)))
def test_input_rules(i):
    a = _args()
    assert qa.mla_index_input_reason(**a) is None
    RULES[i][0](a)
    assert RULES[i][1] in qa.mla_index_input_reason(**a)
    with pytest.raises(ValueError):
        qa.fp8_mla_index_topk_func(a.pop("q"), a.pop("weights"), a.pop("icache"), a.pop("topk"), **a)


def test_append_rules_and_aliasing():
    row = qa.alloc_paged_mla_row_cache_fp8(5, 16, batch_size=2, max_pages_per_seq=2, scale=0.5, dtype=torch.bfloat16, device="cpu")
    icache = qa.alloc_paged_mla_index_cache_fp8(5, 16, batch_size=2, max_pages_per_seq=2, scale=0.5, dtype=torch.bfloat16, device="cpu",
                                                block_table=row.block_table, seqlens=row.seqlens)
    assert icache.block_table is row.block_table and icache.seqlens is row.seqlens and tuple(icache.pool.shape) == (5, 16, 128)
    k = torch.zeros((2, 3, 128), dtype=torch.bfloat16)
    qa.paged_mla_index_cache_append_fp8(icache, k, advance=False)
    assert row.seqlens.tolist() == [0, 0]
    qa.paged_mla_index_cache_append_fp8(icache, k)
    assert row.seqlens.tolist() == [3, 3]
    for bad in (k.half(), k[..., :64], k[:1], torch.zeros((2, 3, 256), dtype=torch.bfloat16)[..., ::2]):
        with pytest.raises(ValueError):
            qa.paged_mla_index_cache_append_fp8(icache, bad)


@pytest.mark.parametrize("Hi,Sq,causal,page,fmt,dtype", [(20, 3, True, 16, "e4m3", torch.bfloat16), (64, 1, False, 1, "e5m2", torch.float16)])
def test_eager_scores_and_entry_are_exact(Hi, Sq, causal, page, fmt, dtype):
    X.check_scores(Hi, Sq, causal, page, fmt, dtype, "cpu")


@pytest.mark.parametrize("kind,N", X.SELECT_CASES)
def test_eager_selection_against_a_stable_sort(kind, N):
    X.check_select(kind, N, "cpu")


@pytest.mark.parametrize("page", [1, 64])
@pytest.mark.parametrize("T,start", [(1, 0), (5, 60), (70, 64)])
def test_eager_append_bytes_against_the_cpu_quantiser(T, start, page):
    X.check_append(T, start, page, "cpu")

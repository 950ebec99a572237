"""GPU tests of the multi-workgroup selection of the lightning indexer (include/qattn_mla_index_split.h): a row cut across workgroups against
the stable sort on crafted rows, several slots behind strides, independence of the workspace's contents, the whole entry against the
one-workgroup selection, and a replayed graph.  Every comparison is exact."""
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import mla_index_cases as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(kind, N, s) for kind in X.ROW_KINDS for N in (1, 63, 2049, X.CAND + 1) for s in (2, 3, 64)]
CASES += [("zeros", 4 * X.CAND, 7), ("two", 4 * X.CAND, 256), ("one_bin", 4 * X.CAND, 256)]   # 128-key segments; the threshold bin holds the row in every pass


@pytest.mark.parametrize("kind,N,s", CASES)
def test_split_selection_against_a_stable_sort(kind, N, s):
    rows = X.make_rows(kind, N).to(DEV)
    used = torch.tensor([N], dtype=torch.int32, device=DEV)
    for topk in X.TOPKS:                                # Sq 3, causal: kend = N - 2, N - 1, N
        got = qa.mla_index_select(rows, topk, seqused_k=used, causal=True, num_splits=s)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), X.ref_select(rows, [N], topk, True)), (kind, N, s, topk)


def test_several_slots_padded_rows_and_per_slot_lengths():
    N, lens = 2049, (0, 70, 2049)
    base = torch.randn((3, 3, N + 37), generator=torch.Generator().manual_seed(5)).to(DEV)
    got = qa.mla_index_select(base[:, :, :N], 64, seqused_k=torch.tensor(lens, dtype=torch.int32, device=DEV), causal=True, num_splits=5)
    assert torch.equal(got.cpu(), X.ref_select(base[:, :, :N], lens, 64, True))


def test_result_does_not_depend_on_the_workspace_contents():
    N, s, topk = 2049, 5, 64
    used = torch.tensor([N], dtype=torch.int32, device=DEV)
    ws = torch.empty((_native.lib().qattn_mla_index_select_split_workspace_bytes(1, 3, N, s),), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0
    for fill, kind in ((0xFF, "special"), (0x00, "special"), (None, "dup16")):   # None: what the call before left behind
        if fill is not None:
            ws.fill_(fill)
        rows = X.make_rows(kind, N).to(DEV)
        got = _native.mla_index_select_split(rows, used, topk, is_causal=True, num_splits=s, workspace=ws)
        assert torch.equal(got.cpu(), X.ref_select(rows, [N], topk, True)), (fill, kind)


@pytest.mark.parametrize("s", [2, 9])
@pytest.mark.parametrize("lens", X.LENS)
def test_whole_entry_equals_the_one_workgroup_selection(lens, s):
    q = X.make_q(20, 3, torch.bfloat16, exact=False).to(DEV)
    w = torch.randn((X.B, 3, 20), generator=torch.Generator().manual_seed(3)).to(DEV)
    icache = X.make_icache(16, lens, device=DEV, exact=False)
    want = qa.fp8_mla_index_topk_func(q, w, icache, 65, max_seqlen_k=X.CAP, return_logits=True, select_splits=1)
    got = qa.fp8_mla_index_topk_func(q, w, icache, 65, max_seqlen_k=X.CAP, return_logits=True, select_splits=s)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(got[0].cpu(), X.ref_select(got[1], lens, 65, True))


def test_replayed_graph_follows_the_logits_and_the_lengths():
    N, topk = 2049, 64
    rows = X.make_rows("dup16", N).to(DEV)
    used = torch.tensor([N], dtype=torch.int32, device=DEV)
    qa.mla_index_select(rows, topk, seqused_k=used, num_splits=4)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = qa.mla_index_select(rows, topk, seqused_k=used, num_splits=4)
    for kind, L in (("special", 1500), ("two", N)):
        rows.copy_(X.make_rows(kind, N))
        used.fill_(L)
        graph.replay()
        assert torch.equal(out, qa.mla_index_select(rows, topk, seqused_k=used, num_splits=4))
        assert torch.equal(out.cpu(), X.ref_select(rows, [L], topk, True))

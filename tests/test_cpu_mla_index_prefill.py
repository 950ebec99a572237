"""CPU tests of the packed (prefill) lightning indexer (include/qattn_mla_index_prefill.h): the eager packed definition against the eager
dense entry per sequence and fp64, the input rules, the C entries' argument codes before any device call, the op's fake shapes."""
import pytest
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native
from tests import mla_index_cases as X
from tests import mla_index_prefill_cases as P


@pytest.mark.parametrize("shape,Hi,page,causal,fmt,dtype", P.CASES[:3])
def test_eager_packed_call_equals_the_dense_entry_per_sequence(shape, Hi, page, causal, fmt, dtype):
    assert P.check(shape, Hi, page, causal, fmt, dtype, "cpu") == 0.0


def _args():
    q, w, cu = P.make_packed("a", 4, torch.bfloat16, "cpu")
    return dict(q=q, weights=w, icache=X.make_icache(16, (1, 2, 3, 4), cap=64), cu_seqlens_q=cu, topk=8)


RULES = [
    (lambda a: a.update(topk=0), "topk"),
    (lambda a: a.update(q=a["q"].half()), "dtype"),
    (lambda a: a.update(q=a["q"][None]), "3-D"),
    (lambda a: a.update(q=a["q"][..., :64]), "head dimension"),
    (lambda a: a.update(q=torch.zeros((9, 65, 128), dtype=torch.bfloat16), weights=torch.ones((9, 65))), "Hi <= 64"),
    (lambda a: a.update(weights=a["weights"][:-1]), "weights"),
    (lambda a: a.update(weights=torch.ones((a["q"].shape[0], 8))[:, ::2]), "dense heads"),
    (lambda a: a.update(cu_seqlens_q=a["cu_seqlens_q"][:-1]), "cu_seqlens_q"),
    (lambda a: a.update(cu_seqlens_q=a["cu_seqlens_q"].long()), "cu_seqlens_q"),
    (lambda a: a.update(max_seqlen_k=65), "max_seqlen_k"),
    (lambda a: a.update(seqused_k=torch.zeros(X.B, dtype=torch.int64)), "seqused_k"),
    (lambda a: a.update(icache=object()), "PagedMLAIndexCacheFP8"),
]


@pytest.mark.parametrize("i", range(len(RULES)))
def test_input_rules(i):
    a = _args()
    assert qa.mla_index_varlen_input_reason(**a) is None
    RULES[i][0](a)
    assert RULES[i][1] in qa.mla_index_varlen_input_reason(**a)
    with pytest.raises(ValueError):
        qa.fp8_mla_index_topk_varlen_func(a.pop("q"), a.pop("weights"), a.pop("icache"), a.pop("cu_seqlens_q"), a.pop("topk"), **a)


def test_exports_and_argument_codes():
    names = {"qattn_fp8_mla_index_varlen_workspace_bytes", "qattn_fp8_mla_index_scores_varlen", "qattn_fp8_mla_index_topk_varlen"}
    assert names <= set(_native.EXPORTS)
    assert all(hasattr(qa, n) and n not in qa.__all__ for n in ("fp8_mla_index_topk_varlen_func", "mla_index_varlen_input_reason"))
    L = _native.lib()
    wsb = L.qattn_fp8_mla_index_varlen_workspace_bytes
    assert wsb(0, 10) == 0 and wsb(10, 0) == 0 and wsb(9, 100) == 256 + 3840 and wsb(1 << 20, 1 << 20) == (1 << 22) + (1 << 42)
    # the argument checks come before any device call (include/qattn.h: QATTN_ERR_INVALID_ARG -1, _UNSUPPORTED_FMT -3)
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = buf.data_ptr() + (-buf.data_ptr()) % 16
    names = ("q", "in_fmt", "qs", "w", "ws", "pool", "table", "tstride", "num_pages", "page", "max_pages", "scale", "cu", "used", "B", "Hi", "tq",
             "N", "topk", "fmt", "causal", "idx", "logits", "q8", "sq", "wsp", "wsb", "stream")
    good = dict.fromkeys(names) | dict(q=p, in_fmt=_native.FMT_BF16, w=p, ws=0, pool=p, table=p, tstride=4, num_pages=8, page=16, max_pages=4, scale=p,
                                       cu=p, used=p, B=1, Hi=4, tq=9, N=64, topk=8, fmt=_native.FMT_E4M3, causal=1, idx=p, wsp=p, wsb=0)
    call = lambda **kw: L.qattn_fp8_mla_index_topk_varlen(*(good | kw).values())
    assert call() == -1 and call(wsb=255) == -1 and call(logits=p, wsb=255) == -1        # the workspace: kend, and the rows without the caller's
    ok = dict(wsb=wsb(9, 64))
    for bad in (dict(q=None), dict(cu=None), dict(q=p + 2), dict(cu=p + 2), dict(Hi=65), dict(tq=0), dict(B=0), dict(B=65536), dict(topk=0),
                dict(topk=2 ** 17 + 1), dict(N=65), dict(tstride=3), dict(ws=-1), dict(idx=None), dict(wsp=p + 4)):
        assert call(**ok, **bad) == -1, bad
    assert call(**ok, in_fmt=_native.FMT_E4M3) == -3 and call(**ok, fmt=_native.FMT_BF16) == -3
    scores = dict(good, logits=p, ls=0, fill=1, kend=p)
    order = names[:18] + ("fmt", "causal", "logits", "ls", "fill", "kend", "q8", "sq", "stream")
    call = lambda **kw: L.qattn_fp8_mla_index_scores_varlen(*[(scores | kw)[n] for n in order])
    assert call(kend=None) == -1 and call(logits=None) == -1 and call(ls=-1) == -1 and call(Hi=0) == -1 and call(fmt=7) == -3


def test_the_op_has_fake_shapes():
    import quantumattention_amd.ops  # noqa: F401  (registers the ops)
    q, w = torch.empty((19, 20, 128), dtype=torch.bfloat16, device="meta"), torch.empty((19, 20), device="meta")
    pool = torch.empty((8, 16, 128), dtype=torch.float8_e4m3fn, device="meta")
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="meta")
    out = torch.ops.quantumattention_amd.fp8_mla_index_topk_varlen_forward(q, w, pool, torch.empty(2, device="meta"), i32(2, 4), i32(3), i32(2),
                                                                            60, 8, 8, 16, "e4m3", True, True, True)
    assert [tuple(t.shape) for t in out] == [(19, 8), (19, 60), (19, 20, 128), (19, 20)]
    assert [t.dtype for t in out] == [torch.int32, torch.float32, torch.float8_e4m3fn, torch.float32]

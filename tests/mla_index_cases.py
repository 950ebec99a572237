"""What tests/test_cpu_mla_index.py and tests/test_gpu_mla_index.py share (include/qattn_mla_index.h), on top of tests/mla_cases.py's grid values:
an index-key cache filled through the append behind a shuffled table, the fp64 logits on the q8 the call returns and the cache's bytes, the
selection's reference (a stable descending sort), crafted logit rows, and the checks both devices run.

EXACT inputs: q, keys and weights from mla_cases.GRID, q's channel 0 +-3.5 (scale_q = 2^-7, q8 = q 2^7), scale_k = 2^-2.  Every product
q8 k8 is a multiple of 8 and at most 1344, every weighted term a multiple of 2^-6, every partial sum below 2^24 of its units: fp32 arithmetic
is exact in ANY order, so the logits must equal the fp64 formula bit for bit."""
import numpy as np
import torch

import quantumattention_amd as qa
from quantumattention_amd import _native, mla_index
from tests import mla_cases as C

WG, CAND = mla_index.WG_KEYS, mla_index.LDS_CANDIDATES
B, D = 4, 128
CAP = 2 * WG + 70                                 # two range seams of the score sweep are crossed
LENS = ((0, 1, 31, CAP), (32, 33, WG - 1, WG), (WG + 1, CAP, 0, 1))
SCALE_K = 2.0 ** -2
SCORE_CASES = [(Hi, Sq, causal, page, "e4m3", torch.bfloat16) for Hi in (64, 20) for Sq in (1, 3) for causal in (True, False) for page in (1, 16, 64)]
SCORE_CASES.append((20, 3, True, 16, "e5m2", torch.float16))
ROW_KINDS = ("zeros", "two", "dup16", "distinct", "special", "one_bin")
SELECT_CASES = [(kind, N) for kind in ROW_KINDS for N in (1, 63, 2049, CAND + 1)] + [("zeros", 4 * CAND), ("two", 4 * CAND)]
TOPKS = (1, 64, 65, 2048)


def make_q(Hi, Sq, dtype, seed=0, exact=True):
    if not exact:
        return torch.randn((B, Hi, Sq, D), generator=torch.Generator().manual_seed(seed)).to(dtype)
    q = C.draw((B, Hi, Sq, D), seed)
    q[..., 0] = 3.5 * torch.where(C.draw((B, Hi, Sq), seed + 1) < 0, -1.0, 1.0)
    return q.to(dtype)


def make_icache(page, lens, dtype=torch.bfloat16, fmt="e4m3", device="cpu", seed=7, exact=True, cap=CAP):
    """an index-key cache whose slot b holds lens[b] keys behind a shuffled table; never-written bytes are 0x7f (NaN)"""
    M = -(-cap // page)
    num_pages = B * M + 3
    g = torch.Generator().manual_seed(seed)
    icache = qa.alloc_paged_mla_index_cache_fp8(num_pages, page, batch_size=B, max_pages_per_seq=M, scale=SCALE_K, dtype=dtype, device=device, fp8_format=fmt)
    icache.pool.view(torch.uint8).fill_(0x7f)
    icache.block_table.copy_(torch.randperm(num_pages, generator=g)[: B * M].reshape(B, M).to(torch.int32))
    keys = (C.draw((B, cap, D), seed + 100) * SCALE_K if exact else torch.randn((B, cap, D), generator=g) * 0.5).to(dtype).to(device)
    qa.paged_mla_index_cache_append_fp8(icache, keys, new_lens=torch.tensor(lens, dtype=torch.int32, device=device))
    assert icache.seqlens.tolist() == list(lens)
    return icache


def kends(lens, N, Sq, causal):
    return [[max(min(L, N) - Sq + i + 1, 0) if causal else min(L, N) for i in range(Sq)] for L in lens]


def ref_logits(q8, scale_q, weights, icache, lens, causal, N):
    """fp64 (logits [B, Sq, N] with -inf at j >= kend, bound [B, Sq, N] = scale_k sum_h |w| scale_q sum_c |q8 k8|) on the cache's bytes"""
    k = icache.pool.view(_native.fp8_dtype_of(icache.fp8_format))[icache.block_table.long()].reshape(B, -1, D)[:, :N].double().cpu().numpy()
    q8, wq = q8.double().cpu().numpy(), (weights.double() * scale_q.double().transpose(1, 2)).cpu().numpy()          # wq [B, Sq, Hi]
    live = np.arange(N)[None, None, :] < np.array(kends(lens, N, q8.shape[2], causal))[..., None]
    k = np.where(np.isnan(k), 0.0, k)                                                                                # (only never-written rows: masked below)
    q8, kt = q8.transpose(0, 2, 1, 3), k[:, None].transpose(0, 1, 3, 2)                                               # [B, Sq, Hi, 128], [B, 1, 128, N]
    s, mag = q8 @ kt, np.abs(q8) @ np.abs(kt)                                                                       # [B, Sq, Hi, N]
    sk = icache.scale.double().cpu().numpy()[:, None, None]
    logits = (np.maximum(s, 0.0) * wq[..., None]).sum(axis=2) * sk
    return np.where(live, logits, -np.inf), (mag * np.abs(wq)[..., None]).sum(axis=2) * sk


def ref_select(logits, lens, topk, causal):
    """the rule: a stable descending sort of the canonical row below kend, its first topk positions ascending, -1 behind them"""
    logits = torch.as_tensor(logits).double().cpu()
    Bn, Sq, N = logits.shape
    out = torch.full((Bn, Sq, topk), -1, dtype=torch.int32)
    for b, ends in enumerate(kends(lens, N, Sq, causal)):
        for i, kend in enumerate(ends):
            row = logits[b, i, :kend].clone()
            row[row.isnan()] = -torch.inf
            row[row == 0] = 0.0
            pick = torch.sort(row, descending=True, stable=True).indices[:topk].sort().values
            out[b, i, : pick.numel()] = pick.to(torch.int32)
    return out


def make_rows(kind, N, seed=0):
    """logits fp32 [1, 3, N]: three different rows of one kind"""
    g = torch.Generator().manual_seed(seed + N)
    if kind == "zeros":
        return torch.zeros((1, 3, N))
    if kind == "two":                                   # 30 % ones: every topk boundary falls inside one of the two ties
        return (torch.rand((1, 3, N), generator=g) < 0.3).float()
    if kind == "dup16":
        return torch.randn(16, generator=g)[torch.randint(0, 16, (1, 3, N), generator=g)]
    if kind == "distinct":
        return torch.stack([torch.randperm(N, generator=g).float() - N // 2 for _ in range(3)])[None]
    if kind == "one_bin":                               # distinct values of ONE exponent: the threshold bin of pass 0 holds the whole row
        return 1.0 + torch.stack([torch.randperm(N, generator=g).float() for _ in range(3)])[None] / (2.0 * N)
    x = torch.randn((1, 3, N), generator=g)             # "special"
    special = torch.tensor([float("inf"), float("-inf"), float("nan"), 0.0, -0.0, 0.0, -0.0, float("nan")])
    pick = torch.randint(0, 16, (1, 3, N), generator=g)
    return torch.where(pick < 8, special[pick.clamp(max=7)], x)


def check_select(kind, N, device):
    rows = make_rows(kind, N).to(device)
    used = torch.tensor([N], dtype=torch.int32, device=device)
    for topk in TOPKS:                                  # Sq 3, causal: kend = N - 2, N - 1, N -- below, equal to and above topk at N = 2049
        got = qa.mla_index_select(rows, topk, seqused_k=used, causal=True)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), ref_select(rows, [N], topk, True)), (kind, N, topk)


def check_scores(Hi, Sq, causal, page, fmt, dtype, device, exact=True, topk=64):
    """the logits against fp64 on the returned q8 and the pool bytes (exact inputs: bit for bit), -inf exactly at j >= kend, and the whole
    entry's indices against the rule applied to its own logits (exact inputs: and to the fp64 logits).  Returns the worst error / bound."""
    q = make_q(Hi, Sq, dtype, exact=exact).to(device)
    g = torch.Generator().manual_seed(Hi + Sq)
    w = (C.draw((B, Sq, Hi), 50) if exact else torch.randn((B, Sq, Hi), generator=g)).to(device)
    worst = 0.0
    for lens in LENS:
        icache = make_icache(page, lens, dtype, fmt, device, exact=exact)
        idx, logits, q8, sq = qa.fp8_mla_index_topk_func(q, w, icache, topk, causal=causal, max_seqlen_k=CAP, return_logits=True, return_q8=True)
        if exact:
            assert torch.equal(q8.float() * sq[..., None], q.float())
        ref, bound = ref_logits(q8, sq, w, icache, lens, causal, CAP)
        got, what = logits.double().cpu().numpy(), (Hi, Sq, causal, page, fmt, lens)
        live = np.isfinite(ref)
        assert np.array_equal(np.isneginf(got), ~live), what
        if exact:
            assert np.array_equal(got[live], ref[live]), what
            assert torch.equal(idx.cpu(), ref_select(ref, lens, topk, causal)), what
        elif live.any():
            assert (bound[live] > 0).all()
            worst = max(worst, float((np.abs(got[live] - ref[live]) / (256 * 2.0 ** -24 * bound[live])).max()))
        assert torch.equal(idx.cpu(), ref_select(logits, lens, topk, causal)), what
    return worst


def check_append(T, start, page, device):
    """the appended bytes against the CPU quantiser: marker-filled pool, saturation, dropped tokens (capacity 128: start 64 + T 70 drops 6)"""
    M, Bn, marker = 128 // page, 2, 0xA5
    num_pages = Bn * M + 3
    for fmt, dtype in (("e4m3", torch.bfloat16), ("e5m2", torch.float16)):
        fp8, qmax = _native.fp8_dtype_of(fmt), torch.finfo(_native.fp8_dtype_of(fmt)).max
        icache = qa.alloc_paged_mla_index_cache_fp8(num_pages, page, batch_size=Bn, max_pages_per_seq=M, scale=torch.tensor([0.5, 0.03125]),
                                                    dtype=dtype, device=device, fp8_format=fmt)
        icache.pool.view(torch.uint8).fill_(marker)
        table = torch.randperm(num_pages, generator=torch.Generator().manual_seed(page))[: Bn * M].reshape(Bn, M).to(torch.int32)
        icache.block_table.copy_(table)
        icache.seqlens.fill_(start)
        proj = (torch.randn((Bn, T, 160), generator=torch.Generator().manual_seed(T * 100 + start)) * 8.0).to(dtype)   # |x| / 0.03125 passes qmax
        proj[0, 0, 3], proj[1, T - 1, 100] = float("inf"), float("-inf")
        n = (T, max(T - 3, 0))
        qa.paged_mla_index_cache_append_fp8(icache, proj.to(device)[..., 16:144], new_lens=torch.tensor(n, dtype=torch.int32, device=device))   # a strided view
        want = torch.full((num_pages, page, D), marker, dtype=torch.uint8)
        for b in range(Bn):
            kept = min(n[b], M * page - start)
            x8 = (proj[b, :kept, 16:144].float() / icache.scale[b].cpu()).to(dtype).clamp(-qmax, qmax).to(fp8).view(torch.uint8)
            for t in range(kept):
                want[table[b, (start + t) // page], (start + t) % page] = x8[t]
            assert int(icache.seqlens[b]) == start + kept
        assert torch.equal(icache.pool.view(torch.uint8).cpu(), want), (T, start, page, fmt)

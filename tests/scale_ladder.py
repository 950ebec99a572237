"""The scale ladder: inputs on which a MIS-INDEXED quantisation scale shows ("Scale ladder").  Plain numpy / torch-CPU helpers
shared by tests/test_cpu_scale_ladder.py (exactness, flatness, teeth, the hole) and tests/test_gpu_scale_ladder.py (the kernels).

On N(0,1) data all scales of one tensor agree to a few percent, so a kernel that reads the neighbour's scale errs by ~5 % in a score and
nothing notices.  Here neighbouring scale groups carry gains of 2^e: the fp8 BYTES do not depend on the gains (powers of two are exact in
every format and in the quantiser's arithmetic), the scales differ by x4 .. x64, and a scale read at the wrong index makes some group's
scores several times too large -- its flat rows collapse onto their top keys.

head ladder   K, Q dense random +-1 codes, V over {-1, 0, 1}.  kv group (b, h_kv): k 2^e; every query head of the group: q 2^(-e + f),
              e = E_HEAD[b, h_kv] (distinct, >= 2 apart), f = F_HEAD[h] (0 / -2 alternating inside a GQA group): scores keep a standard
              deviation of 1 or 0.25 whatever e.  For the packed entries a batch entry is a sequence.
token ladder  token j of K (or row i of Q) is 2^(e_j) c_j, e_j seeded from {0, 1, 2, 3}, c_j a +-1 code on max(1, D / 4^(e_j)) seeded
              channels: q.k_j / sqrt(D) keeps standard deviation 1 whatever e_j, and every non-zero element of a token has the token's
              abs-max, so token-wise quantisation is exact (bytes 0 or +- the largest code).
V chunk ladder (fused head-wise entry, Skv <= 16384: block-scaled V)  chunk c of V is 2^(g_c) v, g_c seeded from G_CHUNK, |V| <= 2.
V head ladder  v[b, h_kv] 2^e, e = E_VHEAD[b, h_kv]: wherever an entry keeps ONE fp8 V scale per head -- the separate calls and the row-major
              entry, every token-wise path, the fused entry beyond 16384 keys.

The reference is the fp64 masked softmax on the CPU quantiser's output (oracle.quantize_fp8 / oracle.quantize_v_block; never a scale a GPU
call returned): `softmax64` here for the teeth and for the masks oracle.attention_forward does not have (window, tiles), asserted equal
to oracle.attention_forward where both exist.  A MUTANT is that reference with one scale table re-indexed."""
import functools
import math

import numpy as np
import torch

import oracle
from tests import probes as P
from tests.vwitness import bits16, fmt16, to16

FMT = {"e4m3": oracle.FMT_E4M3, "e5m2": oracle.FMT_E5M2}
TOP_CODE = {"e4m3": 0x7E, "e5m2": 0x7B}          # the byte of the format's largest finite number (448, 57344)
TOL, TOL_V16, TEETH = P.TOL, P.TOL_V16, P.TEETH
B, HQ, HKV = 2, 4, 2
E_HEAD = np.array([[4, 0], [-2, 2]])              # e of kv group (b, h_kv): distinct, >= 2 apart
F_HEAD = np.array([0, -2, 0, -2])                 # f of query head h: heads that share a kv head still differ in scale_q
# the V head ladder: gains {1, 1/8, 1/2, 1/4}.  Every non-zero element of a ladder V sits AT its group's abs-max, so a head's rms is 0.71 x
# its gain: with the largest gain 1 no head's V has a larger rms than the N(0,1) V for which the project's absolute bound 2^-6 is stated
# (the kernels' own error is proportional to |v|; the chunk ladder's {2, 1, 1/2, 1/4} has rms 0.81 over a head).  Measured with a largest
# gain of 2 (rms 1.41), D 128 token-wise: the one-term sweep's |err| / bound per head was 0.05 / 0.25 / 0.49 / 1.00 for gains 1/8, 1/2, 1, 2
# -- proportional to the gain, i.e. every head read its own scale -- and the gain-2 head touched the bound (0.999;
# profiles/scale_ladder/v_head_gain2_diag.log, docs/ISSUE_one_term_sweep_on_lattice_scores.md).
E_VHEAD = np.array([[0, -3], [-1, -2]])
G_CHUNK = (1, 0, -1, -2)                          # the V chunk ladder: gains {2, 1, 1/2, 1/4}
E_TOKEN = (0, 1, 2, 3)
LARGE = 4.0                                       # a mutant must show on the rows where it makes a score scale >= LARGE x too large
Q_BLOCK, EARLY_KEYS = 256, 1024                   # include/qattn.h: early = query blocks whose first row sees < 1024 keys
FLAT_W, FLAT_KEYS, FLAT_SHARE = 1.0 / 24, 192, 0.99

# ---- the case table: ONE place, so that the CPU teeth are shown on the very inputs the GPU tests run --------------------------------------
# (D, Sq, Skv, causal, dtype, fp8).  Kernel families: D 128 = the hand-scheduled kernel; D 64 / 256 = the templated kernel; causal cases
# and Skv < 1024 hold early blocks (D 128: 16-bit V inline; D 64 / 256: the 16-bit-V launches); Skv 16448 = the per-head V scale
HEAD_CASES = [
    (128, 1100, 1100, False, torch.bfloat16, "e4m3"),
    (128, 1100, 1100, True, torch.float16, "e5m2"),
    (128, 2304, 2304, True, torch.bfloat16, "e4m3"),
    (128, 333, 1090, False, torch.float16, "e4m3"),
    (128, 256, 16448, False, torch.bfloat16, "e4m3"),
    (64, 1100, 1100, True, torch.float16, "e4m3"),
    (64, 333, 1090, False, torch.bfloat16, "e5m2"),
    (256, 1100, 1100, False, torch.float16, "e4m3"),
    (256, 1100, 1100, True, torch.bfloat16, "e4m3"),
]
# the head-wise cases of the separate C calls and the pre-quantised entry (one fp8 V scale per head: V carries the V head ladder), and the
# (D, Sq, Skv, causal, dtype, fp8) at which the exact equivariance is checked through every dense entry, head-wise and token-wise
SEPARATE_HEAD = [HEAD_CASES[i] for i in (0, 1, 5, 7)]
EQUIVARIANCE_CASES = [(64, 1100, 1100, True, torch.float16, "e4m3"), (128, 1100, 1100, False, torch.bfloat16, "e4m3"),
                      (256, 333, 1090, False, torch.bfloat16, "e5m2")]
# (D, Sq, Skv, causal, dtype, fp8, side): side = which tensor carries the token ladder
TOKEN_CASES = [
    (64, 1100, 1100, True, torch.bfloat16, "e4m3", "k"),
    (128, 1100, 1100, False, torch.float16, "e4m3", "k"),
    (256, 333, 1090, False, torch.bfloat16, "e5m2", "k"),
    (128, 256, 16448, False, torch.bfloat16, "e4m3", "k"),
    (128, 2304, 2304, True, torch.bfloat16, "e4m3", "q"),
    (64, 1100, 1100, False, torch.float16, "e5m2", "q"),
    (256, 1100, 1100, True, torch.float16, "e4m3", "q"),
]
VHEAD_TOKEN = TOKEN_CASES[:3]                     # the token-wise cases that also run with the V head ladder: D 64, 128, 256
# the head ladder through the 16-bit-V entries (packed, window, block-sparse, attn_func): (D, S, dtype, fp8); a batch entry is a sequence
PACKED_CASES = [(64, 1100, torch.bfloat16, "e4m3"), (128, 1100, torch.float16, "e5m2"), (256, 1100, torch.bfloat16, "e4m3")]
WINDOW = (300, 37)                                # (left, right) of the window cases
K_ROLLS, Q_ROLLS = (1, -1, 32, -32, 64, -64), (1, -1, 32, -32, 256, -256)
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def case_id(c):
    return "D{}_{}x{}{}_{}_{}".format(c[0], c[1], c[2], "c" if c[3] else "f", NAME[c[4]], c[5]) + ("_" + c[6] if len(c) > 6 else "")


def early_rows(Sq, Skv, causal):
    """bool [Sq]: rows of the query blocks whose first row sees fewer than 1024 keys (the fused entry attends the 16-bit V there)"""
    first = (np.arange(Sq) // Q_BLOCK) * Q_BLOCK
    return (np.minimum(Skv, first + 1) if causal else np.full(Sq, Skv)) < EARLY_KEYS


def kv_of(h=None):
    return (np.arange(HQ) if h is None else h) // (HQ // HKV)


# ---- constructions --------------------------------------------------------------------------------------------------------------------------
class Ladder:
    """q [B, HQ, Sq, D], k, v [B, HKV, Skv, D] float64 (shared: do not write to them) and the exponents they were built with"""

    def __init__(self, q, k, v, **exps):
        self.q, self.k, self.v = q, k, v
        for t in (q, k, v):
            t.setflags(write=False)
        self.__dict__.update(exps)

    def tensors(self, dtype):
        """(q, k, v) torch CPU tensors of `dtype`; every value must be exact in it"""
        return to16(self.q, dtype), to16(self.k, dtype), to16(self.v, dtype)


def _codes(rng, shape):
    return rng.integers(0, 2, shape) * 2.0 - 1.0


def chunk_gains(rng, Skv):
    """g [B, HKV, ceil(Skv / 64)] seeded from G_CHUNK; the first four chunks of every head hold all four gains"""
    nch = (Skv + 63) // 64
    g = np.asarray(G_CHUNK)[rng.integers(0, len(G_CHUNK), (B, HKV, nch))]
    if nch >= len(G_CHUNK):
        g[..., :len(G_CHUNK)] = np.asarray(G_CHUNK)
    return g


def per_key(g, Skv):
    """[.., nch] per-chunk figures -> [.., Skv] per key"""
    return np.repeat(g, 64, axis=-1)[..., :Skv]


@functools.lru_cache(maxsize=None)
def head_ladder(D, Sq, Skv, gains=True, f=True, v_head=False):
    """The head ladder (module docstring).  gains = False: the same codes without any gain (e = f = g = 0); f = False: e only, on q and k -- V
    is the plain one (the exact equivariance: scale_q scale_k, and so every score, is that of the plain inputs); v_head: V carries E_VHEAD
    instead of the chunk gains, whatever q and k carry (one fp8 V scale per head: the separate calls, the row-major entry, token-wise scales).
    Skv > 16384 (one V scale per head in the fused entry): V carries E_VHEAD whenever it carries gains."""
    rng = np.random.default_rng(4001 * D + 17 * Sq + Skv)
    qc, kc = _codes(rng, (B, HQ, Sq, D)), _codes(rng, (B, HKV, Skv, D))
    g = chunk_gains(rng, Skv)
    # V over {-1, 0, 1}: |v| seeded per element, the SIGN seeded per (64-key chunk, channel) -- a chunk's contribution to a flat row is
    # then coherent (~ P_chunk / 2 per channel) and a wrong chunk gain moves O by ~ sqrt(64 / Skv) / 2 x the gain's error, not by the
    # 1 / sqrt(Skv) of element-wise random signs (which leaves the rolled gains {2, 1, 1/2, 1/4} at ~4 x the bound: no margin)
    vc = per_key(_codes(rng, (B, HKV, D, g.shape[-1])), Skv).transpose(0, 1, 3, 2) * rng.integers(0, 2, (B, HKV, Skv, D))
    e = E_HEAD if gains else np.zeros_like(E_HEAD)
    fq = F_HEAD if (gains and f) else np.zeros_like(F_HEAD)
    eq = -e[:, kv_of()] + fq[None, :]                                                  # [B, HQ]
    own_v = gains and f                       # (e only: V is the plain one)
    ev = E_VHEAD if (v_head or (own_v and Skv > 16384)) else np.zeros_like(E_VHEAD)
    if v_head or not own_v or Skv > 16384:
        g = np.zeros_like(g)
    v = vc * np.exp2(per_key(g, Skv) + ev[..., None])[..., None]
    assert np.abs(v).max() <= 2.0
    return Ladder(qc * np.exp2(eq)[..., None, None], kc * np.exp2(e)[..., None, None], v, e_k=e, e_q=eq, g=g, e_v=ev)


def _token_codes(rng, H, S, D):
    """(x [B, H, S, D], e [B, H, S]): token t is 2^e c, c a +-1 code on max(1, D / 4^e) seeded channels"""
    e = np.asarray(E_TOKEN)[rng.integers(0, len(E_TOKEN), (B, H, S))]
    n = np.maximum(1, D // 4 ** e)
    rank = rng.random((B, H, S, D)).argsort(-1).argsort(-1)
    return _codes(rng, (B, H, S, D)) * (rank < n[..., None]) * np.exp2(e)[..., None], e


def _head_v(rng, Skv, D, gain=True):
    """V over {-1, 0, 1} (|v| per element, sign per (64-key chunk, channel): head_ladder) x 2^E_VHEAD[b, h_kv]"""
    nch = (Skv + 63) // 64
    vc = per_key(_codes(rng, (B, HKV, D, nch)), Skv).transpose(0, 1, 3, 2) * rng.integers(0, 2, (B, HKV, Skv, D))
    return vc * (np.exp2(E_VHEAD)[..., None, None] if gain else 1.0)


@functools.lru_cache(maxsize=None)
def token_ladder(D, Sq, Skv, side, v_head=False):
    """The token ladder on K (side "k": Q dense +-1 codes) or on the rows of Q (side "q": K dense).  V: {-1, 0, 1} codes, sign per (chunk,
    channel); v_head: the same q, k and codes with V x 2^E_VHEAD[b, h_kv] -- the V head ladder (token-wise scales keep one fp8 V scale
    per head in every entry).  It is a second input set, not the default: a head whose V is 2^-3 cannot show a collapsed row at 4 x the
    bound, so the K / Q scale mutants have their teeth on the plain V and the V scale mutants theirs on this one"""
    rng = np.random.default_rng(9001 * D + 13 * Sq + Skv + (0 if side == "k" else 7))
    if side == "k":
        q, (k, e) = _codes(rng, (B, HQ, Sq, D)), _token_codes(rng, HKV, Skv, D)
    else:
        (q, e), k = _token_codes(rng, HQ, Sq, D), _codes(rng, (B, HKV, Skv, D))
    return Ladder(q, k, _head_v(rng, Skv, D, v_head), e=e, side=side, e_v=E_VHEAD if v_head else np.zeros_like(E_VHEAD))


@functools.lru_cache(maxsize=None)
def normal_case(D, Sq, Skv, seed=0):
    """N(0,1) q, k, v (as tests/test_gpu_attention.py draws them) rounded to bf16: the inputs WITHOUT a ladder, to show the hole"""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, H, S, D, generator=g).to(torch.bfloat16) for H, S in ((HQ, Sq), (HKV, Skv), (HKV, Skv)))
    return q, k, v


def antithetic(lad, offsets=True):
    """The ladder for the key-smoothing entries: key 2j+1 becomes minus key 2j (the codes of every channel sum to zero over the sequence;
    Skv must be even) and channel d of kv group (b, h) gets the offset c 2^e, c in {-2, 0, 2} seeded.  Every partial sum is a small
    integer times 2^e, so the fp32 channel mean is c 2^e EXACTLY in any summation order, k - mean is the ladder key exactly, and the
    smoothed call must quantise the ladder's own bytes and scales.  Returns (the Ladder the kernel is given, the Ladder it must attend,
    mean [B, HKV, D])."""
    assert lad.k.shape[2] % 2 == 0
    ks = lad.k.copy()
    ks[:, :, 1::2] = -ks[:, :, 0::2]
    rng = np.random.default_rng(ks.shape[2] + ks.shape[3])
    mean = (rng.integers(-1, 2, (B, HKV, ks.shape[3])) * 2.0 if offsets else np.zeros((B, HKV, ks.shape[3]))) * np.exp2(lad.e_k)[..., None]
    extra = {n: getattr(lad, n) for n in ("e_k", "e_q", "g", "e_v")}
    return Ladder(lad.q.copy(), ks + mean[:, :, None, :], lad.v.copy(), **extra), Ladder(lad.q.copy(), ks, lad.v.copy(), **extra), mean


# ---- the CPU quantiser's output and the fp64 reference ------------------------------------------------------------------------------------
class Quantised:
    """q8, k8 (bytes), sq, sk (fp32: [B, H] head / [B, H, S] token) from oracle.quantize_fp8 on the 16-bit tensors; the V the entry
    attends as float64 (`v_fp8`: block-scaled or head-scaled fp8 V de-quantised; `v16`: the caller's numbers) and as 16-bit patterns"""

    def __init__(self, q, k, v, dtype, fp8, mode, v_block=None):
        self.dtype, self.fp8, self.mode = dtype, fp8, mode
        self.vb16 = bits16(v)
        self.q8, self.sq = oracle.quantize_fp8(bits16(q), fmt16(dtype), mode, FMT[fp8])
        self.k8, self.sk = oracle.quantize_fp8(bits16(k), fmt16(dtype), mode, FMT[fp8])
        self.qf = oracle.fp8_to_f32(self.q8, FMT[fp8]).astype(np.float64)
        self.kf = oracle.fp8_to_f32(self.k8, FMT[fp8]).astype(np.float64)
        self.v16 = v.double().numpy()
        self.v_block = (mode == "head" and v.shape[2] <= 16384) if v_block is None else v_block
        if self.v_block:
            self.v8, self.ve, deq = oracle.quantize_v_block(self.vb16, fmt16(dtype), FMT[fp8])
            self.v_fp8 = oracle.bf16_bits_to_f32(deq).astype(np.float64)
        else:
            self.v8, self.sv = oracle.quantize_fp8(self.vb16, fmt16(dtype), "head", FMT[fp8], "compiled")
            self.v_fp8 = oracle.fp8_to_f32(self.v8, FMT[fp8]).astype(np.float64) * self.sv.astype(np.float64)[..., None, None]

    def row_scale(self, sq=None):
        """[B, HQ, Sq] float64"""
        sq = np.asarray(self.sq if sq is None else sq, np.float64)
        return np.broadcast_to(sq[..., None] if sq.ndim == 2 else sq, self.q8.shape[:3])

    def col_scale(self, sk=None):
        """[B, HQ, Skv] float64: the key scales as each QUERY head reads them"""
        sk = np.asarray(self.sk if sk is None else sk, np.float64)
        sk = sk[..., None] if sk.ndim == 2 else sk
        return np.broadcast_to(sk[:, kv_of()], (B, HQ, self.k8.shape[2]))


def quantise(lad_or_tensors, dtype, fp8, mode, v_block=None):
    t = lad_or_tensors.tensors(dtype) if isinstance(lad_or_tensors, Ladder) else lad_or_tensors
    return Quantised(*t, dtype, fp8, mode, v_block)


def mask_of(Sq, Skv, causal=False, window=None, tiles=None):
    """bool [1 or HQ, Sq, Skv]: full / top-left causal / bottom-right window (left, right) / 128 x 128 tile table [H, nQB, nKB]"""
    if tiles is not None:
        return P.tile_mask(tiles, Sq, Skv, Skv)
    if window is not None:
        return P.band_mask(*P.band_edges(Sq, Skv, "window", window), Skv, Skv)[None]
    return P.band_mask(*P.band_edges(Sq, Skv, "causal" if causal else "full"), Skv, Skv)[None]


def sparse_tiles(S):
    """bool [HQ, nb, nb], nb = ceil(S / 128): a checkerboard plus the first key block, the parity of the board alternating with the head"""
    nb = (S + 127) // 128
    i, j, h = np.arange(nb)[None, :, None], np.arange(nb)[None, None, :], np.arange(HQ)[:, None, None]
    return ((i + j + h) % 2 == 0) | (j == 0)


class Scores:
    """The code products q8 . k8 of a case (no scale applied), kept so that a mutant costs one softmax and one P.V, not a new Q.K^T"""

    def __init__(self, qz, mask):
        self.qz, self.D = qz, qz.q8.shape[3]
        self.mask = torch.from_numpy(np.array(mask))
        kf = torch.from_numpy(qz.kf).repeat_interleave(HQ // HKV, dim=1)
        self.raw = torch.from_numpy(qz.qf) @ kf.transpose(-1, -2)                      # [B, HQ, Sq, Skv] fp64, exact (integers x 2^n)

    def softmax(self, rs=None, cs=None, v=None, sm_scale=None):
        """fp64 masked softmax with row scales rs [B, HQ, Sq], column scales cs [B, HQ, Skv] and values v [B, HKV, Skv, D] (default: the
        quantiser's own scales and the fp8 V): (out [B, HQ, Sq, D], lse [B, HQ, Sq]); a row without a key is 0 / -inf"""
        qz = self.qz
        rs = torch.from_numpy(np.array(qz.row_scale() if rs is None else rs))
        cs = torch.from_numpy(np.array(qz.col_scale() if cs is None else cs))
        vv = torch.from_numpy(np.ascontiguousarray(qz.v_fp8 if v is None else v, np.float64)).repeat_interleave(HQ // HKV, dim=1)
        sm = 1.0 / math.sqrt(self.D) if sm_scale is None else sm_scale
        out, lse = [], []
        for b in range(B):
            s = (self.raw[b] * (rs[b][..., None] * sm) * cs[b][:, None, :]).masked_fill(~self.mask, -math.inf)
            l = torch.logsumexp(s, dim=-1)
            out.append(torch.exp(s - l.clamp_min(-1e300)[..., None]) @ vv[b])
            lse.append(l)
        return torch.stack(out).numpy(), torch.stack(lse).numpy()

    def weights_summary(self):
        """(largest weight, effective key count 1 / sum p^2) per row [B, HQ, Sq] of the unmutated reference"""
        qz, sm = self.qz, 1.0 / math.sqrt(self.D)
        rs, cs = torch.from_numpy(np.array(qz.row_scale())), torch.from_numpy(np.array(qz.col_scale()))
        top, eff = [], []
        for b in range(B):
            p = torch.softmax((self.raw[b] * (rs[b][..., None] * sm) * cs[b][:, None, :]).masked_fill(~self.mask, -math.inf), dim=-1)
            top.append(p.amax(-1))
            eff.append(1.0 / (p * p).sum(-1))
        return torch.stack(top).numpy(), torch.stack(eff).numpy()


def oracle_reference(qz, causal, v="fp8", return_lse=False):
    """oracle.attention_forward on the CPU quantiser's output: v = "fp8" (the entry's fp8 V) or "v16" (the caller's 16-bit V)"""
    f = FMT[qz.fp8]
    if v == "v16":
        vv, vf, sv = qz.vb16, fmt16(qz.dtype), None
    elif qz.v_block:
        vv, vf, sv = oracle.f32_to_bf16_bits(qz.v_fp8.astype(np.float32)), oracle.FMT_BF16, None
    else:
        vv, vf, sv = qz.v8, f, qz.sv
    return oracle.attention_forward(qz.q8, qz.k8, vv, f, f, vf, qz.sq, qz.sk, sv, scale_mode=qz.mode, causal=causal, return_lse=return_lse)


# ---- mutants: one scale table re-indexed ------------------------------------------------------------------------------------------------
def head_mutants(qz, packed=False):
    """{name: (rs, cs)} for head-wise scales sq [B, HQ], sk [B, HKV]"""
    sq, sk = qz.sq.astype(np.float64), qz.sk.astype(np.float64)
    h, b = np.arange(HQ), np.arange(B)
    at_q_index = sk.reshape(-1)[(b[:, None] * HKV + h[None, :]) % sk.size]             # [B, HQ]: scale_k[b * Hkv + h_q]
    kq = lambda t: np.broadcast_to(t[..., None], (B, HQ, qz.k8.shape[2]))              # a per-(b, query head) key scale
    res = {
        "scale_k read at the query-head index": (None, kq(at_q_index)),
        "scale_k of the other batch entry": (None, qz.col_scale(sk[::-1])),
        "scale_q of the neighbouring head": (qz.row_scale(np.roll(sq, -1, axis=1)), None),
        "every head reads head 0's scale_q": (qz.row_scale(np.repeat(sq[:, :1], HQ, 1)), None),
        "every head reads head 0's scale_k": (None, qz.col_scale(np.repeat(sk[:, :1], HKV, 1))),
    }
    if packed:
        res["the previous sequence's scale_q"] = (qz.row_scale(np.roll(sq, 1, axis=0)), None)
        res["the previous sequence's scale_k"] = (None, qz.col_scale(np.roll(sk, 1, axis=0)))
    return res


def token_mutants(qz, side):
    """{name: (rs, cs)} for token-wise scales sq [B, HQ, Sq], sk [B, HKV, Skv]: the table of the ladder's side rolled / read at the other head"""
    sq, sk = qz.sq.astype(np.float64), qz.sk.astype(np.float64)
    if side == "k":
        res = {f"scale_k of token j{-r:+d}": (None, qz.col_scale(np.roll(sk, r, axis=-1))) for r in K_ROLLS}
        res["scale_k of the other kv head"] = (None, qz.col_scale(sk[:, ::-1]))
    else:
        res = {f"scale_q of token i{-r:+d}": (qz.row_scale(np.roll(sq, r, axis=-1)), None) for r in Q_ROLLS}
        res["scale_q of the neighbouring head"] = (qz.row_scale(np.roll(sq, -1, axis=1)), None)
    return res


def vchunk_mutants(qz):
    """{name: V [B, HKV, Skv, D] float64} for the block-scaled V: the bytes of chunk c de-quantised with another chunk's exponent"""
    assert qz.v_block
    Skv = qz.v8.shape[2]
    pay = oracle.fp8_to_f32(qz.v8, FMT[qz.fp8]).astype(np.float64)
    e = qz.ve.astype(np.int64) - 127                                                    # [B, HKV, nch]
    with_e = lambda ee: pay * np.exp2(per_key(ee, Skv))[..., None]
    assert np.array_equal(with_e(e), qz.v_fp8)
    last = e.copy()
    last[..., -1] = e[..., -2]
    return {
        "chunk gains rolled by +1": with_e(np.roll(e, 1, axis=-1)),
        "chunk gains rolled by -1": with_e(np.roll(e, -1, axis=-1)),
        "chunk 0's gain for every chunk": with_e(np.repeat(e[..., :1], e.shape[-1], -1)),
        # (the bytes of every chunk times the head's fp32 scale amax / fmax, as oracle.quantize_fp8 computes it for the head)
        "the head's one scale in place of the chunk scales": pay * oracle.quantize_fp8(qz.vb16, fmt16(qz.dtype), "head", FMT[qz.fp8])[1].astype(np.float64)[..., None, None],
        "the last (partial) chunk alone reads its neighbour's gain": with_e(last),
    }


def vhead_mutants(qz):
    """{name: (V [B, HKV, Skv, D] float64, log2 of the wrong / right scale [B, HKV])} for one fp8 V scale per head: the bytes of head
    (b, h_kv) de-quantised with another head's scale"""
    assert not qz.v_block
    pay, sv = oracle.fp8_to_f32(qz.v8, FMT[qz.fp8]).astype(np.float64), qz.sv.astype(np.float64)
    with_s = lambda t: (pay * t[..., None, None], np.log2(t / sv))
    assert np.array_equal(with_s(sv)[0], qz.v_fp8)
    return {"scale_v of the other batch entry": with_s(sv[::-1]), "scale_v of the other kv head": with_s(sv[:, ::-1]),
            "every head reads head 0's scale_v": with_s(np.repeat(sv[:, :1], HKV, 1))}


def too_large(qz, rs, cs, mask):
    """bool [B, HQ, Sq]: rows on which the mutant makes the scale of some attended key's score >= LARGE x too large"""
    r = np.ones((B, HQ, qz.q8.shape[2])) if rs is None else rs / qz.row_scale()
    if cs is None:
        return r >= LARGE
    c = torch.from_numpy(np.array(cs / qz.col_scale()))                     # [B, HQ, Skv]
    m = torch.from_numpy(np.array(mask))
    top = torch.stack([(c[b][:, None, :].expand(HQ, m.shape[1], -1).masked_fill(~m.expand(HQ, -1, -1), 0.0)).amax(-1) for b in range(B)]).numpy()
    return r * top >= LARGE


def flatter(qz, rs, cs):
    """bool [B, HQ, Sq]: rows on which no score scale grows (the mutant makes them flatter, or leaves them: they hide)"""
    r = np.ones((B, HQ, qz.q8.shape[2])) if rs is None else rs / qz.row_scale()
    c = np.ones((B, HQ, 1)) if cs is None else (cs / qz.col_scale()).max(-1, keepdims=True)
    return r * c <= 1.0


def bound_of(ref):
    """the bound the GPU tests apply (tests/gpu_utils.grade), the LARGER of the two wherever the path of a row is the kernel's choice"""
    return P.project_bound(ref, None)


def moved(ref, mut):
    """per row: max over the channels of |mut - ref| / bound"""
    return (np.abs(mut - ref) / bound_of(ref)).max(-1)


# ---- the FP8-PV family: block-sparse / packed / window FP8-PV, split-KV over prepared K / V, the fixed-scale and paged caches ---------------
# (tests/test_cpu_scale_ladder_fp8pv.py: the teeth; tests/test_gpu_scale_ladder_fp8pv.py: the kernels.)  These entries keep ONE fp8 V scale
# per (batch entry, kv head) and apply it once in the epilogue; the split-KV kernels pack the rows of the G query heads of a kv head into
# 128-row tiles (packed row r = g Sq + p), so that `g`, and with it scale_q, differs per lane.
# (D, Sq, Skv, causal, dtype, fp8): the smallest shapes that hold a tile with rows of two heads in one wave (Sq 1), a tile that crosses a
# head boundary (Sq 70: 140 packed rows; Sq 130: 260 rows, a ragged third tile), one-term FAST workgroups (>= 1024 keys in a split: 1100 /
# 1, 2304 / 1) and two-term ones.  Batch entry b uses the first used_lengths(Skv)[b] keys: the second entry ends inside a key block.
FP8PV_CASES = [
    (128, 1, 1100, True, torch.bfloat16, "e4m3"),
    (64, 5, 2304, True, torch.float16, "e4m3"),
    (256, 130, 1100, True, torch.bfloat16, "e4m3"),
    (128, 130, 2304, False, torch.float16, "e5m2"),
    (128, 70, 1100, True, torch.bfloat16, "e4m3"),
]
SPLITS = (1, 3, 9)
TILE = 128                                        # packed query rows per workgroup of the split-KV kernels (include/qattn_splitkv.h)
PACKED_SQ = (130, 5)                              # queries per sequence of the packed-query cases: the ladder's two batch entries
SPARSE_GAIN, SPARSE_SHARE = 4.0, 16               # group ladder: the even heads of a GQA group carry +-4 on D / 16 channels per row


def used_lengths(Skv):
    return [Skv, Skv - 64]


@functools.lru_cache(maxsize=None)
def head_ladder_plain_v(D, Sq, Skv):
    """the head ladder's q and k (e and f) with the plain V over {-1, 0, 1}: no chunk gains -- the FP8-PV family keeps one scale_v per head"""
    lad, plain = head_ladder(D, Sq, Skv), head_ladder(D, Sq, Skv, gains=False)
    return Ladder(lad.q.copy(), lad.k.copy(), plain.v.copy(), e_k=lad.e_k, e_q=lad.e_q, g=plain.g, e_v=plain.e_v)


@functools.lru_cache(maxsize=None)
def group_ladder(D, Sq, Skv, gains=True):
    """The in-group ladder: K dense +-1 codes x 2^e, e = E_HEAD[b, h_kv]; inside every GQA group the EVEN query heads carry sparse codes
    (+-4 on D / 16 seeded channels per row, 0 elsewhere) and the ODD heads dense +-1 codes, all x 2^(-e).  Every row's scores keep a standard
    deviation of 1 (16 D / 16 = D), every non-zero element of a head sits at the head's abs-max (bytes 0 or +- the largest code), and
    scale_q inside a group differs by x4 with the LARGER scale on the group's first head: a row of an odd head that reads the scale of the
    head its tile begins with gets scores 4 x too large and collapses.  V is the plain one.  gains = False: e = 0 (the sparse / dense codes stay)."""
    rng = np.random.default_rng(7001 * D + 19 * Sq + Skv)
    qc, kc = _codes(rng, (B, HQ, Sq, D)), _codes(rng, (B, HKV, Skv, D))
    rank = rng.random((B, HQ, Sq, D)).argsort(-1).argsort(-1)
    sparse = (np.arange(HQ) % (HQ // HKV) == 0)[None, :, None, None]
    qc = np.where(sparse, qc * SPARSE_GAIN * (rank < D // SPARSE_SHARE), qc)
    nch = (Skv + 63) // 64
    vc = per_key(_codes(rng, (B, HKV, D, nch)), Skv).transpose(0, 1, 3, 2) * rng.integers(0, 2, (B, HKV, Skv, D))
    e = E_HEAD if gains else np.zeros_like(E_HEAD)
    eq = -e[:, kv_of()] + np.where(sparse[0, :, 0, 0], int(np.log2(SPARSE_GAIN)), 0)[None, :]        # log2 of scale_q / the plain scale
    return Ladder(qc * np.exp2(-e[:, kv_of()])[..., None, None], kc * np.exp2(e)[..., None, None], vc, e_k=e, e_q=eq, g=np.zeros((B, HKV, nch), np.int64),
                  e_v=np.zeros_like(E_VHEAD), sparse=sparse[0, :, 0, 0])


def used_mask(Sq, Skv, used, causal, sq=None, top_left=False):
    """bool [B, 1, Sq, Skv]: batch entry b has sq[b] <= Sq query rows (default Sq; the rows behind them attend nothing) and attends its first
    used[b] keys, causal bottom-right: position p attends the keys j <= p + used[b] - sq[b] (the split-KV, cache, paged and window entries);
    top_left: the keys j <= p (the packed entries' is_causal, include/qattn_varlen.h)"""
    sq = [Sq] * len(used) if sq is None else sq
    p, j = np.arange(Sq)[:, None], np.arange(Skv)[None, :]
    m = [(p < n) & (j < L) & ((j <= p + (0 if top_left else L - n)) if causal else True) for L, n in zip(used, sq)]
    return np.stack(m)[:, None]


class UsedScores(Scores):
    """Scores with one mask per batch entry (used_mask): the reference of the split-KV / cache / paged entries and of seqused_k"""

    def __init__(self, qz, mask):
        assert mask.ndim == 4 and mask.shape[0] == B
        Scores.__init__(self, qz, mask)

    def _scaled(self, b, rs, cs):
        return (self.raw[b] * (rs[b][..., None] * (1.0 / math.sqrt(self.D))) * cs[b][:, None, :]).masked_fill(~self.mask[b], -math.inf)

    def softmax(self, rs=None, cs=None, v=None, sm_scale=None):
        assert sm_scale is None
        qz = self.qz
        rs = torch.from_numpy(np.array(qz.row_scale() if rs is None else rs))
        cs = torch.from_numpy(np.array(qz.col_scale() if cs is None else cs))
        vv = torch.from_numpy(np.ascontiguousarray(qz.v_fp8 if v is None else v, np.float64)).repeat_interleave(HQ // HKV, dim=1)
        out, lse = [], []
        for b in range(B):
            s = self._scaled(b, rs, cs)
            l = torch.logsumexp(s, dim=-1)
            out.append(torch.exp(s - l.clamp_min(-1e300)[..., None]) @ vv[b])
            lse.append(l)
        return torch.stack(out).numpy(), torch.stack(lse).numpy()

    def weights_summary(self):
        """(largest weight, effective key count) per row [B, HQ, Sq]; rows without a key: (0, 0)"""
        qz = self.qz
        rs, cs = torch.from_numpy(np.array(qz.row_scale())), torch.from_numpy(np.array(qz.col_scale()))
        top, eff = [], []
        for b in range(B):
            s = self._scaled(b, rs, cs)
            p = torch.exp(s - torch.logsumexp(s, dim=-1).clamp_min(-1e300)[..., None])
            top.append(p.amax(-1))
            eff.append(torch.where(p.sum(-1) > 0, 1.0 / (p * p).sum(-1).clamp_min(1e-300), torch.zeros(())))
        return torch.stack(top).numpy(), torch.stack(eff).numpy()


def tile_mutants(qz, sq_per_sequence):
    """{name: (rs, None)}: the two ways the per-lane `g` of the split-KV kernels invites.  Batch entry b has sq_per_sequence[b] query rows;
    row p of head h = h_kv G + g is packed row r = g Sq_b + p of its kv head, in tile r // 128.
    1. every row of a tile reads the scale_q of the head of the tile's FIRST row (g taken from the workgroup-uniform r_first);
    2. g computed with max_seqlen_q in place of the sequence's own Sq (packed queries: sequences shorter than the longest)."""
    sq = qz.sq.astype(np.float64)
    Sq, G, mx = qz.q8.shape[2], HQ // HKV, max(sq_per_sequence)
    first, by_max = qz.row_scale().copy(), qz.row_scale().copy()
    for b, n in enumerate(sq_per_sequence):
        for h in range(HQ):
            hkv, g = h // G, h % G
            r = g * n + np.arange(n)
            first[b, h, :n] = sq[b, hkv * G + np.minimum((r // TILE) * TILE // n, G - 1)]
            by_max[b, h, :n] = sq[b, hkv * G + np.minimum(r // mx, G - 1)]
    return {"scale_q of the tile's first row": (first, None), "g computed with max_seqlen_q": (by_max, None)}

"""FP8 multi-head latent attention (MLA: DeepSeek-V2 / V3 / R1, Kimi-K2) in its NON-ABSORBED prefill form on packed variable-length
sequences: `fp8_mla_prefill_varlen_func` and `mla_prefill_input_reason` (include/qattn_mla_prefill.h).  The decode
side -- the absorbed form over a paged latent cache -- is mla.py.

In prefill every head has its own keys and values: a score is a 192-channel product (the head's 128 "nope" channels followed by 64 rotary
channels), a value has 128 channels, and the rotary slice of K is ONE row per token that all heads attend.

    out = fp8_mla_prefill_varlen_func(q, kv[..., :128], k_pe, kv[..., 128:], cu_q, cu_k, max_q, max_k, scale=model_softmax_scale)
    # q [total_q, H, 192] (q_nope | q_pe, rotated), kv [total_k, H, 256] the k_nope | v projection, k_pe [total_k, 64] rotated

Chunked prefill: one call over the cached context (causal=False), one over the chunk itself (causal=True), merged by `merge_attn_states`.

Numerics (the eager definition `_prefill_eager` below is the specification): q is quantised token-wise to e4m3 by `mla.quantize_q_eager`'s
formula over the 192 channels; K gets one scale per (sequence, head) over the head's k_nope AND the shared k_pe of the sequence's used keys,
V one per (sequence, head); both use the library's head-wise quantiser (`quantize_kv_eager`) in config.attention.fp8_format.

Package attributes, not names of `__all__`.  Not offered: grouped heads, windows, sinks, soft cap, key smoothing, precision "fast" /
"auto", a backward pass."""
import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native, nn
from .mla import quantize_q_eager
from .utils import checks

D_QK, D_NOPE, D_ROPE, D_V = _native.MLA_PREFILL_D_QK, _native.MLA_PREFILL_D_NOPE, _native.MLA_PREFILL_D_ROPE, _native.MLA_PREFILL_D_V


def _is_int(x) -> bool:
    return isinstance(x, (int, torch.SymInt)) and not isinstance(x, bool)


def mla_prefill_input_reason(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, *, scale=None,
                             seqused_k=None) -> Optional[str]:
    """The first rule the arguments of `fp8_mla_prefill_varlen_func` break, or None.  Shapes, dtypes, devices and strides only: the CONTENTS
    of the tables are read on the device, where every extent is clamped to its tensor."""
    if not all(isinstance(t, Tensor) for t in (q, k_nope, k_pe, v)) or q.dim() != 3 or k_nope.dim() != 3 or v.dim() != 3 or k_pe.dim() != 2:
        return "NYI: query, k_nope and value must be 3-D packed tensors [total_tokens, heads, head_dim] and k_pe 2-D [total_tokens, 64]"
    if any(t.requires_grad for t in (q, k_nope, k_pe, v)):
        return "NYI: query, k_nope, k_pe and value must be leaf tensors (no backward)"
    if q.dtype not in (torch.float16, torch.bfloat16):
        return f"Expected query to have dtype torch.float16 or torch.bfloat16, but got query.dtype: {q.dtype} instead."
    if any(t.dtype != q.dtype for t in (k_nope, k_pe, v)):
        return f"Expected query, k_nope, k_pe and value to share a dtype, but got {q.dtype}, {k_nope.dtype}, {k_pe.dtype}, {v.dtype} instead."
    if (q.shape[2], k_nope.shape[2], k_pe.shape[1], v.shape[2]) != (D_QK, D_NOPE, D_ROPE, D_V):
        return (f"Expected head dimensions {D_QK} (query: q_nope | q_pe), {D_NOPE} (k_nope), {D_ROPE} (k_pe) and {D_V} (value), but got "
                f"{q.shape[2]}, {k_nope.shape[2]}, {k_pe.shape[1]} and {v.shape[2]}.")
    if q.shape[1] == 0 or k_nope.shape[1] != q.shape[1] or v.shape[1] != q.shape[1]:
        return f"Expect one head count for query, k_nope and value (MHA) but got {q.shape[1]}, {k_nope.shape[1]} and {v.shape[1]}."
    if k_nope.shape[0] != v.shape[0] or k_pe.shape[0] != v.shape[0]:
        return f"Expect k_nope, k_pe and value to hold the same tokens but got {k_nope.shape[0]}, {k_pe.shape[0]} and {v.shape[0]}."
    if any(t.device != q.device for t in (k_nope, k_pe, v)):
        return f"Expected query, k_nope, k_pe and value to be on the same device, but got {q.device}, {k_nope.device}, {k_pe.device}, {v.device}."
    for name, t in (("query", q), ("k_nope", k_nope), ("k_pe", k_pe), ("value", v)):
        if not _native.mla_rows_addressable(t):
            return f"Expected {name} to have dense channels and 16-byte-aligned rows, but got strides {tuple(t.stride())}; pass {name}.contiguous()"
    for name, t in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if not isinstance(t, Tensor) or t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] < 2:
            return f"Expected {name} to be a 1-D torch.int32 tensor of length B+1 >= 2"
        if t.device != q.device:
            return f"Expected {name} to be on {q.device}, but got {t.device} instead."
    if cu_seqlens_q.shape[0] != cu_seqlens_k.shape[0]:
        return f"Expected cu_seqlens_q and cu_seqlens_k of the same length B+1, but got {cu_seqlens_q.shape[0]} and {cu_seqlens_k.shape[0]}."
    if seqused_k is not None:
        if not isinstance(seqused_k, Tensor) or seqused_k.dtype != torch.int32 or seqused_k.dim() != 1:
            return "Expected seqused_k to be a 1-D torch.int32 tensor of length B"
        if seqused_k.shape[0] != cu_seqlens_q.shape[0] - 1:
            return f"Expected seqused_k of length B = {cu_seqlens_q.shape[0] - 1}, but got {seqused_k.shape[0]}."
        if seqused_k.device != q.device:
            return f"Expected seqused_k to be on {q.device}, but got {seqused_k.device} instead."
    if not (_is_int(max_seqlen_q) and _is_int(max_seqlen_k)) or max_seqlen_q < 0 or max_seqlen_k < 0:
        return "Expected max_seqlen_q and max_seqlen_k to be non-negative host ints"
    if scale is None:
        return "scale is required: MLA's softmax scale is the model's (1/sqrt(192) times its YaRN factor)"
    if not (isinstance(scale, (int, float)) and not isinstance(scale, bool) and math.isfinite(scale) and scale > 0):
        return f"scale must be a finite number > 0, got {scale!r}"
    return None


# ---- the eager definition (CPU tensors, config.attention.force_eager_fallback): the specification ------------------------------------------
def kv_scale_eager(amax: Tensor, fp8_dtype) -> Tensor:
    """the head-wise scale of the library's quantiser: max(amax * (1 / fmax), 2^-23) in fp32"""
    inv = torch.tensor(1.0 / torch.finfo(fp8_dtype).max, dtype=torch.float32, device=amax.device)
    return (amax.float() * inv).clamp_min(torch.finfo(torch.float32).eps)


def quantize_kv_eager(x: Tensor, scale: Tensor, fp8_dtype) -> Tensor:
    """the head-wise quantiser's payload: fp8(clamp(round16(fp32(x) / scale), +-fmax)); scale broadcasts against x"""
    fmax = torch.finfo(fp8_dtype).max
    return (x.float() / scale).to(x.dtype).float().clamp(-fmax, fmax).to(fp8_dtype)


def _prefill_eager(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, seqused_k, scale, causal, fp8_dtype):
    """Per sequence: quantise (q token-wise, K and V per head over the used keys, K's scale over k_nope and the shared k_pe), de-quantise, fp32
    softmax attention under the bottom-right mask.  Tokens outside every sequence keep zero rows.  (Reads the tables on the host.)"""
    total_q, H, _ = q.shape
    total_k = k_nope.shape[0]
    B = cu_seqlens_q.shape[0] - 1
    dev = q.device
    cq, ck = cu_seqlens_q.tolist(), cu_seqlens_k.tolist()
    used = None if seqused_k is None else seqused_k.tolist()
    out = torch.zeros((total_q, H, D_V), dtype=q.dtype, device=dev)
    lse = torch.full((H, total_q), -math.inf, dtype=torch.float32, device=dev)
    q8 = torch.zeros((total_q, H, D_QK), dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)
    sq = torch.zeros((total_q, H), dtype=torch.float32, device=dev)
    zero = torch.zeros((H,), dtype=torch.float32, device=dev)
    sk, sv = (kv_scale_eager(zero, fp8_dtype).expand(B, H).contiguous() for _ in range(2))   # (no used key: amax 0)
    clamp = lambda x, lo, hi: min(max(int(x), lo), hi)
    for i in range(B):
        q0 = clamp(cq[i], 0, total_q)
        lq = clamp(cq[i + 1], q0, total_q) - q0
        k0 = clamp(ck[i], 0, total_k)
        lk = clamp(ck[i + 1], k0, total_k) - k0
        if used is not None:
            lk = clamp(used[i], 0, lk)
        if lq > 0:
            q8[q0:q0 + lq], sq[q0:q0 + lq] = quantize_q_eager(q[q0:q0 + lq])
        if lk == 0:
            continue   # (no key: zero rows, LSE -inf)
        kn, kp, vi = k_nope[k0:k0 + lk], k_pe[k0:k0 + lk], v[k0:k0 + lk]
        sk[i] = kv_scale_eager(torch.maximum(kn.abs().amax(dim=(0, 2)), kp.abs().amax()), fp8_dtype)
        sv[i] = kv_scale_eager(vi.abs().amax(dim=(0, 2)), fp8_dtype)
        if lq == 0:
            continue
        k8 = quantize_kv_eager(torch.cat([kn, kp[:, None, :].expand(lk, H, D_ROPE)], dim=-1), sk[i][None, :, None], fp8_dtype)
        v8 = quantize_kv_eager(vi, sv[i][None, :, None], fp8_dtype)
        qd = q8[q0:q0 + lq].float() * sq[q0:q0 + lq, :, None]
        s = torch.einsum("qhd,khd->hqk", qd, k8.float() * sk[i][None, :, None]) * scale
        if causal:
            rows, keys = torch.arange(lq, device=dev)[:, None], torch.arange(lk, device=dev)[None, :]
            s = s.masked_fill(keys > rows + (lk - lq), -math.inf)
        l = torch.logsumexp(s, dim=-1)
        p = torch.where(torch.isneginf(l)[..., None], torch.zeros_like(s), torch.exp(s - l[..., None]))
        out[q0:q0 + lq] = torch.einsum("hqk,khd->qhd", p, v8.float() * sv[i][None, :, None]).to(q.dtype)
        lse[:, q0:q0 + lq] = l
    return out, lse, q8, sq, sk, sv


# ---- the call ----------------------------------------------------------------------------------------------------------------------------------
def fp8_mla_prefill_varlen_func(q: Tensor, k_nope: Tensor, k_pe: Tensor, v: Tensor, cu_seqlens_q: Tensor, cu_seqlens_k: Tensor,
                                max_seqlen_q: int, max_seqlen_k: int, *, scale: Optional[float] = None, causal: bool = True,
                                seqused_k: Optional[Tensor] = None, return_lse: bool = False, return_quantized: bool = False):
    """Non-absorbed MLA prefill on packed sequences: q [total_q, H, 192] (q_nope | the rotated q_pe), k_nope [total_k, H, 128], k_pe
    [total_k, 64] (rotated, ONE row per token shared by all heads), v [total_k, H, 128], bf16 or fp16 (one dtype); returns out
    [total_q, H, 128] in q's dtype.

    Views are read in place through their token / head strides (dense channels, 16-byte-aligned rows, strides non-negative multiples of 8):
    k_nope and v may be the two halves of one [total_k, H, 256] projection.  MHA only.
    cu_seqlens_*  int32 [B+1] on the device; seqused_k optional int32 [B]: the keys sequence i uses.  Extents are clamped as by
                  `fp8_attn_varlen_func`; max_seqlen_* are host ints, accepted for signature compatibility.
    scale         REQUIRED: the model's softmax scale (1/sqrt(192) times its YaRN factor); there is no default.
    causal        BOTTOM-RIGHT, as in `fp8_mla_paged_func`: row r of a sequence attends keys j <= r + L_k - L_q, L_k the used keys.  A row
                  without a key (L_k = 0; the first rows when L_q > L_k) is a zero row with LSE -inf.
    return_lse    appends lse fp32 [H, total_q]: the natural log-sum-exp of the scaled scores in the packed layout `merge_attn_states` takes.
    return_quantized  appends (q8 [total_q, H, 192] e4m3, scale_q [total_q, H], scale_k [B, H], scale_v [B, H]): what the kernel's quantisers
                  made of the operands (zeros where no sequence has a token).
    Keys at or behind seqused_k and tokens outside every sequence influence no output bit, the scales included.  Everything is read on the
    device: no host synchronisation, graph-capture safe.  CPU tensors and config.attention.force_eager_fallback run the eager definition
    (`_prefill_eager`); on the device there is no fallback.  Unsupported input raises ValueError(reason)."""
    if not checks.config_value("attention.skip_supported_check"):
        reason = mla_prefill_input_reason(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, scale=scale,
                                          seqused_k=seqused_k)
        if reason:
            raise ValueError(reason)
    fp8_format = checks.config_value("attention.fp8_format")
    if (not q.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling():
        out, lse, q8, sq, sk, sv = _prefill_eager(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, seqused_k, float(scale), bool(causal),
                                                  _native.fp8_dtype_of(fp8_format))
    else:
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        out, lse, q8, sq, sk, sv = nn._ops().fp8_mla_prefill_varlen_forward(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, seqused_k, float(scale),
                                                                            fp8_format, bool(causal), bool(return_quantized))
    res: Tuple = (out,)
    if return_lse:
        res += (lse,)
    if return_quantized:
        res += (q8, sq, sk, sv)
    return res if len(res) > 1 else out

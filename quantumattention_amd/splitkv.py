"""Split-KV FP8 attention for short queries over long, PREPARED keys and values: `prepare_kv_fp8` and `fp8_attn_splitkv_func`.

Every other attention entry gives one workgroup one 128-row query tile of one head and lets it sweep all of that head's keys.  With few
queries and many keys -- LLM decode, speculative or chunked decode (Sq 2 .. 16), a prompt suffix against a cached prefix, a few latent
queries reading a long sequence -- that is a few dozen workgroups on a 256-CU chip, each streaming a head's whole K and V.  This entry
cuts the key axis of a head across `num_splits` workgroups, lets the G = Hq / Hkv query heads of a kv head share tiles (K and V are read
once per group, not G times), and merges the partial states with the library's state merge (merge.merge_attn_states).  K and V are
quantised ONCE (`prepare_kv_fp8`) and attended many times: a cached prefix, the text keys of a cross-attention layer over all denoising
steps.

Numerics (include/qattn_splitkv.h): q is quantised head-wise by the quant pre-pass; K / V are the bytes and head-wise scales of
`_native.quant_fp8(..., scaling="head-wise", layout=KFRAG / VFRAG)` -- bit for bit what `fp8_block_sparse_attn_pv_func(pv_precision="fp8")`
attends; both products run on the FP8 matrix pipe.  Package attributes, not names of `__all__` (that list mirrors the reference).

An appendable cache with FIXED scales is kvcache.KVCacheFP8 (kv_cache_append_fp8): a PreparedKV this entry attends
unchanged.  A PAGED cache (a pool of pages behind a block table) is paged.PagedKVCacheFP8 with its own entry, fp8_attn_paged_func
(DESIGN.md section 4.19): the bits of this entry on the gathered cache.  Not offered: scales that grow with the
tensor, key smoothing on prepared keys, precision="auto", the 16-bit-P.V numerics, strided views.  Sliding windows: splitkv_window.py."""
import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native, merge, nn
from .utils import checks

BLOCK_N = 128        # keys per key block: the unit of the split plan
TILE_M = 128         # packed query rows per workgroup
MAX_SPLITS = _native.SPLITKV_MAX_SPLITS
TWO_TERM_KEYS = 1024   # precision="fast": a workgroup that sweeps at least this many keys runs the one-term sweep (csrc kTwoTermKeys)
_CPU_NUM_CUS = 256     # the auto rule on CPU tensors (the eager definition): an MI355X's CU count


def _cdiv(a, b):
    return (a + b - 1) // b


class PreparedKV:
    """K and V in the attention kernels' own format, made once by `prepare_kv_fp8` and attended many times.
      k, v             device tensors: the KFRAG image of k and the VFRAG image of v (flat uint8; the layouts are private to the library);
                       CPU tensors (and config.attention.force_eager_fallback): row-major fp8 [B, Hkv, Skv, D] for the eager definition
      scale_k, scale_v fp32 [B, Hkv], head-wise over the WHOLE tensors
      shape            (B, Hkv, Skv, D);   fp8_format "e4m3" / "e5m2";   dtype: the 16-bit source dtype (the output dtype of a call);
      numerics         the quantiser's numerics ("compiled" / "eager");   layout "frag" / "rowmajor"
    Treat what `prepare_kv_fp8` returns as immutable: its scales cover exactly these keys, so nothing can be appended to it.  The appendable
    kind is the subclass kvcache.KVCacheFP8 -- fixed scales, a capacity and device-side lengths (alloc_kv_cache_fp8,
    kv_cache_from_prefill_fp8, kv_cache_append_fp8); a paged cache is paged.PagedKVCacheFP8 (not a PreparedKV: fp8_attn_paged_func)."""

    __slots__ = ("k", "v", "scale_k", "scale_v", "shape", "fp8_format", "dtype", "numerics", "layout")

    def __init__(self, k, v, scale_k, scale_v, shape, fp8_format, dtype, numerics, layout):
        self.k, self.v, self.scale_k, self.scale_v = k, v, scale_k, scale_v
        self.shape, self.fp8_format, self.dtype, self.numerics, self.layout = tuple(shape), fp8_format, dtype, numerics, layout

    @property
    def device(self):
        return self.k.device

    def nbytes(self) -> int:
        """bytes of the two images: what a call streams at the least"""
        return self.k.numel() * self.k.element_size() + self.v.numel() * self.v.element_size()

    def __repr__(self):
        return (f"PreparedKV(shape={self.shape}, fp8_format={self.fp8_format!r}, dtype={self.dtype}, numerics={self.numerics!r}, "
                f"layout={self.layout!r}, device={self.device})")


def _kv_reason(k, v) -> Optional[str]:
    if not isinstance(k, Tensor) or not isinstance(v, Tensor) or k.dim() != 4 or v.dim() != 4:
        return "NYI: key and value must be 4-D tensors [B, Hkv, Skv, head_dim]"
    if k.requires_grad or v.requires_grad:
        return "NYI: key and value must be leaf tensors (no backward)"
    if k.dtype not in (torch.float16, torch.bfloat16):
        return f"Expected key to have dtype torch.float16 or torch.bfloat16, but got key.dtype: {k.dtype} instead."
    if v.dtype != k.dtype:
        return f"Expected key and value to share a dtype, but got {k.dtype} and {v.dtype} instead."
    if k.shape != v.shape:
        return f"Expect key and value to have the same shape but got {tuple(k.shape)} and {tuple(v.shape)}."
    if k.shape[-1] not in nn._HIP_SUPPORTED_HEAD_DIMS:
        return f"Unsupported head dimension: {k.shape[-1]}"
    if 0 in k.shape:
        return "Expected a non-empty batch, head count and key sequence"
    if k.device != v.device:
        return f"Expected key and value to be on the same device, but got {k.device} and {v.device} instead."
    return None


def prepare_kv_fp8(k: Tensor, v: Tensor, *, fp8_format: Optional[str] = None, numerics: Optional[str] = None) -> PreparedKV:
    """Quantise k and v [B, Hkv, Skv, D] (bf16 / fp16) once, into the format `fp8_attn_splitkv_func` attends: the KFRAG image of k and the
    VFRAG image of v with head-wise scales scale_k, scale_v fp32 [B, Hkv] -- exactly what two
    `_native.quant_fp8(..., scaling="head-wise", layout=KFRAG / VFRAG)` calls leave, i.e. bit for bit what
    `fp8_block_sparse_attn_pv_func(pv_precision="fp8")` attends.  fp8_format / numerics default to config.attention.fp8_format /
    quant_numerics.  V MUST BE FINITE EVERYWHERE (one scale per head over the whole tensor).
    config.attention.smooth_k is NOT followed: prepared keys are never smoothed (the mean would have to travel with every later query).
    CPU tensors (and config.attention.force_eager_fallback) keep row-major fp8 tensors from the eager quantiser, for the eager definition."""
    reason = _kv_reason(k, v)
    if reason:
        raise ValueError(reason)
    fp8_format = checks.config_value("attention.fp8_format") if fp8_format is None else fp8_format
    numerics = checks.config_value("attention.quant_numerics") if numerics is None else numerics
    fp8_dtype = _native.fp8_dtype_of(fp8_format)
    if numerics not in _native.NUMERICS:
        raise ValueError(f"Unsupported quant_numerics: {numerics!r} (expected one of {sorted(_native.NUMERICS)})")
    if not k.is_cuda or checks.config_value("attention.force_eager_fallback"):
        k8, sk = nn._dynamically_quantize_fp8(k, reduction_dim=[2, 3], fp8_dtype=fp8_dtype)
        v8, sv = nn._dynamically_quantize_fp8(v, reduction_dim=[2, 3], fp8_dtype=fp8_dtype)
        return PreparedKV(k8, v8, sk, sv, k.shape, fp8_format, k.dtype, numerics, "rowmajor")
    ok, why = nn._pre_check_can_use_hip_attention(device=k.device)
    if not ok:
        raise ValueError(why)
    kf, sk = _native.quant_fp8(k, scaling="head-wise", fp8_dtype=fp8_dtype, layout=_native.LAYOUT_KFRAG, numerics=numerics)
    vf, sv = _native.quant_fp8(v, scaling="head-wise", fp8_dtype=fp8_dtype, layout=_native.LAYOUT_VFRAG, numerics=numerics)
    return PreparedKV(kf, vf, sk, sv, k.shape, fp8_format, k.dtype, numerics, "frag")


def splitkv_input_reason(q, kv, seqused_k=None, scale=None, num_splits=0) -> Optional[str]:
    """The first rule the arguments break, or None.  Shapes, dtypes and devices only: seqused_k's CONTENTS are read on the device."""
    if not isinstance(q, Tensor) or q.dim() != 4:
        return "NYI: query must be a 4-D tensor [B, Hq, Sq, head_dim]"
    if q.requires_grad:
        return "NYI: query must be a leaf tensor (no backward)"
    if q.dtype not in (torch.float16, torch.bfloat16):
        return f"Expected query to have dtype torch.float16 or torch.bfloat16, but got query.dtype: {q.dtype} instead."
    if not isinstance(kv, PreparedKV):
        return "Expected kv to be a PreparedKV (prepare_kv_fp8) or a (key, value) pair"
    B, Hkv, Skv, D = kv.shape
    if kv.dtype != q.dtype:
        return f"Expected query to have the dtype the keys and values were prepared from, but got {q.dtype} and {kv.dtype} instead."
    if q.shape[-1] != D:
        return f"Expect query, key and value to have the same head dimension but got {q.shape[-1]} and {D}."
    if q.shape[-1] not in nn._HIP_SUPPORTED_HEAD_DIMS:
        return f"Unsupported head dimension: {q.shape[-1]}"
    if q.shape[0] != B:
        return f"Expect query and key/value to have the same batch size but got {q.shape[0]} and {B}."
    if q.shape[1] % Hkv != 0:
        return f"Expect the number of query heads to be a multiple of the key/value heads but got Hq={q.shape[1]} and Hkv={Hkv}."
    if q.shape[0] == 0 or q.shape[1] == 0 or q.shape[2] == 0:
        return "Expected a non-empty batch, head count and query sequence"
    if q.device != kv.device:
        return f"Expected query and the prepared key/value to be on the same device, but got {q.device} and {kv.device} instead."
    if kv.fp8_format not in _native.FP8_DTYPE:
        return f"Unsupported fp8_format of the prepared key/value: {kv.fp8_format!r}"
    if kv.k.dtype != (torch.uint8 if kv.layout == "frag" else _native.FP8_DTYPE[kv.fp8_format]):
        return f"The prepared key/value holds {kv.k.dtype} data, which is not its format {kv.fp8_format!r} in layout {kv.layout!r}"
    if seqused_k is not None:
        if not isinstance(seqused_k, Tensor) or seqused_k.dtype != torch.int32:
            return f"Expected seqused_k to be a torch.int32 tensor, but got {getattr(seqused_k, 'dtype', type(seqused_k))}"
        if tuple(seqused_k.shape) != (B,):
            return f"Expected seqused_k to have shape [{B}], but got {list(seqused_k.shape)}."
        if seqused_k.device != q.device:
            return f"Expected seqused_k to be on {q.device}, but got {seqused_k.device} instead."
    if isinstance(num_splits, bool) or not isinstance(num_splits, int) or not 0 <= num_splits <= MAX_SPLITS:
        return f"num_splits must be 0 (choose) or an integer in 1 .. {MAX_SPLITS}, got {num_splits!r}"
    if scale is not None and not (isinstance(scale, (int, float)) and not isinstance(scale, bool) and math.isfinite(scale) and scale > 0):
        return f"scale must be a finite number > 0 (or None for 1/sqrt(head_dim)), got {scale!r}"
    return None


@torch.compiler.assume_constant_result
def _resolve_splits(num_splits: int, B: int, Hq: int, Hkv: int, Sq: int, Skv: int, D: int, device) -> int:
    """num_splits = 0 -> qattn_splitkv_auto_splits on the device's CU count: a pure function of the shape (it never reads seqused_k), so
    a trace-time constant."""
    if num_splits:
        return num_splits
    cus = torch.cuda.get_device_properties(device).multi_processor_count if torch.device(device).type == "cuda" else _CPU_NUM_CUS
    return _native.splitkv_auto_splits(B, Hq, Hkv, Sq, Skv, D, cus)


def split_plan(L: int, num_splits: int):
    """Key ranges [lo, hi) of the splits of a batch element with L used keys: nkb = ceil(L / 128) key blocks, per = ceil(nkb / ns) per
    split; a split past the last block is empty (lo = hi)."""
    nkb = _cdiv(L, BLOCK_N)
    per = _cdiv(nkb, num_splits)
    return [(min(BLOCK_N * s * per, L), min(BLOCK_N * (s + 1) * per, L)) for s in range(num_splits)]


def window_interval_lo(L: int, Sq: int, window_left: int) -> int:
    """lo_i of include/qattn_splitkv_window.h: the first key any of Sq queries over L keys attends under window_left (-1: 0)."""
    return 0 if window_left < 0 else min(max(L - Sq - window_left, 0), L)


def split_plan_window(L: int, Sq: int, window_left: int, num_splits: int):
    """`split_plan` under a sliding window: the splits cut the key blocks of the interval [lo, L), lo = window_interval_lo(L, Sq,
    window_left), not those of [0, L): kb0 = lo // 128, nkb = ceil(L / 128) - kb0, per = ceil(nkb / ns); split s owns
    [128 (kb0 + s per), 128 (kb0 + (s + 1) per)) cut at L.  window_left = -1: `split_plan`."""
    kb0 = window_interval_lo(L, Sq, window_left) // BLOCK_N
    nkb = _cdiv(L, BLOCK_N) - kb0
    per = _cdiv(nkb, num_splits)
    return [(min(BLOCK_N * (kb0 + s * per), L), min(BLOCK_N * (kb0 + (s + 1) * per), L)) for s in range(num_splits)]


def _splitkv_eager(q, kv, causal, scale, seqused_k, ns, precision, keep_also=None, softcap=None, sinks=None, window=None):
    """CPU tensors and config.attention.force_eager_fallback: the torch definition.  The eager quantiser on q (head-wise), the prepared
    row-major bytes de-quantised; per split an fp32 softmax partial (o_s, lse_s) over the split's keys of every batch element's first L_b
    keys -- a row without a key there: a zero row, LSE -inf --, then merge.merge_attn_states_eager.  The path bytes restate the kernel's
    rule per (kv head, 128-row tile of packed rows, split).  Returns (out, lse, partial_o, partial_lse, partial_path); with one split the
    partials are empty.  (This path reads seqused_k on the host.)
    window = (left, right): the definition of the window entries (include/qattn_splitkv_window.h) -- `causal` is not read; the splits are
    split_plan_window's, position p keeps the keys p + delta - left .. p + delta + right, and the path byte counts the keys klo .. khi.
    sinks = fp32 [Hq] (None: none): the definition of the sink entries (include/qattn_sinks.h) -- one split: the row's LSE becomes
    L = logaddexp(lse, sink_h) and the weights exp(score - L), an empty row a zero row with LSE = sink_h; more splits: the partials stay
    free of the sink and it enters merge.merge_attn_states_eager once.  +inf and NaN make the head's rows NaN.
    softcap = a float > 0 (None: none): the definition of the soft-cap entries (include/qattn_softcap.h) -- every scaled score x becomes
    softcap tanh(x / softcap) BEFORE the mask, so a masked key weighs 0; the LSE and the partials are those of the capped scores.
    keep_also = bool [B, Sq, Skv] (None: none): one more condition on (position, key), on top of the rule above -- the draft tree of
    tree.fp8_attn_paged_varlen_tree_func; the splits and the path bytes do not see it."""
    return _splitkv_eager_depth(q, kv, causal, scale, seqused_k, ns, precision, keep_also, sinks, window, None, softcap=softcap)


def _splitkv_eager_depth(q, kv, causal, scale, seqused_k, ns, precision, keep_also, sinks, window, depth, softcap=None):
    """`_splitkv_eager`, whose definition this is, with one more input for the tree under a window
    (include/qattn_paged_varlen_tree_window.h).  depth = a list per batch element of None or an int64 [Sq] tensor (None: none anywhere),
    with window: an element with depths is a slot of draft tokens -- position p sits at sequence position L - Sq + depth[p], the window's
    lower edge is taken from there and cuts COMMITTED keys (j < L - Sq) only, and the path byte's klo takes the least depth of the
    tile's rows where the window rule takes their least position."""
    fp8_dtype = _native.fp8_dtype_of(kv.fp8_format)
    B, Hq, Sq, D = q.shape
    _, Hkv, Skv, _ = kv.shape
    G = Hq // Hkv
    sm = 1.0 / math.sqrt(D) if scale is None else float(scale)
    q8, sq = nn._dynamically_quantize_fp8(q, reduction_dim=[2, 3], fp8_dtype=fp8_dtype)
    dq = q8.float() * sq[..., None, None]
    dk = nn._expand_kv_heads(kv.k.float() * kv.scale_k[..., None, None], Hq)
    dv = nn._expand_kv_heads(kv.v.float() * kv.scale_v[..., None, None], Hq)
    s_all = (dq @ dk.transpose(-1, -2)) * sm                                    # [B, Hq, Sq, Skv]
    if softcap is not None:   # the cap on the scaled scores, before any mask
        s_all = float(softcap) * torch.tanh(s_all / float(softcap))
    used = [Skv] * B if seqused_k is None else [min(max(int(x), 0), Skv) for x in seqused_k.tolist()]
    pos = torch.arange(Sq, device=q.device)[:, None]
    key = torch.arange(Skv, device=q.device)[None, :]
    outs, lses = [], []
    path = torch.zeros((ns, B, Hq, Sq), dtype=torch.uint8, device=q.device)
    ntile = _cdiv(G * Sq, TILE_M)
    for s in range(ns):
        keep = torch.zeros((B, 1, Sq, Skv), dtype=torch.bool, device=q.device)
        for b, L in enumerate(used):
            lo, hi = split_plan(L, ns)[s] if window is None else split_plan_window(L, Sq, window[0], ns)[s]
            m = (key >= lo) & (key < hi)
            dep = None if depth is None else depth[b]
            if window is not None:
                if window[0] >= 0 and dep is not None:
                    m = m & ((key >= dep[:, None] + (L - Sq - window[0])) | (key >= L - Sq))
                elif window[0] >= 0:
                    m = m & (key >= pos + (L - Sq - window[0]))
                if window[1] >= 0:
                    m = m & (key <= pos + (L - Sq + window[1]))
            elif causal:
                m = m & (key <= pos + (L - Sq))
            if keep_also is not None:
                m = m & keep_also[b]
            keep[b, 0] = m.expand(Sq, Skv)
            # the kernel's path byte: per tile of the kv head's packed rows, by the keys the workgroup sweeps
            for t in range(ntile):
                r0, r1 = t * TILE_M, min((t + 1) * TILE_M, G * Sq) - 1
                smax = Sq - 1 if r0 // Sq != r1 // Sq else r1 % Sq
                if window is not None:
                    smin = 0 if r0 // Sq != r1 // Sq else r0 % Sq
                    if dep is not None:   # the least depth of the tile's rows
                        smin = int(dep[torch.arange(r0, r1 + 1, device=dep.device) % Sq].min())
                    klo = max(lo, 0 if window[0] < 0 else max(smin + L - Sq - window[0], 0))
                    khi = min(hi - 1, L - 1 if window[1] < 0 else smax + L - Sq + window[1])
                    keys = max(khi - klo + 1, 0)
                else:
                    khi = min(hi - 1, smax + L - Sq) if causal else hi - 1
                    keys = max(khi - lo + 1, 0)
                code = _native.PATH_ONE_TERM if (keys == 0 or (precision == "fast" and keys >= TWO_TERM_KEYS)) else _native.PATH_TWO_TERM
                path[s, b].view(Hkv, G * Sq)[:, r0:r1 + 1] = code
        sc = s_all.masked_fill(~keep, -math.inf)
        lse = torch.logsumexp(sc, dim=-1)
        if sinks is not None and ns == 1:
            lse = torch.logaddexp(lse, merge.sink_or_nan(sinks)[None, :, None])
        p = torch.exp(sc - lse.clamp_min(torch.finfo(torch.float32).min)[..., None])   # (a row without keys: exp(-inf) = 0)
        # a key no row of the split attends enters with V = 0, not with its bytes: 0 * NaN would make the row NaN, and bytes behind
        # seqused_k or below a window influence no output bit (the kernels never load them)
        outs.append(p @ dv.masked_fill(~keep.any(2)[..., None], 0))
        lses.append(lse)
    if ns == 1:
        e = lambda dt: torch.empty((0,), dtype=dt, device=q.device)
        return outs[0].to(q.dtype), lses[0], e(torch.float32), e(torch.float32), e(torch.uint8)
    out, lse = merge.merge_attn_states_eager(outs, lses, q.dtype, sinks=sinks)
    return out, lse, torch.stack(outs), torch.stack(lses), path


def fp8_attn_splitkv_func(q, kv, *, causal: bool = False, scale: Optional[float] = None, seqused_k: Optional[Tensor] = None,
                          num_splits: int = 0, precision: str = "accurate", return_lse: bool = False, return_partials: bool = False):
    """FP8 attention of a short query over long prepared keys / values, the key axis of each head cut across `num_splits` workgroups.

    q [B, Hq, Sq, D] bf16 / fp16, Hq a multiple of Hkv, D in {64, 128, 256}; it is made contiguous (it is short).
    kv: a `PreparedKV` (prepare_kv_fp8), or a (k, v) pair [B, Hkv, Skv, D] that is prepared inside the call under config.attention.fp8_format /
    quant_numerics -- the same bits either way.  The fp8 format and the quantiser numerics of a call are the PreparedKV's.
    seqused_k: int32 [B] on q's device; batch element b uses its first L_b = clamp(seqused_k[b], 0, Skv) keys.  Keys beyond that influence
    no output bit -- but they DID count toward the prepared scales, which cover the whole tensors.  Read on the device: no host
    synchronisation, graph-capture safe, and a captured call follows the table's later contents.
    causal: bottom-right, as flash-attn's kv-cache entry and window_size=(-1, 0) here: query s attends keys j <= s + L_b - Sq.
    A row without a key is a zero row with an LSE of -inf.
    num_splits: 1 .. 64, or 0 to choose: a pure function of the shape and the device's CU count (include/qattn_splitkv.h), never of
    seqused_k's contents -- 1 when the unsplit grid already fills the chip.
    precision: "accurate" (exact exponentials, two-term e4m3 P everywhere) or "fast" (a workgroup whose split holds >= 1024 keys, cut at
    L_b and the causal edge, runs the one-term sweep; byte exponentials only with num_splits = 1 and no LSE); "auto" raises ValueError.
    Returns out [B, Hq, Sq, D] in q's dtype; with return_lse (out, lse fp32 [B, Hq, Sq], natural log-sum-exp); with return_partials the
    tuple also ends with the fp32 partial outputs [ns, B, Hq, Sq, D], their LSEs [ns, B, Hq, Sq] and their path bytes uint8 [ns, B, Hq, Sq] (three empty tensors when
    the call ran one split): out, lse = merge_attn_states(list(partial_o), list(partial_lse), out_dtype=q.dtype), bit for bit.
    config.attention.smooth_k is not followed.  CPU tensors and config.attention.force_eager_fallback run the eager definition
    (`_splitkv_eager`); on the device there is no fallback.  Unsupported input raises ValueError(reason)."""
    if precision not in ("accurate", "fast"):
        raise ValueError(f"Unsupported precision: {precision!r} (expected 'accurate' or 'fast'; 'auto' is not offered by the split-KV entry)")
    if isinstance(kv, (tuple, list)):
        if len(kv) != 2:
            raise ValueError("Expected kv to be a PreparedKV (prepare_kv_fp8) or a (key, value) pair")
        if isinstance(q, Tensor) and isinstance(kv[0], Tensor) and kv[0].device != q.device:
            raise ValueError(f"Expected query, key, and value to be on the same device, but got {q.device} and {kv[0].device} instead.")
        kv = prepare_kv_fp8(kv[0], kv[1])
    if not checks.config_value("attention.skip_supported_check"):
        reason = splitkv_input_reason(q, kv, seqused_k, scale, num_splits)
        if reason:
            raise ValueError(reason)
    B, Hq, Sq, D = q.shape
    _, Hkv, Skv, _ = kv.shape
    ns = _resolve_splits(num_splits, B, Hq, Hkv, Sq, Skv, D, q.device)
    eager = (not q.is_cuda or checks.config_value("attention.force_eager_fallback")) and not torch.compiler.is_dynamo_compiling()
    if eager:
        if kv.layout != "rowmajor":
            raise ValueError("the eager definition needs a PreparedKV made on CPU tensors or under config.attention.force_eager_fallback")
        out, lse, po, plse, ppath = _splitkv_eager(q, kv, causal, scale, seqused_k, ns, precision)
    else:
        if kv.layout != "frag":
            raise ValueError("this PreparedKV holds row-major bytes for the eager definition; prepare it on the device without "
                             "config.attention.force_eager_fallback")
        ok, why = nn._pre_check_can_use_hip_attention(device=q.device)
        if not ok:
            raise ValueError(why)
        out, lse, po, plse, ppath = nn._ops().fp8_splitkv_attention_forward(
            q.contiguous(), kv.k, kv.v, kv.scale_k, kv.scale_v, seqused_k, Skv, ns, kv.fp8_format, kv.numerics, bool(causal), precision,
            bool(return_lse), bool(return_partials), scale=scale)
    res: Tuple = (out,)
    if return_lse:
        res += (lse,)
    if return_partials:
        res += (po, plse, ppath)
    return res if len(res) > 1 else out

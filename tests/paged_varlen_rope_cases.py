"""Shared by the tests of the rotary embedding at the paged cache's positions (include/qattn_paged_varlen_rope.h): the tables, the
host-computed positions and THE RULE's composition, on any device."""
import torch

import quantumattention_amd as qa
from quantumattention_amd.rope import apply_rope_eager

HKV = 2
CAP = 256
T = 256
COUNTS = [0, 1, 63, 64, 65, 130, 2, 7]
STARTS = [0, 1, 63, 64, 100, 127, CAP - 3, 5]     # an idle slot, a chunk-aligned start, straddled chunks and pages, a dropped tail (slot 5)
B = len(COUNTS)
SENTINEL = 0x5A


def tables(D, rows=T, device="cpu", base=10000.0):
    """angle[p, i] = p * base^(-i / (D/2)); cos / sin in fp32 [rows, D/2]"""
    h = D // 2
    inv = base ** (-torch.arange(h, dtype=torch.float64) / h)
    ang = torch.arange(rows, dtype=torch.float64)[:, None] * inv[None]
    return ang.cos().to(torch.float32).to(device), ang.sin().to(torch.float32).to(device)


def cu_list(counts):
    cu = [0]
    for n in counts:
        cu.append(cu[-1] + n)
    return cu


def positions(counts, seqlens, total, rows=T, cap=CAP, appended=False, shift=0):
    """pos[start_i + t] = min(max(p_i - (n_i if appended), 0) + t, rows - 1), from host lists; rows no slot owns: 0"""
    pos = [0] * total
    cu = cu_list(counts)
    for i, n in enumerate(counts):
        base = max(min(max(seqlens[i], 0), cap) - (n if appended else 0), 0)
        for t in range(n):
            pos[cu[i] + t] = min(base + t + shift, rows - 1)
    return pos


def rotate_at(x, pos, cos, sin, interleaved):
    """apply_rope_eager on packed x [total, H, D], row j with table row pos[j] -> [total, H, D]"""
    at = torch.tensor(pos, dtype=torch.long, device=cos.device)
    return apply_rope_eager(x.transpose(0, 1)[None], cos[at], sin[at], interleaved=interleaved)[0].transpose(0, 1)


def rule(cache, k_new, v_new, cu_seqlens, counts, seqlens, cos, sin, interleaved, advance, shift=0):
    """THE RULE: rotate K in torch at host positions, then the plain packed append"""
    pos = positions(counts, seqlens, k_new.shape[0], rows=cos.shape[0], cap=cache.capacity, shift=shift)
    k_rot = rotate_at(k_new, pos, cos, sin, interleaved)
    return qa.paged_kv_cache_append_varlen_fp8(cache, k_rot, v_new, cu_seqlens, advance=advance)

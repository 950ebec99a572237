"""What tests/test_cpu_kvcache.py and the GPU tests of the appendable FP8 K/V cache share, restated here and NOT imported from the product
(include/qattn_kvcache.h is the contract): the byte maps of the KFRAG / VFRAG images (csrc/qattn_common.h, written out literally), the
quantiser's formula in torch, and two store schemes for a partly covered VFRAG chunk -- the header's and the mutant it excludes."""
import numpy as np
import torch

KFRAG, VFRAG = 1, 2          # include/qattn.h QATTN_LAYOUT_KFRAG / _VFRAG (literal)
FP8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def kfrag_offset(key, d, D):
    """byte offset of K[key][d] in its 64-key chunk: [t:2][s:D/64][hh:2][half:2][key:32][16 B]"""
    t, kl, s, hh, half = key >> 5, key & 31, d >> 6, (d >> 5) & 1, (d >> 4) & 1
    return ((t * (D // 64) + s) << 11) + (hh << 10) + (half << 9) + (kl << 4) + (d & 15)


def vfrag_offset(key, d, D):
    """byte offset of V[key][d] in its 64-key chunk: [m:D/32][hh:2][half:2][d:32][4 w + i], key = 32 half + 8 w + 4 hh + i"""
    half, w, hh, i = key >> 5, (key >> 3) & 3, (key >> 2) & 1, key & 3
    return ((d >> 5) << 11) + (hh << 10) + (half << 9) + ((d & 31) << 4) + (w << 2) + i


def chunk_map(layout, D):
    """[64, D] int64: the offset of every (key, d) of a chunk"""
    key, d = np.arange(64)[:, None], np.arange(D)[None, :]
    return (kfrag_offset if layout == KFRAG else vfrag_offset)(key, d, D).astype(np.int64)


def image_map(layout, S, D):
    """[Sp, D] int64: the offset of every (key, d) in one head's image, Sp = S padded to 64 keys"""
    Sp = (S + 63) // 64 * 64
    cm = chunk_map(layout, D)
    return (np.arange(Sp // 64)[:, None, None] * 64 * D + cm[None]).reshape(Sp, D)


def to_image(rows, layout):
    """row-major uint8 [..., S, D] (numpy) -> the flat image, keys S .. Sp-1 zero"""
    rows = np.asarray(rows, np.uint8)
    S, D = rows.shape[-2:]
    m = image_map(layout, S, D)
    img = np.zeros(rows.shape[:-2] + (m.shape[0] * D,), np.uint8)
    img[..., m[:S].reshape(-1)] = rows.reshape(rows.shape[:-2] + (S * D,))
    return img.reshape(-1)


def from_image(img, layout, B, H, S, D):
    """the flat image (torch uint8, any device) -> row-major uint8 [B, H, Sp, D]"""
    m = torch.from_numpy(image_map(layout, S, D).reshape(-1)).to(img.device)
    Sp = (S + 63) // 64 * 64
    return img.view(B, H, Sp * D)[:, :, m].view(B, H, Sp, D)


def quant_ref(x, scale, fp8_dtype):
    """fp8_rne(clamp(round_to_dtype(fp32(x) / scale), +-qmax)) as uint8; x [B, H, T, D] 16-bit, scale fp32 [B, H]"""
    qmax = torch.finfo(fp8_dtype).max
    return (x.float() / scale[:, :, None, None]).to(x.dtype).clamp(-qmax, qmax).to(fp8_dtype).view(torch.uint8)


def store_vfrag_chunk(chunk, staged, lo, hi, D, mutant=False):
    """Store the keys [lo, hi) of `staged` (uint8 [64, D], zero outside the range, as the kernel stages them) into the VFRAG chunk `chunk`
    (uint8 [64 D], modified in place) word by word.  The header's scheme: a 32-bit word where the aligned 4-key group lies wholly inside the
    range, single bytes otherwise.  mutant: a whole word for every group the range touches."""
    for kb in range(0, 64, 4):
        if kb + 4 <= lo or kb >= hi:
            continue
        inside = kb >= lo and kb + 4 <= hi
        for d in range(D):
            o = vfrag_offset(kb, d, D)
            assert o % 4 == 0 and [vfrag_offset(kb + i, d, D) for i in range(4)] == [o, o + 1, o + 2, o + 3]
            if inside or mutant:
                chunk[o:o + 4] = staged[kb:kb + 4, d]
            else:
                for i in range(4):
                    if lo <= kb + i < hi:
                        chunk[o + i] = staged[kb + i, d]

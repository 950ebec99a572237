"""Guarded arenas for buffer-contract tests (tests/test_gpu_buffer_contract.py; teeth on the CPU: tests/test_cpu_arena.py).

Every caller-provided buffer of a C entry is carved out of a byte buffer of its own: [front guard | interior | back guard].  The interior has
EXACTLY the size the header promises to be enough and starts at the minimum alignment the header documents and no more (address = align
mod 512), so what the caching allocator's 512-byte rounding and alignment would hide -- a store past the end, an access that needs more
alignment than documented -- lands in a guard or shows.  A guard is at least the larger of 64 KiB and one 256-row tile of the buffer's row
size: a full stray tile store stays inside it.

Roles:
  "out"      guards hold GUARD_BYTE; the interior is pre-filled with a poison chosen per dtype (POISON) before each call, so that an element
             nobody wrote is visible afterwards (`poison_left`).
  "scratch"  guards hold GUARD_BYTE; the interior is pre-filled with a byte the test chooses (0x00, then 0xFF): results must not depend on it.
  "in"       the guards -- and, through `load_view`, the pad elements of a strided view -- hold a HOSTILE pattern (NaN, 0x7f fp8 bytes,
             INT32_MIN / MAX, 0x01 mask bytes) in one run and a BENIGN one (zeros) in another: results must not depend on it either.
`assert_guards_intact` checks every guard of every buffer, inputs included.  Nothing here knows about the device: it runs on CPU tensors too.
"""
import torch

GUARD_MIN = 64 * 1024
TILE_ROWS = 256
GUARD_BYTE = 0xC3

# interior pre-fill of an output, as little-endian bytes of one element: "not written" stays visible
POISON = {
    "bf16": (0xC0, 0x7F),                # 0x7FC0: NaN
    "fp16": (0x00, 0x7E),                # 0x7E00: NaN
    "fp32": (0x00, 0x00, 0xC0, 0x7F),    # 0x7FC00000: NaN
    "fp8": (0x7F,),                      # NaN in e4m3fn and e5m2; the quantisers clamp to +-fmax and never produce it
    "path": (0xA5,),                     # no QATTN_PATH_* code
}
# guards (and view pads) of an input
HOSTILE = {
    "bf16": POISON["bf16"], "fp16": POISON["fp16"], "fp32": POISON["fp32"], "fp8": (0x7F,),
    "int32": (0x00, 0x00, 0x00, 0x80, 0xFF, 0xFF, 0xFF, 0x7F),   # INT32_MIN, INT32_MAX
    "mask": (0x01,),                     # a mask byte read out of range turns a tile ON
}
KIND_OF_DTYPE = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32", torch.float8_e4m3fn: "fp8", torch.float8_e5m2: "fp8",
                 torch.uint8: "fp8", torch.int32: "int32", torch.bool: "mask"}


def _tiled(pattern, nbytes, device):
    p = torch.tensor(list(pattern), dtype=torch.uint8, device=device)
    return p.repeat(-(-nbytes // len(pattern)))[:nbytes]


class Region:
    """One carved buffer.  `interior`: uint8 view of exactly `nbytes` bytes; `ptr`: its address (what the C entry gets)."""

    def __init__(self, name, nbytes, device, align, row_bytes, role, kind):
        assert role in ("in", "out", "scratch") and align in (1, 2, 4, 8, 16, 32, 64, 128, 256) and nbytes >= 0
        assert role != "out" or kind in POISON, (name, kind)
        assert role != "in" or kind in HOSTILE, (name, kind)
        self.name, self.nbytes, self.align, self.role, self.kind = name, int(nbytes), align, role, kind
        guard = max(GUARD_MIN, TILE_ROWS * int(row_bytes))
        self.buf = torch.empty(2 * guard + self.nbytes + 1024, dtype=torch.uint8, device=device)
        self.off = guard + (align - self.buf.data_ptr() - guard) % 512   # the documented alignment and NOT more: address = align mod 512
        self.guard_pattern = (GUARD_BYTE,)
        self.set_guards(hostile=True)
        if role == "out":
            self.fill_poison()

    # ---- what the call gets
    @property
    def interior(self):
        return self.buf[self.off:self.off + self.nbytes]

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def view(self, dtype, shape=None):
        t = self.interior.view(dtype)
        return t if shape is None else t.view(shape)

    # ---- fills
    def set_guards(self, hostile=True):
        """(Re)write both guards; the interior is left alone.  Inputs: the hostile or the benign pattern; others: GUARD_BYTE.
        The pattern's phase is that of the interior's elements (off is a multiple of the element size), so a whole element read from a
        guard is a whole NaN / INT32_MIN."""
        if self.role == "in":
            self.guard_pattern = HOSTILE[self.kind] if hostile else (0x00,) * len(HOSTILE[self.kind])
        end = self.off + self.nbytes
        self._front = self._pattern_at(-self.off, self.off)
        self._back = self._pattern_at(self.nbytes, self.buf.numel() - end)
        self.buf[:self.off] = self._front
        self.buf[end:] = self._back

    def _pattern_at(self, rel, n):
        """n bytes of the guard pattern as they sit at offset `rel` from the interior's start (pattern byte 0 at offset 0)."""
        k = len(self.guard_pattern)
        return _tiled(self.guard_pattern, n + k, self.buf.device)[rel % k:rel % k + n]

    def fill(self, byte):
        self.interior.fill_(byte)

    def fill_poison(self):
        self.interior.copy_(_tiled(POISON[self.kind], self.nbytes, self.buf.device))

    def load(self, t):
        """Copy a dense tensor's bytes into the interior (sizes must agree exactly)."""
        src = t.contiguous().view(-1).view(torch.uint8) if t.dtype != torch.bool else t.contiguous().view(-1).to(torch.uint8)
        assert src.numel() == self.nbytes, (self.name, src.numel(), self.nbytes)
        self.interior.copy_(src)

    def load_view(self, t, strides, hostile=True):
        """Interior = a strided view (element `strides`, innermost 1) holding `t`; every pad element between its rows / heads gets the
        input's hostile or benign pattern.  Returns the view."""
        pattern = HOSTILE[self.kind] if hostile else (0x00,) * len(HOSTILE[self.kind])
        self.interior.copy_(_tiled(pattern, self.nbytes, self.buf.device))
        v = torch.as_strided(self.interior.view(t.dtype), tuple(t.shape), tuple(strides))
        v.copy_(t)
        return v

    # ---- checks
    def changed_guard_bytes(self):
        """(first, last) changed byte offsets relative to the interior's start (negative: front guard; >= nbytes: back guard), or None."""
        end = self.off + self.nbytes
        front = torch.nonzero(self.buf[:self.off] != self._front).view(-1) - self.off
        back = torch.nonzero(self.buf[end:] != self._back).view(-1) + self.nbytes
        idx = torch.cat([front, back])
        if idx.numel() == 0:
            return None
        return int(idx[0]), int(idx[-1])

    def poison_left(self, logical=None):
        """Number of elements of the interior (or of `logical`, a uint8 tensor cut from it, element-aligned) that still hold the poison."""
        assert self.role == "out"
        p = POISON[self.kind]
        b = (self.interior if logical is None else logical).contiguous().view(-1, len(p))
        return int((b == torch.tensor(list(p), dtype=torch.uint8, device=b.device)).all(dim=1).sum())


class Arena:
    """The buffers of one call."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.regions = {}

    def carve(self, name, nbytes, *, align, row_bytes=0, role="out", kind="fp8"):
        assert name not in self.regions, name
        r = Region(name, nbytes, self.device, align, row_bytes, role, kind)
        self.regions[name] = r
        return r

    def __getitem__(self, name):
        return self.regions[name]

    def set_input_guards(self, hostile):
        for r in self.regions.values():
            if r.role == "in":
                r.set_guards(hostile)


def carve(nbytes, *, device, align, row_bytes=0, role="out", kind="fp8", name="buffer"):
    """One guarded buffer outside an Arena."""
    return Region(name, nbytes, torch.device(device), align, row_bytes, role, kind)


def assert_guards_intact(arena):
    """Every guard of every buffer (an Arena, a Region or a list of Regions) holds its pattern; else the first and last changed byte
    offsets relative to the interior of each damaged buffer."""
    regions = arena.regions.values() if isinstance(arena, Arena) else [arena] if isinstance(arena, Region) else arena
    hits = []
    for r in regions:
        c = r.changed_guard_bytes()
        if c is not None:
            where = "before the interior" if c[1] < 0 else "past the interior's end" if c[0] >= r.nbytes else "on both sides"
            hits.append(f"{r.name} ({r.role}, {r.nbytes} bytes): guard bytes changed {where}, first at offset {c[0]}, last at {c[1]} "
                        f"(relative to the interior's start)")
    assert not hits, "; ".join(hits)

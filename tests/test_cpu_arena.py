"""Teeth of tests/arena.py, on the CPU: a fake "kernel" written in torch (out = 2 x, fp32, row-major [rows, 8]) with one planted fault at a
time.  Every fault the GPU buffer-contract tests are there to find must be caught, and the correct kernel must pass every check."""
import pytest
import torch

from tests import arena as A

ROWS, COLS = 37, 8
ROW_BYTES = COLS * 4


def _setup(hostile=True):
    ar = A.Arena("cpu")
    x = torch.arange(ROWS * COLS, dtype=torch.float32).view(ROWS, COLS) / 7 + 1
    rx = ar.carve("x", x.numel() * 4, align=16, row_bytes=ROW_BYTES, role="in", kind="fp32")
    rx.load(x)
    ar.carve("out", x.numel() * 4, align=16, row_bytes=ROW_BYTES, role="out", kind="fp32")
    ar.carve("ws", 100, align=16, role="scratch")
    ar.set_input_guards(hostile)
    return ar, x


def fake_kernel(ar, fault=None):
    """out = 2 x through the flat buffers, as a kernel sees them: indices relative to the interior may leave it."""
    rx, ro = ar["x"], ar["out"]
    xf = rx.buf[:rx.buf.numel() // 4 * 4].view(torch.float32)
    x0 = rx.off // 4                      # element index of the interior's start in the flat fp32 view
    n = ROWS * COLS
    res = 2 * xf[x0:x0 + n].clone()
    if fault == "read_guard":             # the last element is computed from the element one past the input's end
        res[-1] = 2 * xf[x0 + n]
    if fault == "skip_element":
        keep = torch.ones(n, dtype=torch.bool)
        keep[n // 2] = False
        ro.view(torch.float32)[keep] = res[keep]
    else:
        ro.view(torch.float32).copy_(res)
    o = ro.off
    if fault == "byte_past_end":
        ro.buf[o + ro.nbytes] = 0
    if fault == "byte_before_start":
        ro.buf[o - 1] = 0
    if fault == "tile_past_end":          # a ragged tail stored as a whole 256-row tile
        ro.buf[o + ro.nbytes:o + ro.nbytes + A.TILE_ROWS * ROW_BYTES] = 0
    if fault == "ws_overrun":
        w = ar["ws"]
        w.buf[w.off + w.nbytes + 3] = 1
    return ro.interior.clone()


def test_interior_sits_at_the_documented_alignment_and_no_more():
    for align in (1, 4, 16, 256):
        r = A.carve(1000, device="cpu", align=align, row_bytes=4096, role="out", kind="fp8")
        assert r.ptr % 512 == align % 512 and r.ptr % align == 0
        assert r.off >= max(A.GUARD_MIN, 256 * 4096) and r.buf.numel() - r.off - r.nbytes >= max(A.GUARD_MIN, 256 * 4096)
        assert r.interior.numel() == 1000 and r.interior.data_ptr() == r.ptr


def test_correct_kernel_passes_every_check():
    ar, x = _setup()
    got = fake_kernel(ar)
    A.assert_guards_intact(ar)
    assert ar["out"].poison_left() == 0
    assert torch.equal(got.view(torch.float32).view(ROWS, COLS), 2 * x)
    ar2, _ = _setup(hostile=False)
    assert torch.equal(fake_kernel(ar2), got), "hostile and benign guards must give the same bits"
    for byte in (0x00, 0xFF):
        ar["ws"].fill(byte)
        ar["out"].fill_poison()
        assert torch.equal(fake_kernel(ar), got)
        A.assert_guards_intact(ar)


@pytest.mark.parametrize("fault,first,last", [
    ("byte_past_end", ROWS * ROW_BYTES, ROWS * ROW_BYTES),
    ("byte_before_start", -1, -1),
    ("tile_past_end", ROWS * ROW_BYTES, ROWS * ROW_BYTES + A.TILE_ROWS * ROW_BYTES - 1),
])
def test_an_overrun_is_caught_and_located(fault, first, last):
    ar, _ = _setup()
    fake_kernel(ar, fault)
    with pytest.raises(AssertionError) as e:
        A.assert_guards_intact(ar)
    assert ar["out"].changed_guard_bytes() == (first, last)
    assert f"out (out, {ROWS * ROW_BYTES} bytes)" in str(e.value) and f"first at offset {first}, last at {last}" in str(e.value)
    assert ar["x"].changed_guard_bytes() is None and ar["ws"].changed_guard_bytes() is None


def test_a_full_tile_overrun_stays_inside_the_guard():
    r = A.carve(64, device="cpu", align=16, row_bytes=2 * 256 * 3, role="out", kind="bf16")   # a 256-row tile of 1536-byte rows > 64 KiB
    tile = A.TILE_ROWS * 2 * 256 * 3
    assert r.off >= tile and r.buf.numel() - (r.off + r.nbytes) >= tile


def test_an_overrun_of_the_workspace_is_caught():
    ar, _ = _setup()
    fake_kernel(ar, "ws_overrun")
    with pytest.raises(AssertionError, match="ws .scratch, 100 bytes.: guard bytes changed past the interior's end, first at offset 103"):
        A.assert_guards_intact(ar)


def test_an_element_left_unwritten_is_caught():
    ar, _ = _setup()
    fake_kernel(ar, "skip_element")
    A.assert_guards_intact(ar)
    assert ar["out"].poison_left() == 1
    half = ar["out"].interior[:ROWS * ROW_BYTES // 2 // 4 * 4]
    assert ar["out"].poison_left(half) == 0, "the logical part in front of the hole is clean"


def test_a_read_of_one_guard_element_makes_hostile_and_benign_runs_differ():
    ar_h, _ = _setup(hostile=True)
    ar_b, _ = _setup(hostile=False)
    good = fake_kernel(_setup()[0])
    got_h, got_b = fake_kernel(ar_h, "read_guard"), fake_kernel(ar_b, "read_guard")
    assert not torch.equal(got_h, got_b)
    assert not torch.equal(got_h, good) and not torch.equal(got_b, good)
    A.assert_guards_intact(ar_h)      # (a read damages nothing: only the comparison shows it)
    A.assert_guards_intact(ar_b)


@pytest.mark.parametrize("kind,dtype", [("bf16", torch.bfloat16), ("fp16", torch.float16), ("fp32", torch.float32)])
def test_poison_and_hostile_patterns_are_nan_and_int_extremes(kind, dtype):
    r = A.carve(64, device="cpu", align=16, role="out", kind=kind)
    assert torch.isnan(r.view(dtype)).all() and r.poison_left() == 64 // len(A.POISON[kind])
    g = A.carve(64, device="cpu", align=16, role="in", kind=kind)
    sz = len(A.HOSTILE[kind])
    assert torch.isnan(g.buf[g.off - 4 * sz:g.off].view(dtype)).all() and torch.isnan(g.buf[g.off + 64:g.off + 64 + 4 * sz].view(dtype)).all()
    g.set_guards(hostile=False)
    assert (g.buf[:g.off] == 0).all() and g.changed_guard_bytes() is None
    t = A.carve(16, device="cpu", align=4, role="in", kind="int32")
    assert sorted(t.buf[t.off - 8:t.off].view(torch.int32).tolist()) == [-2 ** 31, 2 ** 31 - 1]
    assert A.carve(8, device="cpu", align=1, role="in", kind="mask").buf[0] == 1
    assert (A.carve(8, device="cpu", align=1, role="out", kind="path").interior == 0xA5).all()


def test_pads_of_a_strided_view_carry_the_input_pattern():
    x = torch.randn(2, 3, 8).to(torch.bfloat16)
    strides = (3 * 16, 16, 1)          # rows of 8 elements, 16 apart
    r = A.carve(2 * 3 * 16 * 2, device="cpu", align=16, row_bytes=32, role="in", kind="bf16")
    v = r.load_view(x, strides, hostile=True)
    assert torch.equal(v, x) and v.data_ptr() == r.ptr
    whole = r.view(torch.bfloat16, (2, 3, 16))
    assert torch.isnan(whole[..., 8:]).all()
    r.load_view(x, strides, hostile=False)
    assert (whole[..., 8:] == 0).all() and torch.equal(whole[..., :8], x)

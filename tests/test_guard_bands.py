"""CPU self-test of tests/guard_bands.py: the helper must see a one-byte change at every edge of
its bands, compare bytes (not floats), and give the payload the alignment it promises."""
import re

import pytest
import torch

import guard_bands as gb


def _message(g):
    with pytest.raises(gb.GuardError) as e:
        gb.check(g)
    return str(e.value)


def test_layout_and_patterns():
    g = gb.guarded((5, 3), torch.float32, "cpu", name="y")
    assert g.t.shape == (5, 3) and g.t.dtype == torch.float32 and g.nbytes == 60
    assert g.t.data_ptr() == g.ptr
    lead, tail = g.buf[:g.start], g.buf[g.start + g.nbytes:]
    assert lead.numel() >= gb.BAND_MIN and tail.numel() >= gb.BAND_MIN
    assert bool((lead == 0xA5).all()) and bool((tail == 0xA5).all())
    assert bool((g.payload_bytes() == 0x5A).all())
    gb.check(g)
    assert gb.untouched(g)


def test_band_size_follows_the_payload_up_to_the_cap():
    g = gb.guarded(100000, torch.uint8, "cpu")
    assert g.start >= 100000 and g.buf.numel() - g.start - g.nbytes >= 100000
    g = gb.guarded((5 << 20,), torch.uint8, "cpu")
    assert gb.BAND_MAX <= g.start < gb.BAND_MAX + 256 + 1
    assert gb.BAND_MAX <= g.buf.numel() - g.start - g.nbytes <= gb.BAND_MAX + 256


def test_one_byte_at_the_last_byte_of_the_lead_band():
    g = gb.guarded(7, torch.float32, "cpu", offset=4, name="out")
    g.buf[g.start - 1] = 0
    msg = _message(g)
    assert "out: lead band changed, 1..1 bytes before the payload (elements -1..-1)" in msg


def test_one_byte_at_the_first_byte_after_the_payload():
    g = gb.guarded(7, torch.float32, "cpu", offset=4, name="out")
    g.buf[g.start + g.nbytes] = 0
    msg = _message(g)
    assert "out: tail band changed, bytes 0..0 past the payload's end (elements 0..0 past its last" in msg
    assert "lead" not in msg


def test_one_byte_at_the_last_byte_of_the_tail_band():
    g = gb.guarded(7, torch.float64, "cpu", offset=8, name="S")
    n = g.buf.numel() - (g.start + g.nbytes)
    g.buf[-1] = 0xA4
    msg = _message(g)
    assert f"S: tail band changed, bytes {n - 1}..{n - 1} past the payload's end (elements {(n - 1) // 8}.." in msg


def test_first_and_last_of_a_range_in_bytes_and_elements():
    g = gb.guarded(33, torch.float64, "cpu", offset=8, name="S")
    tail = g.buf[g.start + g.nbytes:]
    tail[:30 * 8].view(torch.float64)[:] = 1.5  # 30 doubles past the end, as a kernel would store them
    msg = _message(g)
    assert "bytes 0..239 past the payload's end (elements 0..29 past its last; the payload has 33)" in msg
    lead = g.buf[:g.start]
    lead[g.start - 16:g.start - 4] = 1
    m = re.search(r"lead band changed, (\d+)\.\.(\d+) bytes before the payload \(elements -(\d+)\.\.-(\d+)\)", _message(g))
    assert m and [int(x) for x in m.groups()] == [5, 16, 1, 2]


def test_nan_and_negative_zero_in_a_band_are_changes():
    for value in (float("nan"), -0.0):
        g = gb.guarded(4, torch.float32, "cpu", name="y")
        tail = g.buf[g.start + g.nbytes:]
        tail[8:12].view(torch.float32)[0] = value
        assert "tail band changed, bytes" in _message(g)
    # the band pattern read as floats is an ordinary number: only the byte comparison is used
    g = gb.guarded(4, torch.float32, "cpu")
    as_float = g.buf[g.start + g.nbytes:][:4].view(torch.float32)
    assert bool(torch.isfinite(as_float).all())


@pytest.mark.parametrize("offset", [0, 4, 16, 8, 2])
def test_offset_gives_the_promised_alignment(offset):
    dtype = {2: torch.float16, 8: torch.float64}.get(offset, torch.float32)
    g = gb.guarded(9, dtype, "cpu", offset=offset)
    assert g.t.data_ptr() % 256 == offset
    assert g.ptr % 256 == offset
    gb.check(g)


def test_align_argument():
    g = gb.guarded(3, torch.float32, "cpu", align=64, offset=16)
    assert g.t.data_ptr() % 64 == 16


def test_offset_must_fit_the_element():
    with pytest.raises(ValueError):
        gb.guarded(3, torch.float64, "cpu", offset=4)


def test_empty_payload():
    g = gb.guarded(0, torch.float32, "cpu", offset=4)
    assert g.nbytes == 0 and g.ptr % 256 == 4 and g.t.numel() == 0
    gb.check(g)
    assert gb.untouched(g)
    g.buf[g.start] = 1  # the first byte after an empty payload
    assert "bytes 0..0 past" in _message(g)


def test_untouched_written_and_zero():
    g = gb.guarded(8, torch.int32, "cpu")
    assert gb.untouched(g) and not bool(gb.written(g).any())
    g.t[2] = 7
    w = gb.written(g)
    assert not gb.untouched(g) and w.shape == (32,)
    assert bool(w[8:12].all()) and not bool(w[:8].any()) and not bool(w[12:].any())
    g.zero_()
    assert bool(gb.written(g).all()) and bool((g.t == 0).all())
    gb.check(g)


def test_check_reports_every_buffer():
    a = gb.guarded(4, torch.float32, "cpu", name="a")
    b = gb.guarded(4, torch.float32, "cpu", name="b")
    gb.check(a, b)
    a.buf[0] = 0
    b.buf[-1] = 0
    with pytest.raises(gb.GuardError) as e:
        gb.check(a, b)
    assert "a: lead band changed" in str(e.value) and "b: tail band changed" in str(e.value)

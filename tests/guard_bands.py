"""Guard bands: buffers that show where a call wrote, not only what.

guarded() lays one uint8 allocation out as  lead band | payload | tail band.  The bands hold the
byte 0xA5 and the payload the byte 0x5A, so three things can be told apart afterwards: a band
byte that changed (an overrun: check() raises and says where), a payload byte that still holds
0x5A (never written: untouched() / written()), and a payload byte that was written.

The wrappers of whisperx_amd._lib cannot show an overrun: their scratch buffers are at least
64 KiB, torch rounds an allocation up to 512 bytes, and the library pads every workspace region
to 256 bytes.  A payload here is exactly as large as the header states, and `offset` moves its
start off the allocator's alignment to the weakest one the header allows, so that its end does
not fall on a 256 / 512-byte boundary and a store one vector too wide lands in the tail band.

Each band is as large as the payload (at least 64 KiB, at most 4 MiB): a store with a wrong
stride still lands inside the test's own allocation.

Everything is compared as bytes, never as floats (a NaN or a -0.0 in a band is a change).
"""
import numpy as np
import torch

BAND, FRESH = 0xA5, 0x5A
BAND_MIN, BAND_MAX = 1 << 16, 4 << 20


class GuardError(AssertionError):
    pass


class Guarded:
    """One guarded buffer: `t` is the payload as a tensor of the asked dtype and shape, `ptr` its
    address (valid for an empty payload too), `nbytes` its size; `buf` the whole allocation,
    whose bytes [0, start) and [start + nbytes, len) are the bands."""

    def __init__(self, buf, start, nbytes, shape, dtype, name):
        self.buf, self.start, self.nbytes, self.name = buf, start, nbytes, name
        self.dtype = dtype
        self.itemsize = torch.empty(0, dtype=dtype).element_size()
        self.ptr = buf.data_ptr() + start
        self.t = buf[start:start + nbytes].view(dtype).reshape(shape)

    def payload_bytes(self):
        return self.buf[self.start:self.start + self.nbytes]

    def zero_(self):
        """Zero the payload (the bands keep their pattern)."""
        self.payload_bytes().zero_()
        return self


def guarded(shape, dtype, device, align=256, offset=0, name=None):
    """A payload of `shape` x `dtype` on `device` that starts `offset` bytes past an `align`-byte
    boundary, between two bands (see the module docstring).  `offset` must be a multiple of the
    element size (the payload is a tensor view)."""
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
    itemsize = torch.empty(0, dtype=dtype).element_size()
    if align < 1 or offset < 0 or offset % itemsize:
        raise ValueError(f"guarded: offset {offset} is no multiple of the {itemsize}-byte element")
    nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize
    band = min(max(BAND_MIN, nbytes), BAND_MAX)
    buf = torch.full((band + align + offset + nbytes + band,), BAND, dtype=torch.uint8, device=device)
    start = band + (-(buf.data_ptr() + band)) % align + offset
    buf[start:start + nbytes] = FRESH
    g = Guarded(buf, start, nbytes, shape, dtype, name or f"{str(dtype).replace('torch.', '')}{list(shape)}")
    assert g.ptr % align == offset % align and start >= band and buf.numel() - start - nbytes >= band
    return g


def _changed(band_bytes):
    """(first, last) index of the band bytes that no longer hold BAND, or None."""
    bad = band_bytes != BAND
    if not bool(bad.any()):
        return None
    idx = bad.nonzero().reshape(-1)
    return int(idx[0]), int(idx[-1])


def check(*gs):
    """Raise GuardError unless every band of every buffer still holds its pattern, byte for byte.
    The message names the buffer, the side, and the first and last changed byte as a distance
    from the payload's edge, in bytes and in elements of the payload's type."""
    msgs = []
    for g in gs:
        end = g.start + g.nbytes
        hit = _changed(g.buf[:g.start])
        if hit is not None:
            # distances before the payload's first byte: 1 = the byte just before it
            far, near = g.start - hit[0], g.start - hit[1]
            msgs.append(f"{g.name}: lead band changed, {near}..{far} bytes before the payload "
                        f"(elements -{-(-near // g.itemsize)}..-{-(-far // g.itemsize)})")
        hit = _changed(g.buf[end:])
        if hit is not None:
            # distances past the payload's last byte: 0 = the first byte after it
            msgs.append(f"{g.name}: tail band changed, bytes {hit[0]}..{hit[1]} past the payload's end "
                        f"(elements {hit[0] // g.itemsize}..{hit[1] // g.itemsize} past its last; the payload has "
                        f"{g.nbytes // g.itemsize})")
    if msgs:
        raise GuardError("; ".join(msgs))


def written(g):
    """Per payload byte: True where it no longer holds the fresh pattern (uint8 -> bool tensor of
    nbytes entries).  A written value may itself contain the byte 0x5A: use this for 'some / none
    of this range was written', not to count."""
    return g.payload_bytes() != FRESH


def untouched(g):
    """True when every payload byte still holds the fresh pattern: nothing was written."""
    return not bool(written(g).any())

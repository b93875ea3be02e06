"""wx_attention_h16_packed against wx_attention_h16 at zero tolerance: a segment's rows of a pack are
bit for bit the per-segment launch's, wherever the segment sits and whatever the other segments
hold; exact probes per segment; validation."""
import ctypes
import functools

import pytest
import torch

import whisper_half_helpers as wh

pytestmark = pytest.mark.gpu

WX_E_INVALID = 1001
SCALE = wh.SCALE
# both sides of the 32-key tile, the 64-query unit and kSplit * 32 = 128 keys; 400: every wave owns
# more than two key tiles; 0: a segment that owns no unit
LENGTHS = (1, 31, 32, 33, 63, 64, 65, 0, 127, 129, 257, 400, 1)


@functools.lru_cache(maxsize=None)
def _segments(dtype, H: int):
    """Per segment id: (q, k, v) [H, T, 64] in dtype on the CPU (a peaked softmax, as attention_case)."""
    out = []
    for i, T in enumerate(LENGTHS):
        g = torch.Generator().manual_seed(7919 * (i + 1) + 31 * H + wh.DTYPES.index(dtype))
        q = torch.randn((H, T, 64), generator=g).to(dtype)
        k = (3.0 * torch.randn((H, T, 64), generator=g)).to(dtype)
        v = torch.randn((H, T, 64), generator=g).to(dtype)
        out.append((q, k, v))
    return out


def _pack(dtype, H: int, order, poison_but=None):
    """The segments `order` (ids) packed back to back in one [rows + 32, 3 * 64 H + 8] buffer whose
    padding holds NaN (the fused q/k/v GEMM output's layout plus slack): (views [1, H, rows, 64],
    PackedSegments).  poison_but: every segment but that position holds NaN too."""
    from whisperx_amd import _lib

    segs = _lib.PackedSegments([LENGTHS[i] for i in order])
    D = 64 * H
    buf = torch.full((segs.rows + 32, 3 * D + 8), float("nan"), dtype=dtype)
    for pos, i in enumerate(order):
        a, b = segs.offsets[pos], segs.offsets[pos + 1]
        if poison_but is not None and pos != poison_but:
            continue
        for j, t in enumerate(_segments(dtype, H)[i]):
            buf[a:b, j * D:(j + 1) * D] = t.transpose(0, 1).reshape(b - a, D)
    buf = buf.cuda()
    views = [buf[None, :segs.rows, j * D:(j + 1) * D].view(1, segs.rows, H, 64).transpose(1, 2) for j in range(3)]
    return views, segs


@functools.lru_cache(maxsize=None)
def _alone(dtype, H: int):
    """wx_attention_h16 on every segment alone (B = 1, T = T_s, the pack's views offset to the segment):
    [T, H, 64] per segment id, None for the empty one."""
    from whisperx_amd import _lib

    order = tuple(range(len(LENGTHS)))
    (q, k, v), segs = _pack(dtype, H, order)
    out = []
    for pos in order:
        a, b = segs.offsets[pos], segs.offsets[pos + 1]
        out.append(_lib.attention_h16(q[:, :, a:b], k[:, :, a:b], v[:, :, a:b], SCALE)[0].cpu() if b > a else None)
    return out


def _check(o, segs, order, want, which=None):
    o = o[0].cpu()
    for pos, i in enumerate(order):
        if which is not None and pos not in which:
            continue
        a, b = segs.offsets[pos], segs.offsets[pos + 1]
        if b == a:
            continue
        got = o[a:b]
        assert bool(torch.isfinite(got.float()).all()), (pos, i, LENGTHS[i])
        assert torch.equal(got.view(torch.int16), want[i].view(torch.int16)), (pos, i, LENGTHS[i])


@pytest.mark.parametrize("dtype", wh.DTYPES, ids=wh.name)
@pytest.mark.parametrize("H", [4, 12, 16])
def test_segments_bit_equal_the_per_segment_launch(H, dtype):
    from whisperx_amd import _lib

    want = _alone(dtype, H)
    n = len(LENGTHS)
    fwd = tuple(range(n))
    # the same segments at other positions, beside other neighbours, in a pack of another size
    other = (10, 3, 7, 0, 11, 5, 8, 1)
    for order in (fwd, fwd[::-1], other):
        (q, k, v), segs = _pack(dtype, H, order)
        o = _lib.attention_h16_packed(q, k, v, SCALE, segs)
        assert o.shape == (1, segs.rows, H, 64) and o.dtype == dtype
        _check(o, segs, order, want)


@pytest.mark.parametrize("dtype", wh.DTYPES, ids=wh.name)
def test_a_segment_reads_only_its_own_rows(dtype):
    """Every other segment's q / k / v (and all the padding) NaN: the segment is bit-equal and finite."""
    from whisperx_amd import _lib

    H = 12
    want = _alone(dtype, H)
    order = tuple(range(len(LENGTHS)))
    for pos in (0, 6, len(LENGTHS) - 1):
        (q, k, v), segs = _pack(dtype, H, order, poison_but=pos)
        o = _lib.attention_h16_packed(q, k, v, SCALE, segs)
        _check(o, segs, order, want, which=(pos,))


PROBE_LENGTHS = (1, 33, 64, 257)


def _probe_pack(probes, dtype, H):
    """probes: one per segment, tensors [H, L, 64]; the pack's views and layout."""
    from whisperx_amd import _lib

    segs = _lib.PackedSegments([p.q.shape[1] for p in probes])
    D = 64 * H
    buf = torch.full((segs.rows + 32, 3 * D + 8), float("nan"), dtype=dtype)
    for pos, p in enumerate(probes):
        a, b = segs.offsets[pos], segs.offsets[pos + 1]
        for j, t in enumerate((p.q, p.k, p.v)):
            buf[a:b, j * D:(j + 1) * D] = t.transpose(0, 1).reshape(b - a, D)
    buf = buf.cuda()
    return [buf[None, :segs.rows, j * D:(j + 1) * D].view(1, segs.rows, H, 64).transpose(1, 2) for j in range(3)], segs


@pytest.mark.parametrize("dtype", wh.DTYPES, ids=wh.name)
def test_permutation_probe_per_segment(dtype):
    """o[i] = v[pi(i)] exactly, a different pi per (segment, head)."""
    from whisperx_amd import _lib

    H = 4
    probes = [wh.Permutation(dtype, H, L, "random") for L in PROBE_LENGTHS]
    (q, k, v), segs = _probe_pack(probes, dtype, H)
    o = _lib.attention_h16_packed(q, k, v, SCALE, segs)[0].cpu()
    for pos, p in enumerate(probes):
        got = o[segs.offsets[pos]: segs.offsets[pos + 1]].transpose(0, 1)  # [H, L, 64]
        assert torch.equal(got, p.want), (pos, PROBE_LENGTHS[pos])


@pytest.mark.parametrize("dtype", wh.DTYPES, ids=wh.name)
def test_uniform_probe_per_segment(dtype):
    """q = 0: o is the mean of the segment's own v; exact where L is a power of two, else one rounding."""
    from whisperx_amd import _lib

    H = 4
    probes = [wh.Uniform(dtype, H, L) for L in PROBE_LENGTHS]
    (q, k, v), segs = _probe_pack(probes, dtype, H)
    o = _lib.attention_h16_packed(q, k, v, SCALE, segs)[0].cpu()
    for pos, p in enumerate(probes):
        got = o[segs.offsets[pos]: segs.offsets[pos + 1]].transpose(0, 1).double()
        if p.exact:
            assert torch.equal(got, p.want), (pos, PROBE_LENGTHS[pos])
        else:  # the fp32 quotient rounded once to dtype (the sums are exact integers)
            err = (got - p.want).abs()
            assert bool((err <= wh.HALF_ULP[dtype] * p.want.abs() * (1 + 2.0 ** -10)).all()), (pos, float(err.max()))


def test_validation():
    from whisperx_amd import _lib

    H = 4
    order = (3, 5)
    (q, k, v), segs = _pack(torch.float16, H, order)
    lib = _lib.load()
    rows_t, units_t, n_units, _ = segs.tables(q.device, H, 64)
    o = torch.empty((1, segs.rows, H, 64), dtype=torch.float16, device="cuda")
    st = [(ctypes.c_int64 * 2)(int(t.stride(1)), int(t.stride(2))) for t in (q, k, v)]

    def call(dtype=1, D=64, strides=st, nseg=len(order), units=n_units):
        return lib.wx_attention_h16_packed(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), nseg, rows_t.data_ptr(),
                                           units_t.data_ptr(), units, H, D, strides[0], strides[1], strides[2], SCALE,
                                           dtype, None)

    torch.cuda.synchronize()
    assert call() == 0
    for bad in (0, 3):
        assert call(dtype=bad) == WX_E_INVALID
    assert call(D=32) == WX_E_INVALID
    odd = [(ctypes.c_int64 * 2)(64, int(q.stride(2)) + 4)] + st[1:]
    assert call(strides=odd) == WX_E_INVALID
    assert call(dtype=3, nseg=0) == WX_E_INVALID  # dtype is checked beside D, before the empty pack returns
    # the binding raises on those
    with pytest.raises(_lib.WXError):
        _lib.attention_h16_packed(q[..., :32], k[..., :32], v[..., :32], SCALE, segs)
    D = 64 * H
    buf = torch.zeros((segs.rows, 3 * D + 4), dtype=torch.float16, device="cuda")
    bad_views = [buf[None, :, j * D:(j + 1) * D].view(1, segs.rows, H, 64).transpose(1, 2) for j in range(3)]
    with pytest.raises(_lib.WXError):
        _lib.attention_h16_packed(*bad_views, SCALE, segs)
    with pytest.raises(_lib.WXError):
        _lib.attention_h16_packed(q.float(), k.float(), v.float(), SCALE, segs)
    # no segment, and only empty segments: WX_OK, nothing written
    o.fill_(7.0)
    assert call(nseg=0, units=0) == 0 and call(units=0) == 0
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())
    for lengths in ((), (0, 0, 0)):
        empty = _lib.PackedSegments(lengths)
        out = _lib.attention_h16_packed(q[:, :, :0], k[:, :, :0], v[:, :, :0], SCALE, empty)
        assert out.shape == (1, 0, H, 64) and out.dtype == torch.float16

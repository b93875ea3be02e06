"""The contract of the f32-MFMA attention body that wx_attention_f32, wx_attention_f32_packed and
wx_prefill_attention_f32 share (csrc/wx_attention_unit.h), at zero tolerance: unmasked square
prefill has the bits of the dense entry, a segment of a pack has the bits of the dense entry on its
rows alone; and the K / V time stride that the body's 32-bit offsets allow, refused by the dense and
packed entries before anything is enqueued."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

WX_E_INVALID = 1001
B, H, HD, SCALE = 2, 3, 64, 0.125
# a lone partial tile, an exact tile, a tail landing in wave 1, all four waves busy, and wave 0's
# second trip with and without a partial last tile
LENGTHS = [1, 31, 32, 33, 97, 129, 161]
PACKED_LENGTHS = (33, 1, 129, 64)


def _fused_views(Bn, T, seed):
    """q, k, v [Bn, H, T, 64] as the three slices of one fused [Bn, T, 3 H 64] buffer."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn((Bn, T, 3 * H * HD), generator=g).cuda()
    return [qkv[..., i * H * HD:(i + 1) * H * HD].view(Bn, T, H, HD).transpose(1, 2) for i in range(3)]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("T", LENGTHS)
def test_unmasked_square_prefill_has_the_dense_entrys_bits(T):
    from whisperx_amd import _lib

    q, k, v = _fused_views(B, T, seed=T)
    dense = _lib.attention_f32(q, k, v, SCALE)
    prefill = _lib.prefill_attention_f32(q, k, v, SCALE, causal=None)
    assert bool(torch.isfinite(dense).all()) and dense.shape == prefill.shape == (B, T, H, HD)
    assert torch.equal(_bits(prefill), _bits(dense))


def test_a_packed_segment_has_the_dense_entrys_bits():
    from whisperx_amd import _lib

    segs = _lib.PackedSegments(PACKED_LENGTHS)
    q, k, v = _fused_views(1, segs.rows, seed=7)
    packed = _lib.attention_f32_packed(q, k, v, SCALE, segs, 4)
    assert bool(torch.isfinite(packed).all())
    for a, b in zip(segs.offsets[:-1], segs.offsets[1:]):
        alone = _lib.attention_f32(q[:, :, a:b], k[:, :, a:b], v[:, :, a:b], SCALE)
        assert torch.equal(_bits(packed[:, a:b]), _bits(alone)), (a, b)


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_kv_time_stride_outside_the_bodys_offsets_is_refused(packed):
    """A K or V time stride that is negative or above 2^23 elements (a made-up stride on small valid
    buffers) is WX_E_INVALID, o untouched; then the accepted call."""
    from whisperx_amd import _lib

    lib = _lib.load()
    T = 40
    segs = _lib.PackedSegments([T])
    q, k, v = _fused_views(1, T, seed=3)
    o = torch.full((1, T, H, HD), 7.0, device="cuda")
    n = 2 if packed else 3
    st = [[int(x) for x in t.stride()[3 - n:3]] for t in (q, k, v)]
    rows_t, units_t, n_units, _ = segs.tables(q.device, H)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ks=st[1], vs=st[2]):
        arrs = [(ctypes.c_int64 * n)(*s) for s in (st[0], ks, vs)]
        if packed:
            return lib.wx_attention_f32_packed(_P(q), _P(k), _P(v), _P(o), 1, _P(rows_t), _P(units_t), n_units, H, HD,
                                               *arrs, SCALE, 4, stream)
        return lib.wx_attention_f32(_P(q), _P(k), _P(v), _P(o), 1, H, T, HD, *arrs, SCALE, stream)

    for bad in (-64, 2 ** 23 + 4, 2 ** 24, 2 ** 40):
        assert call(ks=st[1][:-1] + [bad]) == WX_E_INVALID, bad
        assert call(vs=st[2][:-1] + [bad]) == WX_E_INVALID, bad
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())  # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(o), _bits(_lib.attention_f32(q, k, v, SCALE)))

"""WhisperEncoder on the GPU: wx_whisper_stem against an fp64 torch stem (strided input, bounded
output, chunk isolation), wx_add_layernorm at Whisper's widths, the whole encoder against
transformers' WhisperEncoder, slicing, encode_chunks and streams.

Tolerance (the mel tests' rule): ref_err = max|HF fp32 - HF fp64| on the same inputs (CPU), and
max|ours - HF fp64| <= 4 x ref_err; both are printed.  The stem's reference error is that of the
fp32 torch stem on the CPU against the fp64 one."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from whisper_helpers import case, make_encoder, make_features, stem_ref64

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


def _stem_f32_cpu(enc, x):
    h = F.gelu(F.conv1d(x, enc.conv1.weight, enc.conv1.bias, padding=1))
    h = F.gelu(F.conv1d(h, enc.conv2.weight, enc.conv2.bias, stride=2, padding=1))
    return h.permute(0, 2, 1) + enc.embed_positions.weight


@pytest.mark.parametrize("M,D,Tin,B", [(80, 384, 2, 1), (80, 512, 130, 3), (128, 1280, 66, 2), (80, 384, 3000, 1)])
def test_stem_against_fp64(M, D, Tin, B):
    from whisperx_amd import WhisperEncoder

    enc = make_encoder(D, 0, Tin // 2, M)
    x = make_features(B, M, Tin)
    want = stem_ref64(enc, x)
    ref_err = float((_stem_f32_cpu(enc, x).double() - want).abs().max())
    we = WhisperEncoder(enc, device="cuda")
    # x: a strided view of a wider sentinel-filled buffer; out: a slice of a sentinel-filled tensor
    wide = torch.full((B + 1, M + 3, Tin + 37), SENTINEL, device="cuda")
    xv = wide[:B, :M, 5:5 + Tin]
    xv.copy_(x)
    assert not xv.is_contiguous()
    full = torch.full((B + 2, Tin // 2, D), SENTINEL, device="cuda")
    got = we.stem(xv, out=full[1:B + 1])
    torch.cuda.synchronize()
    assert got.data_ptr() == full[1].data_ptr()
    assert bool((full[0] == SENTINEL).all()) and bool((full[B + 1] == SENTINEL).all())
    err = float((got.cpu().double() - want).abs().max())
    print(f"stem M {M} D {D} Tin {Tin} B {B}: |kernel - fp64| {err:.3e}, ref_err {ref_err:.3e}, bound {4 * ref_err:.3e}")
    assert ref_err > 0 and err <= 4 * ref_err


def test_stem_chunk_isolation():
    """Zero padding is per chunk: chunk 1 between neighbours full of 1e4 equals chunk 1 alone, bit for bit."""
    from whisperx_amd import WhisperEncoder

    we = WhisperEncoder(make_encoder(512, 0, 65, 80), device="cuda")
    x = torch.full((3, 80, 130), 1e4, device="cuda")
    x[1] = make_features(1, 80, 130)[0].cuda()
    both = we.stem(x)
    alone = we.stem(x[1:2].clone())
    assert torch.equal(both[1].view(torch.int32), alone[0].view(torch.int32))
    assert bool(torch.isfinite(both[1]).all())


@pytest.mark.parametrize("D", [384, 1280])
@pytest.mark.parametrize("lead", [(3, 5), (1, 1499)])
def test_add_layernorm_whisper_widths(D, lead):
    from whisperx_amd import _lib

    g = torch.Generator().manual_seed(D + lead[1])
    a = torch.randn((*lead, D), generator=g).cuda()
    wide = torch.randn((*lead, D + 8), generator=g).cuda()
    b = wide[..., 4:4 + D]  # row-strided (stride D + 8), 16-byte aligned
    gamma, beta = (1 + 0.1 * torch.randn(D, generator=g)).cuda(), (0.1 * torch.randn(D, generator=g)).cuda()
    y, s = _lib.add_layernorm(a, b, gamma, beta, 1e-5, want_sum=True)
    assert torch.equal(s, a + b)
    ref = F.layer_norm((a + b).double(), (D,), gamma.double(), beta.double(), 1e-5)
    ref32 = F.layer_norm(a + b, (D,), gamma, beta, 1e-5)
    ref_err = float((ref32.double() - ref).abs().max())
    err = float((y.double() - ref).abs().max())
    print(f"add_layernorm D {D} {lead}: |kernel - fp64| {err:.3e}, torch fp32 {ref_err:.3e}")
    assert err <= 4 * ref_err
    assert torch.equal(_lib.add_layernorm(a, b, gamma, beta, 1e-5), y)


@pytest.mark.parametrize("D,layers,P,B", [(384, 2, 50, 3), (512, 1, 33, 2), (768, 1, 33, 1), (1024, 1, 33, 2),
                                          (1280, 1, 34, 2), (384, 1, 1500, 2)])
def test_encoder_against_the_oracle(D, layers, P, B):
    from whisperx_amd import WhisperEncoder

    enc, x, y64, ref_err = case(D, layers, P, B)
    tol = 4 * ref_err
    we = WhisperEncoder(enc, device="cuda")
    got = we.encode(x)
    assert tuple(got.shape) == (B, P, D) and got.is_cuda
    err = float((got.cpu().double() - y64).abs().max())
    host = we._forward_host(x.cuda())  # the host route's arithmetic on the device
    err_host = float((got - host).abs().max())
    print(f"encoder D {D} layers {layers} P {P} B {B}: |kernel - fp64| {err:.3e}, ref_err {ref_err:.3e}, "
          f"bound {tol:.3e}, |kernel - host route| {err_host:.3e}")
    assert ref_err > 0 and err <= tol
    assert err_host <= 2 * tol


def test_slicing_gives_the_same_rows():
    from whisperx_amd import WhisperEncoder

    enc, _, _, ref_err = case(384, 2, 50, 3)
    x = make_features(5, 80, 100, seed=7).cuda()
    we = WhisperEncoder(enc, device="cuda")
    whole, sliced = we.encode(x, batch_size=16), we.encode(x, batch_size=2)
    assert float((whole - sliced).abs().max()) <= 4 * ref_err
    stem = we.stem(x)
    for a in (0, 2, 4):
        assert torch.equal(we.stem(x[a:a + 2]).view(torch.int32), stem[a:a + 2].view(torch.int32))


def test_encode_chunks_equals_encode_of_log_mel_chunks():
    from whisperx_amd import WhisperEncoder, log_mel_chunks

    we = WhisperEncoder(make_encoder(384, 1, 1500, 80), device="cuda")
    rng = np.random.default_rng(3)
    audio = (0.1 * rng.standard_normal(40 * 16000)).astype(np.float32)
    segments = [{"start": 0.5, "end": 27.25}, {"start": 28.0, "end": 39.9}]
    got = we.encode_chunks(audio, segments)
    want = we.encode(log_mel_chunks(audio, segments, 80, device="cuda"))
    assert tuple(got.shape) == (2, 1500, 384)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool(torch.isfinite(got).all())


def test_side_stream_gives_the_same_result():
    from whisperx_amd import WhisperEncoder

    enc, x, y64, ref_err = case(512, 1, 33, 2)
    we = WhisperEncoder(enc, device="cuda")
    xd = x.cuda()
    want, want_stem = we.encode(xd), we.stem(xd)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, got_stem = we.encode(xd), we.stem(xd)
    side.synchronize()
    assert torch.equal(got_stem.view(torch.int32), want_stem.view(torch.int32))
    # (the GEMM library may pick its kernels per stream: the whole forward is held to the oracle's bound)
    assert float((got.cpu().double() - y64).abs().max()) <= 4 * ref_err
    assert float((got - want).abs().max()) <= 4 * ref_err

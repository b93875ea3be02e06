"""WhisperEncoder(dtype=float16 / bfloat16) on the GPU: the kernel route (wx_whisper_stem,
wx_add_layernorm_h16, 16-bit GEMMs, wx_attention_h16) against transformers' fp64 encoder within
2 x ref_err_half, ref_err_half being what casting the stock model to dtype costs on the CPU
(whisper_half_helpers); the fp32 default unchanged; the decoder on the half encoder's states."""
import pytest
import torch

import whisper_half_helpers as hh
from whisper_helpers import case

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(d, id=hh.name(d)) for d in hh.DTYPES]
GEOMETRIES = [(384, 2, 50, 3), (512, 1, 33, 2), (768, 1, 33, 1), (1024, 1, 33, 2), (1280, 1, 33, 2), (384, 1, 1500, 1)]


@pytest.mark.parametrize("D,layers,P,B", GEOMETRIES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_half_encoder_against_the_oracle(dtype, D, layers, P, B):
    from whisperx_amd import WhisperEncoder

    enc, x, y64, ref_err_half = hh.encoder_case(dtype, D, layers, P, B)
    we = WhisperEncoder(enc, device="cuda", dtype=dtype)
    assert all(t.dtype == dtype for L in we.layers for n in ("qkv", "out", "fc1", "fc2") for t in L[n])
    assert all(t.dtype == torch.float32 for L in we.layers for n in ("ln1", "ln2") for t in L[n])
    got = we.encode(x)
    assert tuple(got.shape) == (B, P, D) and got.is_cuda and got.dtype == torch.float32
    err = float((got.cpu().double() - y64).abs().max())
    host = we._forward_host(x.cuda())  # the host route's arithmetic on the device
    assert host.dtype == torch.float32
    err_host = float((got - host).abs().max())
    print(f"half encoder {hh.name(dtype)} D {D} layers {layers} P {P} B {B}: |kernel - fp64| {err:.3e}, ref_err_half "
          f"{ref_err_half:.3e}, ratio {err / ref_err_half:.3f} (bound 2), |kernel - host route| {err_host:.3e}")
    assert err <= 2 * ref_err_half


def test_float32_is_the_default_bit_for_bit():
    from whisperx_amd import WhisperEncoder

    enc, x, _, _ = case(384, 2, 50, 3)
    a, b = WhisperEncoder(enc, device="cuda"), WhisperEncoder(enc, device="cuda", dtype=torch.float32)
    assert a.dtype == b.dtype == torch.float32
    assert torch.equal(a.encode(x).view(torch.int32), b.encode(x).view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_decoder_takes_the_half_encoders_states(dtype):
    from whisper_decoder_helpers import make_model
    from whisperx_amd import WhisperDecoder, WhisperEncoder

    enc, x, _, _ = case(384, 2, 50, 3)
    states = WhisperEncoder(enc, device="cuda", dtype=dtype).encode(x)
    dec = WhisperDecoder(make_model(384, 1, 50, 96, 16), device="cuda")
    lg = dec.logits(states, torch.tensor([[1, 5, 9]] * 3))
    assert tuple(lg.shape) == (3, 3, 96) and lg.dtype == torch.float32 and bool(torch.isfinite(lg).all())

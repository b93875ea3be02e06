"""WhisperDecoder's half route on the GPU: the kernel route (wx_decode_attention_h16, its grouped form
and wx_add_layernorm_h16) under the rules of whisper_decoder_half_helpers, against the host route's
arithmetic on the device (printed, not bounded) and on a side stream."""
import pytest
import torch

import whisper_decoder_half_helpers as dh
from whisper_decoder_helpers import GEOMETRIES, case

pytestmark = pytest.mark.gpu
BOTH = pytest.mark.parametrize("dtype", dh.DTYPES, ids=dh.name)


def _device(c, dtype):
    from whisperx_amd import WhisperDecoder

    return WhisperDecoder(c.model, device="cuda", dtype=dtype)


@BOTH
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_teacher_forced_logits(geometry, dtype):
    c = case(*geometry)
    dec = _device(c, dtype)
    got = dh.check_forced_logits(c, dec, "kernels")
    host = dec.logits(c.enc, c.forced()[0], kernels=False)  # the host route's arithmetic on the device
    print(f"kernels {dh.name(dtype)} {geometry}: |kernels - host route| max {float((got - host).abs().max()):.3e}")


@BOTH
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_greedy_on_its_own_path(geometry, dtype):
    c = case(*geometry)
    dh.check_greedy(c, _device(c, dtype), "kernels")


@BOTH
def test_stopping_and_suppression(dtype):
    c = case(*GEOMETRIES[0])
    dh.check_stopping_and_suppression(c, _device(c, dtype), "kernels")


@BOTH
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_beam_search(geometry, dtype):
    c = case(*geometry)
    dh.check_beam_search(c, _device(c, dtype), "kernels")


@BOTH
def test_state_reorder_and_detect_language(dtype):
    c = case(*GEOMETRIES[0])
    dec = _device(c, dtype)
    dh.check_state(c, dec)
    dh.check_detect_language(c, dec, "kernels")
    c2 = case(*GEOMETRIES[2])
    dh.check_reorder(c2, _device(c2, dtype))


@BOTH
def test_side_stream_gives_the_same_result(dtype):
    c = case(*GEOMETRIES[2])
    ids, _, _ = c.forced()
    y64, ref_err, ref_rms = dh.path_errors(c, dtype, ids)
    dec = _device(c, dtype)
    want = dec.logits(c.enc, ids)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = dec.start(c.enc)
        got = torch.stack([dec.step(st, ids[:, i]) for i in range(ids.shape[1])], 1)
    side.synchronize()
    # (the GEMM library may pick its kernels per stream: both runs are held to the oracle's rule)
    dh.within_the_rule(got, y64, ref_err, ref_rms, f"side stream {dh.name(dtype)}")
    print(f"side stream {dh.name(dtype)}: |side - default stream| max {float((got - want).abs().max()):.3e}")
    dh.within_the_rule(want, y64, ref_err, ref_rms, f"default stream {dh.name(dtype)}")
    assert float((got - want).abs().max()) <= 4 * ref_err  # (two runs within 2 x ref_err_half of fp64 each)

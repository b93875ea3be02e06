"""WhisperDecoder.prefill on the GPU: the kernel route (wx_prefill_attention_f32 / _h16 on the caches
and the cross-attention tensors in place) under the checks of tests/test_whisper_prefill.py, for the
three geometries in fp32 and both half types, and against the host route's arithmetic on the device."""
import pytest
import torch

import beam_helpers as bh
import prefill_helpers as ph
import whisper_decoder_half_helpers as dh
from whisper_decoder_helpers import (GEOMETRIES, case, check_forced_logits, check_greedy, check_stopping,
                                     check_suppression)

pytestmark = pytest.mark.gpu
BOTH = pytest.mark.parametrize("dtype", dh.DTYPES, ids=dh.name)


def _device(c, dtype=torch.float32):
    from whisperx_amd import WhisperDecoder

    return WhisperDecoder(c.model, device="cuda", dtype=dtype)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_teacher_forced_logits_and_the_host_route(geometry):
    c = case(*geometry)
    dec = _device(c)
    got = check_forced_logits(c, ph.Prefilled(dec), "kernels prefill")
    ids, _, ref_err = c.forced()
    host = dec.logits(c.enc, ids, kernels=False, prefill=True)  # the host route's arithmetic on the device
    d = float((got - host).abs().max())
    print(f"kernels prefill {geometry}: |kernels - host route| max {d:.3e}, bound {8 * ref_err:.3e}")
    assert d <= 8 * ref_err  # (each within 4 x ref_err of fp64)
    check_forced_logits(c, ph.Prefilled(_HostRoute(dec)), "host route on the device, prefill")


class _HostRoute:
    """The decoder with kernels=False on the device."""

    def __init__(self, dec):
        self.dec = dec

    def __getattr__(self, name):
        return getattr(self.dec, name)

    def logits(self, *a, **kw):
        return self.dec.logits(*a, kernels=False, **kw)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_greedy_equals_the_fp64_loop(geometry):
    c = case(*geometry)
    check_greedy(c, ph.Prefilled(_device(c)), "kernels prefill")


def test_stopping_and_suppression():
    c = case(*GEOMETRIES[0])
    dec = ph.Prefilled(_device(c))
    check_stopping(c, dec)
    check_suppression(c, dec, "kernels prefill")


@pytest.mark.parametrize("G", [2, 5])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_beam_search_equals_the_fp64_search(geometry, G):
    c = case(*geometry)
    got = bh.check_beam_search(c, ph.Prefilled(_device(c)), "kernels prefill", bh.EOT[c.D], G=G)
    assert all(len(hs) == G for hs in got)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_every_route_to_a_position_agrees(geometry):
    c = case(*geometry)
    ph.check_routes(_device(c), c, "kernels")


def test_a_chunks_beams_are_bit_equal_after_prefill():
    c = case(*GEOMETRIES[0])
    ph.check_beams(_device(c), c)
    ph.check_empty_batch(_device(c), c)


@BOTH
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_half_teacher_forced_logits_and_the_host_route(geometry, dtype):
    c = case(*geometry)
    dec = _device(c, dtype)
    got = dh.check_forced_logits(c, ph.Prefilled(dec), "kernels prefill")
    ids, _, _ = c.forced()
    y64, ref_err, ref_rms = dh.path_errors(c, dtype, ids)
    host = dec.logits(c.enc, ids, kernels=False, prefill=True)  # the host route's arithmetic on the device
    print(f"kernels prefill {dh.name(dtype)} {geometry}: |kernels - host route| max {float((got - host).abs().max()):.3e}")
    dh.within_the_rule(host, y64, ref_err, ref_rms, f"host route on the device, prefill {dh.name(dtype)} {geometry}")
    assert float((got - host).abs().max()) <= 4 * ref_err  # (two runs within 2 x ref_err_half of fp64 each)


@BOTH
def test_half_beam_search(dtype):
    c = case(*GEOMETRIES[0])
    dh.check_beam_search(c, ph.Prefilled(_device(c, dtype)), "kernels prefill")


@BOTH
def test_half_beams_and_routes(dtype):
    c = case(*GEOMETRIES[0])
    dec = _device(c, dtype)
    ph.check_beams(dec, c)
    ids, _, _ = c.forced()
    y64, ref_err, ref_rms = dh.path_errors(c, dtype, ids)
    st = dec.start(c.enc)
    dec.prefill(st, ids[:, :5])
    lg = dec.prefill(st, ids[:, 5:])
    assert st.pos == ids.shape[1]
    dh.within_the_rule(lg[:, None], y64[:, -1:], ref_err, ref_rms, f"prefill(5) prefill(7) {dh.name(dtype)}")

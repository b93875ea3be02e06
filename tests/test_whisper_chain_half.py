"""The half chain without a GPU: WhisperEncoder(dtype).encode -> WhisperDecoder(dtype).generate on
the small geometry, no fp32 detour but the encoder's fp32 output, which start() rounds."""
import pytest
import torch

from whisper_decoder_helpers import GEOMETRIES, PROMPT, case
from whisper_half_helpers import DTYPES, name
from whisper_helpers import case as encoder_case


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_encoder_into_decoder(dtype):
    from whisperx_amd import WhisperDecoder, WhisperEncoder

    D, layers, P, V, T, B = GEOMETRIES[0]
    enc_model, x, _, _ = encoder_case(D, 1, P, B)
    enc = WhisperEncoder(enc_model, device="cpu", dtype=dtype)
    dec = WhisperDecoder(case(*GEOMETRIES[0]).model, device="cpu", dtype=dtype)
    states = enc.encode(x)
    assert tuple(states.shape) == (B, P, D) and states.dtype == torch.float32
    st = dec.start(states)
    assert all(t.dtype == dtype for t in st.cross)
    ids = dec.generate(states, PROMPT, eot=V - 1, max_length=len(PROMPT) + 6)
    assert len(ids) == B and all(1 <= len(row) <= 6 or row == [] for row in ids)
    assert all(0 <= t < V - 1 for row in ids for t in row)
    beams = dec.generate(states, PROMPT, eot=V - 1, max_length=len(PROMPT) + 6, beam_size=3)
    assert len(beams) == B and all(0 <= t < V - 1 for row in beams for t in row)

"""WhisperDecoder's half route (dtype float16 / bfloat16) without a GPU: construction (what is stored
in dtype, what is refused), and the host route against the oracle under the rules of
whisper_decoder_half_helpers: teacher-forced logits, greedy decoding on the decoder's own path,
stopping and suppression, beam search, reorder and language detection."""
import pytest
import torch

import whisper_decoder_half_helpers as dh
from whisper_decoder_helpers import GEOMETRIES, case

SMALL = GEOMETRIES[0]
BOTH = pytest.mark.parametrize("dtype", dh.DTYPES, ids=dh.name)


def _host(c, dtype):
    from whisperx_amd import WhisperDecoder

    return WhisperDecoder(c.model, device="cpu", dtype=dtype)


def test_the_default_is_float32_bit_for_bit():
    from whisperx_amd import WhisperDecoder

    c = case(*SMALL)
    ids, _, _ = c.forced()
    plain, named = WhisperDecoder(c.model, device="cpu"), WhisperDecoder(c.model, device="cpu", dtype=torch.float32)
    assert plain.dtype == named.dtype == torch.float32 and plain.embed.dtype == torch.float32
    a, b = plain.logits(c.enc, ids), named.logits(c.enc, ids)
    assert a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
    st = plain.start(c.enc)
    assert all(x.dtype == torch.float32 for x in (*st.cross, *st.self_k, *st.self_v))


@BOTH
def test_stored_dtypes(dtype):
    """GEMM weights and biases and the embedding are kept in dtype only; the positional table and the
    LayerNorm parameters stay fp32."""
    c = case(*SMALL)
    dec = _host(c, dtype)
    assert dec.dtype == dtype and dec.embed.dtype == dtype and tuple(dec.embed.shape) == (c.V, c.D)
    assert dec.pos.dtype == torch.float32 and all(t.dtype == torch.float32 for t in dec.ln_f)
    for L in dec.layers:
        for key, pair in L.items():
            want = torch.float32 if key.startswith("ln") else dtype
            assert all(t.dtype == want for t in pair), key
    # no fp32 copy of a matrix is kept anywhere on the decoder but the positional table
    kept = [v for v in vars(dec).values() if torch.is_tensor(v)]
    kept += [t for L in dec.layers for pair in L.values() for t in pair]
    assert [tuple(t.shape) for t in kept if t.dtype == torch.float32 and t.dim() == 2] == [tuple(dec.pos.shape)]
    assert torch.equal(dec.embed, c.model.model.decoder.embed_tokens.weight.to(dtype))
    dh.check_state(c, dec)


def test_refusals():
    from whisperx_amd import WhisperDecoder

    c = case(*SMALL)
    sd = dict(c.model.model.decoder.state_dict())
    for bad in (torch.float64, torch.int8, "float16", None):
        with pytest.raises(ValueError, match="WhisperDecoder: dtype must be"):
            WhisperDecoder(sd, device="cpu", dtype=bad)
    for key in ("layers.1.fc1.weight", "layers.0.encoder_attn.v_proj.bias", "embed_tokens.weight"):
        big = sd[key].clone()
        big.view(-1)[3] = 1e5
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            WhisperDecoder({**sd, key: big}, device="cpu", dtype=torch.float16)
        WhisperDecoder({**sd, key: big}, device="cpu", dtype=torch.bfloat16)  # (finite in bf16)
    # the tie to proj_out is checked on the fp32 tensors, before any rounding
    nudged = sd["embed_tokens.weight"].clone()
    nudged[0, 0] += 2.0 ** -20
    with pytest.raises(ValueError, match=r"proj_out\.weight"):
        WhisperDecoder({**sd, "proj_out.weight": nudged}, device="cpu", dtype=torch.float16)


@BOTH
def test_load_whisper_decoder_takes_the_dtype(dtype, tmp_path):
    from safetensors.torch import save_file

    from whisperx_amd import load_whisper_decoder

    c = case(*SMALL)
    sd = {"model.decoder." + k: v.clone().contiguous() for k, v in c.model.model.decoder.state_dict().items()}
    save_file(sd, str(tmp_path / "dec.safetensors"))
    got, want = load_whisper_decoder(str(tmp_path / "dec.safetensors"), device="cpu", dtype=dtype), _host(c, dtype)
    assert got.dtype == dtype and torch.equal(got.embed, want.embed)
    assert all(torch.equal(x, y) for a, b in zip(got.layers, want.layers) for k in a for x, y in zip(a[k], b[k]))


@BOTH
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_teacher_forced_logits(geometry, dtype):
    c = case(*geometry)
    dh.check_forced_logits(c, _host(c, dtype), "host")


@BOTH
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_greedy_on_its_own_path(geometry, dtype):
    c = case(*geometry)
    dh.check_greedy(c, _host(c, dtype), "host")


@BOTH
def test_stopping_and_suppression(dtype):
    c = case(*SMALL)
    dh.check_stopping_and_suppression(c, _host(c, dtype), "host")


@BOTH
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_beam_search(geometry, dtype):
    c = case(*geometry)
    dh.check_beam_search(c, _host(c, dtype), "host")


@BOTH
def test_reorder_keeps_the_dtype(dtype):
    c = case(*GEOMETRIES[2])
    dh.check_reorder(c, _host(c, dtype))


@BOTH
def test_detect_language(dtype):
    c = case(*SMALL)
    dh.check_detect_language(c, _host(c, dtype), "host")

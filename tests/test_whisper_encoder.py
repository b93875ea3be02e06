"""WhisperEncoder without a GPU: the host route against transformers' WhisperEncoder (fp64 as the
reference, 4 x the stock fp32 route's own error as the bound), the accepted weight forms, the file
loader, the refusals, and wx_whisper_stem's argument validation (no device needed: it returns
before anything is enqueued)."""
import ctypes

import pytest
import torch

from whisper_helpers import case, make_encoder, make_features, openai_names


def _host(weights):
    from whisperx_amd import WhisperEncoder

    return WhisperEncoder(weights, device="cpu")


@pytest.mark.parametrize("D,layers,P,B,n_mels", [(384, 2, 50, 3, 80), (1280, 1, 34, 2, 80), (384, 2, 50, 3, 128),
                                                 (1280, 1, 34, 2, 128)])
def test_host_route_against_the_oracle(D, layers, P, B, n_mels):
    enc, x, y64, ref_err = case(D, layers, P, B, n_mels)
    got = _host(enc).encode(x)
    assert tuple(got.shape) == (B, P, D) and got.dtype == torch.float32
    err = float((got.double() - y64).abs().max())
    print(f"D {D} layers {layers} P {P} B {B} mels {n_mels}: |host - fp64| {err:.3e}, ref_err {ref_err:.3e}, "
          f"bound {4 * ref_err:.3e}, |out| max {float(y64.abs().max()):.2f}")
    assert ref_err > 0 and err <= 4 * ref_err


def test_every_weight_form_gives_the_same_output():
    from transformers import WhisperConfig, WhisperForConditionalGeneration, WhisperModel

    enc, x, _, _ = case(384, 2, 50, 3)
    want = _host(enc).encode(x)
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    for prefix in ("", "encoder.", "model.encoder."):
        assert torch.equal(_host({prefix + k: v for k, v in sd.items()}).encode(x), want), prefix
    assert torch.equal(_host(openai_names(sd, "encoder")).encode(x), want)
    # a dict of a whole model: the decoder's tensors are ignored
    with_dec = {"model.encoder." + k: v for k, v in sd.items()}
    with_dec["model.decoder.layers.0.fc1.weight"] = torch.zeros(4, 4)
    assert torch.equal(_host(with_dec).encode(x), want)
    # the two wrapping modules
    cfg = WhisperConfig(d_model=384, encoder_layers=2, encoder_attention_heads=6, encoder_ffn_dim=1536,
                        max_source_positions=50, decoder_layers=1, decoder_attention_heads=1, decoder_ffn_dim=64,
                        vocab_size=64, pad_token_id=0, bos_token_id=1, eos_token_id=2, decoder_start_token_id=1)
    for cls in (WhisperModel, WhisperForConditionalGeneration):
        m = cls(cfg).eval()
        (m.model if hasattr(m, "model") else m).encoder.load_state_dict(sd)
        before = {k: v.clone() for k, v in m.state_dict().items()}
        assert torch.equal(_host(m).encode(x), want), cls.__name__
        assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())  # the module is only read


def test_load_whisper_encoder_round_trip(tmp_path):
    from safetensors.torch import save_file

    from whisperx_amd import load_whisper_encoder

    enc, x, _, _ = case(384, 2, 50, 3)
    want = _host(enc).encode(x)
    sd = {"model.encoder." + k: v.clone().contiguous() for k, v in enc.state_dict().items()}
    save_file(sd, str(tmp_path / "enc.safetensors"))
    torch.save(sd, tmp_path / "enc.pt")
    for name in ("enc.safetensors", "enc.pt"):
        got = load_whisper_encoder(str(tmp_path / name), device="cpu")
        assert (got.D, got.n_mels, got.P, len(got.layers), got.H) == (384, 80, 50, 2, 6)
        assert torch.equal(got.encode(x), want), name


def test_2d_input_and_numpy_equal_3d():
    enc, x, y64, ref_err = case(384, 2, 50, 3)
    we = _host(enc)
    want = we.encode(x[:1])
    assert torch.equal(we.encode(x[0]), want)
    assert torch.equal(we.encode(x[0].numpy()), want)
    # slices of two chunks: the same rows (torch's GEMMs are not bit-stable across batch sizes)
    assert float((we.encode(x, batch_size=2).double() - y64).abs().max()) <= 4 * ref_err


def test_refusals_name_the_tensor():
    enc, x, _, _ = case(384, 2, 50, 3)
    we = _host(enc)
    with pytest.raises(ValueError, match="frames"):
        we.encode(x[:, :, :98])
    with pytest.raises(ValueError, match="80"):
        we.encode(make_features(1, 64, 100))
    sd = dict(enc.state_dict())
    missing = {k: v for k, v in sd.items() if k != "layers.1.fc2.bias"}
    with pytest.raises(ValueError, match=r"layers\.1\.fc2\.bias"):
        _host(missing)
    with pytest.raises(ValueError, match=r"k_proj\.bias"):
        _host({**sd, "layers.0.self_attn.k_proj.bias": torch.zeros(384)})
    # head size 96: a width that is no multiple of 64
    wide = make_encoder(64, 1, 10).state_dict()
    bad = {k: (torch.zeros(96, 80, 3) if k == "conv1.weight" else v) for k, v in wide.items()}
    with pytest.raises(ValueError, match=r"conv1\.weight"):
        _host(bad)
    with pytest.raises(ValueError):
        _host(42)


def test_stem_entry_validates_before_anything_is_enqueued():
    """No device: every case returns before a launch (dummy, aligned, never dereferenced pointers)."""
    from whisperx_amd import _lib

    lib = _lib.load(require_device=False)
    p = ctypes.c_void_p(1 << 20)

    def call(B=1, M=80, Tin=100, D=384, row=None, ws=None, x=p, out=p):
        need = lib.wx_whisper_stem_workspace_bytes(B, Tin, D)
        return lib.wx_whisper_stem(x, M * (row or Tin), row or Tin, B, M, Tin, p, p, p, p, p, D, out, p,
                                   need if ws is None else ws, None)

    need = lib.wx_whisper_stem_workspace_bytes(2, 100, 384)
    assert need >= 2 * 100 * 384 * 4
    assert call(Tin=101) == 1001 and call(Tin=0) == 1001
    assert call(M=64) == 1001
    assert call(D=96) == 1001 and call(D=1344) == 1001
    assert call(B=-1) == 1001
    assert call(row=99) == 1001
    assert call(x=None) == 1001 and call(out=ctypes.c_void_p((1 << 20) + 4)) == 1001
    assert call(B=2, ws=need - 1) == 1004
    assert call(B=0) == 0 and call(B=0, ws=0) == 0

"""The half route (float16 / bfloat16) of the packed wav2vec2 forward on the CPU: the host route's
rounding plan against fp64 (emission_half_helpers' rule), and the public interface's dtype
plumbing and refusals.  (align() itself needs a HIP device for its DP: tests/test_gpu_emission_half.py.)"""
import json
import os

import pytest
import torch

import emission_half_helpers as hh


@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
@pytest.mark.parametrize("kind", ["post", "stable"])
def test_host_route_within_twice_the_cast_models_error(kind, dtype):
    """emission.packed_logits(dtype=...) on a CPU model (torch ops with the kernels' rounding points)."""
    from whisperx_amd import _lib, emission

    model, wavs, _ = hh.case(kind)
    Ts = hh.frames(kind)
    lg = emission.packed_logits(model, wavs, _lib.PackedSegments(Ts), None, dtype=dtype)
    assert lg.dtype == torch.float32 and lg.shape == (sum(Ts), hh.VOCAB)
    hh.check_rule(kind, dtype, list(torch.log_softmax(lg, -1).split(Ts)), "host route")


@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
def test_emissions_on_cpu_take_the_host_route(dtype, monkeypatch):
    """alignment._emissions(device="cpu", dtype=...) goes through packed_logits, not the stock forward."""
    from whisperx_amd import alignment, emission

    model, wavs, _ = hh.case("post")
    calls = []
    real = emission.packed_logits

    def spy(*a, **k):
        calls.append(k.get("dtype"))
        return real(*a, **k)

    monkeypatch.setattr(emission, "packed_logits", spy)
    rows = alignment._emissions(model, "huggingface", wavs, "cpu", dtype=dtype)
    assert calls == [dtype]
    hh.check_rule("post", dtype, rows, "_emissions on cpu")


def test_model_and_cache_are_left_alone():
    """The caller's model stays fp32 and attribute-free; the rounded operands are built once per
    (model, dtype) and again only after a parameter changes."""
    from whisperx_amd import emission

    model, _, _ = hh.case("post")
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    attrs0 = {id(m): set(m.__dict__) for m in model.modules()}
    a = emission.half_operands(model, torch.float16)
    assert emission.half_operands(model, torch.float16) is a
    b = emission.half_operands(model, torch.bfloat16)
    assert b is not a and b.dtype == torch.bfloat16 and emission.half_operands(model, torch.float16) is a
    assert a.head[0].dtype == torch.float16 and a.layers[0].qkv[0].shape == (3 * 256, 256)
    assert torch.equal(a.layers[1].ff1[0], model.wav2vec2.encoder.layers[1].feed_forward.intermediate_dense.weight.half())
    assert all(p.dtype == torch.float32 for p in model.parameters())
    assert {id(m): set(m.__dict__) for m in model.modules()} == attrs0
    sd1 = model.state_dict()
    assert sd0.keys() == sd1.keys() and all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    w = model.lm_head.weight
    with torch.no_grad():
        w.add_(0.0)  # (an in-place write: a new version of the same values)
    c = emission.half_operands(model, torch.float16)
    assert c is not a and torch.equal(c.head[0], a.head[0])


def _save_local_model(d, hidden=256, poison=None):
    """A Wav2Vec2ForCTC + processor directory the packed encoder supports (hidden 256: 4 heads of 64,
    positional conv K 128 in 4 groups of 64); hidden 64 gives one it rejects."""
    from transformers import (Wav2Vec2Config, Wav2Vec2CTCTokenizer, Wav2Vec2FeatureExtractor, Wav2Vec2ForCTC,
                              Wav2Vec2Processor)

    from whisperx_amd.synthetic import W2V_VOCAB

    vocab = {c: i for i, c in enumerate(W2V_VOCAB)}
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump(vocab, f)
    tok = Wav2Vec2CTCTokenizer(os.path.join(d, "vocab.json"), unk_token="<unk>", pad_token="<pad>",
                               word_delimiter_token="|")
    fe = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True,
                                  return_attention_mask=False)
    Wav2Vec2Processor(feature_extractor=fe, tokenizer=tok).save_pretrained(d)
    torch.manual_seed(0)
    cfg = Wav2Vec2Config(vocab_size=len(vocab), hidden_size=hidden, num_hidden_layers=1, num_attention_heads=hidden // 64 or 1,
                         intermediate_size=2 * hidden, conv_dim=(32,) * 7, num_conv_pos_embedding_groups=4)
    m = Wav2Vec2ForCTC(cfg)
    if poison is not None:
        with torch.no_grad():
            dict(m.named_parameters())[poison].view(-1)[3] = 1e6
    m.save_pretrained(d)


def test_load_align_model_dtype(tmp_path):
    from whisperx_amd import load_align_model

    _save_local_model(str(tmp_path))
    _, meta0 = load_align_model("en", "cpu", model_name=str(tmp_path))
    assert set(meta0) == {"language", "dictionary", "type"}  # a default call's metadata is unchanged
    _, meta32 = load_align_model("en", "cpu", model_name=str(tmp_path), dtype=torch.float32)
    assert meta32 == meta0
    for dtype in hh.DTYPES:
        model, meta = load_align_model("en", "cpu", model_name=str(tmp_path), dtype=dtype)
        assert meta["dtype"] == dtype and {k: v for k, v in meta.items() if k != "dtype"} == meta0
        assert all(p.dtype == torch.float32 for p in model.parameters())  # the model itself stays fp32


def test_load_align_model_refusals(tmp_path):
    from whisperx_amd import load_align_model

    good, small, hot = (str(tmp_path / n) for n in ("good", "small", "hot"))
    for d in (good, small, hot):
        os.makedirs(d)
    _save_local_model(good)
    with pytest.raises(ValueError, match="dtype must be torch.float32, torch.float16 or torch.bfloat16"):
        load_align_model("en", "cpu", model_name=good, dtype=torch.float64)
    _save_local_model(small, hidden=64)  # (one head of 64, but no LayerNorm width the kernels take)
    with pytest.raises(ValueError, match="the half route needs a model the packed encoder runs"):
        load_align_model("en", "cpu", model_name=small, dtype=torch.float16)
    load_align_model("en", "cpu", model_name=small)  # fp32: loads as ever
    name = "wav2vec2.encoder.layers.0.feed_forward.output_dense.weight"
    _save_local_model(hot, poison=name)
    with pytest.raises(ValueError, match=f"tensor '{name}' is not finite when rounded to float16"):
        load_align_model("en", "cpu", model_name=hot, dtype=torch.float16)
    load_align_model("en", "cpu", model_name=hot, dtype=torch.bfloat16)  # 1e6 is finite in bfloat16


def test_align_refuses_what_the_half_route_cannot_run():
    """A torchaudio-type model, an unknown dtype in the metadata and a model packed_supported rejects
    are ValueErrors of align() itself (before any forward), not silent fp32 runs."""
    from transformers import Wav2Vec2Config, Wav2Vec2ForCTC

    from whisperx_amd import align

    model, wavs, _ = hh.case("post")
    segs, meta = hh.transcript()
    with pytest.raises(ValueError, match="does not run torchaudio models"):
        align(segs, model, dict(meta, type="torchaudio", dtype=torch.float16), wavs[0][0], "cpu")
    with pytest.raises(ValueError, match="dtype must be"):
        align(segs, model, dict(meta, dtype=torch.int8), wavs[0][0], "cpu")
    torch.manual_seed(0)
    small = Wav2Vec2ForCTC(Wav2Vec2Config(vocab_size=hh.VOCAB, hidden_size=64, num_hidden_layers=1, num_attention_heads=1,
                                          intermediate_size=128, conv_dim=(32,) * 7)).eval()
    with pytest.raises(ValueError, match="the half route needs a model the packed encoder runs"):
        align(segs, small, dict(meta, dtype=torch.bfloat16), wavs[0][0], "cpu")

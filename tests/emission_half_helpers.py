"""Shared by the tests of the half route (float16 / bfloat16) of the packed wav2vec2 forward:
random-weight Wav2Vec2ForCTC models of both encoder families, their waveforms, the fp64
log-probabilities and what simply casting the stock model to the type costs.  Everything here is
computed once on the CPU and shared; the tests leave it unchanged.

Cases.  "post": post-norm encoder (Wav2Vec2Encoder), group-norm feature encoder, D 256 x 2
layers, 4 heads.  "stable": pre-norm encoder (Wav2Vec2EncoderStableLayerNorm), layer-norm feature
encoder with conv biases, D 1024 x 2 layers, 16 heads.  conv_dim is 128 to keep the fp64 reference
short, except in "post512", which keeps wav2vec2's 512.  The positional conv has D / 64 groups (the
packed encoder's positional-conv kernel takes 48 or 64 channels per group).

Waveforms: 0.1 randn of 8 s + 77, 5000, 400 and 250 samples: a segment of several 64-query units,
a short one, the minimum, and one the reference pads to 400 samples (alignment.py:217-224).

The rule.  ref_err_half = max |stock model cast to dtype, on the CPU - its fp64 log-probabilities|
over all segments.  The half route rounds a strict subset of what the cast model rounds (not the
waveform, layer 0's arithmetic, the positional conv, the residual stream or any encoder norm), so
every segment's log-probabilities must be within 2 x ref_err_half of fp64 (the project's factor for
such a route; a CPU emulation sits at 0.6 .. 1.1 x), and the frame argmax must equal fp64's at every
frame whose fp64 top-2 margin exceeds 4 x ref_err_half (two rows each within 2 x ref_err_half cannot
swap an order that is further apart).  The share of frames passing that filter is asserted here
(>= 3/4 in fp16, >= 1/3 in bf16), so the filter cannot hide a failure."""
import copy
import functools

import torch
import torch.nn.functional as F

DTYPES = (torch.float16, torch.bfloat16)
LENGTHS = (8 * 16000 + 77, 5000, 400, 250)
MIN_SHARE = {torch.float16: 3 / 4, torch.bfloat16: 1 / 3}
VOCAB = 32
# seeds for which the margin filter keeps MIN_SHARE of the frames (asserted in `case`)
SEEDS = {"post": 0, "stable": 0, "post512": 0}


def name(dtype) -> str:
    return str(dtype).replace("torch.", "")


def config(kind: str):
    from transformers import Wav2Vec2Config

    conv_dim = (512 if kind == "post512" else 128,) * 7
    if kind == "stable":
        return Wav2Vec2Config(vocab_size=VOCAB, hidden_size=1024, num_hidden_layers=2, num_attention_heads=16,
                              intermediate_size=4096, conv_dim=conv_dim, do_stable_layer_norm=True,
                              feat_extract_norm="layer", conv_bias=True, num_conv_pos_embedding_groups=16)
    return Wav2Vec2Config(vocab_size=VOCAB, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                          intermediate_size=1024, conv_dim=conv_dim, num_conv_pos_embedding_groups=4)


def _pad(w):
    return F.pad(w, (0, max(0, 400 - w.shape[-1])))  # alignment.py:217-224


def _log_probs(model, wavs, dtype):
    with torch.no_grad():
        return [torch.log_softmax(model(_pad(w).to(dtype)).logits[0].double(), -1) for w in wavs]


@functools.lru_cache(maxsize=None)
def case(kind: str):
    """(fp32 model in eval mode on the CPU, waveforms [1, n], fp64 log-probabilities per segment)."""
    from transformers import Wav2Vec2ForCTC

    torch.manual_seed(SEEDS[kind])
    model = Wav2Vec2ForCTC(config(kind)).eval()
    g = torch.Generator().manual_seed(1000 + SEEDS[kind])
    wavs = [0.1 * torch.randn(1, n, generator=g) for n in LENGTHS]
    ref = _log_probs(copy.deepcopy(model).double(), wavs, torch.float64)
    return model, wavs, ref


@functools.lru_cache(maxsize=None)
def ref_err_half(kind: str, dtype) -> float:
    """max |stock model cast to dtype - fp64| over the case's segments; asserts the margin filter's share."""
    model, wavs, ref = case(kind)
    got = _log_probs(copy.deepcopy(model).to(dtype), wavs, dtype)
    err = max(float((a - b).abs().max()) for a, b in zip(got, ref))
    assert err > 0
    kept = sum(int(_decided(r, err).sum()) for r in ref)
    total = sum(r.shape[0] for r in ref)
    assert kept >= MIN_SHARE[dtype] * total, (kind, name(dtype), kept, total, err)
    return err


def _decided(ref64: torch.Tensor, err: float) -> torch.Tensor:
    """Frames whose fp64 top-2 margin exceeds 4 x err."""
    top = ref64.topk(2, -1).values
    return (top[:, 0] - top[:, 1]) > 4 * err


def frames(kind: str):
    from whisperx_amd import emission

    model, wavs, _ = case(kind)
    return [emission.n_frames(int(w.shape[-1]), model) for w in wavs]


def check_rule(kind: str, dtype, rows, what: str):
    """`rows`: one [T, V] log-probability matrix per segment of the case (any device)."""
    _, _, ref = case(kind)
    err = ref_err_half(kind, dtype)
    assert len(rows) == len(ref)
    for i, (got, want) in enumerate(zip(rows, ref)):
        got = got.detach().double().cpu()
        assert got.shape == want.shape, (what, i, got.shape, want.shape)
        d = float((got - want).abs().max())
        print(f"{what} {kind} {name(dtype)} segment {i} (T {want.shape[0]}): max |got - fp64| {d:.3e}, "
              f"ref_err_half {err:.3e}, ratio {d / err:.2f}")
        assert d <= 2 * err, (what, kind, name(dtype), i, d, err)
        keep = _decided(want, err)
        assert torch.equal(got.argmax(-1)[keep], want.argmax(-1)[keep]), (what, kind, name(dtype), i)


def transcript():
    """Segments over the first 5 s of the 8 s waveform, and a dictionary over VOCAB ids."""
    letters = "abcdefghijklmnopqrstuvwxyz"
    dictionary = {c: i + 4 for i, c in enumerate(letters)}
    dictionary.update({"<pad>": 0, "|": 1})
    segs = [{"start": 0.0, "end": 2.5, "text": "hello world"}, {"start": 2.5, "end": 5.0, "text": "again here"}]
    return segs, {"language": "en", "dictionary": dictionary, "type": "huggingface"}

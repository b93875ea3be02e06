"""Shared by the Whisper tests: a random transformers WhisperEncoder as the encoder's oracle, and the
weight recipe and OpenAI renaming that the decoder's helpers (whisper_decoder_helpers) use too.

No weights are downloaded: the module is built from a tiny WhisperConfig with
max_source_positions = P and its weights are drawn here.  transformers' default 0.02 init makes
every softmax flat (a wrong scale or head split would pass), so the weights get unit-variance
fan-in scaling, the q and k projections about 3x that, biases ~0.1, and the inputs are
0.5 randn - 0.5 (the range of log-mel features).  With this recipe the logits are spread, the
outputs are O(1), and the stock fp32 route is 4e-6 to 7e-6 from fp64 on the CPU.

Tolerance rule (the mel tests'): ref_err = max|HF fp32 - HF fp64| on the same inputs, and the
code under test must be within 4 x ref_err of HF fp64.
"""
import copy
import functools

import torch


def make_encoder(D: int, layers: int, P: int, n_mels: int = 80, seed: int = 0):
    """A transformers WhisperEncoder (fp32, eval, CPU) of width D, D / 64 heads, ffn 4 D."""
    from transformers import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoder

    heads = D // 64
    cfg = WhisperConfig(d_model=D, encoder_layers=layers, encoder_attention_heads=heads, encoder_ffn_dim=4 * D,
                        num_mel_bins=n_mels, max_source_positions=P, decoder_layers=1, decoder_attention_heads=1,
                        decoder_ffn_dim=64, vocab_size=64, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                        decoder_start_token_id=1, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0,
                        encoder_layerdrop=0.0)
    return draw_weights(WhisperEncoder(cfg).eval(), seed)


def draw_weights(module, seed: int, embed_tokens_div: float = 1.0):
    """The recipe of this file's docstring on every parameter of `module`, in named_parameters()
    order from one generator, then frozen; embed_tokens.weight (the decoder's, tied to its output
    projection) is randn / embed_tokens_div.  Returns `module`."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "layer_norm" in name:  # LayerNorm gains around 1
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif name == "embed_positions.weight":
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            elif name == "embed_tokens.weight":
                p.copy_(torch.randn(p.shape, generator=g) / embed_tokens_div)
            else:
                fan_in = p[0].numel()
                scale = 3.0 if (".q_proj." in name or ".k_proj." in name) else 1.0
                p.copy_(scale * torch.randn(p.shape, generator=g) / fan_in ** 0.5)
    return module.requires_grad_(False)


def make_features(B: int, n_mels: int, frames: int, seed: int = 1) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return 0.5 * torch.randn((B, n_mels, frames), generator=g) - 0.5


@functools.lru_cache(maxsize=None)
def case(D: int, layers: int, P: int, B: int, n_mels: int = 80):
    """(encoder, features, HF fp64 output, ref_err) of one geometry, computed once on the CPU and
    shared (the tests leave all four unchanged)."""
    enc = make_encoder(D, layers, P, n_mels)
    x = make_features(B, n_mels, 2 * P)
    with torch.no_grad():
        y32 = enc(x).last_hidden_state
        y64 = copy.deepcopy(enc).double()(x.double()).last_hidden_state
    ref_err = float((y32.double() - y64).abs().max())
    return enc, x, y64, ref_err


# transformers' names inside `layers.N.` -> OpenAI's inside `blocks.N.`; the top-level names per part
_OPENAI_BLOCK = {"self_attn.q_proj": "attn.query", "self_attn.k_proj": "attn.key", "self_attn.v_proj": "attn.value",
                 "self_attn.out_proj": "attn.out", "self_attn_layer_norm": "attn_ln", "encoder_attn.q_proj": "cross_attn.query",
                 "encoder_attn.k_proj": "cross_attn.key", "encoder_attn.v_proj": "cross_attn.value",
                 "encoder_attn.out_proj": "cross_attn.out", "encoder_attn_layer_norm": "cross_attn_ln", "fc1": "mlp.0",
                 "fc2": "mlp.2", "final_layer_norm": "mlp_ln"}
_OPENAI_TOP = {"encoder": {"embed_positions.weight": "positional_embedding", "layer_norm": "ln_post", "conv1": "conv1",
                           "conv2": "conv2"},
               "decoder": {"embed_positions.weight": "positional_embedding", "layer_norm": "ln",
                           "embed_tokens": "token_embedding"}}


def openai_names(sd: dict, part: str) -> dict:
    """An HF-named state dict of `part` ("encoder" / "decoder", no prefix) under OpenAI's names
    (`<part>.blocks.N...`).  A key that OpenAI's model does not have is a KeyError."""
    top, out = _OPENAI_TOP[part], {}
    for k, v in sd.items():
        mod, leaf = k.rsplit(".", 1)
        if k.startswith("layers."):
            _, n, mod = mod.split(".", 2)
            out[f"{part}.blocks.{n}.{_OPENAI_BLOCK[mod]}.{leaf}"] = v
        else:
            out[f"{part}." + (top[k] if k in top else f"{top[mod]}.{leaf}")] = v
    return out


def stem_ref64(enc, x: torch.Tensor) -> torch.Tensor:
    """The stem in fp64 torch ops on the CPU: [B, M, Tin] -> [B, Tin / 2, D]."""
    import torch.nn.functional as F

    w1, b1, w2, b2 = (t.detach().double().cpu() for t in (enc.conv1.weight, enc.conv1.bias, enc.conv2.weight,
                                                          enc.conv2.bias))
    h = F.gelu(F.conv1d(x.double().cpu(), w1, b1, padding=1))
    h = F.gelu(F.conv1d(h, w2, b2, stride=2, padding=1))
    return h.permute(0, 2, 1) + enc.embed_positions.weight.detach().double().cpu()

"""Whisper's audio encoder and text decoder, run from their weights on the MI355X.

The audio encoder (whisperx/asr.py:77-86, WhisperModel.encode): the reference hands the log-mel
features of its 30 s windows to CTranslate2; the arithmetic is transformers'
`WhisperEncoder.forward` (fp32, eval, no mask), and that is what this module computes from the
weights alone:

    h = gelu(conv2(gelu(conv1(x)))) + pos                  wx_whisper_stem (one fused HIP stem)
    per layer:  y = LN1(h);  h = h + out(attn(q(y), k(y), v(y)))        one q/k/v GEMM, wx_attention_f32
                y = LN2(h);  h = h + fc2(gelu(fc1(y)))                   wx_add_layernorm(want_sum)
    out = LN_post(h)

The result is what `WhisperForConditionalGeneration.generate(encoder_outputs=...)` accepts, and what
`WhisperDecoder` below starts from.

Whisper's text decoder (whisperx/asr.py:31-75 generate_segment_batched, :245-257 detect_language:
the reference hands the encoder output to CTranslate2) is transformers' `WhisperDecoder.forward`
with its key / value cache, one position per step:

    h = embed_tokens[id] + embed_positions[pos]
    per layer:  h = h + out(attn(q(LN1 h), cache_k, cache_v))           wx_decode_attention_f32
                h = h + out_x(attn(q_x(LN2 h), K_x, V_x))               wx_decode_attention_f32
                h = h + fc2(gelu(fc1(LN3 h)))                           wx_add_layernorm(want_sum)
    logits = LN_f(h) . embed_tokens^T

Greedy decoding (beam_size 1, temperature 0) and language detection are built on it; beam search,
temperature fallback, timestamps and the tokenizer are not.

Without a GPU the same arithmetic runs in torch ops on the host (`F.conv1d`, `F.layer_norm`,
`F.scaled_dot_product_attention`).  Both halves read their weights through one loader (`_Half`,
`_Taker`) and run their layers as stages of one residual chain (`_chain`) on either route.
"""
from __future__ import annotations

import contextlib
import re
import weakref
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .audio import log_mel_chunks

_LN_EPS = 1e-5


# ---------------------------------------------------------------------- weights, for both halves
class _Half(NamedTuple):
    """What tells the encoder's weights from the decoder's."""
    who: str         # the class, for messages
    part: str        # `model.<part>.` / `<part>.` prefixes and module paths
    other: tuple     # key prefixes of the rest of a model, dropped from a dict without a prefix
    anchors: tuple   # a key starting with one of these (after the prefix) locates the prefix
    has: tuple       # attributes by which the module is recognised
    sniff: bool      # rename OpenAI's keys only when the dict looks like OpenAI's
    top: dict        # OpenAI's top-level keys -> transformers'
    block: dict      # OpenAI's names inside `blocks.N.` -> transformers' inside `layers.N.`
    keep: Optional[str] = None  # a key beside this half that is kept under this name


# OpenAI's names (whisper/model.py AudioEncoder, TextDecoder) -> transformers' (WhisperEncoder, WhisperDecoder)
_OPENAI_BLOCK = {"attn.query": "self_attn.q_proj", "attn.key": "self_attn.k_proj", "attn.value": "self_attn.v_proj",
                 "attn.out": "self_attn.out_proj", "attn_ln": "self_attn_layer_norm", "mlp.0": "fc1", "mlp.2": "fc2",
                 "mlp_ln": "final_layer_norm"}
_ENCODER = _Half("WhisperEncoder", "encoder", ("decoder.", "model.decoder.", "proj_out."), ("conv1.",),
                 ("conv1", "embed_positions"), True,
                 {"positional_embedding": "embed_positions.weight", "ln_post.weight": "layer_norm.weight",
                  "ln_post.bias": "layer_norm.bias"}, _OPENAI_BLOCK)
_DECODER = _Half("WhisperDecoder", "decoder", ("encoder.", "model.encoder."), ("embed_tokens.", "token_embedding."),
                 ("embed_tokens", "embed_positions"), False,
                 {"token_embedding.weight": "embed_tokens.weight", "positional_embedding": "embed_positions.weight",
                  "ln.weight": "layer_norm.weight", "ln.bias": "layer_norm.bias"},
                 {**_OPENAI_BLOCK, "cross_attn.query": "encoder_attn.q_proj", "cross_attn.key": "encoder_attn.k_proj",
                  "cross_attn.value": "encoder_attn.v_proj", "cross_attn.out": "encoder_attn.out_proj",
                  "cross_attn_ln": "encoder_attn_layer_norm"}, keep="proj_out.weight")


def _hf_names(sd: dict, half: _Half) -> dict:
    """A state dict under transformers' names of one half without a prefix: strips `model.<part>.` /
    `<part>.`, and renames OpenAI's keys.  Keys of other parts of a model drop out, but for
    `half.keep` (the decoder's `proj_out.weight`, under any of its spellings)."""
    keys = list(sd.keys())
    rename = not half.sniff or any(k.endswith("positional_embedding") or ".blocks." in k or k.startswith("blocks.")
                                   for k in keys)
    for prefix in (f"model.{half.part}.", f"{half.part}.", ""):
        if any(k.startswith(tuple(prefix + a for a in half.anchors)) for k in keys):
            break
    else:
        raise ValueError(f"{half.who}: the state dict has no {' / '.join(a + 'weight' for a in half.anchors)} (under "
                         f"'model.{half.part}.', '{half.part}.' or no prefix)")
    out = {}
    for k, v in sd.items():
        if half.keep and k in (half.keep, "model." + half.keep, prefix + half.keep):
            out[half.keep] = v
            continue
        if not k.startswith(prefix):
            continue
        k = k[len(prefix):]
        if prefix == "" and k.startswith(half.other):
            continue
        if rename:
            m = re.match(r"blocks\.(\d+)\.(.+)\.(weight|bias)$", k)
            if k in half.top:
                k = half.top[k]
            elif m and m.group(2) in half.block:
                k = f"layers.{m.group(1)}.{half.block[m.group(2)]}.{m.group(3)}"
        out[k] = v
    return out


def _state_dict(weights, half: _Half) -> dict:
    """The tensors of one half under transformers' names, from a module (which is only read) or a
    state dict."""
    if isinstance(weights, dict):
        return _hf_names(weights, half)
    if not isinstance(weights, torch.nn.Module):
        raise ValueError(f"{half.who}: weights must be a module or a state dict, not {type(weights).__name__}")
    for path in (("model", half.part), (half.part,), ()):
        mod = weights
        for name in path:
            mod = getattr(mod, name, None)
        if mod is not None and all(hasattr(mod, a) for a in half.has):
            break
    else:
        raise ValueError(f"{half.who}: the module has no Whisper {half.part} ({' / '.join(half.has)})")
    sd = dict(mod.state_dict())
    kept = getattr(getattr(weights, half.keep.split(".")[0], None), "weight", None) if half.keep else None
    if kept is not None:
        sd[half.keep] = kept
    return sd


def _device(device) -> torch.device:
    """`device`, by default the current HIP device when one is visible, else the CPU; `cuda`
    without an index is the current device."""
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class _Taker:
    """take(name, shape): tensor `name` of `sd` as contiguous fp32 on `device`, its shape checked;
    every refusal is a ValueError that names the class and the tensor."""

    def __init__(self, sd: dict, device: torch.device, who: str):
        self.sd, self.device, self.who = sd, device, who

    def __call__(self, name, shape=None):
        t = self.sd.get(name)
        if t is None:
            raise ValueError(f"{self.who}: tensor '{name}' is missing")
        t = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{self.who}: tensor '{name}' has shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t

    def pair(self, prefix: str, n_out: int, n_in: Optional[int] = None):
        """(weight, bias) of the LayerNorm (n_out) or Linear (n_out x n_in) under `prefix`."""
        return self(prefix + ".weight", (n_out,) if n_in is None else (n_out, n_in)), self(prefix + ".bias", (n_out,))

    def layer_prefixes(self) -> list:
        """`layers.N.` for every layer of `sd`; the indices must be 0 .. n - 1."""
        ids = sorted({int(m.group(1)) for m in (re.match(r"layers\.(\d+)\.", k) for k in self.sd) if m})
        if ids != list(range(len(ids))):
            raise ValueError(f"{self.who}: layer indices {ids} are not 0 .. n - 1")
        return [f"layers.{i}." for i in ids]

    def attention(self, p: str, D: int):
        """The attention block under `p`: ([Wq; Wk; Wv] and its bias with a zero block for k, which
        Whisper's k_proj does not have), (Wo, bo)."""
        if self.sd.get(p + ".k_proj.bias") is not None:
            raise ValueError(f"{self.who}: tensor '{p}.k_proj.bias' exists; Whisper's k_proj has no bias")
        wq, wk, wv = (self(p + f".{n}_proj.weight", (D, D)) for n in "qkv")
        bq, bv = self(p + ".q_proj.bias", (D,)), self(p + ".v_proj.bias", (D,))
        return (torch.cat([wq, wk, wv], 0), torch.cat([bq, torch.zeros_like(bq), bv])), self.pair(p + ".out_proj", D, D)

    def table(self, name: str, rows: str, D: int) -> torch.Tensor:
        """A [rows, D] tensor whose row count is read from it."""
        t = self(name)
        if t.dim() != 2 or t.shape[1] != D:
            raise ValueError(f"{self.who}: tensor '{name}' has shape {tuple(t.shape)}, expected [{rows}, {D}]")
        return t

    def mlp(self, p: str, D: int):
        """fc1 and fc2 under the layer prefix `p`, the ffn width read from fc1."""
        fc1 = self.table(p + "fc1.weight", "ffn", D)
        ffn = int(fc1.shape[0])
        return (fc1, self(p + "fc1.bias", (ffn,))), self.pair(p + "fc2", D, ffn)


# ----------------------------------------------------------------- the residual stream, for both
def _mlp(L: dict):
    return lambda y: F.linear(F.gelu(F.linear(y, *L["fc1"])), *L["fc2"])


def _chain(h: torch.Tensor, stages: list, final, add_norm=None) -> torch.Tensor:
    """The pre-LN residual stream: h = h + fn(LN(h)) for every stage (ln, fn), then LN_final(h).
    `ln` and `final` are (weight, bias) pairs.  With `add_norm` (_lib.add_layernorm on the HIP
    route) every add is fused with the norm after it: the first norm has no residual to add and
    is a plain layer_norm, the last add has no sum to keep."""
    D = (h.shape[-1],)
    if add_norm is None:
        for ln, fn in stages:
            h = h + fn(F.layer_norm(h, D, *ln, _LN_EPS))
        return F.layer_norm(h, D, *final, _LN_EPS)
    y = F.layer_norm(h, D, *(stages[0][0] if stages else final), _LN_EPS)
    for (_, fn), (ln, _) in zip(stages, stages[1:]):
        y, h = add_norm(h, fn(y), *ln, _LN_EPS, want_sum=True)
    return add_norm(h, stages[-1][1](y), *final, _LN_EPS) if stages else y


class WhisperEncoder:
    """Whisper's audio encoder run from its weights.

    `weights`: a transformers `WhisperEncoder`, `WhisperModel` or `WhisperForConditionalGeneration`
    module, or a state dict under transformers' names (with a `model.encoder.` / `encoder.` prefix
    or none) or OpenAI's (`encoder.blocks.N.attn.query` ...).  The geometry comes from the tensors:
    D and n_mels from conv1.weight, the layer count from the keys, P from the positional table,
    D / 64 heads.  Anything that does not fit raises ValueError naming the tensor.  The derived
    weights (packed stem weights, [Wq; Wk; Wv] with a zero bias block for k) are built once here;
    the caller's module is read, never patched.  `device`: where the weights go (default: the
    current HIP device when one is visible, else the CPU)."""

    def __init__(self, weights, device=None):
        self.device = _device(device)
        take = _Taker(_state_dict(weights, _ENCODER), self.device, "WhisperEncoder")
        w1 = take("conv1.weight")
        if w1.dim() != 3 or w1.shape[2] != 3:
            raise ValueError(f"WhisperEncoder: tensor 'conv1.weight' has shape {tuple(w1.shape)}, expected [D, n_mels, 3]")
        D, M = int(w1.shape[0]), int(w1.shape[1])
        if M not in (80, 128):
            raise ValueError(f"WhisperEncoder: tensor 'conv1.weight' has {M} input channels; n_mels must be 80 or 128")
        if D % 64 or D > 1280:
            raise ValueError(f"WhisperEncoder: tensor 'conv1.weight' has {D} output channels; the model width must be a "
                             "multiple of the head size 64, at most 1280")
        self.D, self.n_mels, self.H = D, M, D // 64
        self.w1, self.b1 = w1, take("conv1.bias", (D,))
        self.w2, self.b2 = take("conv2.weight", (D, D, 3)), take("conv2.bias", (D,))
        self.pos = take.table("embed_positions.weight", "P", D)
        self.P = int(self.pos.shape[0])
        self.layers = []
        for p in take.layer_prefixes():
            L = {"ln1": take.pair(p + "self_attn_layer_norm", D), "ln2": take.pair(p + "final_layer_norm", D)}
            L["qkv"], L["out"] = take.attention(p + "self_attn", D)
            L["fc1"], L["fc2"] = take.mlp(p, D)
            self.layers.append(L)
        self.ln_post = take.pair("layer_norm", D)
        if self.device.type == "cuda":
            self.w1_packed = _lib.pack_conv3_weight(self.w1)
            self.w2_packed = _lib.pack_conv3_weight(self.w2)

    # ------------------------------------------------------------------------------ forward
    def _features(self, features) -> torch.Tensor:
        if not torch.is_tensor(features):
            features = torch.from_numpy(np.ascontiguousarray(features))
        if features.dim() == 2:  # asr.py:82-83
            features = features.unsqueeze(0)
        if features.dim() != 3 or features.shape[1] != self.n_mels:
            raise ValueError(f"WhisperEncoder.encode: features must be [B, {self.n_mels}, {2 * self.P}], "
                             f"got {tuple(features.shape)}")
        if features.shape[2] != 2 * self.P:
            raise ValueError(f"WhisperEncoder.encode: {int(features.shape[2])} frames; this model takes exactly "
                             f"{2 * self.P} (2 x {self.P} positions)")
        return features.to(device=self.device, dtype=torch.float32)

    @torch.inference_mode()
    def encode(self, features, batch_size: int = 16) -> torch.Tensor:
        """features [B, n_mels, 2 P] (numpy or torch; 2-D: one chunk) -> the encoder's last hidden
        state [B, P, D] fp32 on the encoder's device.  Slices of `batch_size` chunks bound the
        activation memory.  Runs on the current stream."""
        x = self._features(features)
        if int(batch_size) < 1:
            raise ValueError("WhisperEncoder.encode: batch_size must be at least 1")
        B = int(x.shape[0])
        out = torch.empty((B, self.P, self.D), dtype=torch.float32, device=self.device)
        kernel = self.device.type == "cuda"
        if kernel and x.stride(2) != 1 and x.shape[2] > 1:
            x = x.contiguous()
        with torch.cuda.device(self.device) if kernel else contextlib.nullcontext():
            for a in range(0, B, int(batch_size)):
                out[a:a + int(batch_size)].copy_(self._forward(x[a:a + int(batch_size)], kernel))
        return out

    def encode_chunks(self, audio, segments, n_mels: Optional[int] = None) -> torch.Tensor:
        """encode(log_mel_chunks(audio, segments, n_mels)): from a file's waveform and its VAD chunks
        to the encoder states of every chunk, features and encoder on this encoder's device."""
        n_mels = self.n_mels if n_mels is None else int(n_mels)
        return self.encode(log_mel_chunks(audio, segments, n_mels, device=self.device))

    def stem(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The stem alone on the device: x [B, n_mels, 2 P] -> [B, P, D] (wx_whisper_stem)."""
        return _lib.whisper_stem(x, self.w1_packed, self.b1, self.w2_packed, self.b2, self.pos, out)

    def _forward_host(self, x: torch.Tensor) -> torch.Tensor:
        """The host route's arithmetic on x's device (a HIP device too: the two routes are compared there)."""
        return self._forward(x, False)

    def _forward(self, x: torch.Tensor, kernel: bool) -> torch.Tensor:
        """One slice [B, n_mels, 2 P] -> [B, P, D]: on the HIP route (stem, attention and the fused
        add-norms are kernels, the residual stream is [B P, D]) or in torch ops on x's device."""
        B, P, D, H = int(x.shape[0]), self.P, self.D, self.H
        if kernel:
            h = self.stem(x).reshape(B * P, D)

            def attend(q, k, v):
                return _lib.attention_f32(q, k, v, 0.125).reshape(B * P, D)
        else:
            h = F.gelu(F.conv1d(x, self.w1, self.b1, padding=1))
            h = F.gelu(F.conv1d(h, self.w2, self.b2, stride=2, padding=1))
            h = h.permute(0, 2, 1) + self.pos

            def attend(q, k, v):
                return F.scaled_dot_product_attention(q, k, v, scale=0.125).transpose(1, 2).reshape(B, P, D)

        def attention(y, L):
            qkv = F.linear(y, *L["qkv"])  # [..., 3D]: one GEMM
            q, k, v = (qkv[..., j * D:(j + 1) * D].view(B, P, H, 64).transpose(1, 2) for j in range(3))
            return F.linear(attend(q, k, v), *L["out"])

        stages = [s for L in self.layers for s in ((L["ln1"], lambda y, L=L: attention(y, L)), (L["ln2"], _mlp(L)))]
        return _chain(h, stages, self.ln_post, _lib.add_layernorm if kernel else None).view(B, P, D)


def _load_state_dict(path: str, who: str) -> dict:
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file

        sd = load_file(str(path))
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{who}: {path} does not hold a state dict")
    return sd


def load_whisper_encoder(path: str, device=None) -> WhisperEncoder:
    """A WhisperEncoder from a state-dict file: `.safetensors` through safetensors, anything else
    through torch.load(weights_only=True).  The file may hold a whole model; only the encoder's
    tensors are used."""
    return WhisperEncoder(_load_state_dict(path, "load_whisper_encoder"), device=device)


# ------------------------------------------------------------------------------------ decoder
class DecoderState:
    """What `WhisperDecoder.start` returns and `step` advances: per layer the cross-attention keys
    and values (`cross`: [B, P, 2D], the k half then the v half of one GEMM), the self-attention
    caches (`self_k` / `self_v`: [B, H, max_target_positions, 64]) and `pos`, the tokens so far.
    `stages`: the decoder's layers bound to these tensors, built at the first step."""

    def __init__(self, B: int, P: int, cross, self_k, self_v, kernels: bool):
        self.B, self.P, self.pos = B, P, 0
        self.cross, self.self_k, self.self_v = cross, self_k, self_v
        self.kernels = kernels
        self.stages = None


class WhisperDecoder:
    """Whisper's text decoder run from its weights, one position per step.

    `weights`: a transformers `WhisperDecoder`, `WhisperModel` or `WhisperForConditionalGeneration`
    module, or a state dict under transformers' names (with a `model.decoder.` / `decoder.` prefix
    or none) or OpenAI's (`decoder.blocks.N.attn.query`, `decoder.token_embedding` ...).  The
    geometry comes from the tensors: the vocabulary and D from embed_tokens.weight, the ffn width
    from fc1, the layer count from the keys, `max_target_positions` from the positional table,
    D / 64 heads.  Anything that does not fit raises ValueError naming the tensor.  The output
    projection is the token embedding (tied, as in both sources); a `proj_out.weight` is accepted
    only if it equals the embedding.  The derived weights ([Wq; Wk; Wv] with a zero bias block for
    k, [Wk_x; Wv_x]) are built once here; the caller's module is read, never patched.  `device`:
    where the weights go (default: the current HIP device when one is visible, else the CPU)."""

    def __init__(self, weights, device=None):
        self.device = _device(device)
        take = _Taker(_state_dict(weights, _DECODER), self.device, "WhisperDecoder")
        self.embed = take("embed_tokens.weight")
        if self.embed.dim() != 2:
            raise ValueError(f"WhisperDecoder: tensor 'embed_tokens.weight' has shape {tuple(self.embed.shape)}, expected [V, D]")
        V, D = int(self.embed.shape[0]), int(self.embed.shape[1])
        if D % 64 or D > 1280:
            raise ValueError(f"WhisperDecoder: tensor 'embed_tokens.weight' has width {D}; the model width must be a "
                             "multiple of the head size 64, at most 1280")
        self.V, self.D, self.H = V, D, D // 64
        if take.sd.get("proj_out.weight") is not None and not torch.equal(take("proj_out.weight", (V, D)), self.embed):
            raise ValueError("WhisperDecoder: tensor 'proj_out.weight' differs from embed_tokens.weight; the output "
                             "projection must be tied to the token embedding")
        self.pos = take.table("embed_positions.weight", "T", D)
        self.max_target_positions = int(self.pos.shape[0])
        self.layers = []
        for p in take.layer_prefixes():
            L = {"ln1": take.pair(p + "self_attn_layer_norm", D), "ln2": take.pair(p + "encoder_attn_layer_norm", D),
                 "ln3": take.pair(p + "final_layer_norm", D)}
            L["qkv"], L["out"] = take.attention(p + "self_attn", D)
            (w, b), L["out_x"] = take.attention(p + "encoder_attn", D)
            L["q_x"], L["kv_x"] = (w[:D], b[:D]), (w[D:], b[D:])  # q per step; [Wk_x; Wv_x] once, in start()
            L["fc1"], L["fc2"] = take.mlp(p, D)
            self.layers.append(L)
        self.ln_f = take.pair("layer_norm", D)

    # --------------------------------------------------------------------------------- steps
    def _ctx(self):
        return torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()

    @torch.inference_mode()
    def start(self, encoder_states: torch.Tensor, kernels: Optional[bool] = None) -> DecoderState:
        """encoder_states [B, P, D] (WhisperEncoder.encode's output) -> the state of a batch of B
        sequences at position 0: per layer one GEMM with [Wk_x; Wv_x] gives the cross-attention
        keys and values [B, P, 2D], which every step then reads in place, and the self-attention
        caches are allocated at [B, H, max_target_positions, 64].  `kernels`: the HIP route (the
        default on a HIP device) or the same arithmetic in torch ops on the decoder's device."""
        x = encoder_states
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[2] != self.D or x.shape[1] < 1:
            raise ValueError(f"WhisperDecoder.start: encoder_states must be [B, P, {self.D}], got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        kernels = self.device.type == "cuda" if kernels is None else bool(kernels)
        if kernels and self.device.type != "cuda":
            raise ValueError("WhisperDecoder.start: the HIP route needs the decoder on a HIP device")
        x = x.to(device=self.device, dtype=torch.float32)
        B, P = int(x.shape[0]), int(x.shape[1])
        with self._ctx():
            cross = [F.linear(x, *L["kv_x"]) for L in self.layers]
            shape = (B, self.H, self.max_target_positions, 64)
            self_k = [torch.zeros(shape, dtype=torch.float32, device=self.device) for _ in self.layers]
            self_v = [torch.zeros(shape, dtype=torch.float32, device=self.device) for _ in self.layers]
        return DecoderState(B, P, cross, self_k, self_v, kernels)

    def _tokens(self, tokens, shape, who: str) -> torch.Tensor:
        """Token ids as an int64 tensor of `shape` on the decoder's device, every id in [0, V)."""
        t = tokens if torch.is_tensor(tokens) else torch.as_tensor(tokens)
        if tuple(t.shape) != tuple(shape) or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f"WhisperDecoder.{who}: tokens must be integer ids of shape {tuple(shape)}, got "
                             f"{t.dtype} {tuple(t.shape)}")
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= self.V):
            raise ValueError(f"WhisperDecoder.{who}: token ids must lie in [0, {self.V})")
        return t.to(device=self.device, dtype=torch.int64)

    @torch.inference_mode()
    def step(self, state: DecoderState, tokens) -> torch.Tensor:
        """One position for every row: tokens [B] (ids at position state.pos) -> the logits of the
        next token [B, V] fp32, and the state moves on by one.  Runs on the current stream."""
        return self._step(state, self._tokens(tokens, (state.B,), "step"))

    def _step(self, st: DecoderState, tok: torch.Tensor) -> torch.Tensor:
        """step() on checked ids already on the device."""
        if st.pos >= self.max_target_positions:
            raise ValueError(f"WhisperDecoder.step: position {st.pos} is past max_target_positions "
                             f"({self.max_target_positions})")
        if st.stages is None:  # once per state: the step path only calls them
            st.stages = self._stages(weakref.proxy(st))  # (a proxy: the state owns its stages, not they it)
        with self._ctx():
            h = F.embedding(tok, self.embed) + self.pos[st.pos]
            y = _chain(h, st.stages, self.ln_f, _lib.add_layernorm if st.kernels else None)
            st.pos += 1
            return F.linear(y, self.embed)

    def _stages(self, st: DecoderState) -> list:
        """The three stages of every layer on the state's tensors and route, at the position the
        state is at when they are called: both attentions on wx_decode_attention_f32 or on
        torch's; the first writes the cache rows."""
        B, P, D, H = st.B, st.P, self.D, self.H
        if st.kernels:
            def attend(q, k, v, n=None):
                return _lib.decode_attention_f32(q, k, v, 0.125, L=n).view(B, D)
        else:
            def attend(q, k, v, n=None):
                return F.scaled_dot_product_attention(q.unsqueeze(2), k[:, :, :n], v[:, :, :n], scale=0.125).reshape(B, D)

        def self_attention(L, ck, cv):
            def fn(y):
                pos = st.pos
                qkv = F.linear(y, *L["qkv"])  # [B, 3D]
                q, k, v = (qkv[:, j * D:(j + 1) * D].view(B, H, 64) for j in range(3))
                ck[:, :, pos].copy_(k)
                cv[:, :, pos].copy_(v)
                return F.linear(attend(q, ck, cv, pos + 1), *L["out"])
            return fn

        def cross_attention(L, kv):
            kx, vx = (kv[:, :, j * D:(j + 1) * D].view(B, P, H, 64).transpose(1, 2) for j in range(2))  # views, in place
            return lambda y: F.linear(attend(F.linear(y, *L["q_x"]).view(B, H, 64), kx, vx), *L["out_x"])

        return [s for L, kv, ck, cv in zip(self.layers, st.cross, st.self_k, st.self_v)
                for s in ((L["ln1"], self_attention(L, ck, cv)), (L["ln2"], cross_attention(L, kv)), (L["ln3"], _mlp(L)))]

    @torch.inference_mode()
    def logits(self, encoder_states: torch.Tensor, tokens, kernels: Optional[bool] = None) -> torch.Tensor:
        """Teacher-forced logits: tokens [B, n] -> [B, n, V], entry [:, i] the logits of the token
        after tokens[:, :i + 1] (n calls to step; there is no batched prefill)."""
        st = self.start(encoder_states, kernels)
        t = tokens if torch.is_tensor(tokens) else torch.as_tensor(tokens)
        if t.dim() != 2:
            raise ValueError(f"WhisperDecoder.logits: tokens must be [B, n], got {tuple(t.shape)}")
        tok = self._tokens(t, (st.B, int(t.shape[1])), "logits")
        out = torch.empty((st.B, int(t.shape[1]), self.V), dtype=torch.float32, device=self.device)
        for i in range(int(t.shape[1])):
            out[:, i] = self._step(st, tok[:, i])
        return out

    def _id_list(self, ids, name: str) -> Optional[torch.Tensor]:
        ids = [int(i) for i in ids]
        if any(i < 0 for i in ids):
            raise ValueError(f"WhisperDecoder.generate: {name} holds a negative id (the reference's -1 stands for a "
                             "tokenizer-side list: pass the ids themselves)")
        if any(i >= self.V for i in ids):
            raise ValueError(f"WhisperDecoder.generate: {name} holds an id outside the vocabulary of {self.V}")
        return torch.tensor(sorted(set(ids)), dtype=torch.int64, device=self.device) if ids else None

    @torch.inference_mode()
    def generate(self, encoder_states: torch.Tensor, prompt, eot: int, max_length: int = 448, suppress_tokens=(),
                 suppress_at_start=(), kernels: Optional[bool] = None) -> list:
        """Greedy decoding (asr.py:53-62 at beam_size 1, temperature 0): `prompt` (a list of ids,
        the same for every row) is fed one id per step; then every step takes the argmax of the
        logits with `suppress_tokens` at -inf, and at the first generated position also
        `suppress_at_start` (suppress_blank: tokenizer.encode(" ") + [eot]).  A row stops at `eot`;
        finished rows are fed `eot` and their output ignored.  The loop ends when every row is done
        or prompt + generated ids number min(max_length, max_target_positions).  Returns the
        generated ids per row, without the prompt and without `eot`.  The completion check
        synchronises once per step."""
        prompt = [int(t) for t in prompt]
        eot = int(eot)
        if not prompt:
            raise ValueError("WhisperDecoder.generate: the prompt is empty")
        if not 0 <= eot < self.V:
            raise ValueError(f"WhisperDecoder.generate: eot {eot} is outside the vocabulary of {self.V}")
        always, first = self._id_list(suppress_tokens, "suppress_tokens"), self._id_list(suppress_at_start, "suppress_at_start")
        st = self.start(encoder_states, kernels)
        B = st.B
        ptok = self._tokens(torch.tensor(prompt).unsqueeze(0).expand(B, -1), (B, len(prompt)), "generate")
        limit = min(int(max_length), self.max_target_positions)
        if B == 0 or len(prompt) >= limit:
            return [[] for _ in range(B)]
        for i in range(len(prompt)):
            lg = self._step(st, ptok[:, i])
        done = torch.zeros(B, dtype=torch.bool, device=self.device)
        steps = []
        while True:
            if always is not None:
                lg.index_fill_(1, always, float("-inf"))
            if first is not None and not steps:
                lg.index_fill_(1, first, float("-inf"))
            nxt = torch.where(done, eot, lg.argmax(-1))
            steps.append(nxt)
            done = done | (nxt == eot)
            if len(prompt) + len(steps) >= limit or bool(done.all()):
                break
            lg = self._step(st, nxt)
        out = []
        for row in torch.stack(steps, 1).cpu().tolist():
            out.append(row[:row.index(eot)] if eot in row else row)
        return out

    @torch.inference_mode()
    def detect_language(self, encoder_states: torch.Tensor, sot: int, language_tokens,
                        kernels: Optional[bool] = None) -> torch.Tensor:
        """asr.py:245-257: one step on [sot], then softmax over the ids of `language_tokens` only
        -> probabilities [B, len(language_tokens)] on the decoder's device."""
        ids = [int(i) for i in language_tokens]
        if not ids or any(not 0 <= i < self.V for i in ids):
            raise ValueError(f"WhisperDecoder.detect_language: language_tokens must be ids in [0, {self.V})")
        st = self.start(encoder_states, kernels)
        lg = self.step(st, torch.full((st.B,), int(sot), dtype=torch.int64))
        return torch.softmax(lg[:, torch.tensor(ids, dtype=torch.int64, device=self.device)], -1)


def load_whisper_decoder(path: str, device=None) -> WhisperDecoder:
    """A WhisperDecoder from a state-dict file (as load_whisper_encoder reads it).  The file may
    hold a whole model; only the decoder's tensors are used."""
    return WhisperDecoder(_load_state_dict(path, "load_whisper_decoder"), device=device)

"""Whisper's audio encoder (whisperx/asr.py:77-86, WhisperModel.encode) on the MI355X.

The reference hands the log-mel features of its 30 s windows to CTranslate2; the arithmetic is
transformers' `WhisperEncoder.forward` (fp32, eval, no mask), and that is what this module
computes from the weights alone:

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
`F.scaled_dot_product_attention`).
"""
from __future__ import annotations

import re
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from .audio import log_mel_chunks

_LN_EPS = 1e-5

# OpenAI's names (whisper/model.py AudioEncoder) -> transformers' (WhisperEncoder)
_OPENAI_TOP = {"conv1": "conv1", "conv2": "conv2", "ln_post": "layer_norm"}
_OPENAI_BLOCK = {"attn.query": "self_attn.q_proj", "attn.key": "self_attn.k_proj", "attn.value": "self_attn.v_proj",
                 "attn.out": "self_attn.out_proj", "attn_ln": "self_attn_layer_norm", "mlp.0": "fc1", "mlp.2": "fc2",
                 "mlp_ln": "final_layer_norm"}


def _hf_names(sd: dict) -> dict:
    """A state dict under transformers' encoder names without a prefix: strips `model.encoder.` /
    `encoder.`, and renames OpenAI's keys.  Keys of other parts of a model (the decoder) drop out."""
    keys = list(sd.keys())
    openai = any(k.endswith("positional_embedding") or ".blocks." in k or k.startswith("blocks.") for k in keys)
    for prefix in ("model.encoder.", "encoder.", ""):
        if any(k.startswith(prefix + "conv1.") for k in keys):
            break
    else:
        raise ValueError("WhisperEncoder: the state dict has no conv1.weight (under 'model.encoder.', 'encoder.' or no prefix)")
    out = {}
    for k, v in sd.items():
        if not k.startswith(prefix):
            continue
        k = k[len(prefix):]
        if prefix == "" and k.startswith(("decoder.", "model.decoder.", "proj_out.")):
            continue
        if openai:
            if k == "positional_embedding":
                k = "embed_positions.weight"
            else:
                m = re.match(r"blocks\.(\d+)\.(.+)\.(weight|bias)$", k)
                if m and m.group(2) in _OPENAI_BLOCK:
                    k = f"layers.{m.group(1)}.{_OPENAI_BLOCK[m.group(2)]}.{m.group(3)}"
                else:
                    m = re.match(r"(conv1|conv2|ln_post)\.(weight|bias)$", k)
                    if m:
                        k = f"{_OPENAI_TOP[m.group(1)]}.{m.group(2)}"
        out[k] = v
    return out


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
        if isinstance(weights, torch.nn.Module):
            for path in ("model.encoder", "encoder", ""):
                mod = weights
                for name in filter(None, path.split(".")):
                    mod = getattr(mod, name, None)
                    if mod is None:
                        break
                if mod is not None and hasattr(mod, "conv1") and hasattr(mod, "embed_positions"):
                    break
            else:
                raise ValueError("WhisperEncoder: the module has no Whisper encoder (conv1 / embed_positions)")
            sd = {k: v for k, v in mod.state_dict().items()}
        elif isinstance(weights, dict):
            sd = _hf_names(weights)
        else:
            raise ValueError(f"WhisperEncoder: weights must be a module or a state dict, not {type(weights).__name__}")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

        def take(name, shape=None):
            t = sd.get(name)
            if t is None:
                raise ValueError(f"WhisperEncoder: tensor '{name}' is missing")
            t = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
            if shape is not None and tuple(t.shape) != tuple(shape):
                raise ValueError(f"WhisperEncoder: tensor '{name}' has shape {tuple(t.shape)}, expected {tuple(shape)}")
            return t

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
        self.pos = take("embed_positions.weight")
        if self.pos.dim() != 2 or self.pos.shape[1] != D:
            raise ValueError(f"WhisperEncoder: tensor 'embed_positions.weight' has shape {tuple(self.pos.shape)}, expected [P, {D}]")
        self.P = int(self.pos.shape[0])
        ids = sorted({int(m.group(1)) for m in (re.match(r"layers\.(\d+)\.", k) for k in sd) if m})
        if ids != list(range(len(ids))):
            raise ValueError(f"WhisperEncoder: layer indices {ids} are not 0 .. n - 1")
        self.layers = []
        for i in ids:
            p = f"layers.{i}."
            if sd.get(p + "self_attn.k_proj.bias") is not None:
                raise ValueError(f"WhisperEncoder: tensor '{p}self_attn.k_proj.bias' exists; Whisper's k_proj has no bias")
            fc1 = take(p + "fc1.weight")
            if fc1.dim() != 2 or fc1.shape[1] != D:
                raise ValueError(f"WhisperEncoder: tensor '{p}fc1.weight' has shape {tuple(fc1.shape)}, expected [ffn, {D}]")
            ffn = int(fc1.shape[0])
            wq, wk, wv = (take(p + f"self_attn.{n}_proj.weight", (D, D)) for n in "qkv")
            bq, bv = take(p + "self_attn.q_proj.bias", (D,)), take(p + "self_attn.v_proj.bias", (D,))
            self.layers.append({
                "ln1": (take(p + "self_attn_layer_norm.weight", (D,)), take(p + "self_attn_layer_norm.bias", (D,))),
                "qkv": (torch.cat([wq, wk, wv], 0).contiguous(), torch.cat([bq, torch.zeros_like(bq), bv]).contiguous()),
                "out": (take(p + "self_attn.out_proj.weight", (D, D)), take(p + "self_attn.out_proj.bias", (D,))),
                "ln2": (take(p + "final_layer_norm.weight", (D,)), take(p + "final_layer_norm.bias", (D,))),
                "fc1": (fc1, take(p + "fc1.bias", (ffn,))),
                "fc2": (take(p + "fc2.weight", (D, ffn)), take(p + "fc2.bias", (D,))),
            })
        self.ln_post = (take("layer_norm.weight", (D,)), take("layer_norm.bias", (D,)))
        if self.device.type == "cuda":
            from . import _lib

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
        with torch.cuda.device(self.device) if kernel else _NullCtx():
            for a in range(0, B, int(batch_size)):
                xs, o = x[a:a + int(batch_size)], out[a:a + int(batch_size)]
                if kernel:
                    self._forward_kernels(xs, o)
                else:
                    o.copy_(self._forward_host(xs))
        return out

    def encode_chunks(self, audio, segments, n_mels: Optional[int] = None) -> torch.Tensor:
        """encode(log_mel_chunks(audio, segments, n_mels)): from a file's waveform and its VAD chunks
        to the encoder states of every chunk, features and encoder on this encoder's device."""
        n_mels = self.n_mels if n_mels is None else int(n_mels)
        return self.encode(log_mel_chunks(audio, segments, n_mels, device=self.device))

    def stem(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The stem alone on the device: x [B, n_mels, 2 P] -> [B, P, D] (wx_whisper_stem)."""
        from . import _lib

        return _lib.whisper_stem(x, self.w1_packed, self.b1, self.w2_packed, self.b2, self.pos, out)

    def _forward_kernels(self, x: torch.Tensor, out: torch.Tensor) -> None:
        """One slice on the HIP route, from the weights in the manner of emission._packed_layer."""
        from . import _lib

        B, P, D, H = int(x.shape[0]), self.P, self.D, self.H
        s = self.stem(x).reshape(B * P, D)  # the residual stream
        # (the first norm has no residual to add; every later one is fused with the add before it)
        y = F.layer_norm(s, (D,), *(self.layers[0]["ln1"] if self.layers else self.ln_post), _LN_EPS)
        for i, L in enumerate(self.layers):
            qkv = F.linear(y, *L["qkv"])  # [B P, 3D]
            q, k, v = (qkv[:, j * D:(j + 1) * D].view(B, P, H, 64).transpose(1, 2) for j in range(3))
            o = _lib.attention_f32(q, k, v, 0.125).reshape(B * P, D)
            o = F.linear(o, *L["out"])
            y, s = _lib.add_layernorm(s, o, *L["ln2"], _LN_EPS, want_sum=True)
            f = F.linear(F.gelu(F.linear(y, *L["fc1"])), *L["fc2"])
            nxt = self.layers[i + 1]["ln1"] if i + 1 < len(self.layers) else self.ln_post
            if i + 1 < len(self.layers):
                y, s = _lib.add_layernorm(s, f, *nxt, _LN_EPS, want_sum=True)
            else:
                y = _lib.add_layernorm(s, f, *nxt, _LN_EPS)
        out.copy_(y.view(B, P, D))

    def _forward_host(self, x: torch.Tensor) -> torch.Tensor:
        """The same arithmetic in torch ops on x's device."""
        B, P, D, H = int(x.shape[0]), self.P, self.D, self.H
        h = F.gelu(F.conv1d(x, self.w1, self.b1, padding=1))
        h = F.gelu(F.conv1d(h, self.w2, self.b2, stride=2, padding=1))
        h = h.permute(0, 2, 1) + self.pos
        for L in self.layers:
            y = F.layer_norm(h, (D,), *L["ln1"], _LN_EPS)
            qkv = F.linear(y, *L["qkv"])
            q, k, v = (qkv[..., j * D:(j + 1) * D].view(B, P, H, 64).transpose(1, 2) for j in range(3))
            o = F.scaled_dot_product_attention(q, k, v, scale=0.125).transpose(1, 2).reshape(B, P, D)
            h = h + F.linear(o, *L["out"])
            y = F.layer_norm(h, (D,), *L["ln2"], _LN_EPS)
            h = h + F.linear(F.gelu(F.linear(y, *L["fc1"])), *L["fc2"])
        return F.layer_norm(h, (D,), *self.ln_post, _LN_EPS)


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


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
# OpenAI's names (whisper/model.py TextDecoder) -> transformers' (WhisperDecoder)
_OPENAI_DEC_TOP = {"token_embedding.weight": "embed_tokens.weight", "positional_embedding": "embed_positions.weight",
                   "ln.weight": "layer_norm.weight", "ln.bias": "layer_norm.bias"}
_OPENAI_DEC_BLOCK = {**_OPENAI_BLOCK, "cross_attn.query": "encoder_attn.q_proj", "cross_attn.key": "encoder_attn.k_proj",
                     "cross_attn.value": "encoder_attn.v_proj", "cross_attn.out": "encoder_attn.out_proj",
                     "cross_attn_ln": "encoder_attn_layer_norm"}


def _hf_decoder_names(sd: dict) -> dict:
    """A state dict under transformers' decoder names without a prefix: strips `model.decoder.` /
    `decoder.`, and renames OpenAI's keys.  Keys of other parts of a model (the encoder) drop out;
    a `proj_out.weight` beside the decoder is kept under that name."""
    keys = list(sd.keys())
    for prefix in ("model.decoder.", "decoder.", ""):
        if any(k.startswith((prefix + "embed_tokens.", prefix + "token_embedding.")) for k in keys):
            break
    else:
        raise ValueError("WhisperDecoder: the state dict has no embed_tokens.weight / token_embedding.weight (under "
                         "'model.decoder.', 'decoder.' or no prefix)")
    out = {}
    for k, v in sd.items():
        if k in ("proj_out.weight", "model.proj_out.weight", prefix + "proj_out.weight"):
            out["proj_out.weight"] = v
            continue
        if not k.startswith(prefix):
            continue
        k = k[len(prefix):]
        if prefix == "" and k.startswith(("encoder.", "model.encoder.")):
            continue
        if k in _OPENAI_DEC_TOP:
            k = _OPENAI_DEC_TOP[k]
        else:
            m = re.match(r"blocks\.(\d+)\.(.+)\.(weight|bias)$", k)
            if m and m.group(2) in _OPENAI_DEC_BLOCK:
                k = f"layers.{m.group(1)}.{_OPENAI_DEC_BLOCK[m.group(2)]}.{m.group(3)}"
        out[k] = v
    return out


class DecoderState:
    """What `WhisperDecoder.start` returns and `step` advances: per layer the cross-attention keys
    and values (`cross`: [B, P, 2D], the k half then the v half of one GEMM), the self-attention
    caches (`self_k` / `self_v`: [B, H, max_target_positions, 64]) and `pos`, the tokens so far."""

    def __init__(self, B: int, P: int, cross, self_k, self_v, kernels: bool):
        self.B, self.P, self.pos = B, P, 0
        self.cross, self.self_k, self.self_v = cross, self_k, self_v
        self.kernels = kernels


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
        if isinstance(weights, torch.nn.Module):
            for path in ("model.decoder", "decoder", ""):
                mod = weights
                for name in filter(None, path.split(".")):
                    mod = getattr(mod, name, None)
                    if mod is None:
                        break
                if mod is not None and hasattr(mod, "embed_tokens") and hasattr(mod, "embed_positions"):
                    break
            else:
                raise ValueError("WhisperDecoder: the module has no Whisper decoder (embed_tokens / embed_positions)")
            sd = {k: v for k, v in mod.state_dict().items()}
            proj = getattr(weights, "proj_out", None)
            if proj is not None and getattr(proj, "weight", None) is not None:
                sd["proj_out.weight"] = proj.weight
        elif isinstance(weights, dict):
            sd = _hf_decoder_names(weights)
        else:
            raise ValueError(f"WhisperDecoder: weights must be a module or a state dict, not {type(weights).__name__}")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

        def take(name, shape=None):
            t = sd.get(name)
            if t is None:
                raise ValueError(f"WhisperDecoder: tensor '{name}' is missing")
            t = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
            if shape is not None and tuple(t.shape) != tuple(shape):
                raise ValueError(f"WhisperDecoder: tensor '{name}' has shape {tuple(t.shape)}, expected {tuple(shape)}")
            return t

        self.embed = take("embed_tokens.weight")
        if self.embed.dim() != 2:
            raise ValueError(f"WhisperDecoder: tensor 'embed_tokens.weight' has shape {tuple(self.embed.shape)}, expected [V, D]")
        V, D = int(self.embed.shape[0]), int(self.embed.shape[1])
        if D % 64 or D > 1280:
            raise ValueError(f"WhisperDecoder: tensor 'embed_tokens.weight' has width {D}; the model width must be a "
                             "multiple of the head size 64, at most 1280")
        self.V, self.D, self.H = V, D, D // 64
        if sd.get("proj_out.weight") is not None and not torch.equal(take("proj_out.weight", (V, D)), self.embed):
            raise ValueError("WhisperDecoder: tensor 'proj_out.weight' differs from embed_tokens.weight; the output "
                             "projection must be tied to the token embedding")
        self.pos = take("embed_positions.weight")
        if self.pos.dim() != 2 or self.pos.shape[1] != D:
            raise ValueError(f"WhisperDecoder: tensor 'embed_positions.weight' has shape {tuple(self.pos.shape)}, expected [T, {D}]")
        self.max_target_positions = int(self.pos.shape[0])
        ids = sorted({int(m.group(1)) for m in (re.match(r"layers\.(\d+)\.", k) for k in sd) if m})
        if ids != list(range(len(ids))):
            raise ValueError(f"WhisperDecoder: layer indices {ids} are not 0 .. n - 1")
        self.layers = []
        for i in ids:
            p = f"layers.{i}."
            for a in ("self_attn", "encoder_attn"):
                if sd.get(p + a + ".k_proj.bias") is not None:
                    raise ValueError(f"WhisperDecoder: tensor '{p}{a}.k_proj.bias' exists; Whisper's k_proj has no bias")
            fc1 = take(p + "fc1.weight")
            if fc1.dim() != 2 or fc1.shape[1] != D:
                raise ValueError(f"WhisperDecoder: tensor '{p}fc1.weight' has shape {tuple(fc1.shape)}, expected [ffn, {D}]")
            ffn = int(fc1.shape[0])
            wq, wk, wv = (take(p + f"self_attn.{n}_proj.weight", (D, D)) for n in "qkv")
            bq, bv = take(p + "self_attn.q_proj.bias", (D,)), take(p + "self_attn.v_proj.bias", (D,))
            xk, xv = take(p + "encoder_attn.k_proj.weight", (D, D)), take(p + "encoder_attn.v_proj.weight", (D, D))
            xbv = take(p + "encoder_attn.v_proj.bias", (D,))

            def ln(name, p=p):
                return take(p + name + ".weight", (D,)), take(p + name + ".bias", (D,))

            self.layers.append({
                "ln1": ln("self_attn_layer_norm"),
                "qkv": (torch.cat([wq, wk, wv], 0).contiguous(), torch.cat([bq, torch.zeros_like(bq), bv]).contiguous()),
                "out": (take(p + "self_attn.out_proj.weight", (D, D)), take(p + "self_attn.out_proj.bias", (D,))),
                "ln2": ln("encoder_attn_layer_norm"),
                "q_x": (take(p + "encoder_attn.q_proj.weight", (D, D)), take(p + "encoder_attn.q_proj.bias", (D,))),
                "kv_x": (torch.cat([xk, xv], 0).contiguous(), torch.cat([torch.zeros_like(xbv), xbv]).contiguous()),
                "out_x": (take(p + "encoder_attn.out_proj.weight", (D, D)), take(p + "encoder_attn.out_proj.bias", (D,))),
                "ln3": ln("final_layer_norm"),
                "fc1": (fc1, take(p + "fc1.bias", (ffn,))),
                "fc2": (take(p + "fc2.weight", (D, ffn)), take(p + "fc2.bias", (D,))),
            })
        self.ln_f = (take("layer_norm.weight", (D,)), take("layer_norm.bias", (D,)))

    # --------------------------------------------------------------------------------- steps
    def _ctx(self):
        return torch.cuda.device(self.device) if self.device.type == "cuda" else _NullCtx()

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
        with self._ctx():
            h = F.embedding(tok, self.embed) + self.pos[st.pos]
            y = self._layers_kernels(st, h) if st.kernels else self._layers_host(st, h)
            st.pos += 1
            return F.linear(y, self.embed)

    def _layers_kernels(self, st: DecoderState, s: torch.Tensor) -> torch.Tensor:
        """LN_f of the residual stream after every layer, on the HIP route: both attentions on
        wx_decode_attention_f32, every residual add fused with the norm after it."""
        from . import _lib

        B, D, H, n, pos = st.B, self.D, self.H, len(self.layers), st.pos
        y = F.layer_norm(s, (D,), *(self.layers[0]["ln1"] if n else self.ln_f), _LN_EPS)
        for i, L in enumerate(self.layers):
            qkv = F.linear(y, *L["qkv"])  # [B, 3D]
            q, k, v = (qkv[:, j * D:(j + 1) * D].view(B, H, 64) for j in range(3))
            st.self_k[i][:, :, pos].copy_(k)
            st.self_v[i][:, :, pos].copy_(v)
            o = _lib.decode_attention_f32(q, st.self_k[i], st.self_v[i], 0.125, L=pos + 1).view(B, D)
            y, s = _lib.add_layernorm(s, F.linear(o, *L["out"]), *L["ln2"], _LN_EPS, want_sum=True)
            kx, vx = (st.cross[i][:, :, j * D:(j + 1) * D].view(B, st.P, H, 64).transpose(1, 2) for j in range(2))
            o = _lib.decode_attention_f32(F.linear(y, *L["q_x"]).view(B, H, 64), kx, vx, 0.125).view(B, D)
            y, s = _lib.add_layernorm(s, F.linear(o, *L["out_x"]), *L["ln3"], _LN_EPS, want_sum=True)
            f = F.linear(F.gelu(F.linear(y, *L["fc1"])), *L["fc2"])
            if i + 1 < n:
                y, s = _lib.add_layernorm(s, f, *self.layers[i + 1]["ln1"], _LN_EPS, want_sum=True)
            else:
                y = _lib.add_layernorm(s, f, *self.ln_f, _LN_EPS)
        return y

    def _layers_host(self, st: DecoderState, h: torch.Tensor) -> torch.Tensor:
        """The same arithmetic in torch ops on the state's device."""
        B, D, H, pos = st.B, self.D, self.H, st.pos
        for i, L in enumerate(self.layers):
            qkv = F.linear(F.layer_norm(h, (D,), *L["ln1"], _LN_EPS), *L["qkv"])
            q, k, v = (qkv[:, j * D:(j + 1) * D].view(B, H, 64) for j in range(3))
            st.self_k[i][:, :, pos].copy_(k)
            st.self_v[i][:, :, pos].copy_(v)
            o = F.scaled_dot_product_attention(q.unsqueeze(2), st.self_k[i][:, :, :pos + 1], st.self_v[i][:, :, :pos + 1],
                                               scale=0.125).reshape(B, D)
            h = h + F.linear(o, *L["out"])
            q = F.linear(F.layer_norm(h, (D,), *L["ln2"], _LN_EPS), *L["q_x"]).view(B, H, 1, 64)
            kx, vx = (st.cross[i][:, :, j * D:(j + 1) * D].view(B, st.P, H, 64).transpose(1, 2) for j in range(2))
            o = F.scaled_dot_product_attention(q, kx, vx, scale=0.125).reshape(B, D)
            h = h + F.linear(o, *L["out_x"])
            h = h + F.linear(F.gelu(F.linear(F.layer_norm(h, (D,), *L["ln3"], _LN_EPS), *L["fc1"])), *L["fc2"])
        return F.layer_norm(h, (D,), *self.ln_f, _LN_EPS)

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

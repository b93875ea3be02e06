"""Whisper's audio encoder (whisperx/asr.py:77-86, WhisperModel.encode) on the MI355X.

The reference hands the log-mel features of its 30 s windows to CTranslate2; the arithmetic is
transformers' `WhisperEncoder.forward` (fp32, eval, no mask), and that is what this module
computes from the weights alone:

    h = gelu(conv2(gelu(conv1(x)))) + pos                  wx_whisper_stem (one fused HIP stem)
    per layer:  y = LN1(h);  h = h + out(attn(q(y), k(y), v(y)))        one q/k/v GEMM, wx_attention_f32
                y = LN2(h);  h = h + fc2(gelu(fc1(y)))                   wx_add_layernorm(want_sum)
    out = LN_post(h)

The result is what `WhisperForConditionalGeneration.generate(encoder_outputs=...)` accepts.  The
decoder is not part of this module.  Without a GPU the same arithmetic runs in torch ops on the
host (`F.conv1d`, `F.layer_norm`, `F.scaled_dot_product_attention`).
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


def load_whisper_encoder(path: str, device=None) -> WhisperEncoder:
    """A WhisperEncoder from a state-dict file: `.safetensors` through safetensors, anything else
    through torch.load(weights_only=True).  The file may hold a whole model; only the encoder's
    tensors are used."""
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file

        sd = load_file(str(path))
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"load_whisper_encoder: {path} does not hold a state dict")
    return WhisperEncoder(sd, device=device)

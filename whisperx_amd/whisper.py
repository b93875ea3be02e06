"""Whisper's audio encoder and text decoder, run from their weights on the MI355X.

The audio encoder (whisperx/asr.py:77-86, WhisperModel.encode): the reference hands the log-mel
features of its 30 s windows to CTranslate2; the arithmetic is transformers'
`WhisperEncoder.forward` (fp32, eval, no mask), and that is what this module computes from the
weights alone:

    h = gelu(conv2(gelu(conv1(x)))) + pos                  wx_whisper_stem (one fused HIP stem)
    per layer:  y = LN1(h);  h = h + out(attn(q(y), k(y), v(y)))        one q/k/v GEMM, wx_attention_f32
                y = LN2(h);  h = h + fc2(gelu(fc1(y)))                   wx_add_layernorm(want_sum)
    out = LN_post(h)

With `dtype` float16 or bfloat16 (asr.py:262: the reference's compute_type is "float16") the GEMMs,
the GELU and the attention take and return that type, and nothing else does:

    the stem, the residual stream h, the LayerNorm parameters and the positional table stay fp32;
    every LayerNorm is computed in fp32 on the fp32 stream and its output rounded once to dtype
                                                            wx_add_layernorm_h16
    the q/k/v, out, fc1 and fc2 weights and biases are rounded once, at construction;
    attention on the slices of the q/k/v GEMM's output      wx_attention_h16
    a GEMM's output joins the stream as h + float(out); LN_post writes fp32.

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

Greedy decoding (beam_size 1, temperature 0), beam search (asr.py:301-304: beam_size 5, patience 1,
length_penalty 1 are the reference's defaults) and language detection are built on it.  In beam
search the G beams of a chunk are rows b G + g of the state; their cross-attention reads the chunk's
one K_x / V_x (wx_decode_attention_f32_grouped), and the 2G best continuations of every chunk come
from wx_beam_topk.  `prefill` runs n positions in one pass instead (the prompt of generate /
beam_search / logits with prefill=True): the same layers on [B n, D] rows, with
wx_prefill_attention_f32 for the n queries against the cache under a causal mask and against
K_x / V_x.

Sampling and the temperature fallback (asr.py:305-312: temperatures 0 .. 1, compression_ratio_threshold
2.4, log_prob_threshold -1, no_speech_threshold 0.6): `sample` decodes best_of candidates per chunk
as the rows of a `start(beams=best_of)` state, every selection one wx_sample_token launch (the mask,
the argmax or the Gumbel-max draw from a counter-based generator keyed on (seed, row, step), the
token's log-probability at temperature 1, the done / eot handling), and `decode_with_fallback` is
faster-whisper's generate_with_fallback on a batch: the chunks that fail a threshold are decoded
again at the next temperature.  `repetition_penalty` and `no_repeat_ngram_size` (asr.py:302-303)
rewrite a step's logits ahead of every one of these selections from the ids decoded so far, one
wx_penalize_logits launch on a history kept on the device (`_Penalty`).  Timestamps, the tokenizer,
condition_on_previous_text and top-k / top-p truncation are not built.

With `graph=True` (start, generate, beam_search, logits; off by default, HIP route only) a step is
one replay of a captured graph: the self-attention is wx_decode_self_attention_f32 (_h16), which
reads the position from device memory and appends the cache row itself, the positional row is an
index_select by that device position, and the graph's last node adds 1 to it.  The graph and its
static tensors are a plan the decoder keeps per (B, G, P) and hands to the next state of that shape.

With `dtype` float16 or bfloat16 the decoder runs the reference's compute type too (asr.py:262).
Rounded to dtype: the GEMMs (weights and biases once, at construction; q/k/v, out, fc1, fc2 and the
cross-attention k/v GEMM of start()), the GELU, both attentions with the self-attention caches and
the cross-attention keys and values they read (wx_decode_attention_h16, and
wx_decode_attention_h16_grouped for a chunk's beams), the token embedding (kept only as its dtype
copy: the lookup is float(embed[id]) + pos, the output projection a dtype GEMM) and so the logits,
which are the dtype GEMM's output widened to fp32.  Not rounded: the residual stream, every
LayerNorm (computed in fp32, its output rounded once: wx_add_layernorm_h16), the positional table,
the softmax statistics of the attention kernels (fp32 maxima, sums and accumulators; one rounding
on the store) and everything after the logits: the log-probabilities, the running sums and the
selection of beam search (wx_beam_topk on the fp32 logits).

Without a GPU the same arithmetic runs in torch ops on the host (`F.conv1d`, `F.layer_norm`,
`F.scaled_dot_product_attention`).  Both halves read their weights through one loader (`_Half`,
`_Taker`) and run their layers as stages of one residual chain on either route (`_run_chain`:
`_chain`, or `_chain_half` for float16 / bfloat16).  The decoder builds its stages in one place
(`_layer_stages`; the direct step, the graph step and prefill supply what "attend" means) between one
pair of ends (`_embed`, `_project`).  generate, beam_search and sample open alike (`_check_prompt`,
`_open`, `_budget`, `_feed_prompt`) and close alike (`_cut`, `_rank`); generate and sample are one
row-wise loop (`_decode_rows`) around their selection, which on a graph state goes on as one loop of
replays (`_decode_on_device`) on one `_Selection` per plan.
"""
from __future__ import annotations

import collections
import contextlib
import gc
import re
import weakref
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .audio import log_mel_chunks
from .utils import compression_ratio

_LN_EPS = 1e-5
_MAX_PLANS = 2  # graph plans a WhisperDecoder keeps (start(graph=True))
_MAX_SELECT_GRAPHS = 8  # selection graphs a plan keeps (generate's one; sample's one per eot, temperature and seed)
_MAX_BEAMS = _lib.DECODE_MAX_GROUP  # beams per chunk: the group size of wx_decode_attention_f32_grouped / wx_beam_topk


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
    every refusal is a ValueError that names the class and the tensor.  With `gemm_dtype` (float16 /
    bfloat16) the weights and biases of the Linear layers (`gemm`) come rounded to it, and one whose
    rounding is not finite is refused."""

    def __init__(self, sd: dict, device: torch.device, who: str, gemm_dtype: Optional[torch.dtype] = None):
        self.sd, self.device, self.who, self.gemm_dtype = sd, device, who, gemm_dtype

    def __call__(self, name, shape=None):
        t = self.sd.get(name)
        if t is None:
            raise ValueError(f"{self.who}: tensor '{name}' is missing")
        t = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{self.who}: tensor '{name}' has shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t

    def gemm(self, name, shape=None):
        """take(name, shape) of a Linear layer's weight or bias: in `gemm_dtype` when there is one."""
        t = self(name, shape)
        if self.gemm_dtype is None:
            return t
        r = t.to(self.gemm_dtype)
        if not bool(torch.isfinite(r).all()):
            raise ValueError(f"{self.who}: tensor '{name}' is not finite when rounded to "
                             f"{str(self.gemm_dtype).replace('torch.', '')}")
        return r

    def pair(self, prefix: str, n_out: int, n_in: Optional[int] = None):
        """(weight, bias) of the LayerNorm (n_out) or Linear (n_out x n_in) under `prefix`."""
        if n_in is None:
            return self(prefix + ".weight", (n_out,)), self(prefix + ".bias", (n_out,))
        return self.gemm(prefix + ".weight", (n_out, n_in)), self.gemm(prefix + ".bias", (n_out,))

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
        wq, wk, wv = (self.gemm(p + f".{n}_proj.weight", (D, D)) for n in "qkv")
        bq, bv = self.gemm(p + ".q_proj.bias", (D,)), self.gemm(p + ".v_proj.bias", (D,))
        return (torch.cat([wq, wk, wv], 0), torch.cat([bq, torch.zeros_like(bq), bv])), self.pair(p + ".out_proj", D, D)

    def table(self, name: str, rows: str, D: int) -> torch.Tensor:
        """A [rows, D] tensor whose row count is read from it."""
        t = self(name)
        if t.dim() != 2 or t.shape[1] != D:
            raise ValueError(f"{self.who}: tensor '{name}' has shape {tuple(t.shape)}, expected [{rows}, {D}]")
        return t

    def mlp(self, p: str, D: int):
        """fc1 and fc2 under the layer prefix `p`, the ffn width read from fc1."""
        ffn = int(self.table(p + "fc1.weight", "ffn", D).shape[0])
        return self.pair(p + "fc1", ffn, D), self.pair(p + "fc2", D, ffn)


# ----------------------------------------------------------------- the residual stream, for both
def _mlp(L: dict):
    return lambda y: F.linear(F.gelu(F.linear(y, *L["fc1"])), *L["fc2"])


def _chain(h: torch.Tensor, stages: list, final, add_norm=None, select=None) -> torch.Tensor:
    """The pre-LN residual stream: h = h + fn(LN(h)) for every stage (ln, fn), then LN_final(h).
    `ln` and `final` are (weight, bias) pairs.  With `add_norm` (_lib.add_layernorm on the HIP
    route) every add is fused with the norm after it: the first norm has no residual to add and
    is a plain layer_norm, the last add has no sum to keep.  `select` (a prefill that wants one
    position's logits) picks the rows of the stream that the last stage and the final norm run on;
    the last stage must then be row-wise (the MLP)."""
    D = (h.shape[-1],)
    if select is None:
        select = lambda t: t  # noqa: E731
    if add_norm is None:
        for i, (ln, fn) in enumerate(stages):
            if i == len(stages) - 1:
                h = select(h)
            h = h + fn(F.layer_norm(h, D, *ln, _LN_EPS))
        return F.layer_norm(h if stages else select(h), D, *final, _LN_EPS)
    y = F.layer_norm(h if stages else select(h), D, *(stages[0][0] if stages else final), _LN_EPS)
    for (_, fn), (ln, _) in zip(stages, stages[1:]):
        y, h = add_norm(h, fn(y), *ln, _LN_EPS, want_sum=True)
    return add_norm(select(h), stages[-1][1](select(y)), *final, _LN_EPS) if stages else y


def _chain_half(h: torch.Tensor, stages: list, final, dtype: torch.dtype, kernels: bool, select=None) -> torch.Tensor:
    """_chain with 16-bit stages: the stream h and every norm are fp32, a norm's output is rounded
    once to `dtype`, `fn` takes and returns `dtype`, and its result joins the stream as
    h + float(fn(y)); the final norm writes fp32.  On the HIP route the first norm and every fused
    add-norm but the last are wx_add_layernorm_h16; the last add is wx_add_layernorm on float(fn(y)).
    `select`: _chain's."""
    D = (h.shape[-1],)
    if select is None:
        select = lambda t: t  # noqa: E731
    if not kernels or not stages:
        for i, (ln, fn) in enumerate(stages):
            if i == len(stages) - 1:
                h = select(h)
            h = h + fn(F.layer_norm(h, D, *ln, _LN_EPS).to(dtype)).float()
        return F.layer_norm(h if stages else select(h), D, *final, _LN_EPS)
    y = _lib.add_layernorm_h16(h, None, *stages[0][0], _LN_EPS, dtype)
    for (_, fn), (ln, _) in zip(stages, stages[1:]):
        y, h = _lib.add_layernorm_h16(h, fn(y), *ln, _LN_EPS, dtype, want_sum=True)
    return _lib.add_layernorm(select(h), stages[-1][1](select(y)).float(), *final, _LN_EPS)


def _run_chain(h: torch.Tensor, stages: list, final, dtype: torch.dtype, kernels: bool, select=None) -> torch.Tensor:
    """The residual chain of a model of `dtype`, on the HIP route (`kernels`: the fused add-norm
    kernels) or in torch ops: _chain for float32, _chain_half for float16 / bfloat16."""
    if dtype != torch.float32:
        return _chain_half(h, stages, final, dtype, kernels, select)
    return _chain(h, stages, final, _lib.add_layernorm if kernels else None, select)


_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


class WhisperEncoder:
    """Whisper's audio encoder run from its weights.

    `weights`: a transformers `WhisperEncoder`, `WhisperModel` or `WhisperForConditionalGeneration`
    module, or a state dict under transformers' names (with a `model.encoder.` / `encoder.` prefix
    or none) or OpenAI's (`encoder.blocks.N.attn.query` ...).  The geometry comes from the tensors:
    D and n_mels from conv1.weight, the layer count from the keys, P from the positional table,
    D / 64 heads.  Anything that does not fit raises ValueError naming the tensor.  The derived
    weights (packed stem weights, [Wq; Wk; Wv] with a zero bias block for k) are built once here;
    the caller's module is read, never patched.  `device`: where the weights go (default: the
    current HIP device when one is visible, else the CPU).  `dtype`: float32 (the default), or
    float16 / bfloat16 for the half route of the module's docstring: the GEMM weights and biases are
    rounded to it here (a float16 rounding that is not finite is a ValueError naming the tensor)
    and only those copies are kept; `encode` returns fp32 either way."""

    def __init__(self, weights, device=None, dtype: torch.dtype = torch.float32):
        if dtype not in _DTYPES:
            raise ValueError(f"WhisperEncoder: dtype must be torch.float32, torch.float16 or torch.bfloat16, got {dtype!r}")
        self.device, self.dtype = _device(device), dtype
        take = _Taker(_state_dict(weights, _ENCODER), self.device, "WhisperEncoder",
                      None if dtype == torch.float32 else dtype)
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
        half = self.dtype != torch.float32
        if kernel:
            h = self.stem(x).reshape(B * P, D)
            attention_kernel = _lib.attention_h16 if half else _lib.attention_f32

            def attend(q, k, v):
                return attention_kernel(q, k, v, 0.125).reshape(B * P, D)
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
        return _run_chain(h, stages, self.ln_post, self.dtype, kernel).view(B, P, D)


def _load_state_dict(path: str, who: str) -> dict:
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file

        sd = load_file(str(path))
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{who}: {path} does not hold a state dict")
    return sd


def load_whisper_encoder(path: str, device=None, dtype: torch.dtype = torch.float32) -> WhisperEncoder:
    """A WhisperEncoder from a state-dict file: `.safetensors` through safetensors, anything else
    through torch.load(weights_only=True).  The file may hold a whole model; only the encoder's
    tensors are used.  `dtype`: WhisperEncoder's."""
    return WhisperEncoder(_load_state_dict(path, "load_whisper_encoder"), device=device, dtype=dtype)


# ------------------------------------------------------------------------------------ decoder
class Hypothesis(NamedTuple):
    """One result of WhisperDecoder.beam_search: the generated ids (no prompt, no eot), the sum of
    their log-probabilities (and eot's when the hypothesis ended on it), and
    sum_logprob / n ** length_penalty over the n scored positions."""
    ids: list
    sum_logprob: float
    score: float


class DecodingResult(NamedTuple):
    """One chunk's result of WhisperDecoder.decode_with_fallback: the chosen attempt's generated ids
    (no prompt, no eot), the sum of their log-probabilities (eot's included), that sum per scored
    position, the temperature of the attempt, the chunk's no-speech probability (None when no
    token was given), the compression ratio of its text (None without `text_of`), whether the
    silence exception made it final, and how many temperatures the chunk was decoded at."""
    ids: list
    sum_logprob: float
    avg_logprob: float
    temperature: float
    no_speech_prob: Optional[float]
    compression_ratio: Optional[float]
    is_silence: bool
    attempts: int


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
    SC'11) on numpy arrays: `counter` four broadcastable arrays of 32-bit words, `key` two words ->
    the four output words as uint64 arrays below 2^32."""
    lo32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & lo32 for c in counter)
    k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2  # (32 x 32 bits: no overflow)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & lo32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & lo32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def gumbel_uniforms(seed: int, R: int, V: int, step: int) -> np.ndarray:
    """wx_sample_token's uniforms u [R, V] fp64 for `seed` and `step` (include/wx_align.h):
    u[r][t] = ((x >> 9) + 0.5) 2^-23, x = word t & 3 of the Philox block with counter
    (t >> 2, r, low word of step, high word of step) and key (low, high word of seed)."""
    seed, step = int(seed), int(step)
    q = np.arange((V + 3) // 4, dtype=np.uint64)[None, :]
    r = np.arange(R, dtype=np.uint64)[:, None]
    words = philox4x32_10((q, r, step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    x = np.stack(np.broadcast_arrays(*words), -1).reshape(R, -1)[:, :V]
    return ((x >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def penalize_logits_host(lg: torch.Tensor, history: torch.Tensor, repetition_penalty: float,
                         no_repeat_ngram_size: int) -> torch.Tensor:
    """wx_penalize_logits' definition (include/wx_align.h) in torch ops, for the host route: lg [R, V]
    fp32 rewritten in place, history [L, R] int64 (element [i, r] id i of row r; the decoder's ids,
    all in [0, V): this route has no out-of-range id to skip).  Every history id's logit x becomes
    x rho below 0, else x / rho (a true fp32 division: the divisor is a tensor, never a host scalar
    that a backend may turn into a reciprocal), from the value read before any write, so an id that
    occurs twice is penalised once; then the ids that would complete a repeated n-gram go to -inf."""
    L, n = int(history.shape[0]), int(no_repeat_ngram_size)
    if L and repetition_penalty != 1:
        idx = history.t()
        x = lg.gather(1, idx)
        rho = torch.full_like(x, repetition_penalty)
        lg.scatter_(1, idx, torch.where(x < 0, x * rho, x / rho))  # (equal ids carry equal values)
    if n >= 1 and L >= n:
        win = history.unfold(0, n, 1)  # [L - n + 1, R, n]: window j of row r
        match = (win[:, :, :n - 1] == history[L - n + 1:].t()).all(-1)
        j, r = match.nonzero(as_tuple=True)
        lg[r, win[j, r, n - 1]] = float("-inf")
    return lg


class _Penalty:
    """The one place where generate, beam_search and sample rewrite a step's logits by
    repetition_penalty `rho` and no_repeat_ngram_size `n`: made by WhisperDecoder._penalty from the
    checked arguments (None at the defaults, and then nothing below exists), bound to a state by
    `bind`.  `hist` [max_target_positions, rows] int64 is the history, step-major as the selection's
    record is: rows [0, P0) the prompt's part (`prefix`), row P0 + i the ids fed after generated
    step i.  `counter`: element i is i, so counter[i:] is a device pointer to the count i for a
    launch outside a graph, as sample's step counter is.  On a graph state `hist` is the
    selection's own (`_Selection.for_penalty`), and hist[P0:] takes the place of its record."""

    def __init__(self, rho: float, n: int, prefix: list):
        self.rho, self.n, self.prefix, self.P0 = rho, n, prefix, len(prefix)
        self.key = (rho, n, self.P0)  # what a captured launch is bound to
        self.hist = self.counter = self.record = None
        self.kernels, self.cap = False, 0

    def bind(self, dec: "WhisperDecoder", st: "DecoderState") -> "_Penalty":
        dev, T = dec.device, dec.max_target_positions
        with dec._ctx():
            if st.graph is not None:
                plan = st.graph
                plan.selection = plan.selection or _Selection(dec, st.rows)
                self.hist = plan.selection.for_penalty()
            else:
                self.hist = torch.zeros((T, st.rows), dtype=torch.int64, device=dev)
            if self.P0:
                self.hist[:self.P0] = torch.tensor(self.prefix, dtype=torch.int64).to(dev)[:, None]
            self.counter = torch.arange(T + 1, dtype=torch.int64, device=dev)
        self.record = self.hist[self.P0:]
        self.kernels, self.cap = st.kernels, min(T, _lib.PENALTY_MAX_HISTORY)
        return self

    def apply(self, lg: torch.Tensor, i: int) -> None:
        """The logits of generated step i (i ids generated so far), rewritten in place."""
        if self.kernels:
            _lib.penalize_logits(lg, self.hist, self.counter[i:], self.P0, self.cap, self.rho, self.n)
        else:
            penalize_logits_host(lg, self.hist[:self.P0 + i], self.rho, self.n)

    def apply_counted(self, lg: torch.Tensor, count: torch.Tensor) -> None:
        """`apply` inside a captured selection: the count is the selection's, read on the device."""
        _lib.penalize_logits(lg, self.hist, count, self.P0, self.cap, self.rho, self.n)

    def append(self, i: int, ids: torch.Tensor) -> None:
        """The ids [rows] chosen at generated step i join the history (no synchronisation)."""
        self.record[i].copy_(ids)

    def follow(self, parents: torch.Tensor, i: int) -> None:
        """Row r's history before generated step i becomes row parents[r]'s, as `reorder` moves the
        caches."""
        live = self.hist[:self.P0 + i]
        live.copy_(live.index_select(1, parents))


class DecoderState:
    """What `WhisperDecoder.start` returns and `step` advances: per layer the cross-attention keys
    and values (`cross`: [B, P, 2D], the k half then the v half of one GEMM), the self-attention
    caches (`self_k` / `self_v`: [B, H, max_target_positions, 64]) and `pos`, the tokens so far.
    `stages`: the decoder's layers bound to these tensors, built at the first step.  With `G` > 1
    beams per chunk (`start(beams=G)`) there are `rows` = B G sequences, row b G + g beam g of chunk
    b: the caches are [B G, H, max_target_positions, 64] and `cross` stays [B, P, 2D], shared by a
    chunk's beams.  `cross` and the caches have the decoder's dtype.  `graph`: the _GraphPlan of a
    state from `start(graph=True)` (its tensors are the plan's; `pos` is then the host mirror of the
    plan's device position), else None."""

    def __init__(self, B: int, P: int, cross, self_k, self_v, kernels: bool, beams: int = 1):
        self.B, self.P, self.pos = B, P, 0
        self.G, self.rows = beams, B * beams
        self.cross, self.self_k, self.self_v = cross, self_k, self_v
        self.kernels = kernels
        self.stages = None
        self.graph = None


class _GraphPlan:
    """What a graph-replayed decode step owns, kept by the decoder per (B, G, P): the static tensors
    (the state's `cross` and caches, `pos_dev` int32 [1], the token buffer `tok` [rows] int64, the
    logits buffer [rows, V] fp32, the attention workspaces), the stages bound to them, and the
    captured step graph (`graph`, None until the first step).  `owner`: a weak reference to the state
    the plan is bound to; the plan is free again when that state is gone.  `selection`: the
    _Selection of generate's and sample's device-side loop, made at its first use."""

    def __init__(self, dec: "WhisperDecoder", B: int, G: int, P: int):
        dev, dt, R = dec.device, dec.dtype, B * G
        shape = (R, dec.H, dec.max_target_positions, 64)
        self.key = (B, G, P)
        self.cross = [torch.empty((B, P, 2 * dec.D), dtype=dt, device=dev) for _ in dec.layers]
        self.self_k = [torch.zeros(shape, dtype=dt, device=dev) for _ in dec.layers]
        self.self_v = [torch.zeros(shape, dtype=dt, device=dev) for _ in dec.layers]
        self.pos_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.tok = torch.zeros(R, dtype=torch.int64, device=dev)
        self.logits = torch.empty((R, dec.V), dtype=torch.float32, device=dev)
        self.ws_self = _lib.decode_attention_workspace(R, dec.H, dec.max_target_positions, dev)
        self.ws_cross = _lib.decode_attention_workspace(B, dec.H, P, dev, G if G > 1 else None)
        self.stages = None
        self.graph = None
        self.owner = lambda: None
        self.selection = None


class _Selection:
    """What the device-side selection of a plan owns, for generate and for sample: `suppress` [V]
    bool (the ids at -inf), `done` [rows] bool, `count` int64 [1] (generated steps so far:
    wx_sample_token's step counter), `record` [max_target_positions, rows] int64 (the ids of every
    step), greedy's `eot` int64 [1], and `graphs`: the captured selections, greedy's one under
    "greedy" and sample's under (eot, temperature, seed), which are arguments of its launch; at
    most _MAX_SELECT_GRAPHS in all (a penalised call's key also holds its _Penalty's).  Sample's own
    `sums` and `logprob` [rows] fp32 and its kernel's workspace `ws` are made by `for_sample` at
    sample's first use, and `history` by `for_penalty` at the first penalised call."""

    def __init__(self, dec: "WhisperDecoder", R: int):
        dev = dec.device
        self.suppress = torch.zeros(dec.V, dtype=torch.bool, device=dev)
        self.eot = torch.zeros(1, dtype=torch.int64, device=dev)
        self.done = torch.zeros(R, dtype=torch.bool, device=dev)
        self.count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.record = torch.zeros((dec.max_target_positions, R), dtype=torch.int64, device=dev)
        self.graphs = {}
        self.sums = self.logprob = self.ws = self.history = None

    def for_penalty(self) -> torch.Tensor:
        """`history`, a second record [max_target_positions, rows] int64 made at the first penalised
        call: a _Penalty's history, whose rows from the prompt's part on stand in for `record`."""
        if self.history is None:
            self.history = torch.zeros_like(self.record)
        return self.history

    def for_sample(self) -> "_Selection":
        if self.ws is None:
            R, V, dev = int(self.done.shape[0]), int(self.suppress.shape[0]), self.done.device
            self.sums = torch.zeros(R, dtype=torch.float32, device=dev)
            self.logprob = torch.zeros(R, dtype=torch.float32, device=dev)
            self.ws = _lib.sample_token_workspace(R, V, dev)
        return self


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
    where the weights go (default: the current HIP device when one is visible, else the CPU).
    `dtype`: float32 (the default: the fp32 code path, unchanged), or float16 / bfloat16 for the half
    route of the module's docstring.  The Linear layers' weights and biases and the token embedding
    are rounded to it here (a rounding that is not finite is a ValueError naming the tensor; the
    `proj_out.weight` check runs on the fp32 tensors first) and only those copies are kept; the
    positional table and the LayerNorm parameters stay fp32.  The state then holds the
    cross-attention keys and values and the self-attention caches in dtype, half the bytes.  The
    GEMMs, the GELU, the attention, the embedding and the logits are rounded; the residual stream,
    the norms, the positional table, the softmax statistics and the log-probabilities are not.
    `step` and `logits` return fp32 either way, and `generate`, `beam_search`, `reorder` and
    `detect_language` are the same algorithms."""

    def __init__(self, weights, device=None, dtype: torch.dtype = torch.float32):
        if dtype not in _DTYPES:
            raise ValueError(f"WhisperDecoder: dtype must be torch.float32, torch.float16 or torch.bfloat16, got {dtype!r}")
        self.device, self.dtype = _device(device), dtype
        half = dtype != torch.float32
        take = _Taker(_state_dict(weights, _DECODER), self.device, "WhisperDecoder", dtype if half else None)
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
        if half:  # only the rounded copy stays: the lookup and the output projection read it
            self.embed = take.gemm("embed_tokens.weight")
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
        self._plans = collections.OrderedDict()  # (B, G, P) -> _GraphPlan, least recently used first
        self.graph_captures = 0  # step graphs captured so far (one per plan)

    # --------------------------------------------------------------------------------- steps
    def _ctx(self):
        return torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()

    @torch.inference_mode()
    def start(self, encoder_states: torch.Tensor, kernels: Optional[bool] = None, beams: int = 1,
              graph: bool = False) -> DecoderState:
        """encoder_states [B, P, D] (WhisperEncoder.encode's output) -> the state of a batch of B
        sequences at position 0: per layer one GEMM with [Wk_x; Wv_x] gives the cross-attention
        keys and values [B, P, 2D], which every step then reads in place, and the self-attention
        caches are allocated at [B, H, max_target_positions, 64].  `kernels`: the HIP route (the
        default on a HIP device) or the same arithmetic in torch ops on the decoder's device.
        `beams` = G > 1: B G sequences, G per chunk (row b G + g), for beam search: the caches
        have B G rows, the cross-attention keys and values stay [B, P, 2D] and a chunk's G beams
        read them through wx_decode_attention_f32_grouped (an expanded view on the host route).
        `graph`: every `step` of the state is one replay of a captured graph (HIP route only, else
        ValueError; both dtypes, any `beams`).  The state's tensors are then those of a plan that
        the decoder keeps per (B, G, P), at most two plans, the least recently used dropped first:
        a start of a known shape refills the plan's cross-attention tensors and resets its device
        position, and nothing is captured again (`graph_captures` counts the step graphs captured
        so far).  The caches are not cleared: rows at and above the position are never read.  A
        plan is bound to one live state: while that state exists, a start of its shape builds
        another plan, which takes the first one's place in the decoder's list (the first lives on
        with its state).  `release_graphs()` drops the decoder's plans."""
        beams = int(beams)
        if not 1 <= beams <= _MAX_BEAMS:
            raise ValueError(f"WhisperDecoder.start: beams must lie in 1..{_MAX_BEAMS}, got {beams}")
        x = encoder_states
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[2] != self.D or x.shape[1] < 1:
            raise ValueError(f"WhisperDecoder.start: encoder_states must be [B, P, {self.D}], got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        kernels = self.device.type == "cuda" if kernels is None else bool(kernels)
        if kernels and self.device.type != "cuda":
            raise ValueError("WhisperDecoder.start: the HIP route needs the decoder on a HIP device")
        if graph and not kernels:
            raise ValueError("WhisperDecoder.start: graph=True replays HIP kernels and needs the HIP route; this state "
                             f"is on the torch route (kernels=False, decoder on '{self.device}')")
        x = x.to(device=self.device, dtype=self.dtype)
        B, P = int(x.shape[0]), int(x.shape[1])
        if graph:
            return self._start_graph(x, B, P, beams)
        with self._ctx():
            cross = [F.linear(x, *L["kv_x"]) for L in self.layers]
            shape = (B * beams, self.H, self.max_target_positions, 64)
            self_k = [torch.zeros(shape, dtype=self.dtype, device=self.device) for _ in self.layers]
            self_v = [torch.zeros(shape, dtype=self.dtype, device=self.device) for _ in self.layers]
        return DecoderState(B, P, cross, self_k, self_v, kernels, beams)

    def _start_graph(self, x: torch.Tensor, B: int, P: int, G: int) -> DecoderState:
        """start(graph=True) on the checked encoder states: a free plan of this shape, or a new one."""
        key = (B, G, P)
        with self._ctx():
            plan = self._plans.get(key)
            if plan is None or plan.owner() is not None:
                plan = self._plans[key] = _GraphPlan(self, B, G, P)
            self._plans.move_to_end(key)
            while len(self._plans) > _MAX_PLANS:
                self._plans.popitem(last=False)
            for c, L in zip(plan.cross, self.layers):
                c.copy_(F.linear(x, *L["kv_x"]))
            plan.pos_dev.zero_()
        st = DecoderState(B, P, plan.cross, plan.self_k, plan.self_v, True, G)
        st.graph, plan.owner = plan, weakref.ref(st)
        return st

    def release_graphs(self) -> None:
        """Drops the plans the decoder keeps for `start(graph=True)`: their tensors and graphs are
        freed once no state uses them.  A later start captures again."""
        self._plans.clear()

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
        """One position for every row: tokens [B] (ids at position state.pos; [B G] for a state of
        G beams) -> the logits of the next token [B, V] fp32 ([B G, V]), and the state moves on by
        one.  Runs on the current stream.  On a state from `start(graph=True)` the first step
        runs the step's kernels directly (twice, as a warm-up: without the position's increment the
        step only rewrites cache row `pos` with the same values) and captures them as one linear
        graph whose last node adds 1 to the device position; that step and every later one is a
        copy of `tokens` into the plan's token buffer and one replay.  It returns the plan's logits
        buffer, which is valid until the next step of the state."""
        return self._step(state, self._tokens(tokens, (state.rows,), "step"))

    def _step(self, st: DecoderState, tok: torch.Tensor) -> torch.Tensor:
        """step() on checked ids already on the device."""
        if st.pos >= self.max_target_positions:
            raise ValueError(f"WhisperDecoder.step: position {st.pos} is past max_target_positions "
                             f"({self.max_target_positions})")
        if st.graph is not None:
            return self._graph_step(st, tok)
        if st.stages is None:  # once per state: the step path only calls them
            st.stages = self._stages(weakref.proxy(st))  # (a proxy: the state owns its stages, not they it)
        with self._ctx():
            y = _run_chain(self._embed(tok, self.pos[st.pos]), st.stages, self.ln_f, self.dtype, st.kernels)
            st.pos += 1
            return self._project(y)

    def _embed(self, tok: torch.Tensor, pos_rows: torch.Tensor) -> torch.Tensor:
        """Ids and the rows of the positional table at their positions -> the fp32 stream: the
        embedding's rows (widened, on a float16 / bfloat16 decoder) + pos_rows."""
        return F.embedding(tok, self.embed).float() + pos_rows

    def _project(self, y: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The final norm's output -> the fp32 logits (into `out`, when given): the tied output
        projection as a GEMM in the decoder's dtype, its result widened."""
        lg = F.linear(y.to(self.dtype), self.embed)
        return lg.float() if out is None else out.copy_(lg)

    def _graph_step(self, st: DecoderState, tok: Optional[torch.Tensor]) -> torch.Tensor:
        """_step on a graph state (the position already checked on the host mirror): the ids into
        the plan's token buffer (None: they are there), then one replay."""
        plan = st.graph
        with self._ctx():
            if tok is not None:
                plan.tok.copy_(tok)
            if plan.graph is None:
                self._capture(plan)
            plan.graph.replay()
        st.pos += 1
        return plan.logits

    def _graph_body(self, plan: _GraphPlan) -> None:
        """One step on the plan's tensors at the position in plan.pos_dev, which it leaves as it
        is: _step's arithmetic, the position read on the device."""
        h = self._embed(plan.tok, self.pos.index_select(0, plan.pos_dev))
        self._project(_run_chain(h, plan.stages, self.ln_f, self.dtype, True), out=plan.logits)

    @staticmethod
    @contextlib.contextmanager
    def _capturing(g):
        """torch.cuda.graph(g) with Python's cyclic collector run before it and held off during it:
        a graph object that the collector frees while a stream is capturing (one left in a dead
        reference cycle by anyone) makes a HIP call that is illegal then, and its destructor ends
        the process."""
        gc.collect()
        was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g):
                yield
        finally:
            if was_on:
                gc.enable()

    def _captured(self, body, warm=None, state=()):
        """`body` as a captured graph, one linear chain on the capture stream.  `warm` (by default
        `body`) runs once before on a side stream, ordered after and before the current one: what
        torch asks for before a capture (libraries initialised, kernels loaded); its effects on
        the tensors `state` are undone."""
        keep = [t.clone() for t in state]
        cur, side = torch.cuda.current_stream(self.device), torch.cuda.Stream(self.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            (warm or body)()
        cur.wait_stream(side)
        for t, k in zip(state, keep):
            t.copy_(k)
        g = torch.cuda.CUDAGraph()
        with self._capturing(g):
            body()
        return g

    def _capture(self, plan: _GraphPlan) -> None:
        """The plan's step graph: body, then pos_dev += 1.  The warm-up is the body twice: without
        the increment it only rewrites cache row `pos` with the same values."""
        if plan.stages is None:  # (a proxy: the plan owns its stages, not they it, so it dies by reference count)
            plan.stages = self._graph_stages(weakref.proxy(plan))
        plan.graph = self._captured(lambda: (self._graph_body(plan), plan.pos_dev.add_(1)),
                                    warm=lambda: (self._graph_body(plan), self._graph_body(plan)))
        self.graph_captures += 1

    def _layer_stages(self, cross, self_k, self_v, B: int, P: int, attend_self, attend_cross) -> list:
        """The three stages (ln, fn) of every layer on a state's or a plan's tensors, for _run_chain.
        What "attend" means is the caller's: attend_self(q, k, v, ck, cv) on the [rows, H, 64] thirds
        of the q/k/v GEMM's output and the layer's caches, attend_cross(q, kx, vx) on the q GEMM's
        output [rows, D] and the layer's [B, H, P, 64] views of `cross`; both return [rows, D]."""
        D, H = self.D, self.H

        def self_attention(L, ck, cv):
            def fn(y):
                q, k, v = F.linear(y, *L["qkv"]).view(-1, 3, H, 64).unbind(1)  # one GEMM, [rows, 3D]
                return F.linear(attend_self(q, k, v, ck, cv), *L["out"])
            return fn

        def cross_attention(L, kv):
            kx, vx = (kv[:, :, j * D:(j + 1) * D].view(B, P, H, 64).transpose(1, 2) for j in range(2))  # views, in place
            return lambda y: F.linear(attend_cross(F.linear(y, *L["q_x"]), kx, vx), *L["out_x"])

        return [s for L, kv, ck, cv in zip(self.layers, cross, self_k, self_v)
                for s in ((L["ln1"], self_attention(L, ck, cv)), (L["ln2"], cross_attention(L, kv)), (L["ln3"], _mlp(L)))]

    def _cross_kernel(self, B: int, G: int, workspace: Optional[torch.Tensor] = None):
        """_layer_stages' attend_cross of one position on the HIP route: wx_decode_attention_f32
        (_h16) on the B rows, or its grouped form on a chunk's G beams and the chunk's one K / V."""
        R, D, H = B * G, self.D, self.H
        half = self.dtype != torch.float32
        if G == 1:
            one = _lib.decode_attention_h16 if half else _lib.decode_attention_f32
            return lambda q, kx, vx: one(q.view(R, H, 64), kx, vx, 0.125, workspace=workspace).view(R, D)
        grouped = _lib.decode_attention_h16_grouped if half else _lib.decode_attention_f32_grouped
        return lambda q, kx, vx: grouped(q.view(B, G, H, 64), kx, vx, 0.125, workspace=workspace).view(R, D)

    def _graph_stages(self, plan: _GraphPlan) -> list:
        """_stages on a plan's tensors for the graph: the self-attention is one call of
        wx_decode_self_attention_f32 (_h16), which reads the position on the device and appends the
        cache row itself; the cross-attention is _stages' (its L = P is a constant).  Every call
        uses the plan's workspaces."""
        B, G, P = plan.key
        R, D = B * G, self.D
        fused = _lib.decode_self_attention_f32 if self.dtype == torch.float32 else _lib.decode_self_attention_h16

        def attend_self(q, k, v, ck, cv):
            return fused(q, k, v, ck, cv, plan.pos_dev, 0.125, workspace=plan.ws_self).view(R, D)

        return self._layer_stages(plan.cross, plan.self_k, plan.self_v, B, P, attend_self,
                                  self._cross_kernel(B, G, plan.ws_cross))

    def _stages(self, st: DecoderState) -> list:
        """_layer_stages on the state's tensors and route, at the position the state is at when they
        are called: the self-attention writes the cache rows and runs over the R = B G rows, the
        cross-attention of a chunk's G beams reads the chunk's one K / V; wx_decode_attention_f32
        (_h16) and _cross_kernel, or torch's attention (on a view expanded over the beams) in the
        decoder's dtype."""
        B, G, R, P, D, H = st.B, st.G, st.rows, st.P, self.D, self.H
        if st.kernels:
            one = _lib.decode_attention_f32 if self.dtype == torch.float32 else _lib.decode_attention_h16
            attend_cross = self._cross_kernel(B, G)

            def attend(q, ck, cv, n):
                return one(q, ck, cv, 0.125, L=n).view(R, D)
        else:
            def attend(q, ck, cv, n):
                return F.scaled_dot_product_attention(q.unsqueeze(2), ck[:, :, :n], cv[:, :, :n], scale=0.125).reshape(R, D)

            def attend_cross(q, kx, vx):
                if G == 1:
                    return F.scaled_dot_product_attention(q.view(R, H, 1, 64), kx, vx, scale=0.125).reshape(R, D)
                kx, vx = (t.unsqueeze(1).expand(B, G, H, P, 64) for t in (kx, vx))  # views, stride 0 over the beams
                return F.scaled_dot_product_attention(q.view(B, G, H, 1, 64), kx, vx, scale=0.125).reshape(R, D)

        def attend_self(q, k, v, ck, cv):
            pos = st.pos
            ck[:, :, pos].copy_(k)
            cv[:, :, pos].copy_(v)
            return attend(q, ck, cv, pos + 1)

        return self._layer_stages(st.cross, st.self_k, st.self_v, B, P, attend_self, attend_cross)

    @torch.inference_mode()
    def prefill(self, state: DecoderState, tokens, all_positions: bool = False) -> torch.Tensor:
        """n positions for every chunk in one pass: tokens [B, n] (ids at positions state.pos ..
        state.pos + n - 1, one row per chunk) -> the fp32 logits after the last of them as
        [state.rows, V] (step's contract; for a state of G beams a chunk's row repeated over its
        beams), or with `all_positions` the logits after every one of them as [B, n, V]; the state
        moves on by n.  Per layer: one q/k/v GEMM on the B n rows, the k and v rows written into
        the cache at their positions, wx_prefill_attention_f32 on the cache under the causal mask
        (query i sees positions 0 .. state.pos + i), and again without a mask on the
        cross-attention keys and values in place; the norms and the MLP on B n rows; the last MLP,
        the final norm and the logits GEMM on the last position's rows only, unless
        `all_positions`.  A float16 / bfloat16 decoder takes wx_prefill_attention_h16 and rounds
        where step rounds.  The host route runs the same structure on torch's attention with a
        boolean mask.  G = 1: any state.pos with state.pos + n <= max_target_positions (prefill in
        pieces and prefill after steps are both legal).  G > 1: state.pos must be 0; a chunk's
        beams are identical during the prompt, so the B chunks are computed through the caches'
        [::G] rows, which are then copied to the chunk's other G - 1 beams.  The GEMMs run at
        another row count than step's, so the logits agree with n steps to rounding, not bit for
        bit.  On a state from `start(graph=True)` prefill runs directly, as on any other, and the
        plan's device position is then set to the new state.pos.  Runs on the current stream."""
        t = tokens if torch.is_tensor(tokens) else torch.as_tensor(tokens)
        if t.dim() != 2 or int(t.shape[1]) < 1:
            raise ValueError(f"WhisperDecoder.prefill: tokens must be [B, n] with n >= 1, got {tuple(t.shape)}")
        return self._prefill(state, self._tokens(t, (state.B, int(t.shape[1])), "prefill"), bool(all_positions))

    def _prefill(self, st: DecoderState, tok: torch.Tensor, all_positions: bool, identical: bool = False) -> torch.Tensor:
        """prefill() on checked ids [B, n] (n >= 1) already on the device.  `identical`: the caller
        vouches that a chunk's beams hold the same rows below state.pos (a prompt fed in pieces), so
        a state of G beams may be prefilled there too."""
        B, G, P, D, H, pos, n = st.B, st.G, st.P, self.D, self.H, st.pos, int(tok.shape[1])
        if pos + n > self.max_target_positions:
            raise ValueError(f"WhisperDecoder.prefill: positions {pos} .. {pos + n - 1} run past max_target_positions "
                             f"({self.max_target_positions})")
        if G > 1 and pos != 0 and not identical:
            raise ValueError(f"WhisperDecoder.prefill: a state of {G} beams is prefilled at position 0 only (its beams "
                             f"differ from position {pos} on)")
        half = self.dtype != torch.float32
        if st.kernels:
            kernel = _lib.prefill_attention_h16 if half else _lib.prefill_attention_f32

            def attend(q, k, v, causal=None, Tk=None):
                return kernel(q, k, v, 0.125, causal=causal, Tk=Tk).view(B * n, D)
        else:
            def attend(q, k, v, causal=None, Tk=None):
                mask = None
                if causal is not None:  # query i at position causal + i sees keys 0 .. causal + i
                    mask = torch.arange(Tk, device=q.device)[None, :] <= causal + torch.arange(n, device=q.device)[:, None]
                o = F.scaled_dot_product_attention(q, k[:, :, :Tk], v[:, :, :Tk], attn_mask=mask, scale=0.125)
                return o.transpose(1, 2).reshape(B * n, D)

        def attend_self(q, k, v, ck, cv):
            ck, cv = ck[::G], cv[::G]  # one row per chunk: views, in place
            q, k, v = (t.view(B, n, H, 64).transpose(1, 2) for t in (q, k, v))  # [B, H, n, 64] views
            ck[:, :, pos:pos + n].copy_(k)
            cv[:, :, pos:pos + n].copy_(v)
            return attend(q, ck, cv, pos, pos + n)

        def attend_cross(q, kx, vx):
            return attend(q.view(B, n, H, 64).transpose(1, 2), kx, vx)

        stages = self._layer_stages(st.cross, st.self_k, st.self_v, B, P, attend_self, attend_cross)
        select = None if all_positions else (lambda t: t.view(B, n, t.shape[-1])[:, n - 1])
        with self._ctx():
            h = self._embed(tok, self.pos[pos:pos + n]).view(B * n, D)
            lg = self._project(_run_chain(h, stages, self.ln_f, self.dtype, st.kernels, select))
            if G > 1:  # the chunk's rows to its other beams
                for cache in (*st.self_k, *st.self_v):
                    rows = cache.view(B, G, H, self.max_target_positions, 64)[:, :, :, pos:pos + n]
                    rows[:, 1:].copy_(rows[:, :1].expand(B, G - 1, H, n, 64))
            st.pos += n
            if st.graph is not None:  # the device position follows the host mirror
                st.graph.pos_dev.fill_(st.pos)
            if all_positions:
                return lg.view(B, n, self.V)
            return lg.repeat_interleave(G, 0) if G > 1 else lg

    @torch.inference_mode()
    def reorder(self, state: DecoderState, parents) -> None:
        """Row r of every self-attention cache (positions < state.pos) becomes row parents[r]:
        `parents` are B G int64 ids in [0, B G), the rows the new beams continue.  A copy in place
        (a gather, then a copy back: 2 x 2 x layers x B G x state.pos x D x 4 bytes read and as many
        written); the stages stay bound to the same tensors.  The identity is a no-op."""
        t = parents if torch.is_tensor(parents) else torch.as_tensor(parents)
        if tuple(t.shape) != (state.rows,) or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f"WhisperDecoder.reorder: parents must be {state.rows} integer row ids, got {t.dtype} "
                             f"{tuple(t.shape)}")
        host = t.cpu().tolist()
        if any(not 0 <= p < state.rows for p in host):
            raise ValueError(f"WhisperDecoder.reorder: parents must lie in [0, {state.rows})")
        if host == list(range(state.rows)) or state.pos == 0:
            return
        idx = t.to(device=self.device, dtype=torch.int64)
        with self._ctx():
            for cache in (*state.self_k, *state.self_v):
                live = cache[:, :, :state.pos]
                live.copy_(live.index_select(0, idx))

    @torch.inference_mode()
    def logits(self, encoder_states: torch.Tensor, tokens, kernels: Optional[bool] = None,
               prefill: bool = False, graph: bool = False) -> torch.Tensor:
        """Teacher-forced logits: tokens [B, n] -> [B, n, V], entry [:, i] the logits of the token
        after tokens[:, :i + 1]: n calls to step, or with `prefill` one call to
        prefill(all_positions=True).  `prefill` is off by default: its GEMMs run on B n rows and
        need not round as the stepwise ones do, and generate's tokens are pinned to the argmax of
        this method's stepwise output exactly.  `graph`: the steps are replays (start's `graph`)."""
        st = self.start(encoder_states, kernels, graph=graph)
        t = tokens if torch.is_tensor(tokens) else torch.as_tensor(tokens)
        if t.dim() != 2:
            raise ValueError(f"WhisperDecoder.logits: tokens must be [B, n], got {tuple(t.shape)}")
        tok = self._tokens(t, (st.B, int(t.shape[1])), "logits")
        if prefill and int(t.shape[1]) >= 1:
            return self._prefill(st, tok, True)
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
                 suppress_at_start=(), kernels: Optional[bool] = None, beam_size: int = 1, patience: float = 1.0,
                 length_penalty: float = 1.0, prefill: bool = False, graph: bool = False, sync_every: int = 8,
                 repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                 history_from: Optional[int] = None) -> list:
        """Greedy decoding (asr.py:53-62 at beam_size 1, temperature 0): `prompt` (a list of ids,
        the same for every row) is fed one id per step; then every step takes the argmax of the
        logits with `suppress_tokens` at -inf, and at the first generated position also
        `suppress_at_start` (suppress_blank: tokenizer.encode(" ") + [eot]).  A row stops at `eot`;
        finished rows are fed `eot` and their output ignored.  The loop ends when every row is done
        or prompt + generated ids number min(max_length, max_target_positions).  Returns the
        generated ids per row, without the prompt and without `eot`.  The completion check
        synchronises once per step.  `beam_size` > 1: the ids of beam_search's best hypothesis of
        every row (`patience` and `length_penalty` are beam_search's; greedy decoding ignores them).
        `prefill`: the prompt goes through one call to prefill instead of one step per id.  Off by
        default: prefill's GEMMs run at another row count and need not round as the stepwise ones
        do, so the default keeps the tokens it gives today, bit for bit.  `graph` (HIP route only):
        every step is a replay of start's captured graph; the prompt goes through replays too, or
        through an ordinary prefill.  The first selection runs as above; from then on the masking,
        the argmax, the `done` update, the write of the ids into the step's token buffer and their
        recording run on the device in a second small graph of the plan, and the host asks whether
        every row is done only every `sync_every` generated steps (and never replays at a position
        >= min(max_length, max_target_positions)).  Steps taken after every row finished feed
        `eot` and are discarded, so the result equals graph=False token for token.

        `repetition_penalty` rho and `no_repeat_ngram_size` n (asr.py:302-303; faster-whisper hands
        both to every pass): before the masks, every step's logits are rewritten from the row's
        history by wx_penalize_logits' definition (include/wx_align.h; the same in torch ops on
        the host route).  Every distinct id of the history has its logit x replaced by x rho
        below 0 and x / rho otherwise, and with n >= 1 every id that would complete an n-gram the
        history already holds goes to -inf.  The argmax, and in `sample` and `beam_search` the
        draw, the log-probabilities and the sums, are those of the rewritten logits.  A row whose
        logits are then all -inf ends as if it had chosen `eot`.  The history of a row is
        prompt[history_from:] followed by its generated ids; `history_from` None (the default)
        means the generated ids alone, 0 the whole prompt as transformers' generate counts it,
        and any Python index into the prompt is accepted.  Which of the start ids CTranslate2
        counts could not be checked against it (it is not a dependency of this package), so the
        choice is the caller's.  At rho 1 and n 0 nothing is launched or allocated and the result is
        bit for bit the unpenalised one.  On a graph state the rewrite is one more kernel of the
        captured selection, reading the history's length from the selection's device counter."""
        if int(sync_every) < 1:
            raise ValueError(f"WhisperDecoder.generate: sync_every must be at least 1, got {sync_every}")
        if int(beam_size) != 1:
            hyps = self.beam_search(encoder_states, prompt, eot, beam_size, patience, length_penalty, max_length,
                                    suppress_tokens, suppress_at_start, kernels, prefill, graph, repetition_penalty,
                                    no_repeat_ngram_size, history_from)
            return [h[0].ids if h else [] for h in hyps]
        prompt, eot = [int(t) for t in prompt], int(eot)
        self._check_prompt("generate", prompt, eot)
        pen = self._penalty("generate", prompt, max_length, repetition_penalty, no_repeat_ngram_size, history_from)
        always, first, st = self._open(encoder_states, suppress_tokens, suppress_at_start, kernels, 1, graph)
        ptok = self._prompt_rows(st, prompt, "generate")
        budget = self._budget(st, prompt, max_length)
        if not budget:
            return [[] for _ in range(st.B)]
        lg, _ = self._feed_prompt(st, ptok, prefill)
        if pen is not None:
            pen.bind(self, st)

        def select(lg, n, done):
            if pen is not None:
                pen.apply(lg, n)
            if always is not None:
                lg.index_fill_(1, always, float("-inf"))
            if first is not None and not n:
                lg.index_fill_(1, first, float("-inf"))
            best = lg.argmax(-1)
            if pen is not None:  # (a row with nothing left ends)
                done = done | (lg.gather(1, best[:, None])[:, 0] == float("-inf"))
            nxt = torch.where(done, eot, best)
            if pen is not None:
                pen.append(n, nxt)
            return nxt, done | (nxt == eot)

        def fill(sel):
            sel.suppress.zero_()
            if always is not None:
                sel.suppress.index_fill_(0, always, True)
            sel.eot.fill_(eot)

        key = "greedy" if pen is None else ("greedy", *pen.key)
        rows = self._decode_rows(st, lg, budget, select, int(sync_every), key, lambda plan: self._select_body(plan, pen),
                                 fill, None, pen)
        return [self._cut(row, eot) for row in rows]

    # --------------------------------------------------- what generate, beam_search and sample share
    def _check_prompt(self, who: str, prompt: list, eot: int) -> None:
        if not prompt:
            raise ValueError(f"WhisperDecoder.{who}: the prompt is empty")
        if not 0 <= eot < self.V:
            raise ValueError(f"WhisperDecoder.{who}: eot {eot} is outside the vocabulary of {self.V}")

    def _penalty(self, who: str, prompt: list, max_length, repetition_penalty, no_repeat_ngram_size,
                 history_from) -> Optional[_Penalty]:
        """The checked repetition_penalty / no_repeat_ngram_size / history_from of a decoding call
        (generate's docstring) as a _Penalty still to be bound, or None when they change nothing."""
        with np.errstate(over="ignore"):
            rho = float(np.float32(repetition_penalty))  # the value the kernel is handed
        if not (rho > 0 and rho != float("inf")):
            raise ValueError(f"WhisperDecoder.{who}: repetition_penalty must be finite and positive (in fp32), got "
                             f"{repetition_penalty}")
        n = no_repeat_ngram_size
        if isinstance(n, bool) or int(n) != n or int(n) < 0 or int(n) >= 1 << 31:
            raise ValueError(f"WhisperDecoder.{who}: no_repeat_ngram_size must be an integer of at least 0, got {n}")
        if history_from is not None and not -len(prompt) <= int(history_from) <= len(prompt):
            raise ValueError(f"WhisperDecoder.{who}: history_from {history_from} is no index into the prompt of "
                             f"{len(prompt)} ids")
        if rho == 1 and int(n) == 0:
            return None
        prefix = [] if history_from is None else prompt[int(history_from):]
        longest = len(prefix) + max(0, min(int(max_length), self.max_target_positions) - len(prompt))
        if longest > _lib.PENALTY_MAX_HISTORY:
            raise ValueError(f"WhisperDecoder.{who}: history_from {history_from} and max_length {max_length} allow a "
                             f"history of {longest} ids, more than the {_lib.PENALTY_MAX_HISTORY} the penalty reads")
        return _Penalty(rho, int(n), prefix)

    def _open(self, encoder_states, suppress_tokens, suppress_at_start, kernels, beams: int, graph):
        """-> (the ids of `suppress_tokens` and of `suppress_at_start` on the device or None, the
        state of `start(beams=beams)`): what a decoding call sets up once its own arguments pass."""
        always, first = self._id_list(suppress_tokens, "suppress_tokens"), self._id_list(suppress_at_start, "suppress_at_start")
        return always, first, self.start(encoder_states, kernels, beams=beams, graph=graph)

    def _budget(self, st: DecoderState, prompt: list, max_length) -> int:
        """How many ids may be generated before prompt + generated ids number min(max_length,
        max_target_positions); 0 for an empty batch too: nothing is decoded then."""
        limit = min(int(max_length), self.max_target_positions)
        return max(0, limit - len(prompt)) if st.B else 0

    def _prompt_rows(self, st: DecoderState, prompt: list, who: str) -> torch.Tensor:
        """The prompt as checked ids [rows, n], the same in every row of the state."""
        return self._tokens(torch.tensor(prompt).unsqueeze(0).expand(st.rows, -1), (st.rows, len(prompt)), who)

    @staticmethod
    def _cut(row: list, eot: int) -> list:
        """A row's generated ids up to its first `eot`."""
        return row[:row.index(eot)] if eot in row else row

    @staticmethod
    def _rank(chunks: list, length_penalty: float = 1.0):
        """Per chunk its (ids, sum, n) -> (per chunk its Hypotheses by score = sum / n **
        length_penalty, the earlier first on ties; per chunk their n in the same order)."""
        out, ns = [], []
        for hyps in chunks:
            ranked = [(Hypothesis(i, s, s / n ** float(length_penalty)), n) for i, s, n in hyps]
            ranked.sort(key=lambda h: -h[0].score)  # (stable)
            out.append([h for h, _ in ranked])
            ns.append([n for _, n in ranked])
        return out, ns

    def _decode_rows(self, st: DecoderState, lg: torch.Tensor, budget: int, select, sync_every: int, *on_device) -> list:
        """generate's and sample's loop from the logits after the prompt: select(lg, n, done) -> (the
        ids [rows] of generated step n, `done` [rows] with the rows that ended on it), and the ids
        are fed to the next step, until every row is done or `budget` ids are generated (the check
        synchronises once per step).  On a graph state the steps after the first selection are
        _decode_on_device's, `on_device` its last arguments.  Returns the ids per row, with
        whatever a finished row was fed, as lists."""
        with self._ctx():
            done = torch.zeros(st.rows, dtype=torch.bool, device=self.device)
            steps = []
            while True:
                nxt, done = select(lg, len(steps), done)
                steps.append(nxt)
                if len(steps) >= budget or bool(done.all()):
                    break
                if st.graph is not None:
                    steps = self._decode_on_device(st, nxt, done, budget, sync_every, *on_device)
                    break
                lg = self._step(st, nxt)
            return torch.stack(steps, 1).cpu().tolist()

    def _select_body(self, plan: _GraphPlan, pen: Optional[_Penalty] = None) -> None:
        """generate's selection on the plan's tensors: the logits buffer masked by `suppress`, the
        argmax (`eot` for the rows that are done), `done`, the ids into the token buffer and into
        row `count` of the record, count += 1.  `pen`: the logits are rewritten by it first, its
        history's length `count` plus its prompt part; a row left without a finite logit is done;
        the ids go into its history, which is the record then."""
        sel = plan.selection
        if pen is not None:
            pen.apply_counted(plan.logits, sel.count)
        plan.logits.masked_fill_(sel.suppress, float("-inf"))
        best = plan.logits.argmax(-1)
        ended = sel.done if pen is None else sel.done | (plan.logits.gather(1, best[:, None])[:, 0] == float("-inf"))
        nxt = torch.where(ended, sel.eot, best)
        sel.done.logical_or_(nxt == sel.eot)
        plan.tok.copy_(nxt)
        (sel.record if pen is None else pen.record).index_copy_(0, sel.count, nxt.unsqueeze(0))
        sel.count.add_(1)

    def _decode_on_device(self, st: DecoderState, nxt: torch.Tensor, done: torch.Tensor, budget: int, sync_every: int,
                          key, body, fill, sums: Optional[torch.Tensor] = None, pen: Optional[_Penalty] = None) -> list:
        """_decode_rows' loop after the first selection (ids `nxt`, `done`; at least one row is live
        and budget >= 2 ids may be generated in all) on the plan's _Selection, made here at its
        first use: per step one replay of the step graph and one of the selection graph `key`,
        which is captured from body(plan) when the plan has none, and the completion asked of the
        device every `sync_every` generated steps.  fill(selection) sets `suppress` (and `eot`);
        `sums`: sample's running sums [rows], carried on in the selection's and updated at the end.
        `pen`: the call's _Penalty, whose history the bodies record into (it is bound to the
        selection's `history`).  Returns the ids of every step, the first included."""
        plan = st.graph
        with self._ctx():
            sel = plan.selection = plan.selection or _Selection(self, st.rows)
            fill(sel)
            sel.done.copy_(done)
            state = (sel.done, sel.count, plan.tok)  # what body updates: a capture's warm-up must leave it as it is
            if sums is not None:
                sel.for_sample().sums.copy_(sums)
                state = (sel.done, sel.sums, sel.count, plan.tok)
            record = sel.record
            if pen is not None:  # (the rewrite is not idempotent as the mask is: the logits are state too)
                record, state = pen.record, (*state, plan.logits)
            plan.tok.copy_(nxt)
            record[0].copy_(nxt)
            sel.count.fill_(1)
            n = 1
            while n < budget:
                self._graph_step(st, None)  # at position len(prompt) + n - 1 <= limit - 2
                g = sel.graphs.get(key)
                if g is None:  # once per plan and key
                    if len(sel.graphs) >= _MAX_SELECT_GRAPHS:
                        sel.graphs.clear()
                    g = sel.graphs[key] = self._captured(lambda: body(plan), state=state)
                g.replay()
                n += 1
                if n % sync_every == 0 and n < budget and bool(sel.done.all()):
                    break
            if sums is not None:
                sums.copy_(sel.sums)
            return list(record[:n].unbind(0))

    def _select(self, lg: torch.Tensor, cum: torch.Tensor, G: int, kernels: bool):
        """wx_beam_topk's definition: per chunk the 2G best of cum[r] + log_softmax(lg[r])[t] as
        (scores [B, 2G] fp32, index [B, 2G] int32 = g V + t), by score descending, then lower g,
        higher logit, lower t.  The host route preselects 2G per row by logit as the kernel does."""
        if kernels:
            return _lib.beam_topk(lg, cum, G)
        R, V = int(lg.shape[0]), int(lg.shape[1])
        K = 2 * G
        x, t = torch.sort(lg, dim=1, descending=True, stable=True)  # (logit descending, t ascending)
        x, t = x[:, :K], t[:, :K]
        sc = cum[:, None] + (x - torch.logsumexp(lg, 1)[:, None])
        sc = torch.where((x == float("-inf")) | (cum[:, None] == float("-inf")), float("-inf"), sc)
        idx = (torch.arange(R, device=lg.device)[:, None] % G) * V + t  # rows of a chunk: g ascending
        sc, order = torch.sort(sc.view(R // G, G * K), dim=1, descending=True, stable=True)
        return sc[:, :K], idx.view(R // G, G * K).gather(1, order)[:, :K].to(torch.int32)

    @torch.inference_mode()
    def beam_search(self, encoder_states: torch.Tensor, prompt, eot: int, beam_size: int = 5, patience: float = 1.0,
                    length_penalty: float = 1.0, max_length: int = 448, suppress_tokens=(), suppress_at_start=(),
                    kernels: Optional[bool] = None, prefill: bool = False, graph: bool = False,
                    repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                    history_from: Optional[int] = None) -> list:
        """Beam search (asr.py:301-304: the reference's default is beam_size 5, patience 1,
        length_penalty 1).  The structure is that of OpenAI's BeamSearchDecoder and
        MaximumLikelihoodRanker; this docstring is the specification.

        G = beam_size beams per chunk are fed the prompt.  At the first generated step only beam 0
        of a chunk is live (running sum 0; the others -inf).  Every step masks the logits as
        generate does, takes the chunk's 2G best candidates (beam g, token t) by
        sum[g] + log_softmax(logits[g])[t] (wx_beam_topk's order) and walks them best first until G
        live beams are chosen: a candidate whose token is `eot` becomes a finished hypothesis (its
        sum the candidate's score, its ids the beam's generated ids) unless the chunk already has
        max(1, round(beam_size patience)) of them; any other becomes the next live beam.  At most
        G of the candidates are `eot` (one per beam), so 2G suffice.  A chunk with that many
        finished hypotheses is done: its rows are fed `eot` and ignored.  The loop ends when every
        chunk is done or prompt + generated ids number min(max_length, max_target_positions); live
        beams then fill a chunk's list up to beam_size, in order of their sums.

        Returns per chunk its hypotheses, best first, as Hypothesis(ids, sum_logprob, score):
        score = sum / n ** length_penalty with n the scored positions (the ids, plus one for an
        `eot`; at least 1), ranked by score, earlier-found first on ties.  The self-attention
        caches follow the beams by `reorder`; the 2G scores and indices of every chunk are the one
        host synchronisation of a step.  `prefill`: the prompt goes through one call to prefill on
        the B chunks (a chunk's beams are identical during the prompt) instead of one step per id
        on B G rows; off by default, as in generate.  `graph`: the step on the B G rows is a
        replay of start's captured graph (HIP route only); the top-k, the host walk and `reorder`
        are unchanged, and so are the hypotheses.  `repetition_penalty`, `no_repeat_ngram_size` and
        `history_from` are generate's: every beam's logits are rewritten from that beam's own
        history before the masks, so the candidates' scores and the hypotheses' sums are those of
        the rewritten logits (a banned candidate scores -inf and ranks last, as a masked one does),
        and the histories follow the beams whenever the caches do."""
        return self._beam_search(encoder_states, prompt, eot, beam_size, patience, length_penalty, max_length,
                                 suppress_tokens, suppress_at_start, kernels, prefill, graph,
                                 penalty=(repetition_penalty, no_repeat_ngram_size, history_from))[0]

    def _feed_prompt(self, st: DecoderState, ptok: torch.Tensor, prefill: bool, probe=None):
        """The prompt ptok [rows, n] (the same ids in every row) into a fresh state, one step per id
        or by prefill -> (the logits after its last id [rows, V], probabilities [B] or None).
        `probe` = (sot_index, no_speech_token): the second value is
        softmax(logits after prompt[sot_index])[no_speech_token] over the whole vocabulary, per
        chunk, read on the way; prefill then feeds the prompt in two pieces, around sot_index."""
        n, G = int(ptok.shape[1]), st.G
        cut = n if probe is None else int(probe[0]) + 1
        prob = None

        def read(lg):
            return torch.softmax(lg[::G], -1)[:, int(probe[1])].clone()

        if prefill:
            lg = self._prefill(st, ptok[::G, :cut], False)
            if probe is not None:
                prob = read(lg)
            if cut < n:
                lg = self._prefill(st, ptok[::G, cut:], False, identical=True)
        else:
            for i in range(n):
                lg = self._step(st, ptok[:, i])
                if i + 1 == cut and probe is not None:
                    prob = read(lg)
        return lg, prob

    def _beam_search(self, encoder_states, prompt, eot, beam_size, patience, length_penalty, max_length,
                     suppress_tokens, suppress_at_start, kernels, prefill, graph, probe=None, penalty=(1.0, 0, None)):
        """beam_search -> (its result, per chunk the scored positions n of every hypothesis in the
        same order, _feed_prompt's probabilities for `probe` or None).  `penalty`:
        (repetition_penalty, no_repeat_ngram_size, history_from)."""
        prompt = [int(t) for t in prompt]
        eot, G = int(eot), int(beam_size)
        self._check_prompt("beam_search", prompt, eot)
        if not 1 <= G <= _MAX_BEAMS:
            raise ValueError(f"WhisperDecoder.beam_search: beam_size must lie in 1..{_MAX_BEAMS}, got {beam_size}")
        if not float(patience) > 0:
            raise ValueError(f"WhisperDecoder.beam_search: patience must be positive, got {patience}")
        if self.V < 2 * G:
            raise ValueError(f"WhisperDecoder.beam_search: a vocabulary of {self.V} is smaller than 2 x beam_size")
        pen = self._penalty("beam_search", prompt, max_length, *penalty)
        always, first, st = self._open(encoder_states, suppress_tokens, suppress_at_start, kernels, G, graph)
        max_finished = max(1, round(G * float(patience)))
        B, R, V = st.B, st.rows, self.V
        budget = self._budget(st, prompt, max_length)
        if not budget:
            return [[] for _ in range(B)], [[] for _ in range(B)], None
        lg, prob = self._feed_prompt(st, self._prompt_rows(st, prompt, "beam_search"), prefill, probe)
        if pen is not None:
            pen.bind(self, st)
        ninf = float("-inf")
        sums = [[0.0] + [ninf] * (G - 1) for _ in range(B)]
        ids = [[[] for _ in range(G)] for _ in range(B)]
        finished = [[] for _ in range(B)]  # (ids, sum, n) in the order found
        steps = 0
        identity = list(range(R))
        while True:
            if pen is not None:
                pen.apply(lg, steps)
            if always is not None:
                lg.index_fill_(1, always, ninf)
            if first is not None and not steps:
                lg.index_fill_(1, first, ninf)
            cum = torch.tensor([x for row in sums for x in row], dtype=torch.float32).to(self.device)
            with self._ctx():
                sc, idx = self._select(lg, cum, G, st.kernels)
                both = torch.cat([sc, idx.view(torch.float32)], 1).cpu()  # one synchronisation
            sc, idx = both[:, :2 * G].tolist(), both[:, 2 * G:].contiguous().view(torch.int32).tolist()
            steps += 1
            parents, feed = list(identity), [eot] * R
            for b in range(B):
                if len(finished[b]) >= max_finished:
                    continue
                live = []  # (parent beam, token, sum)
                for s, i in zip(sc[b], idx[b]):
                    g, t = divmod(i, V)
                    if t == eot:
                        if len(finished[b]) < max_finished:
                            finished[b].append((list(ids[b][g]), s, len(ids[b][g]) + 1))
                    else:
                        live.append((g, t, s))
                        if len(live) == G:
                            break
                ids[b] = [ids[b][g] + [t] for g, t, _ in live]
                sums[b] = [s for _, _, s in live]
                for j, (g, t, _) in enumerate(live):
                    parents[b * G + j], feed[b * G + j] = b * G + g, t
            done = all(len(f) >= max_finished for f in finished)
            if steps >= budget or done:
                break
            feed = torch.tensor(feed, dtype=torch.int64).to(self.device)
            if parents != identity:
                self.reorder(st, torch.tensor(parents, dtype=torch.int64))
                if pen is not None:
                    pen.follow(torch.tensor(parents, dtype=torch.int64).to(self.device), steps - 1)
            if pen is not None:
                pen.append(steps - 1, feed)
            lg = self._step(st, feed)
        chunks = []
        for b in range(B):
            hyps = list(finished[b])
            if len(hyps) < max_finished:  # not done: the live beams, already in order of their sums
                for g in range(len(ids[b])):
                    if len(hyps) >= G:
                        break
                    hyps.append((ids[b][g], sums[b][g], max(1, len(ids[b][g]))))
            chunks.append(hyps)
        return (*self._rank(chunks, length_penalty), prob)  # (the earlier-found first on ties)

    # ------------------------------------------------------------- sampling, temperature fallback
    def _select_token(self, lg: torch.Tensor, mask, temperature: float, seed: int, step: int, done: torch.Tensor,
                      sums: torch.Tensor, eot: int):
        """wx_sample_token's definition (include/wx_align.h) in torch ops, for the host route: lg
        [R, V] fp32 logits, mask [V] bool or None, done [R] bool and sums [R] fp32 updated in place
        -> (token [R] int64, logprob [R] fp32).  z and the log-probability are evaluated in fp64 on
        the fp32 logits and the log-probability rounded to fp32 once; the sum is an fp32 addition."""
        R, V = int(lg.shape[0]), int(lg.shape[1])
        m = lg.double()
        if mask is not None:
            m = m.masked_fill(mask, float("-inf"))
        z = m
        if temperature > 0:
            u = torch.from_numpy(gumbel_uniforms(seed, R, V, step)).to(m.device)
            z = m / float(np.float32(temperature)) - torch.log(-torch.log(u))  # (the kernel's argument is an fp32)
        top = z.max(-1, keepdim=True).values
        cols = torch.arange(V, device=m.device).expand(R, V)
        tok = torch.where(z == top, cols, V).min(-1).values.clamp_(max=V - 1)  # the lowest t on ties
        lp = (m.gather(1, tok[:, None])[:, 0] - torch.logsumexp(m, -1)).float()
        live = ~done & (m.max(-1).values > float("-inf"))
        tok = torch.where(live, tok, eot)
        sums.add_(torch.where(live, lp, 0.0))
        done.logical_or_(~live | (tok == eot))
        return tok, torch.where(live, lp, 0.0)

    @torch.inference_mode()
    def sample(self, encoder_states: torch.Tensor, prompt, eot: int, temperature: float = 0.0, best_of: int = 1,
               seed: int = 0, max_length: int = 448, suppress_tokens=(), suppress_at_start=(),
               kernels: Optional[bool] = None, prefill: bool = False, graph: bool = False, sync_every: int = 8,
               repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
               history_from: Optional[int] = None) -> list:
        """Greedy decoding or sampling with the sequences' log-probabilities (faster-whisper's
        `temperature` and `best_of`; one pass of decode_with_fallback).  Per chunk `best_of`
        candidates are decoded side by side as the rows b best_of + g of a `start(beams=best_of)`
        state: they share the chunk's cross-attention keys and values and never change rows, so no
        `reorder` is needed.  The prompt, the masks (`suppress_tokens` always, `suppress_at_start`
        at the first generated position) and the stopping rules are generate's.

        Every generated step is one wx_sample_token launch on the step's logits (include/wx_align.h
        states the definition; the host route evaluates the same definition in torch ops): at
        temperature 0 the argmax, the lowest id on ties; above 0 the Gumbel-max draw from
        softmax(logits / temperature) with the uniforms of Philox4x32-10 keyed on `seed` and
        counted by (id, row, step), the step being the number of ids generated so far, so the same
        seed gives the same draws on every route.  A token's log-probability is
        log_softmax(masked logits)[token] at temperature 1 whatever the temperature is (OpenAI's
        rule: the sum scores the model's distribution, not the tempered one), summed per row in
        fp32, the `eot` that ends a row included.  `temperature` 0 requires `best_of` 1: the ids are
        then generate's.

        Returns per chunk `best_of` Hypothesis(ids, sum_logprob, score), best first: ids without
        the prompt and without `eot`, score = sum_logprob / n with n the ids plus one for an `eot`,
        at least 1 (beam_search's rule at length_penalty 1), the earlier row first on ties.
        `graph` (HIP route only): after the first selection a step is one replay of the step graph
        and one of a small selection graph of the plan (wx_sample_token reading the step counter
        from device memory, the ids into the token buffer and the record), and the host asks
        whether every row is done every `sync_every` generated steps; the result equals
        graph=False exactly, ids and sums.  A selection graph is captured per (temperature, seed,
        eot) of a plan and kept; `graph_captures` counts step graphs only.  `repetition_penalty`,
        `no_repeat_ngram_size` and `history_from` are generate's: every candidate's logits are
        rewritten from its own history before the selection, which then masks, draws and scores
        the rewritten logits (on a graph state one more launch of the captured selection, whose
        key gains the three values' (rho, n, length of the prompt's part))."""
        return self._sample(encoder_states, prompt, eot, temperature, best_of, seed, max_length, suppress_tokens,
                            suppress_at_start, kernels, prefill, graph, sync_every,
                            penalty=(repetition_penalty, no_repeat_ngram_size, history_from))[0]

    def _sample(self, encoder_states, prompt, eot, temperature, best_of, seed, max_length, suppress_tokens,
                suppress_at_start, kernels, prefill, graph, sync_every, probe=None, penalty=(1.0, 0, None)):
        """sample -> (its result, per chunk the scored positions n of every hypothesis in the same
        order, _feed_prompt's probabilities for `probe` or None).  `penalty`: (repetition_penalty,
        no_repeat_ngram_size, history_from)."""
        prompt = [int(t) for t in prompt]
        eot, G, seed, T = int(eot), int(best_of), int(seed), float(temperature)
        self._check_prompt("sample", prompt, eot)
        if not 1 <= G <= _MAX_BEAMS:
            raise ValueError(f"WhisperDecoder.sample: best_of must lie in 1..{_MAX_BEAMS}, got {best_of}")
        if not (T >= 0 and T != float("inf")):
            raise ValueError(f"WhisperDecoder.sample: temperature must be finite and not negative, got {temperature}")
        if T == 0 and G != 1:
            raise ValueError(f"WhisperDecoder.sample: temperature 0 draws nothing, so best_of must be 1, got {best_of}")
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"WhisperDecoder.sample: seed must be an unsigned 64-bit integer, got {seed}")
        if int(sync_every) < 1:
            raise ValueError(f"WhisperDecoder.sample: sync_every must be at least 1, got {sync_every}")
        pen = self._penalty("sample", prompt, max_length, *penalty)
        always, first, st = self._open(encoder_states, suppress_tokens, suppress_at_start, kernels, G, graph)
        B, R, dev = st.B, st.rows, self.device
        budget = self._budget(st, prompt, max_length)
        if not budget:
            return [[Hypothesis([], 0.0, 0.0) for _ in range(G)] for _ in range(B)], [[1] * G for _ in range(B)], None
        lg, prob = self._feed_prompt(st, self._prompt_rows(st, prompt, "sample"), prefill, probe)
        if pen is not None:
            pen.bind(self, st)
        with self._ctx():
            mask = mask0 = None
            if always is not None or first is not None:
                mask0 = torch.zeros(self.V, dtype=torch.bool, device=dev)
                if always is not None:
                    mask = mask0.index_fill(0, always, True)
                    mask0 = mask.clone()
                if first is not None:
                    mask0.index_fill_(0, first, True)
            sums = torch.zeros(R, dtype=torch.float32, device=dev)
            counter = torch.arange(len(prompt) + budget, dtype=torch.int64, device=dev)  # element n: the step counter of step n
        key = (eot, T, seed)  # arguments of wx_sample_token's launch, and so part of a captured selection
        if pen is not None:
            key += pen.key

        def select(lg, n, done):  # (the kernel and its definition update done and sums in place)
            if pen is not None:
                pen.apply(lg, n)
            if st.kernels:
                tok = _lib.sample_token(lg, counter[n:], eot, done, T, seed, mask if n else mask0, sums)[0]
            else:
                tok = self._select_token(lg, mask if n else mask0, T, seed, n, done, sums, eot)[0]
            if pen is not None:
                pen.append(n, tok)
            return tok, done

        def fill(sel):
            if mask is None:
                sel.suppress.zero_()
            else:
                sel.suppress.copy_(mask)

        rows = self._decode_rows(st, lg, budget, select, int(sync_every), key,
                                 lambda plan: self._sample_body(plan, eot, T, seed, pen), fill, sums, pen)
        totals = sums.cpu().tolist()
        chunks = [[] for _ in range(B)]
        for r, (row, total) in enumerate(zip(rows, totals)):
            ids = self._cut(row, eot)
            chunks[r // G].append((ids, total, max(1, len(ids) + (eot in row))))
        return (*self._rank(chunks), prob)  # (the earlier row first on ties)

    def _sample_body(self, plan: _GraphPlan, eot: int, temperature: float, seed: int,
                     pen: Optional[_Penalty] = None) -> None:
        """sample's selection on the plan's tensors: wx_sample_token on the logits buffer with the
        step counter `count` read on the device, the ids straight into the step's token buffer,
        then into row `count` of the record, count += 1.  `pen`: as in _select_body."""
        sm = plan.selection
        if pen is not None:
            pen.apply_counted(plan.logits, sm.count)
        _lib.sample_token(plan.logits, sm.count, eot, sm.done, temperature, seed, sm.suppress, sm.sums, token=plan.tok,
                          logprob=sm.logprob, workspace=sm.ws)
        (sm.record if pen is None else pen.record).index_copy_(0, sm.count, plan.tok.unsqueeze(0))
        sm.count.add_(1)

    @torch.inference_mode()
    def decode_with_fallback(self, encoder_states: torch.Tensor, prompt, eot: int,
                             temperatures=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0), beam_size: int = 5, patience: float = 1.0,
                             length_penalty: float = 1.0, best_of: int = 5, log_prob_threshold: Optional[float] = -1.0,
                             no_speech_threshold: Optional[float] = 0.6, no_speech_token: Optional[int] = None,
                             sot_index: int = 0, compression_ratio_threshold: Optional[float] = 2.4, text_of=None,
                             seed: int = 0, max_length: int = 448, suppress_tokens=(), suppress_at_start=(),
                             kernels: Optional[bool] = None, prefill: bool = False, graph: bool = False,
                             sync_every: int = 8, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                             history_from: Optional[int] = None) -> list:
        """Temperature fallback (asr.py:305-312: temperatures 0 .. 1, compression_ratio_threshold
        2.4, log_prob_threshold -1, no_speech_threshold 0.6): faster-whisper's
        generate_with_fallback on a batch of chunks; this docstring is the specification.

        All chunks start pending.  For every temperature, in order, the pending chunks are decoded
        as one batch (an index_select of `encoder_states`, in their order): at temperature 0 by
        beam_search with `beam_size`, `patience` and `length_penalty` (by sample at temperature 0
        when beam_size is 1), above 0 by sample(temperature, best_of); the chunk's attempt is the
        best hypothesis.  The pass at index i of `temperatures` uses `seed` + i.  Per attempt:

            avg_logprob        sum_logprob / n, n the scored positions (the ids, plus one for an
                               `eot`; at least 1)
            compression_ratio  utils.compression_ratio(text_of(ids)) when `text_of` (ids -> str: the
                               tokenizer stays with the caller) is given, else None
            needs another temperature   compression_ratio > compression_ratio_threshold, or
                               avg_logprob < log_prob_threshold
            is_silence         no_speech_prob > no_speech_threshold and avg_logprob <
                               log_prob_threshold: the chunk is final whatever the line above says

        A threshold of None switches its check off.  A chunk that needs no other temperature is
        final with that attempt.  After the last temperature a chunk that is still pending takes
        its attempt with the highest avg_logprob, the earliest on ties.  `no_speech_prob` is
        softmax(logits after prompt[sot_index])[no_speech_token] over the whole vocabulary, read
        during the first pass's prompt (with `prefill` the prompt is then fed in two pieces, around
        sot_index); None when `no_speech_token` is None.  The remaining arguments are generate's;
        `repetition_penalty`, `no_repeat_ngram_size` and `history_from` go to every pass, as
        faster-whisper hands them to every generate call of its loop (the no-speech probability is
        read during the prompt, before any rewrite).

        Returns per chunk DecodingResult(ids, sum_logprob, avg_logprob, temperature,
        no_speech_prob, compression_ratio, is_silence, attempts): the chosen attempt, the
        temperature it was decoded at and the number of attempts the chunk took."""
        temps = [float(t) for t in temperatures]
        if not temps:
            raise ValueError("WhisperDecoder.decode_with_fallback: temperatures is empty")
        if any(not (t >= 0 and t != float("inf")) for t in temps):
            raise ValueError(f"WhisperDecoder.decode_with_fallback: temperatures must be finite and not negative, got {temps}")
        n_prompt = len(list(prompt))
        if not 0 <= int(sot_index) < n_prompt:
            raise ValueError(f"WhisperDecoder.decode_with_fallback: sot_index {sot_index} is outside the prompt of "
                             f"{n_prompt} ids")
        if no_speech_token is not None and not 0 <= int(no_speech_token) < self.V:
            raise ValueError(f"WhisperDecoder.decode_with_fallback: no_speech_token {no_speech_token} is outside the "
                             f"vocabulary of {self.V}")
        penalty = (repetition_penalty, no_repeat_ngram_size, history_from)
        on = self._penalty("decode_with_fallback", [int(t) for t in prompt], max_length, *penalty) is not None
        extra = {"penalty": penalty} if on else {}  # (at the defaults the passes are called as they always were)
        x = encoder_states
        if not torch.is_tensor(x) or x.dim() != 3:
            raise ValueError("WhisperDecoder.decode_with_fallback: encoder_states must be a [B, P, D] tensor")
        B = int(x.shape[0])
        pending, tried = list(range(B)), [[] for _ in range(B)]
        final, silence_prob = [None] * B, [None] * B
        for i, T in enumerate(temps):
            if not pending:
                break
            sub = x if len(pending) == B else x.index_select(0, torch.tensor(pending, dtype=torch.int64, device=x.device))
            probe = (int(sot_index), int(no_speech_token)) if i == 0 and no_speech_token is not None else None
            if T == 0 and int(beam_size) != 1:
                hyps, ns, prob = self._beam_search(sub, prompt, eot, beam_size, patience, length_penalty, max_length,
                                                   suppress_tokens, suppress_at_start, kernels, prefill, graph, probe,
                                                   **extra)
            else:
                hyps, ns, prob = self._sample(sub, prompt, eot, T, 1 if T == 0 else best_of, int(seed) + i, max_length,
                                              suppress_tokens, suppress_at_start, kernels, prefill, graph, sync_every, probe,
                                              **extra)
            if prob is not None:
                for b, p in zip(pending, prob.cpu().tolist()):
                    silence_prob[b] = p
            still = []
            for j, b in enumerate(pending):
                h, n = (hyps[j][0], ns[j][0]) if hyps[j] else (Hypothesis([], 0.0, 0.0), 1)
                avg = h.sum_logprob / n
                ratio = None if text_of is None else compression_ratio(text_of(h.ids))
                low = log_prob_threshold is not None and avg < log_prob_threshold
                again = low or (compression_ratio_threshold is not None and ratio is not None
                                and ratio > compression_ratio_threshold)
                silent = low and no_speech_threshold is not None and silence_prob[b] is not None \
                    and silence_prob[b] > no_speech_threshold
                tried[b].append(DecodingResult(h.ids, h.sum_logprob, avg, T, silence_prob[b], ratio, silent, len(tried[b]) + 1))
                if again and not silent:
                    still.append(b)
                else:
                    final[b] = tried[b][-1]
            pending = still
        for b in pending:  # every temperature failed: the attempt with the highest avg_logprob, the earliest on ties
            best = max(tried[b], key=lambda a: a.avg_logprob)
            final[b] = best._replace(attempts=len(tried[b]))
        return final

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


def load_whisper_decoder(path: str, device=None, dtype: torch.dtype = torch.float32) -> WhisperDecoder:
    """A WhisperDecoder from a state-dict file (as load_whisper_encoder reads it).  The file may
    hold a whole model; only the decoder's tensors are used.  `dtype`: WhisperDecoder's."""
    return WhisperDecoder(_load_state_dict(path, "load_whisper_decoder"), device=device, dtype=dtype)

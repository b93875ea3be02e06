"""Emission producer on the GPU (reference alignment.py:209-235).

The reference runs one wav2vec2 forward per segment, unpadded (padding a batch changes
wav2vec2's logits), then ``log_softmax`` and a device->host copy.  Here the forward stays a
PyTorch-ROCm model call, one per segment, but:

* **Length-agnostic convolutions.**  Every segment of a VAD-cut file has its own length, and
  MIOpen treats each new length as a new problem: it looks the shape up in its find-db, falls
  back to heuristics (``GetSolutionsFallback``), rejects solvers whose workspace PyTorch did
  not provide (``IsEnoughWorkspace``) and compiles kernels for the one it keeps.  On a fresh
  MI355X that cost tens of ms per new length (BENCH_r01 config 3: 34-47 ms per chunk against
  8.7 ms per fixed-length segment).  ``prepare_model`` re-routes each ``nn.Conv1d`` of the
  model through GEMMs whose only shape dependence is the row count (hipBLASLt/rocBLAS):

  - activations are kept *time-major* (``[L, C]``); the conv output is returned as the
    ``[B, C, L]`` transposed view of that buffer, so the next conv's ``transpose(1, 2)`` is free;
  - ungrouped convs with ``Cin > 1`` are a sum over the k taps of ``x[j::s] @ W_j^T``: each
    tap's operand is a strided view (row stride ``s*Cin``), no im2col copy;
  - ``Cin == 1`` (the waveform layer) and grouped convs (wav2vec2's positional conv,
    k=128, 16 groups) gather ``k*Cin`` patch rows and run one (batched) GEMM, tap blocks of
    32 at a time to bound the patch buffer.

  Parameters are read from the module on every call (``conv.weight`` re-evaluates a
  weight_norm parametrisation), so the module's state_dict and training behaviour are
  untouched; only inference forwards on a HIP device take the GEMM route.
* **Time-major GroupNorm + GELU.**  The first feature-encoder layer's GroupNorm (one group
  per channel, i.e. a per-channel normalisation over time) runs as the HIP kernel
  wx_channel_norm on the time-major conv output with the erf GELU fused, instead of torch's
  channel-major GroupNorm (which first copied the 96k x 512 activation).
* **fp32 self-attention on the f32 MFMA.**  The encoder's attention layers go through
  wx_attention_f32 (a flash-attention forward, one wave per 32-query tile; see
  csrc/wx_emission.hip) via transformers' attention interface; torch's fused fp32 attention
  was a third of config 3's GPU time.
* **One q/k/v GEMM.**  Each self-attention's three projections run as one GEMM on the
  concatenated weights (cached, _QKV_CACHE); k_proj / v_proj return column slices of its output,
  which wx_attention_f32 reads in place (strided views).
* **No concatenation copy.**  ``log_softmax`` writes each segment's ``[T, V]`` rows straight
  into its slice of the CSR emission matrix the DP kernel reads (``emissions_csr``).
* **Half precision, opt-in.**  ``packed_logits(..., dtype=torch.float16 | torch.bfloat16)`` runs
  the packed forward's GEMMs, GELUs and attention (wx_attention_h16_packed) in the 16-bit type
  from rounded copies of the weights cached outside the model; the residual stream, the norms
  and the positional conv stay fp32 (the last section of this file).
"""
from __future__ import annotations

import contextlib
import os
import threading
import types
import weakref
from typing import Optional

import torch
import torch.nn.functional as F

_TAP_BLOCK = 32  # grouped/Cin==1 convs: taps per patch block


# Derived weights (the weight_norm'd positional conv's weight, per-tap GEMM operands, the fused
# q/k/v matrix), per module, outside the module (the caller's model keeps no attributes of
# ours) and kept across align() calls (rebuilding them took ~0.8 ms of GPU time per call);
# each entry is keyed on its parameters' (data_ptr, version), so an update rebuilds it, and
# dies with its module.
_W_CACHE: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
_TAP_CACHE: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
_QKV_CACHE: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _weight(conv: torch.nn.Conv1d) -> torch.Tensor:
    """conv.weight, with a parametrised weight (weight_norm: wav2vec2's positional conv, whose
    re-evaluation is a 0.45 ms kernel per forward) cached until one of its originals changes.

    The cache is filled by ``materialize_weights`` on the caller's stream *before* align()
    fans the forwards out over side streams (which wait on that stream): a weight built
    lazily inside a side stream's first forward would be read by the other side streams
    without any ordering against the kernels that compute it."""
    par = getattr(conv, "parametrizations", None)
    if par is None or "weight" not in par:
        return conv.weight
    key = tuple((p.data_ptr(), p._version) for p in par["weight"].parameters())
    cached = _W_CACHE.get(conv)
    if cached is not None and cached[0] == key:
        return cached[1]
    w = conv.weight.detach()
    _W_CACHE[conv] = (key, w)
    return w


def _version(t: torch.Tensor) -> int:
    """t._version; -1 for an inference tensor (it has no version counter)."""
    try:
        return t._version
    except RuntimeError:
        return -1


def _tap_weights(conv: torch.nn.Conv1d) -> torch.Tensor:
    """The GEMM operands of _conv1d_gemm, contiguous and cached until the weight changes:
    [k, Cin, Cout] (one [Cin, Cout] matrix per tap) for an ungrouped conv, [G, k, Cg, Cout/G]
    for a grouped one.  (A permuted view of the weight has no unit stride, so every GEMM on
    it made torch copy the operand first: 26 copy kernels per 30 s forward, ~5% of its time.)"""
    # keyed on the module's parameters (a weight_norm'd conv's `weight` is recomputed from
    # weight_g / weight_v by a hook — a new, possibly inference, tensor at every call)
    key = tuple((t.data_ptr(), _version(t)) for t in conv.parameters())
    cached = _TAP_CACHE.get(conv)
    if cached is not None and cached[0] == key:
        return cached[1]
    w = _weight(conv)
    G = conv.groups
    Cout, Cg, k = w.shape
    with torch.no_grad():
        if G == 1 and Cg > 1:
            t = w.detach().permute(2, 1, 0).contiguous()
        else:
            t = w.detach().reshape(G, Cout // G, Cg, k).permute(0, 3, 2, 1).contiguous()
    _TAP_CACHE[conv] = (key, t)
    return t


def materialize_weights(model: torch.nn.Module) -> None:
    """Evaluate every parametrised Conv1d weight of a prepared model on the current stream, so
    that streams which then wait on it read a finished tensor (see _weight)."""
    if not getattr(model, "_wx_gemm_conv", False):
        return
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.Conv1d) and hasattr(mod, "_wx_orig_forward"):
                _tap_weights(mod)
            if "_wx_qkv" in mod.__dict__ and next(mod.parameters()).is_cuda:
                _qkv_weights(mod)


def _conv1d_gemm(conv: torch.nn.Conv1d, x: torch.Tensor) -> torch.Tensor:
    """nn.Conv1d.forward through GEMMs (zeros padding, dilation 1).  x: [B, Cin, L]."""
    w = _weight(conv)  # [Cout, Cin/g, k]
    b = conv.bias
    (k,) = conv.kernel_size
    (s,) = conv.stride
    (p,) = conv.padding if not isinstance(conv.padding, str) else (0,)
    G = conv.groups
    B, Cin, L = x.shape
    Cout = w.shape[0]
    xt = x.transpose(1, 2)  # [B, L, Cin]; a view of a time-major buffer needs no copy
    if p:
        xt = F.pad(xt, (0, 0, p, p))
    xt = xt.contiguous()
    Lp = xt.shape[1]
    Lout = (Lp - k) // s + 1
    out = torch.empty((B, Lout, Cout), dtype=x.dtype, device=x.device)
    if Lout <= 0:
        return out.transpose(1, 2)
    if G == 1 and Cin > 1:
        # y = sum_j x[j::s] @ W[:, :, j]^T  (strided row views, no patch copy)
        wt = _tap_weights(conv)  # [k, Cin, Cout]
        for bi in range(B):
            xb = xt[bi]
            ob = out[bi]
            for j in range(k):
                xj = xb[j: j + s * (Lout - 1) + 1: s]
                if j == 0:
                    if b is not None:
                        torch.addmm(b, xj, wt[j], out=ob)
                    else:
                        torch.mm(xj, wt[j], out=ob)
                else:
                    ob.addmm_(xj, wt[j])
        return out.transpose(1, 2)
    # patches: Cin == 1, or grouped.  wg: [G, k, Cg, Coutg]
    Cg = Cin // G
    Cog = Cout // G
    wg = _tap_weights(conv)  # [G, k, Cg, Cog]
    for bi in range(B):
        xb = xt[bi]  # [Lp, Cin] contiguous
        if G == 1:  # (the first feature-encoder conv: accumulate into the output, bias first)
            o3 = out[bi].unsqueeze(0)  # [1, Lout, Cout] view
            if b is not None:
                o3.copy_(b.reshape(1, 1, Cout).expand(1, Lout, Cout))
            else:
                o3.zero_()
            for j0 in range(0, k, _TAP_BLOCK):
                kb = min(_TAP_BLOCK, k - j0)
                pt = xb[j0:].as_strided((1, Lout, kb * Cg), (Cg, s * Cin, 1))
                o3.baddbmm_(pt, wg[:, j0:j0 + kb].reshape(1, kb * Cg, Cog))
            continue
        acc = torch.zeros((G, Lout, Cog), dtype=x.dtype, device=x.device)
        for j0 in range(0, k, _TAP_BLOCK):
            kb = min(_TAP_BLOCK, k - j0)
            base = xb[j0:]
            # patch[g, t, j, i] = x[t*s + j0 + j, g*Cg + i]
            pt = base.as_strided((G, Lout, kb, Cg), (Cg, s * Cin, Cin, 1)).reshape(G, Lout, kb * Cg)
            acc.baddbmm_(pt, wg[:, j0:j0 + kb].reshape(G, kb * Cg, Cog))
        ob = acc.permute(1, 0, 2).reshape(Lout, Cout)
        if b is not None:
            ob = ob + b
        out[bi].copy_(ob)
    return out.transpose(1, 2)


def _is_erf_gelu(act) -> bool:
    if isinstance(act, torch.nn.GELU):
        return act.approximate == "none"
    inner = getattr(act, "act", None)  # transformers' GELUActivation wraps F.gelu
    return type(act).__name__ == "GELUActivation" and inner is F.gelu


def _patched_gn_layer(self, x):
    """conv -> GroupNorm(one group per channel) -> activation (HF Wav2Vec2GroupNormConvLayer,
    the feature encoder's first layer) on time-major activations: for its 1-channel conv, all
    three in wx_conv0_channel_norm (the conv recomputed per pass, the output written once);
    otherwise the GEMM conv, then wx_channel_norm with the erf GELU fused (one HBM read for
    statistics, one read + write)."""
    if not (x.is_cuda and not torch.is_grad_enabled() and x.dim() == 3):
        return self._wx_orig_forward(x)
    from . import _lib

    gn = self.layer_norm
    gelu = _is_erf_gelu(self.activation)
    conv = self.conv
    (k,) = conv.kernel_size
    if (not os.environ.get("WX_NO_CONV0_FUSED") and conv.in_channels == 1 and conv.groups == 1
            and conv.dilation == (1,) and not isinstance(conv.padding, str) and conv.padding == (0,)
            and gn.num_groups == conv.out_channels and k <= 16 and x.dtype == torch.float32):
        # conv + GroupNorm + GELU in one pass over the output (wx_conv0_channel_norm): the K = 10
        # GEMM's 196 MB output is never written and read back
        w = _weight(conv)
        (s_,) = conv.stride
        L = (x.shape[-1] - k) // s_ + 1
        y = torch.empty((x.shape[0], max(L, 0), conv.out_channels), dtype=x.dtype, device=x.device)
        for b in range(x.shape[0]):
            _lib.conv0_channel_norm(x[b, 0].contiguous(), w, conv.bias, s_, gn.weight, gn.bias, gn.eps, gelu, out=y[b])
        out = y.transpose(1, 2)
        return out if gelu else self.activation(out)
    y = _conv1d_gemm(self.conv, x).transpose(1, 2)  # [B, L, C] contiguous (time-major)
    for b in range(y.shape[0]):
        _lib.channel_norm(y[b], gn.weight, gn.bias, gn.eps, gelu, out=y[b])
    out = y.transpose(1, 2)
    return out if gelu else self.activation(out)


def _patched_forward(self, x):
    if (x.is_cuda and not torch.is_grad_enabled() and x.dim() == 3 and self.padding_mode == "zeros"
            and self.dilation == (1,) and not isinstance(self.padding, str)):
        return _conv1d_gemm(self, x)
    return self._wx_orig_forward(x)


_ATTN_NAME = "wx_f32"
_PACK_SPLIT = int(os.environ.get("WX_ATTN_PACKED_SPLIT", "0"))  # waves per query tile (0: by size)


def _wx_attention(module, query, key, value, attention_mask, dropout: float = 0.0, scaling=None, **kwargs):
    """transformers attention interface (`config._attn_implementation = "wx_f32"`): the
    encoder's unmasked fp32 self-attention of an inference forward on a HIP device through
    wx_attention_f32 (f32 MFMA flash attention); anything else (masks, dropout, other dtypes
    or head sizes, attention weights requested) through transformers' SDPA interface."""
    if (query.is_cuda and attention_mask is None and not (dropout and module.training) and not torch.is_grad_enabled()
            and not any(v is not None and v is not False for v in kwargs.values())
            and query.dtype == torch.float32 and query.shape[-1] == 64
            and key.shape == query.shape and value.shape == query.shape and query.stride(-1) == 1
            and key.stride(-1) == 1 and value.stride(-1) == 1):
        from . import _lib

        scale = scaling if scaling is not None else query.shape[-1] ** -0.5
        return _lib.attention_f32(query, key, value, scale), None
    return _orig_attention(module)(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling,
                                   **kwargs)


# config id -> the attention implementation prepare_model replaced (its fallback target)
_ORIG_ATTN: dict = {}


def _orig_attention(module):
    """The attention function the model used before prepare_model: the interface registered
    under its original `_attn_implementation`, or the modeling file's eager attention."""
    import sys

    from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS

    eager = getattr(sys.modules.get(type(module).__module__), "eager_attention_forward", None)
    name = _ORIG_ATTN.get(id(getattr(module, "config", None)), "sdpa")
    if name and name != "eager" and name in ALL_ATTENTION_FUNCTIONS:
        return ALL_ATTENTION_FUNCTIONS[name]
    return eager if eager is not None else ALL_ATTENTION_FUNCTIONS["sdpa"]


def _use_wx_attention(model: torch.nn.Module) -> None:
    """Point an HF model's attention interface at _wx_attention (WX_NO_ATTN=1: keep torch's)."""
    cfg = getattr(model, "config", None)
    if os.environ.get("WX_NO_ATTN") or cfg is None or not hasattr(cfg, "_attn_implementation"):
        return
    try:
        from transformers import AttentionInterface
        from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS

        if _ATTN_NAME not in ALL_ATTENTION_FUNCTIONS:
            AttentionInterface.register(_ATTN_NAME, _wx_attention)
        orig = cfg._attn_implementation
        cfg._attn_implementation = _ATTN_NAME
        model._wx_orig_attn = orig
        _ORIG_ATTN[id(cfg)] = orig
    except Exception:  # an older transformers without the interface: torch's attention stays
        pass


_QKV_TLS = threading.local()  # the fused projection's k / v results until k_proj / v_proj take them


def _qkv_weights(q: torch.nn.Linear, k: Optional[torch.nn.Linear] = None, v: Optional[torch.nn.Linear] = None):
    """The attention's [Wq; Wk; Wv] (and biases) concatenated, cached until a parameter
    changes (filled by materialize_weights on the caller's stream before any fan-out).  k / v
    default to the projections _fuse_qkv paired with q."""
    if k is None:
        st = q.__dict__["_wx_qkv"]
        k, v = st["k"], st["v"]
    params = [m.weight for m in (q, k, v)] + [m.bias for m in (q, k, v) if m.bias is not None]
    key = tuple((p.data_ptr(), p._version) for p in params)
    c = _QKV_CACHE.get(q)
    if c is None or c[0] != key:
        with torch.no_grad():
            w = torch.cat([q.weight, k.weight, v.weight], 0).detach().contiguous()
            b = torch.cat([q.bias, k.bias, v.bias]).detach() if all(m.bias is not None for m in (q, k, v)) else None
        c = (key, w, b)
        _QKV_CACHE[q] = c
    return c[1], c[2]


def _fused_q_forward(self, x):
    """q_proj of a self-attention layer: one GEMM for q, k and v (768 -> 2304 for wav2vec2-base,
    1024 -> 3072 for large) instead of three narrow ones; k_proj / v_proj then return their
    column slices of the same output when called on the same input (Wav2Vec2Attention calls
    them right after q_proj).  The slices are strided views (row stride 3D) that the attention
    kernel reads in place."""
    st = self.__dict__["_wx_qkv"]
    if x.is_cuda and not torch.is_grad_enabled() and x.dtype == torch.float32:
        w, b = _qkv_weights(self)
        y = F.linear(x, w, b)
        dq, dk = self.out_features, st["k"].out_features
        _QKV_TLS.pending = (st["k"], x, y[..., dq:dq + dk], st["v"], y[..., dq + dk:])
        return y[..., :dq]
    _QKV_TLS.pending = None
    return self._wx_orig_forward(x)


def _fused_k_forward(self, x):
    p = getattr(_QKV_TLS, "pending", None)
    if p is not None and p[0] is self and p[1] is x:
        return p[2]
    return self._wx_orig_forward(x)


def _fused_v_forward(self, x):
    p = getattr(_QKV_TLS, "pending", None)
    _QKV_TLS.pending = None
    if p is not None and p[3] is self and p[1] is x:
        return p[4]
    return self._wx_orig_forward(x)


def _fuse_qkv(model: torch.nn.Module) -> None:
    """Route every self-attention's q/k/v projections through one fused GEMM (WX_NO_QKV=1: keep
    three).  Applies to modules holding q_proj / k_proj / v_proj Linears of equal input width."""
    if os.environ.get("WX_NO_QKV"):
        return
    for mod in model.modules():
        q, k, v = (getattr(mod, n, None) for n in ("q_proj", "k_proj", "v_proj"))
        if not all(isinstance(m, torch.nn.Linear) for m in (q, k, v)):
            continue
        if not (q.in_features == k.in_features == v.in_features) or any(hasattr(m, "_wx_orig_forward") for m in (q, k, v)):
            continue
        q.__dict__["_wx_qkv"] = {"k": k, "v": v}
        for m, f in ((q, _fused_q_forward), (k, _fused_k_forward), (v, _fused_v_forward)):
            m._wx_orig_forward = m.forward
            m.forward = types.MethodType(f, m)


_ADDLN_WIDTHS = (256, 384, 512, 768, 1024, 1280)  # wx_add_layernorm's (384 and 1280: Whisper tiny / large)


def _addln_ok(layer, x: torch.Tensor, norms) -> bool:
    """Whether wx_add_layernorm can stand in for `norm(residual + x)` in this call."""
    if (os.environ.get("WX_NO_ADDLN") or not x.is_cuda or x.dtype != torch.float32 or torch.is_grad_enabled()
            or layer.training or x.dim() < 2 or x.shape[-1] not in _ADDLN_WIDTHS or x.stride(-1) != 1):
        return False
    D = x.shape[-1]
    return all(isinstance(n, torch.nn.LayerNorm) and tuple(n.normalized_shape) == (D,) and n.weight is not None
               and n.bias is not None for n in norms)


def _fused_post_ln_layer(self, hidden_states, attention_mask=None, output_attentions=False, **kwargs):
    """transformers' Wav2Vec2EncoderLayer.forward (post-norm: wav2vec2-base) with both
    `layer_norm(residual + x)` steps as one wx_add_layernorm each (one pass instead of an add
    and a LayerNorm kernel)."""
    if kwargs or not _addln_ok(self, hidden_states, (self.layer_norm, self.final_layer_norm)):
        return self._wx_orig_forward(hidden_states, attention_mask=attention_mask, output_attentions=output_attentions,
                                     **kwargs)
    from . import _lib

    ln, fln = self.layer_norm, self.final_layer_norm
    h, attn_weights, _ = self.attention(hidden_states, attention_mask=attention_mask, output_attentions=output_attentions)
    h = self.dropout(h)
    h = _lib.add_layernorm(hidden_states, h, ln.weight, ln.bias, ln.eps)
    h = _lib.add_layernorm(h, self.feed_forward(h), fln.weight, fln.bias, fln.eps)
    return (h, attn_weights) if output_attentions else (h,)


def _fused_stable_ln_layer(self, hidden_states, attention_mask=None, output_attentions=False, **kwargs):
    """transformers' Wav2Vec2EncoderLayerStableLayerNorm.forward (pre-norm: the large models)
    with `residual + attention` and the feed-forward's `final_layer_norm` of that sum as one
    wx_add_layernorm that also returns the sum."""
    if (kwargs or getattr(self, "adapter_layer", None) is not None
            or not _addln_ok(self, hidden_states, (self.final_layer_norm,))):
        return self._wx_orig_forward(hidden_states, attention_mask=attention_mask, output_attentions=output_attentions,
                                     **kwargs)
    from . import _lib

    fln = self.final_layer_norm
    h = self.layer_norm(hidden_states)
    h, attn_weights, _ = self.attention(h, attention_mask=attention_mask, output_attentions=output_attentions)
    h = self.dropout(h)
    y, s = _lib.add_layernorm(hidden_states, h, fln.weight, fln.bias, fln.eps, want_sum=True)
    h = s + self.feed_forward(y)
    return (h, attn_weights) if output_attentions else (h,)


_LAYER_FORWARDS = {"Wav2Vec2EncoderLayer": _fused_post_ln_layer,
                   "Wav2Vec2EncoderLayerStableLayerNorm": _fused_stable_ln_layer}


def prepare_model(model: torch.nn.Module) -> torch.nn.Module:
    """Route the model's Conv1d inference forwards through length-agnostic GEMMs and its
    self-attention through wx_attention_f32 (idempotent).  Returns the same model object."""
    if getattr(model, "_wx_gemm_conv", False):
        return model
    _use_wx_attention(model)
    _fuse_qkv(model)
    for mod in model.modules():
        if isinstance(mod, torch.nn.Conv1d) and not hasattr(mod, "_wx_orig_forward"):
            mod._wx_orig_forward = mod.forward
            mod.forward = types.MethodType(_patched_forward, mod)
        fwd = _LAYER_FORWARDS.get(type(mod).__name__)
        if (fwd is not None and not hasattr(mod, "_wx_orig_forward") and hasattr(mod, "attention")
                and hasattr(mod, "feed_forward") and isinstance(getattr(mod, "layer_norm", None), torch.nn.LayerNorm)
                and isinstance(getattr(mod, "final_layer_norm", None), torch.nn.LayerNorm)):
            mod._wx_orig_forward = mod.forward
            mod.forward = types.MethodType(fwd, mod)
        gn = getattr(mod, "layer_norm", None)
        if (not os.environ.get("WX_NO_CHANNEL_NORM") and isinstance(getattr(mod, "conv", None), torch.nn.Conv1d) and isinstance(gn, torch.nn.GroupNorm)
                and gn.num_groups == gn.num_channels and gn.num_channels % 4 == 0 and hasattr(mod, "activation")
                and not hasattr(mod, "_wx_orig_forward")):
            mod._wx_orig_forward = mod.forward
            mod.forward = types.MethodType(_patched_gn_layer, mod)
    try:
        model._wx_gemm_conv = True
    except Exception:
        pass
    return model


def restore_model(model: torch.nn.Module) -> torch.nn.Module:
    """Undo prepare_model: the original forwards and attention implementation (the model is
    then exactly what the caller passed in; derived weights stay cached outside it, _W_CACHE)."""
    for mod in model.modules():
        if hasattr(mod, "_wx_orig_forward"):
            orig = mod._wx_orig_forward
            if getattr(orig, "__func__", None) is getattr(type(mod), "forward", None):
                mod.__dict__.pop("forward", None)  # the class's forward again, no instance attribute
            else:
                mod.forward = orig  # the module had its own instance-level forward
            del mod._wx_orig_forward
        mod.__dict__.pop("_wx_qkv", None)
    if "_wx_gemm_conv" in model.__dict__:
        del model._wx_gemm_conv
    if hasattr(model, "_wx_orig_attn"):
        _ORIG_ATTN.pop(id(model.config), None)
        model.config._attn_implementation = model._wx_orig_attn
        del model._wx_orig_attn
    return model


_PREP_MU = threading.Lock()


@contextlib.contextmanager
def prepared(model: torch.nn.Module):
    """prepare_model for the duration of one align() call (reference alignment.py:226-233
    takes the caller's model and leaves it as it was).  Concurrent calls on one model share
    the preparation; the last one to leave restores the model, unless the caller had
    prepared it already."""
    with _PREP_MU:
        refs = model.__dict__.get("_wx_prep_refs", 0)
        if refs == 0:
            model.__dict__["_wx_prep_owned"] = not getattr(model, "_wx_gemm_conv", False)
            prepare_model(model)
        model.__dict__["_wx_prep_refs"] = refs + 1
    try:
        yield model
    finally:
        with _PREP_MU:
            model.__dict__["_wx_prep_refs"] -= 1
            if model.__dict__["_wx_prep_refs"] == 0:
                if model.__dict__.pop("_wx_prep_owned", False):
                    restore_model(model)
                del model.__dict__["_wx_prep_refs"]


def n_frames(n_samples: int, model: Optional[torch.nn.Module] = None) -> int:
    """Emission frames of a wav2vec2 forward over n_samples (>= 400 after the reference's
    pad, alignment.py:217-224): the feature encoder's conv chain.  Uses the model's conv
    geometry when it exposes an HF config, else wav2vec2's (k, s) = (10,5),(3,2)x4,(2,2)x2."""
    ks = None
    cfg = getattr(model, "config", None)
    if cfg is not None and hasattr(cfg, "conv_kernel") and hasattr(cfg, "conv_stride"):
        ks = list(zip(cfg.conv_kernel, cfg.conv_stride))
    if ks is None:
        ks = [(10, 5)] + [(3, 2)] * 4 + [(2, 2)] * 2
    L = max(int(n_samples), 400)
    for k, s in ks:
        L = (L - k) // s + 1
    return L


def log_softmax_into(logits: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """torch.log_softmax(logits, -1) written into `out` (a row slice of the CSR matrix)."""
    return torch._log_softmax(logits, -1, False, out=out)


# ------------------------------------------------------------------------------------------
# Packed encoder: many segments in one transformer pass.
#
# The reference runs one unpadded forward per segment (alignment.py:217-233); a 30 s segment
# gives the encoder 1,499 rows, too few to fill 256 CUs: its GEMMs pick 32 x 64 tiles and its
# attention launches 564 query tiles.  Everything in the encoder except attention, the
# positional conv and the feature encoder is row-wise (LayerNorm, the q/k/v / out / feed-forward
# projections, GELU, lm_head), so segments can be stacked along rows with no padding and no
# interaction: the positional conv runs per segment (its zero padding at each segment's ends),
# attention through wx_attention_f32_packed (each segment attends to its own rows only), the
# rest once over all rows.  Per segment this is the reference's computation; only the GEMMs'
# tiling (their fp32 summation order) differs.  The packed rows are exactly the CSR emission
# layout the DP reads, so log_softmax writes the whole pack at once.

_PACK_ENCODERS = ("Wav2Vec2Encoder", "Wav2Vec2EncoderStableLayerNorm")


def _layer_ok(layer, D: int) -> bool:
    """A transformers Wav2Vec2 encoder layer the packed encoder can run from its weights: q/k/v/out
    Linears with biases, head size 64, LayerNorms of width D, a feed-forward of two Linears."""
    att = getattr(layer, "attention", None)
    ff = getattr(layer, "feed_forward", None)
    lins = [getattr(att, n, None) for n in ("q_proj", "k_proj", "v_proj", "out_proj")]
    if (att is None or ff is None or not all(isinstance(m, torch.nn.Linear) and m.bias is not None for m in lins)
            or getattr(att, "head_dim", 0) != 64 or getattr(att, "is_causal", False)
            or getattr(layer, "adapter_layer", None) is not None):
        return False
    norms = (getattr(layer, "layer_norm", None), getattr(layer, "final_layer_norm", None))
    return (all(isinstance(n, torch.nn.LayerNorm) and tuple(n.normalized_shape) == (D,) and n.weight is not None
                and n.bias is not None for n in norms)
            and isinstance(getattr(ff, "intermediate_dense", None), torch.nn.Linear)
            and isinstance(getattr(ff, "output_dense", None), torch.nn.Linear))


_SUPPORT_CACHE: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def packed_supported(model: torch.nn.Module) -> bool:
    """Whether packed_logits can run this model: a transformers Wav2Vec2ForCTC-shaped model in
    eval mode (no adapters) whose feature encoder, positional conv and encoder layers the
    packed encoder runs from their weights (WX_NO_PACKED=1: never).  The model needs no
    prepare_model: the packed path calls no patched forward.  The structural check is cached
    per model (keyed on its encoder and layer list: ~0.4 ms of host time per call otherwise)."""
    if os.environ.get("WX_NO_PACKED") or model.training:
        return False
    enc = getattr(getattr(model, "wav2vec2", None), "encoder", None)
    layers = getattr(enc, "layers", None)
    n = (id(enc), id(layers), len(layers) if layers is not None else -1)
    hit = _SUPPORT_CACHE.get(model)
    if hit is not None and hit[0] == n:
        return hit[1]
    ok = _packed_structure_ok(model)
    try:
        _SUPPORT_CACHE[model] = (n, ok)
    except TypeError:  # (a model that cannot be weakly referenced: not cached)
        pass
    return ok


def _packed_structure_ok(model: torch.nn.Module) -> bool:
    w2v = getattr(model, "wav2vec2", None)
    head = getattr(model, "lm_head", None)
    if w2v is None or not isinstance(head, torch.nn.Linear) or getattr(w2v, "adapter", None) is not None:
        return False
    enc = getattr(w2v, "encoder", None)
    fp = getattr(w2v, "feature_projection", None)
    if (type(enc).__name__ not in _PACK_ENCODERS or fp is None or not hasattr(w2v, "feature_extractor")
            or not hasattr(enc, "pos_conv_embed") or _fe_layers(w2v.feature_extractor) is None
            or _posconv_weights(enc.pos_conv_embed, probe=True) is None):
        return False
    D = getattr(getattr(enc, "layer_norm", None), "normalized_shape", (0,))[0]
    return D in _ADDLN_WIDTHS and all(_layer_ok(layer, D) for layer in enc.layers)


_PC_CACHE: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _posconv_weights(pce, probe: bool = False):
    """(w_packed, bias, G, K) for wx_posconv_packed when the positional conv embedding is
    wav2vec2's (Conv1d K = 128, padding 64, G groups of 48 or 64 channels, the last output
    dropped, erf GELU), else None.  w_packed [G][K][Cg / 4][Cg][4] is cached per module until
    a parameter changes."""
    conv = getattr(pce, "conv", None)
    pad = getattr(pce, "padding", None)
    if (os.environ.get("WX_NO_POSCONV") or not isinstance(conv, torch.nn.Conv1d)
            or conv.kernel_size != (128,) or conv.stride != (1,) or conv.dilation != (1,)
            or isinstance(conv.padding, str) or conv.padding != (64,) or conv.padding_mode != "zeros"
            or getattr(pad, "num_pad_remove", None) != 1 or not _is_erf_gelu(getattr(pce, "activation", None))):
        return None
    G = conv.groups
    D = conv.out_channels
    if conv.in_channels != D or D % G or D // G not in (48, 64):
        return None
    if probe:
        return True
    w = _weight(conv)
    key = (w.data_ptr(), _version(w)) + tuple((t.data_ptr(), _version(t)) for t in conv.parameters())
    c = _PC_CACHE.get(conv)
    if c is None or c[0] != key:
        Cg = D // G
        with torch.no_grad():
            wp = (w.detach().reshape(G, Cg, Cg, 128).permute(0, 3, 2, 1)   # [G, K, Cg_in, Cg_out]
                  .reshape(G, 128, Cg // 4, 4, Cg).permute(0, 1, 2, 4, 3).contiguous())
        c = (key, wp)
        _PC_CACHE[conv] = c
    return c[1], conv.bias, G, 128


def _packed_encoder(enc, h: torch.Tensor, segs) -> torch.Tensor:
    """Wav2Vec2Encoder(.StableLayerNorm).forward (no mask, eval) over packed rows h [1, R, D]."""
    from . import _lib

    stable = type(enc).__name__ == "Wav2Vec2EncoderStableLayerNorm"
    ln = enc.layer_norm
    pc = _posconv_weights(enc.pos_conv_embed) if h.is_contiguous() and h.data_ptr() % 16 == 0 else None
    if pc is not None:
        # h + GELU(positional conv) per segment in one kernel (wx_posconv_packed)
        s = _lib.posconv_packed(h, pc[0], pc[1], pc[2], pc[3], segs, residual=True)
        h = s if stable else ln(s)
    else:
        pos = torch.empty_like(h)
        for a, b in zip(segs.offsets[:-1], segs.offsets[1:]):
            if b > a:
                pos[:, a:b] = enc.pos_conv_embed(h[:, a:b])
        if stable:
            h = h + pos
        elif _addln_ok(enc, h, (ln,)):
            h = _lib.add_layernorm(h, pos, ln.weight, ln.bias, ln.eps)
        else:
            h = ln(h + pos)
    for layer in enc.layers:
        h = _packed_layer(layer, h, segs, stable)
    return ln(h) if stable else h


def _packed_layer(layer, h: torch.Tensor, segs, stable: bool) -> torch.Tensor:
    """Wav2Vec2EncoderLayer (post-norm) / Wav2Vec2EncoderLayerStableLayerNorm (pre-norm) of an
    eval forward over packed rows h [1, R, D], from the layer's weights: one q/k/v GEMM,
    per-segment attention (wx_attention_f32_packed), the output projection, each
    `norm(residual + x)` as one wx_add_layernorm."""
    from . import _lib

    att = layer.attention
    ln, fln = layer.layer_norm, layer.final_layer_norm
    R, D = h.shape[1], h.shape[2]
    H = D // 64
    w, b = _qkv_weights(att.q_proj, att.k_proj, att.v_proj)
    x = ln(h) if stable else h
    qkv = F.linear(x, w, b)  # [1, R, 3D]
    q, k, v = (qkv[..., i * D:(i + 1) * D].view(1, R, H, 64).transpose(1, 2) for i in range(3))
    scale = getattr(att, "scaling", None) or 64 ** -0.5
    o = _lib.attention_f32_packed(q, k, v, scale, segs, _PACK_SPLIT).reshape(1, R, D)
    o = att.out_proj(o)
    if stable:
        y, s = _lib.add_layernorm(h, o, fln.weight, fln.bias, fln.eps, want_sum=True)
        return s + layer.feed_forward(y)
    h1 = _lib.add_layernorm(h, o, ln.weight, ln.bias, ln.eps)
    return _lib.add_layernorm(h1, layer.feed_forward(h1), fln.weight, fln.bias, fln.eps)


_FE_KINDS = {"Wav2Vec2GroupNormConvLayer": "group", "Wav2Vec2LayerNormConvLayer": "layer",
             "Wav2Vec2NoLayerNormConvLayer": "none"}


def _fe_layers(fe):
    """(kind, conv, norm, activation) per feature-encoder layer when every layer is one of
    transformers' three conv-layer classes with a plain (ungrouped, unpadded, dilation 1) conv;
    None otherwise."""
    out = []
    for layer in getattr(fe, "conv_layers", ()):
        kind = _FE_KINDS.get(type(layer).__name__)
        conv = getattr(layer, "conv", None)
        if (kind is None or not isinstance(conv, torch.nn.Conv1d) or conv.groups != 1 or conv.dilation != (1,)
                or isinstance(conv.padding, str) or conv.padding != (0,) or conv.padding_mode != "zeros"):
            return None
        norm = getattr(layer, "layer_norm", None) if kind != "none" else None
        if kind == "group" and not (isinstance(norm, torch.nn.GroupNorm) and norm.num_groups == conv.out_channels
                                    and conv.out_channels % 4 == 0):
            return None
        if kind == "layer" and not isinstance(norm, torch.nn.LayerNorm):
            return None
        out.append((kind, conv, norm, layer.activation))
    return out or None


def _tm_conv(conv: torch.nn.Conv1d, x: torch.Tensor, Lout: int, operands=None) -> torch.Tensor:
    """Time-major conv of a packed buffer: x [L, Cin] (or [L] samples for Cin == 1) ->
    [Lout, Cout], y[t] = bias + sum_j x[s t + j] W_j (tap GEMMs on strided row views).
    `operands`: (tap weights as _tap_weights lays them out, bias) in x's dtype instead of the
    conv's own (the half route's rounded copies)."""
    (k,) = conv.kernel_size
    (s,) = conv.stride
    wt, b = operands if operands is not None else (_tap_weights(conv), conv.bias)
    Cout = conv.out_channels
    if conv.in_channels == 1:
        x1 = x.reshape(-1)
        patches = x1.as_strided((Lout, k), (s, 1))
        w = wt.reshape(k, Cout)
        return torch.addmm(b, patches, w) if b is not None else torch.mm(patches, w)
    # wt: [k, Cin, Cout]
    out = torch.empty((Lout, Cout), dtype=x.dtype, device=x.device)
    Cin = conv.in_channels
    if os.environ.get("WX_FE_TAPS"):  # (A/B: one GEMM per tap)
        groups = [(j, 1) for j in range(k)]
        rs = s * Cin
    else:
        # taps s g .. s g + s - 1 read s consecutive rows of x: one contiguous s Cin-wide row of
        # the view with row stride s Cin, so they are ONE GEMM with K = s Cin (k = 3, s = 2: two
        # GEMMs, K = 1024 and 512, instead of three; k = 2, s = 2: one GEMM, no accumulation)
        groups = [(j, min(s, k - j)) for j in range(0, k, s)]
        rs = s * Cin
    for n, (j, r) in enumerate(groups):
        xj = x.as_strided((Lout, r * Cin), (rs, 1), x.storage_offset() + j * Cin)
        wj = wt[j:j + r].reshape(r * Cin, Cout)
        if n == 0:
            if b is not None:
                torch.addmm(b, xj, wj, out=out)
            else:
                torch.mm(xj, wj, out=out)
        else:
            out.addmm_(xj, wj)
    return out


def _act_(act, y: torch.Tensor) -> torch.Tensor:
    if _is_erf_gelu(act):
        torch._C._nn.gelu_(y)
        return y
    return act(y)


def packed_features(fe, layers, waveforms, segs, dev, half=None, kernels: bool = True) -> torch.Tensor:
    """The feature encoder of every waveform in one pass per layer: [segs.rows, C] time-major,
    rows packed like `segs`.  `half` (half_operands' result): the half route, whose layers run in
    _fe_layer_half on the same layout and return half.dtype (`kernels`: its HIP kernels or torch).

    The waveforms are laid out back to back in one sample buffer, each from an offset that is
    a multiple of the product P of the layers' strides (320 for wav2vec2), zero-filled between
    (and up to the reference's 400-sample minimum, alignment.py:217-224).  A layer of stride s
    maps input row s (o + t) + j to output row o + t, so with every segment's input offset a
    multiple of s its outputs start at offset / s and read only its own inputs: one GEMM per
    tap over the whole buffer computes every segment's conv exactly as alone; the few rows
    between segments (outputs that straddle two of them) are computed and ignored.  The
    group-norm layer (per-channel statistics over one segment's time) runs per segment on its
    own rows.  The last layer's segment rows are gathered into the packed layout."""
    from . import _lib

    ks = [(c.kernel_size[0], c.stride[0]) for _, c, _, _ in layers]
    P = 1
    for _, st in ks:
        P *= st
    ns = [max(int(w.shape[-1]), 400) for w in waveforms]
    regions = [-(-n // P) * P for n in ns]
    offs = [0]
    for r in regions:
        offs.append(offs[-1] + r)
    x = torch.zeros(offs[-1] + P, dtype=torch.float32, device=dev)
    for w, o in zip(waveforms, offs):
        w1 = w.reshape(-1)
        x[o: o + w1.shape[0]].copy_(w1, non_blocking=True)
    offs = offs[:-1]
    lens = ns
    X = x
    for i, ((kind, conv, norm, act), (k, st)) in enumerate(zip(layers, ks)):
        Lg = X.shape[0]
        Lout = (Lg - k) // st + 1
        new_offs = [o // st for o in offs]
        new_lens = [(n - k) // st + 1 if n >= k else 0 for n in lens]
        if half is not None:
            Y = _fe_layer_half(half, kernels, i, layers[i], X, Lout, offs, lens, new_offs, new_lens)
        elif kind == "group":
            gelu = _is_erf_gelu(act)
            if (conv.in_channels == 1 and k <= 16 and not os.environ.get("WX_NO_CONV0_FUSED")):
                Y = torch.empty((Lout, conv.out_channels), dtype=torch.float32, device=dev)
                w = _weight(conv)
                for o, n, oo, lo in zip(offs, lens, new_offs, new_lens):
                    _lib.conv0_channel_norm(X[o: o + n], w, conv.bias, st, norm.weight, norm.bias, norm.eps, gelu,
                                            out=Y[oo: oo + lo])
            else:
                Y = _tm_conv(conv, X, Lout)
                for oo, lo in zip(new_offs, new_lens):
                    _lib.channel_norm(Y[oo: oo + lo], norm.weight, norm.bias, norm.eps, gelu, out=Y[oo: oo + lo])
            if not gelu:
                Y = act(Y)
        else:
            Y = _tm_conv(conv, X, Lout)
            if kind == "layer":
                Y = norm(Y)
            Y = _act_(act, Y)
        X, offs, lens = Y, new_offs, new_lens
    if lens != segs.lengths:
        raise ValueError(f"feature encoder frame counts {lens} differ from the packed layout's {segs.lengths}")
    if offs == segs.offsets[:-1]:
        return X[: segs.rows]
    idx = torch.cat([torch.arange(o, o + n, dtype=torch.int64) for o, n in zip(offs, lens)])
    return X.index_select(0, idx.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else idx)


def packed_logits(model: torch.nn.Module, waveforms, segs, streams, dtype: torch.dtype = torch.float32,
                  kernels: Optional[bool] = None) -> torch.Tensor:
    """The [R, V] logits of every waveform (segments packed by rows as `segs`, a
    _lib.PackedSegments of their frame counts) on the current stream: feature encoders per
    segment, round-robin over `streams` (each segment's features joined into the pack by a
    copy on the current stream), then one packed projection / encoder / lm_head pass.
    Raises ValueError when a feature encoder's frame count is not segs' (caller falls back).
    `dtype` float16 / bfloat16: the half route (_packed_logits_half; fp32 logits all the same),
    on its HIP kernels when the model is on a HIP device, in torch ops otherwise (`kernels`
    overrides that choice)."""
    if dtype != torch.float32:
        return _packed_logits_half(model, waveforms, segs, dtype, kernels)
    from . import _lib

    w2v = model.wav2vec2
    cur = torch.cuda.current_stream()
    dev = cur.device
    C = int(w2v.config.conv_dim[-1])
    layers = None if os.environ.get("WX_NO_PACKED_FE") else _fe_layers(w2v.feature_extractor)
    if layers is not None:
        with torch.inference_mode():
            feats = packed_features(w2v.feature_extractor, layers, waveforms, segs, dev)
            h, _ = w2v.feature_projection(feats[None])
            del feats
            h = _packed_encoder(w2v.encoder, h, segs)
            return model.lm_head(h)[0]
    feats = torch.empty((segs.rows, C), dtype=torch.float32, device=dev)
    with torch.inference_mode():
        for st in streams:
            st.wait_stream(cur)
        for i, w in enumerate(waveforms):
            a, b = segs.offsets[i], segs.offsets[i + 1]
            st = streams[i % len(streams)]
            with torch.cuda.stream(st):
                x = w.to(dev, non_blocking=True)
                if x.dim() == 1:
                    x = x[None]
                if x.shape[-1] < 400:  # alignment.py:217-224 (the model's receptive field)
                    x = F.pad(x, (0, 400 - x.shape[-1]))
                f = w2v.feature_extractor(x)  # [1, C, T] (a view of a time-major buffer)
            if tuple(f.shape) != (1, C, b - a):
                cur.wait_stream(st)
                raise ValueError(f"feature encoder gave {tuple(f.shape)} for segment {i}, expected (1, {C}, {b - a})")
            cur.wait_stream(st)
            feats[a:b].copy_(f[0].transpose(0, 1))
            f.record_stream(cur)
        h, _ = w2v.feature_projection(feats[None])
        del feats
        h = _packed_encoder(w2v.encoder, h, segs)
        return model.lm_head(h)[0]


# ------------------------------------------------------------------------------------------
# The half route of the packed forward (float16 / bfloat16), opt-in through packed_logits' dtype.
#
# Rounded to dtype: the feature encoder's activations from layer 0's output on (layers >= 1 run
# in dtype through torch: tap GEMMs, bias, the "layer" family's norm, GELU); the feature
# projection's operand and result; in every encoder layer the norm's output as a GEMM operand,
# the q/k/v GEMM, attention (wx_attention_h16_packed in place on that GEMM's output), the out
# projection, FF1, GELU, FF2; the lm_head's operand and logits; every weight and bias of those
# GEMMs and convolutions (half_operands' cached copies).
# Not rounded: the waveform and layer 0's arithmetic (conv, GroupNorm / LayerNorm, GELU: fp32,
# rounded once on the store), the feature projection's LayerNorm statistics, the positional
# conv (wx_posconv_packed on the fp32 stream), the residual stream and every LayerNorm of the
# encoder (fp32 in, fp32 statistics), attention's scores, softmax statistics and accumulators,
# log_softmax and everything after it.  The caller's model stays fp32.

_HALF_DTYPES = (torch.float16, torch.bfloat16)
_HALF_CACHE: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()  # model -> {dtype: (key, operands)}


def half_operands(model: torch.nn.Module, dtype: torch.dtype):
    """The model's GEMM and conv operands rounded to `dtype` (float16 / bfloat16), cached outside
    the model until a parameter changes (keyed on every parameter's storage and version, and on
    dtype).  ValueError for another dtype, for a model packed_supported rejects, and for a tensor
    that is not finite after rounding (named)."""
    if dtype not in _HALF_DTYPES:
        raise ValueError(f"the half route runs in float16 or bfloat16, not {dtype}")
    if not packed_supported(model):
        raise ValueError(f"the half route needs a model the packed encoder runs (a transformers Wav2Vec2ForCTC in eval "
                         f"mode, head size 64, no adapters): {type(model).__name__} is not one")
    key = tuple((t.data_ptr(), _version(t)) for t in model.parameters())
    per = _HALF_CACHE.get(model)
    hit = per.get(dtype) if per is not None else None
    if hit is not None and hit[0] == key:
        return hit[1]
    ops = _build_half_operands(model, dtype)
    if per is None:
        per = _HALF_CACHE[model] = {}
    per[dtype] = (key, ops)
    return ops


def _build_half_operands(model: torch.nn.Module, dtype: torch.dtype):
    names = {id(t): n for n, t in model.named_parameters()}
    checks = []

    def r(t):
        if t is None:
            return None
        h = t.detach().to(dtype).contiguous()
        checks.append((names.get(id(t), "?"), torch.isfinite(h).all()))
        return h

    w2v = model.wav2vec2
    ops = types.SimpleNamespace(dtype=dtype, fe=[], layers=[])
    with torch.no_grad():
        for i, (kind, conv, norm, _) in enumerate(_fe_layers(w2v.feature_extractor)):
            if i == 0:  # layer 0 runs in fp32 on the fp32 waveform
                ops.fe.append(None)
                continue
            ops.fe.append(types.SimpleNamespace(
                conv=(r(conv.weight).permute(2, 1, 0).contiguous(), r(conv.bias)),  # taps as _tap_weights: [k, Cin, Cout]
                norm=(r(norm.weight), r(norm.bias)) if kind == "layer" else None))
        proj = w2v.feature_projection.projection
        ops.proj = (r(proj.weight), r(proj.bias))
        for layer in w2v.encoder.layers:
            att, ff = layer.attention, layer.feed_forward
            qkv = (att.q_proj, att.k_proj, att.v_proj)
            ops.layers.append(types.SimpleNamespace(
                qkv=(torch.cat([r(m.weight) for m in qkv], 0), torch.cat([r(m.bias) for m in qkv])),
                out=(r(att.out_proj.weight), r(att.out_proj.bias)),
                ff1=(r(ff.intermediate_dense.weight), r(ff.intermediate_dense.bias)),
                ff2=(r(ff.output_dense.weight), r(ff.output_dense.bias))))
        ops.head = (r(model.lm_head.weight), r(model.lm_head.bias))
        finite = torch.stack([ok for _, ok in checks]).tolist()  # (one device->host copy for all of them)
    for (name, _), ok in zip(checks, finite):
        if not ok:
            raise ValueError(f"the half route: tensor '{name}' is not finite when rounded to "
                             f"{str(dtype).replace('torch.', '')}")
    return ops


def _fe_layer_half(half, kernels: bool, i: int, layer, X, Lout, offs, lens, new_offs, new_lens) -> torch.Tensor:
    """Feature-encoder layer i of packed_features on the half route: [Lout, C] in half.dtype.
    Layer 0 reads the fp32 waveform and computes in fp32, rounded once on the way out (the
    "group" family: wx_conv0_channel_norm_h16, whose store is the rounding); later layers run in
    half.dtype through torch on the rounded operands."""
    from . import _lib

    kind, conv, norm, act = layer
    dtype = half.dtype
    if i > 0:
        Y = _tm_conv(conv, X, Lout, half.fe[i].conv)
        if kind == "layer":
            Y = F.layer_norm(Y, (conv.out_channels,), *half.fe[i].norm, norm.eps)
        return _act_(act, Y)
    (k,) = conv.kernel_size
    (st,) = conv.stride
    if kind != "group":
        Y = _tm_conv(conv, X, Lout)
        if kind == "layer":
            Y = norm(Y)
        return _act_(act, Y).to(dtype)
    gelu = _is_erf_gelu(act)
    if kernels and gelu and conv.in_channels == 1 and k <= 16:
        Y = torch.empty((Lout, conv.out_channels), dtype=dtype, device=X.device)
        w = _weight(conv)
        for o, n, oo, lo in zip(offs, lens, new_offs, new_lens):
            _lib.conv0_channel_norm_h16(X[o: o + n], w, conv.bias, st, norm.weight, norm.bias, norm.eps, True, dtype,
                                        out=Y[oo: oo + lo])
        return Y
    Y = _tm_conv(conv, X, Lout)
    for oo, lo in zip(new_offs, new_lens):
        seg = Y[oo: oo + lo]
        if kernels:
            _lib.channel_norm(seg, norm.weight, norm.bias, norm.eps, gelu, out=seg)
        elif lo:
            mean, var = seg.mean(0), seg.var(0, unbiased=False)
            seg.copy_((seg - mean) * torch.rsqrt(var + norm.eps) * norm.weight + norm.bias)
            if gelu:
                torch._C._nn.gelu_(seg)
    return (Y if gelu else act(Y)).to(dtype)


def _attention_half_host(qkv: torch.Tensor, segs, H: int, scale: float) -> torch.Tensor:
    """Per-segment attention of the half route in torch ops: the rounded q / k / v [R, 3 * 64 H]
    widened, an fp32 softmax, the result [R, 64 H] rounded to qkv's dtype."""
    R, D = qkv.shape[0], 64 * H
    o = torch.empty((R, D), dtype=qkv.dtype, device=qkv.device)
    for a, b in zip(segs.offsets[:-1], segs.offsets[1:]):
        if b > a:
            q, k, v = (qkv[a:b, j * D:(j + 1) * D].float().view(b - a, H, 64).transpose(0, 1) for j in range(3))
            p = torch.softmax(scale * (q @ k.transpose(1, 2)), -1)
            o[a:b] = (p @ v).transpose(0, 1).reshape(b - a, D).to(qkv.dtype)
    return o


def _packed_encoder_half(enc, h: torch.Tensor, segs, ops, kernels: bool) -> torch.Tensor:
    """_packed_encoder on the half route over packed rows h [R, D] (the fp32 residual stream):
    the encoder's output rounded to ops.dtype, the lm_head's operand.  The stream and every
    LayerNorm are fp32; a norm's output is rounded once as the next GEMM's operand.  Post-norm
    layers need each norm in both forms (wx_add_layernorm_h16_dual); pre-norm layers fuse each
    add with the norm after it and keep the sum (wx_add_layernorm_h16)."""
    from . import _lib

    dtype = ops.dtype
    stable = type(enc).__name__ == "Wav2Vec2EncoderStableLayerNorm"
    R, D = h.shape
    H = D // 64

    def dual(a, b, n, want_y32=True):  # norm(a + float(b)) in fp32 and rounded
        if kernels:
            return _lib.add_layernorm_h16_dual(a, b, n.weight, n.bias, n.eps, dtype, want_y32=want_y32)
        y = F.layer_norm(a if b is None else a + b.float(), (D,), n.weight, n.bias, n.eps)
        return y, y.to(dtype)

    def pre(a, b, n, want_sum=True):  # round(norm(a + float(b))), a + float(b)
        if kernels:
            if b is None or not want_sum:
                return _lib.add_layernorm_h16(a, b, n.weight, n.bias, n.eps, dtype), a
            return _lib.add_layernorm_h16(a, b, n.weight, n.bias, n.eps, dtype, want_sum=True)
        s = a if b is None else a + b.float()
        return F.layer_norm(s, (D,), n.weight, n.bias, n.eps).to(dtype), s

    def attention(x, layer, L):
        qkv = F.linear(x, *L.qkv)  # [R, 3D]
        scale = getattr(layer.attention, "scaling", None) or 64 ** -0.5
        if kernels:
            q, k, v = (qkv[None, :, j * D:(j + 1) * D].view(1, R, H, 64).transpose(1, 2) for j in range(3))
            o = _lib.attention_h16_packed(q, k, v, scale, segs).reshape(R, D)
        else:
            o = _attention_half_host(qkv, segs, H, scale)
        return F.linear(o, *L.out)

    def feed_forward(x, layer, L):
        return F.linear(layer.feed_forward.intermediate_act_fn(F.linear(x, *L.ff1)), *L.ff2)

    pc = _posconv_weights(enc.pos_conv_embed) if kernels and h.is_contiguous() and h.data_ptr() % 16 == 0 else None
    if pc is not None:
        s = _lib.posconv_packed(h, pc[0], pc[1], pc[2], pc[3], segs, residual=True)
    else:
        s = h.clone()
        for a, b in zip(segs.offsets[:-1], segs.offsets[1:]):
            if b > a:
                s[a:b] += enc.pos_conv_embed(h[None, a:b])[0]
    ln = enc.layer_norm
    n = len(ops.layers)
    if not stable:
        x32, x16 = dual(s, None, ln)
        for i, (layer, L) in enumerate(zip(enc.layers, ops.layers)):
            x32, x16 = dual(x32, attention(x16, layer, L), layer.layer_norm)
            x32, x16 = dual(x32, feed_forward(x16, layer, L), layer.final_layer_norm, want_y32=i < n - 1)
        return x16
    x, pending = s, None
    for layer, L in zip(enc.layers, ops.layers):
        y, x = pre(x, pending, layer.layer_norm)
        pending = attention(y, layer, L)
        y, x = pre(x, pending, layer.final_layer_norm)
        pending = feed_forward(y, layer, L)
    return pre(x, pending, ln, want_sum=False)[0]


def _packed_logits_half(model: torch.nn.Module, waveforms, segs, dtype: torch.dtype,
                        kernels: Optional[bool] = None) -> torch.Tensor:
    """packed_logits on the half route: the same chain with the rounding points listed above, on
    the HIP kernels (`kernels`; the default on a HIP device) or in torch ops with the same
    rounding points (a CPU model; attention per segment in _attention_half_host).  fp32 logits."""
    w2v = model.wav2vec2
    ops = half_operands(model, dtype)
    dev = ops.head[0].device
    if kernels is None:
        kernels = dev.type == "cuda"
    layers = _fe_layers(w2v.feature_extractor)
    with torch.inference_mode():
        feats = packed_features(w2v.feature_extractor, layers, waveforms, segs, dev, half=ops, kernels=kernels)
        fln = w2v.feature_projection.layer_norm
        y = F.layer_norm(feats.float(), tuple(fln.normalized_shape), fln.weight, fln.bias, fln.eps).to(dtype)
        del feats
        h = F.linear(y, *ops.proj).float()
        y = _packed_encoder_half(w2v.encoder, h, segs, ops, kernels)
        return F.linear(y, *ops.head).float()

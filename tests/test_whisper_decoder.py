"""WhisperDecoder without a GPU: the accepted weight forms and the refusals, the host route
against transformers' decoder (fp64 as the reference, 4 x the stock fp32 route's own error as the
bound; greedy decoding token for token against the fp64 greedy loop), the limits, and the four
wx_decode_attention_* entry points' argument validation (no device needed: they return before
anything is enqueued)."""
import ctypes

import pytest
import torch

from whisper_decoder_helpers import (GEOMETRIES, PROMPT, case, check_detect_language, check_forced_logits, check_greedy,
                                     check_stopping, check_suppression)
from whisper_helpers import openai_names

SMALL = GEOMETRIES[0]


def _host(weights):
    from whisperx_amd import WhisperDecoder

    return WhisperDecoder(weights, device="cpu")


def _tensors(dec):
    out = [dec.embed, dec.pos, *dec.ln_f]
    for L in dec.layers:
        for pair in L.values():
            out += list(pair)
    return out


def _same(a, b):
    ta, tb = _tensors(a), _tensors(b)
    return len(ta) == len(tb) and all(torch.equal(x, y) for x, y in zip(ta, tb)) and \
        (a.D, a.H, a.V, a.max_target_positions, len(a.layers)) == (b.D, b.H, b.V, b.max_target_positions, len(b.layers))


def test_every_weight_form_gives_the_same_tensors():
    c = case(*SMALL)
    model = c.model
    want = _host(model)
    assert (want.D, want.H, want.V, want.max_target_positions, len(want.layers)) == (384, 6, 96, 40, 2)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert _same(_host(model.model), want) and _same(_host(model.model.decoder), want)
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())  # the module is only read
    sd = {k: v.clone() for k, v in model.model.decoder.state_dict().items()}
    for prefix in ("", "decoder.", "model.decoder."):
        assert _same(_host({prefix + k: v for k, v in sd.items()}), want), prefix
    assert _same(_host(openai_names(sd, "decoder")), want)
    # a dict of a whole model: the encoder's tensors are ignored, the tied proj_out.weight accepted
    whole = dict(model.state_dict())
    assert "proj_out.weight" in whole and any(k.startswith("model.encoder.") for k in whole)
    assert _same(_host(whole), want)


def test_load_whisper_decoder_round_trip(tmp_path):
    from safetensors.torch import save_file

    from whisperx_amd import load_whisper_decoder

    c = case(*SMALL)
    want = _host(c.model)
    sd = {"model.decoder." + k: v.clone().contiguous() for k, v in c.model.model.decoder.state_dict().items()}
    save_file(sd, str(tmp_path / "dec.safetensors"))
    torch.save(sd, tmp_path / "dec.pt")
    for name in ("dec.safetensors", "dec.pt"):
        assert _same(load_whisper_decoder(str(tmp_path / name), device="cpu"), want), name


def test_refusals_name_the_tensor():
    c = case(*SMALL)
    sd = dict(c.model.model.decoder.state_dict())
    with pytest.raises(ValueError, match=r"layers\.1\.encoder_attn\.out_proj\.bias"):
        _host({k: v for k, v in sd.items() if k != "layers.1.encoder_attn.out_proj.bias"})
    with pytest.raises(ValueError, match=r"layers\.0\.fc2\.weight"):
        _host({**sd, "layers.0.fc2.weight": torch.zeros(384, 100)})
    with pytest.raises(ValueError, match=r"encoder_attn\.k_proj\.bias"):
        _host({**sd, "layers.0.encoder_attn.k_proj.bias": torch.zeros(384)})
    with pytest.raises(ValueError, match=r"embed_tokens\.weight"):
        _host({**sd, "embed_tokens.weight": torch.zeros(96, 96)})  # head size: no multiple of 64
    with pytest.raises(ValueError, match=r"embed_positions\.weight"):
        _host({**sd, "embed_positions.weight": torch.zeros(40, 64)})
    with pytest.raises(ValueError, match="embed_tokens"):
        _host({k: v for k, v in sd.items() if k != "embed_tokens.weight"})
    with pytest.raises(ValueError):
        _host(42)


def test_untied_output_projection_is_refused():
    c = case(*SMALL)
    sd = dict(c.model.state_dict())
    _host(sd)  # tied: accepted
    untied = {**sd, "proj_out.weight": sd["proj_out.weight"] + 1e-3}
    with pytest.raises(ValueError, match=r"proj_out\.weight"):
        _host(untied)
    with pytest.raises(ValueError, match=r"proj_out\.weight"):
        _host({**dict(c.model.model.decoder.state_dict()), "proj_out.weight": torch.zeros(96, 384)})


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_host_route_logits_against_the_oracle(geometry):
    c = case(*geometry)
    check_forced_logits(c, _host(c.model), "host")


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_host_route_greedy_equals_the_fp64_loop(geometry):
    c = case(*geometry)
    check_greedy(c, _host(c.model), "host")


def test_host_route_stopping_and_suppression():
    c = case(*SMALL)
    dec = _host(c.model)
    check_stopping(c, dec)
    check_suppression(c, dec, "host")


def test_host_route_detect_language():
    c = case(*SMALL)
    check_detect_language(c, _host(c.model), "host")


def test_limits():
    c = case(*SMALL)
    dec = _host(c.model)
    st = dec.start(c.enc)
    tok = torch.zeros(c.B, dtype=torch.int64)
    for _ in range(dec.max_target_positions):
        dec.step(st, tok)
    with pytest.raises(ValueError, match="max_target_positions"):
        dec.step(st, tok)
    with pytest.raises(ValueError, match="negative"):
        dec.generate(c.enc, PROMPT, 2, suppress_tokens=[-1])
    with pytest.raises(ValueError, match="negative"):
        dec.generate(c.enc, PROMPT, 2, suppress_at_start=[3, -1])
    with pytest.raises(ValueError, match=r"\[0, 96\)"):
        dec.step(dec.start(c.enc), torch.tensor([0, 96, 1]))
    with pytest.raises(ValueError):
        dec.start(c.enc[:, :, :100])
    # the total length is bounded by min(max_length, max_target_positions)
    assert [len(r) for r in dec.generate(c.enc, PROMPT, 95, max_length=3 + 5)] == [5] * c.B
    assert max(len(r) for r in dec.generate(c.enc, PROMPT, 95, max_length=448)) <= 40 - 3


@pytest.mark.parametrize("half", [False, True], ids=["f32", "h16"])
@pytest.mark.parametrize("grouped", [False, True], ids=["ungrouped", "grouped"])
def test_decode_attention_entry_validates_before_anything_is_enqueued(half, grouped):
    """No device: every case of every entry point returns before a launch (dummy, aligned, never
    dereferenced pointers).  One table for the four: the grouped forms take G and three q strides,
    the half forms a dtype and strides in multiples of 8."""
    from whisperx_amd import _lib

    lib = _lib.load(require_device=False)
    fn = getattr(lib, f"wx_decode_attention_{'h16' if half else 'f32'}{'_grouped' if grouped else ''}")
    p = ctypes.c_void_p(1 << 20)
    qs = (ctypes.c_int64 * 3)(5 * 6 * 64, 6 * 64, 64) if grouped else (ctypes.c_int64 * 2)(6 * 64, 64)
    ks = (ctypes.c_int64 * 3)(6 * 448 * 64, 448 * 64, 64)

    def needed(B, G, H, L):
        if grouped:
            return lib.wx_decode_attention_grouped_workspace_bytes(B, G, H, L)
        return lib.wx_decode_attention_workspace_bytes(B, H, L)

    def call(B=2, G=5, H=6, L=300, D=64, ws=None, q=p, o=p, q_strides=qs, k_strides=ks, dtype=1):
        dims = (B, G, H, L, D) if grouped else (B, H, L, D)
        return fn(q, p, p, o, *dims, q_strides, k_strides, ks, 0.125, *((dtype,) if half else ()), p,
                  needed(B, G, H, L) if ws is None else ws, None)

    assert call(D=32) == 1001 and call(L=0) == 1001 and call(B=-1) == 1001 and call(H=0) == 1001
    assert call(B=0) == 0 and call(B=0, ws=0) == 0
    assert call(B=0, D=32) == 1001  # the shape is judged first
    if grouped:  # G outside 1 .. 8, before B == 0
        assert call(G=0) == 1001 and call(G=9) == 1001 and call(B=0, G=0) == 1001 and call(B=0, G=9) == 1001
        assert call(B=0, G=1) == 0 and call(B=0, G=8) == 0
    if half:  # a dtype that is neither fp16 nor bf16, before B == 0
        assert call(dtype=0) == 1001 and call(dtype=3) == 1001 and call(B=0, dtype=0) == 1001 and call(B=0, dtype=3) == 1001
        assert call(B=0, dtype=2) == 0
    assert call(q=None) == 1001 and call(o=ctypes.c_void_p((1 << 20) + 4)) == 1001
    assert call(k_strides=(ctypes.c_int64 * 3)(6 * 448 * 64, 448 * 64, 66)) == 1001  # rows off 16 bytes
    assert call(q_strides=(ctypes.c_int64 * 3)(5 * 6 * 64, 6 * 64 + 2, 64)) == 1001
    if half:  # 16 bytes are 8 elements: a multiple of 4 is not enough
        assert call(k_strides=(ctypes.c_int64 * 3)(6 * 448 * 64, 448 * 64, 68)) == 1001
        assert call(q_strides=(ctypes.c_int64 * 3)(5 * 6 * 64 + 4, 6 * 64, 64)) == 1001
    assert call(B=70000) == 1001
    need = needed(2, 5, 6, 300)
    assert call(ws=need - 1) == 1004
    assert need >= 2 * (5 if grouped else 1) * 6 * 3 * 66 * 4  # (m, l, acc[64]) per chunk
    wsb = lib.wx_decode_attention_workspace_bytes
    assert wsb(1, 1, 1) > 0
    assert wsb(1, 6, 1500) < wsb(2, 6, 1500) < wsb(16, 6, 1500)
    assert wsb(2, 6, 1) <= wsb(2, 6, 448) < wsb(2, 6, 1500) < wsb(2, 6, 30000)
    assert _lib.DECODE_CHUNK == 128 and wsb(1, 1, 128) == wsb(1, 1, 1) < wsb(1, 1, 129 + 128 * 64)

"""WhisperEncoder(dtype=float16 / bfloat16) without a GPU: the host route within 2 x ref_err_half of
transformers' fp64 encoder (whisper_half_helpers), the dtype argument's refusals, the file loader,
and the argument validation of wx_attention_h16 and wx_add_layernorm_h16 (no device needed: they
return before anything is enqueued)."""
import ctypes

import pytest
import torch

import whisper_half_helpers as hh
from whisper_helpers import case

DTYPES = [pytest.param(d, id=hh.name(d)) for d in hh.DTYPES]


@pytest.mark.parametrize("D,layers,P,B", [(384, 2, 50, 3), (512, 1, 33, 2), (768, 1, 33, 1), (1024, 1, 33, 2),
                                          (1280, 1, 33, 2)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_route_against_the_oracle(dtype, D, layers, P, B):
    from whisperx_amd import WhisperEncoder

    enc, x, y64, ref_err_half = hh.encoder_case(dtype, D, layers, P, B)
    we = WhisperEncoder(enc, device="cpu", dtype=dtype)
    assert we.dtype == dtype
    assert all(t.dtype == dtype for L in we.layers for n in ("qkv", "out", "fc1", "fc2") for t in L[n])
    assert all(t.dtype == torch.float32 for t in (we.w1, we.b1, we.w2, we.b2, we.pos, *we.ln_post))
    got = we.encode(x)
    assert tuple(got.shape) == (B, P, D) and got.dtype == torch.float32
    err = float((got.double() - y64).abs().max())
    print(f"half host route {hh.name(dtype)} D {D} layers {layers} P {P} B {B}: |host - fp64| {err:.3e}, ref_err_half "
          f"{ref_err_half:.3e}, ratio {err / ref_err_half:.3f} (bound 2)")
    assert err <= 2 * ref_err_half


def test_float32_is_the_default():
    from whisperx_amd import WhisperEncoder

    enc, x, _, _ = case(384, 2, 50, 3)
    a, b = WhisperEncoder(enc, device="cpu"), WhisperEncoder(enc, device="cpu", dtype=torch.float32)
    assert a.dtype == b.dtype == torch.float32
    assert torch.equal(a.encode(x), b.encode(x))


@pytest.mark.parametrize("dtype", [torch.float64, torch.int8, "float16", None])
def test_other_dtypes_are_refused(dtype):
    from whisperx_amd import WhisperEncoder

    enc, _, _, _ = case(384, 2, 50, 3)
    with pytest.raises(ValueError, match="dtype"):
        WhisperEncoder(enc, device="cpu", dtype=dtype)


@pytest.mark.parametrize("name", ["layers.1.self_attn.k_proj.weight", "layers.0.fc1.bias", "layers.1.self_attn.out_proj.weight"])
def test_a_weight_that_overflows_float16_is_named(name):
    from whisperx_amd import WhisperEncoder

    enc, x, _, _ = case(384, 2, 50, 3)
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    sd[name].view(-1)[3] = 7.0e4  # finite in fp32 and bf16, past fp16's 65504
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        WhisperEncoder(sd, device="cpu", dtype=torch.float16)
    for dtype in (torch.bfloat16, torch.float32):
        assert bool(torch.isfinite(WhisperEncoder(sd, device="cpu", dtype=dtype).encode(x)).all())
    # the stem and the norms stay fp32: the same value there is accepted
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    sd["conv1.bias"][0] = 7.0e4
    WhisperEncoder(sd, device="cpu", dtype=torch.float16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_load_whisper_encoder_takes_the_dtype(dtype, tmp_path):
    from whisperx_amd import WhisperEncoder, load_whisper_encoder

    enc, x, _, _ = case(384, 2, 50, 3)
    path = tmp_path / "encoder.pt"
    torch.save({"model.encoder." + k: v for k, v in enc.state_dict().items()}, path)
    we = load_whisper_encoder(str(path), device="cpu", dtype=dtype)
    assert we.dtype == dtype
    assert torch.equal(we.encode(x), WhisperEncoder(enc, device="cpu", dtype=dtype).encode(x))
    assert load_whisper_encoder(str(path), device="cpu").dtype == torch.float32


@pytest.fixture(scope="module")
def lib():
    from whisperx_amd import _lib

    _lib.build()
    return _lib.load(require_device=False)


def test_attention_h16_validation_without_device(lib):
    from whisperx_amd import _lib

    assert _lib.HALF_DTYPES == {torch.float16: 1, torch.bfloat16: 2}
    p = ctypes.c_void_p(4096)
    st = (ctypes.c_int64 * 3)(64 * 40 * 3, 64, 64 * 3)

    def call(q=p, k=p, v=p, o=p, B=2, H=3, T=40, D=64, sq=st, sk=st, sv=st, dtype=1):
        return lib.wx_attention_h16(q, k, v, o, B, H, T, D, sq, sk, sv, 0.125, dtype, None)

    INVALID = 1001
    assert call(B=-1) == INVALID and call(H=0) == INVALID and call(T=0) == INVALID and call(D=128) == INVALID
    assert call(dtype=0) == INVALID and call(dtype=3) == INVALID
    assert call(B=0) == 0 and call(B=0, q=None, k=None, v=None, o=None, sq=None, sk=None, sv=None) == 0
    assert call(B=0, dtype=4) == INVALID
    for name in ("q", "k", "v", "o", "sq", "sk", "sv"):
        assert call(**{name: None}) == INVALID
    for name in ("q", "k", "v", "o"):
        assert call(**{name: ctypes.c_void_p(4096 + 8)}) == INVALID
    for name in ("sq", "sk", "sv"):
        for i in range(3):
            bad = (ctypes.c_int64 * 3)(*(s + 4 if j == i else s for j, s in enumerate(st)))
            assert call(**{name: bad}) == INVALID
    assert call(B=1 << 20, H=1 << 12) == INVALID


def test_add_layernorm_h16_validation_without_device(lib):
    p = ctypes.c_void_p(4096)

    def call(a=p, b=p, rows=4, D=256, sa=256, sb=256, gamma=p, beta=p, dtype=2, y=p, s=None):
        return lib.wx_add_layernorm_h16(a, b, rows, D, sa, sb, gamma, beta, 1e-5, dtype, y, s, None)

    INVALID = 1001
    assert call(rows=-1) == INVALID and call(D=320) == INVALID and call(dtype=0) == INVALID
    assert call(rows=0, a=None, y=None) == 0 and call(rows=0, dtype=5) == INVALID
    for name in ("a", "gamma", "beta", "y"):
        assert call(**{name: None}) == INVALID
    for name in ("a", "b", "gamma", "beta", "y", "s"):
        assert call(**{name: ctypes.c_void_p(4096 + 8)}) == INVALID
    assert call(sa=252) == INVALID and call(sa=258) == INVALID and call(sb=248) == INVALID and call(sb=260) == INVALID

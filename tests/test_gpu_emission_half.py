"""The half route (float16 / bfloat16) of the packed wav2vec2 forward on the GPU: the kernel route
against fp64 (emission_half_helpers' rule), its plumbing through alignment._emissions and align(),
and the fp32 route left as it was."""
import copy
import warnings

import pytest
import torch

import emission_half_helpers as hh

pytestmark = pytest.mark.gpu


def _gpu_case(kind):
    model, wavs, _ = hh.case(kind)
    return copy.deepcopy(model).cuda().eval(), [w.cuda() for w in wavs]


def _spies(monkeypatch):
    from whisperx_amd import _lib

    calls = {"h16": 0, "f32": 0}
    h16, f32 = _lib.attention_h16_packed, _lib.attention_f32_packed

    def spy_h16(*a, **k):
        calls["h16"] += 1
        return h16(*a, **k)

    def spy_f32(*a, **k):
        calls["f32"] += 1
        return f32(*a, **k)

    monkeypatch.setattr(_lib, "attention_h16_packed", spy_h16)
    monkeypatch.setattr(_lib, "attention_f32_packed", spy_f32)
    return calls


@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
@pytest.mark.parametrize("kind", ["post", "stable", "post512"])
def test_kernel_route_within_twice_the_cast_models_error(kind, dtype, monkeypatch):
    from whisperx_amd import _lib, emission

    m, wavs = _gpu_case(kind)
    Ts = hh.frames(kind)
    calls = _spies(monkeypatch)
    lg = emission.packed_logits(m, wavs, _lib.PackedSegments(Ts), [torch.cuda.current_stream()], dtype=dtype)
    assert lg.dtype == torch.float32 and lg.shape == (sum(Ts), hh.VOCAB)
    assert calls == {"h16": 2, "f32": 0}  # one launch per layer
    hh.check_rule(kind, dtype, list(torch.log_softmax(lg, -1).split(Ts)), "kernel route")


@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
@pytest.mark.parametrize("kind", ["post", "stable"])
def test_kernel_route_and_host_arithmetic_agree_on_the_device(kind, dtype):
    """The same rounding plan in torch ops on the GPU: within 2 x ref_err_half of the kernels."""
    from whisperx_amd import _lib, emission

    m, wavs = _gpu_case(kind)
    Ts = hh.frames(kind)
    segs = _lib.PackedSegments(Ts)
    a = torch.log_softmax(emission.packed_logits(m, wavs, segs, None, dtype=dtype), -1)
    b = torch.log_softmax(emission.packed_logits(m, wavs, segs, None, dtype=dtype, kernels=False), -1)
    d = float((a.double() - b.double()).abs().max())
    err = hh.ref_err_half(kind, dtype)
    print(f"kernel vs host route, {kind} {hh.name(dtype)}: {d:.3e} (ref_err_half {err:.3e})")
    assert d <= 2 * err


@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
def test_emissions_take_the_half_packed_route(dtype, monkeypatch):
    from whisperx_amd import alignment

    m, wavs = _gpu_case("post")
    calls = _spies(monkeypatch)
    csr = alignment._emissions(m, "huggingface", wavs, "cuda:0", dtype=dtype)
    assert isinstance(csr, alignment._EmissionsCSR) and csr.groups, "not the packed route"
    main = torch.cuda.current_stream()
    for st in csr.streams:
        main.wait_stream(st)
    torch.cuda.synchronize()
    assert calls["h16"] > 0 and calls["f32"] == 0
    hh.check_rule("post", dtype, [csr[i] for i in range(len(wavs))], "_emissions")
    with pytest.raises(ValueError):
        alignment._emissions(m, "huggingface", wavs, "cuda:0", dtype=dtype, allow_packed=False)


def _words(out):
    return [[w["word"] for w in s["words"]] for s in out["segments"]]


def test_align_half_end_to_end(monkeypatch):
    """align() with {"dtype": torch.float16}: the fp32 call's segments and words, on the half route,
    the caller's model untouched, the rounded operands built once."""
    from whisperx_amd import align, emission

    m, wavs = _gpu_case("post")
    x = wavs[0]
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    attrs0 = {id(mod): set(mod.__dict__) for mod in m.modules()}
    with torch.inference_mode():
        y0 = m(x).logits.clone()
    segs, meta = hh.transcript()
    ref = align(copy.deepcopy(segs), m, meta, x[0], "cuda:0")
    calls = _spies(monkeypatch)
    built = []
    build = emission._build_half_operands

    def spy_build(*a, **k):
        built.append(1)
        return build(*a, **k)

    monkeypatch.setattr(emission, "_build_half_operands", spy_build)
    got = align(copy.deepcopy(segs), m, dict(meta, dtype=torch.float16), x[0], "cuda:0")
    assert calls["h16"] > 0 and calls["f32"] == 0, calls
    assert len(got["segments"]) == len(ref["segments"]) == 2
    assert [s["text"] for s in got["segments"]] == [s["text"] for s in ref["segments"]]
    assert _words(got) == _words(ref) and len(got["word_segments"]) == len(ref["word_segments"]) == 4
    n = calls["h16"]
    again = align(copy.deepcopy(segs), m, dict(meta, dtype=torch.float16), x[0], "cuda:0")
    assert built == [1], "the second call rebuilt the rounded operands"
    assert calls["h16"] == 2 * n and _words(again) == _words(ref)
    # the caller's model: fp32, no attribute of ours, the same state and the same stock forward
    assert {id(mod): set(mod.__dict__) for mod in m.modules()} == attrs0
    sd1 = m.state_dict()
    assert sd0.keys() == sd1.keys() and all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    with torch.inference_mode():
        assert torch.equal(m(x).logits, y0)


def test_align_on_cpu_with_a_half_model_runs_the_host_route(monkeypatch):
    """A CPU model and device="cpu" (the DP still runs on the GPU): the fp32 call's words."""
    from whisperx_amd import align, emission

    model, wavs, _ = hh.case("post")
    segs, meta = hh.transcript()
    ref = align(copy.deepcopy(segs), model, meta, wavs[0][0], "cpu")
    seen = []
    real = emission._packed_logits_half

    def spy(model_, waveforms, segs_, dtype, kernels=None):
        seen.append((dtype, next(model_.parameters()).device.type))
        return real(model_, waveforms, segs_, dtype, kernels)

    monkeypatch.setattr(emission, "_packed_logits_half", spy)
    got = align(copy.deepcopy(segs), model, dict(meta, dtype=torch.bfloat16), wavs[0][0], "cpu")
    assert seen == [(torch.bfloat16, "cpu")]
    assert _words(got) == _words(ref)


def test_geometry_fallback_of_a_half_call_warns_once_and_runs_fp32(monkeypatch):
    from whisperx_amd import align, emission

    m, wavs = _gpu_case("post")
    segs, meta = hh.transcript()
    ref = align(copy.deepcopy(segs), m, meta, wavs[0][0], "cuda:0")

    def refuse(*a, **k):
        raise ValueError("frame geometry")

    monkeypatch.setattr(emission, "packed_logits", refuse)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = align(copy.deepcopy(segs), m, dict(meta, dtype=torch.float16), wavs[0][0], "cuda:0")
    mine = [w for w in caught if issubclass(w.category, RuntimeWarning) and "float32" in str(w.message)]
    assert len(mine) == 1, [str(w.message) for w in caught]
    assert _words(got) == _words(ref)
    assert not any("forward" in mod.__dict__ or hasattr(mod, "_wx_orig_forward") for mod in m.modules())


def test_fp32_route_is_untouched():
    """packed_logits without dtype and with dtype=torch.float32: the same code path, bit-identical logits."""
    from whisperx_amd import _lib, emission

    m, wavs = _gpu_case("post512")
    Ts = hh.frames("post512")
    streams = [torch.cuda.current_stream()]
    a = emission.packed_logits(m, wavs, _lib.PackedSegments(Ts), streams)
    b = emission.packed_logits(m, wavs, _lib.PackedSegments(Ts), streams, dtype=torch.float32)
    assert a.dtype == b.dtype == torch.float32 and torch.equal(a, b)
    assert m not in emission._HALF_CACHE  # (and nothing of the half route was built for it)

"""whisperx_amd.audio's restatement of the reference's audio module (audio.py:13-22, :68-159) on
the CPU: constants, pad_or_trim, the computed mel filterbank, the host route of
log_mel_spectrogram / log_mel_chunks against the golden cases, and install()'s binding."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from mel_helpers import MelCases, check_against_f64


@pytest.fixture(scope="module")
def cases():
    return MelCases()


def test_mel_filters_equal_the_reference_asset_bit_for_bit():
    from whisperx_amd import audio

    with np.load(os.path.join(GOLDEN, "mel_filters.npz")) as f:
        for n in (80, 128):
            got = audio.mel_filters("cpu", n)
            assert got.dtype == torch.float32 and tuple(got.shape) == (n, 201)
            assert np.array_equal(got.numpy().view(np.uint32), f[f"mel_{n}"].view(np.uint32)), n
    assert audio.mel_filters("cpu", 80) is audio.mel_filters("cpu", 80)  # cached


def test_mel_filters_refuses_other_sizes():
    from whisperx_amd import audio

    with pytest.raises(AssertionError, match="Unsupported n_mels: 64"):
        audio.mel_filters("cpu", 64)
    with pytest.raises(AssertionError, match="Unsupported n_mels: 40"):
        audio.log_mel_spectrogram(np.zeros(1000, np.float32), 40)


def test_host_route_within_tol_of_fp64_on_every_case(cases):
    from whisperx_amd import audio

    worst = 0.0
    for i in range(len(cases)):
        c = cases[i]
        got = audio.log_mel_spectrogram(c["x"], c["n_mels"], padding=c["padding"])
        assert got.dtype == torch.float32 and got.device.type == "cpu"
        worst = max(worst, check_against_f64(got.numpy(), c, cases.tol))
    print(f"host route: max |got - fp64| = {worst:.3e} (ref_err {cases.ref_err:.3e}, TOL {cases.tol:.3e})")


def test_constants_and_pad_or_trim_match_the_reference(cases):
    from whisperx_amd import audio

    d = cases.d
    for name, value in zip(d["const_names"], d["const_values"]):
        assert getattr(audio, str(name)) == int(value), name
    a = d["pot_in"]
    for got, key in ((audio.pad_or_trim(a, 3), "pot_trim3"), (audio.pad_or_trim(a, 8), "pot_pad8"),
                     (audio.pad_or_trim(a, 4, axis=0), "pot_pad4_axis0")):
        assert isinstance(got, np.ndarray) and got.dtype == d[key].dtype and np.array_equal(got, d[key]), key
    t = torch.from_numpy(a)
    for got, key in ((audio.pad_or_trim(t, 8), "pot_tensor_pad8"), (audio.pad_or_trim(t, 1, axis=0), "pot_tensor_trim1_axis0")):
        assert torch.is_tensor(got) and np.array_equal(got.numpy(), d[key]), key
    assert audio.pad_or_trim(np.zeros(7, np.float32)).shape[0] == int(d["pot_default_len"]) == audio.N_SAMPLES
    assert audio.pad_or_trim(a, 5) is a


def _buffer(seconds=12, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(seconds * 16000) * np.repeat(rng.uniform(0.01, 0.5, seconds), 16000)).astype(np.float32)


def test_log_mel_chunks_host_route_equals_per_chunk_calls():
    from whisperx_amd import audio

    wav = _buffer()
    segs = [{"start": 0.0, "end": 1.3}, {"start": 1.2345, "end": 6.789}, {"start": 7.0, "end": 7.0},
            {"start": 8.25, "end": 30.0}]  # (the last one runs past the end: sliced as audio[f1:f2] is)
    got = audio.log_mel_chunks(wav, segs, n_mels=80, device="cpu")
    assert tuple(got.shape) == (4, 80, audio.N_FRAMES) and got.dtype == torch.float32 and got.device.type == "cpu"
    bounds = []
    for b, s in enumerate(segs):
        f1, f2 = int(s["start"] * 16000), int(s["end"] * 16000)
        chunk = wav[f1:f2]
        bounds.append((f1, min(f2, len(wav))))
        want = audio.log_mel_spectrogram(chunk, 80, padding=audio.N_SAMPLES - chunk.shape[0])
        assert torch.equal(got[b], want), b
    assert torch.all(got[2] == -1.5)  # an empty chunk
    assert len({float(got[b].max()) for b in range(4)}) == 4  # every chunk has its own maximum
    again = audio.log_mel_chunks(torch.from_numpy(wav), np.asarray(bounds, dtype=np.int64), n_mels=80, device="cpu")
    assert torch.equal(again, got)
    empty = audio.log_mel_chunks(wav, [], n_mels=128, device="cpu")
    assert tuple(empty.shape) == (0, 128, audio.N_FRAMES)


def test_log_mel_chunks_messages():
    from whisperx_amd import audio

    wav = np.zeros(40 * 16000, np.float32)
    with pytest.raises(ValueError, match=r"chunk 1 has 480001 samples \(30\.00 s\): more than N_SAMPLES = 480000"):
        audio.log_mel_chunks(wav, np.array([[0, 16000], [5, 480006]]), device="cpu")
    with pytest.raises(ValueError, match="chunk 0 has 496000 samples"):
        audio.log_mel_chunks(wav, [{"start": 1.0, "end": 32.0}], device="cpu")
    with pytest.raises(ValueError, match="integer array of sample bounds"):
        audio.log_mel_chunks(wav, np.array([[0.0, 1.0]]), device="cpu")
    with pytest.raises(AssertionError, match="Unsupported n_mels: 100"):
        audio.log_mel_chunks(wav, [], n_mels=100, device="cpu")


def test_package_exports():
    import whisperx_amd
    from whisperx_amd import audio

    for name in ("N_FFT", "HOP_LENGTH", "CHUNK_LENGTH", "N_SAMPLES", "N_FRAMES", "N_SAMPLES_PER_TOKEN",
                 "FRAMES_PER_SECOND", "TOKENS_PER_SECOND", "pad_or_trim", "mel_filters", "log_mel_spectrogram",
                 "log_mel_chunks"):
        assert getattr(whisperx_amd, name) is getattr(audio, name), name


@pytest.mark.parametrize("how", ["worker", "env"])
def test_bound_function_takes_the_host_route(monkeypatch, how):
    """Inside a DataLoader worker (get_worker_info() is not None) and with WX_MEL_HOST=1 the
    function install() binds must not touch the GPU, even where one is visible."""
    from whisperx_amd import _lib, audio

    def no_gpu(*a, **k):
        raise AssertionError("the host route must not reach wx_log_mel")

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(_lib, "log_mel", no_gpu)
    x = _buffer(2, seed=9)
    if how == "worker":
        monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    else:
        monkeypatch.setenv("WX_MEL_HOST", "1")
    got = audio.drop_in_log_mel_spectrogram(x, n_mels=80, padding=audio.N_SAMPLES - x.shape[0])
    assert got.device.type == "cpu" and tuple(got.shape) == (80, audio.N_FRAMES)
    assert torch.equal(got, audio._log_mel_host(torch.from_numpy(x), 80, audio.N_SAMPLES - x.shape[0]))


def test_argument_validation_returns_before_any_launch():
    """wx_log_mel's checks (host arrays of chunk bounds) return wx_strerror codes without a device."""
    import ctypes

    from whisperx_amd import _lib

    _lib.build()
    lib = _lib.load(require_device=False)
    dummy = ctypes.c_void_p(256)
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731

    def call(B=1, n_mels=80, first=0, length=1000, pad=0, n_wave=1000, frames=3000, ws=1 << 12):
        return lib.wx_log_mel(dummy, n_wave, i64(first), i64(length), i64(pad), dummy, B, n_mels, dummy, dummy, dummy,
                              frames, frames, dummy, ws, None)

    assert call(B=-1) == 1001
    assert call(B=0) == 0
    assert call(n_mels=64) == 1001
    assert call(length=200) == 1001 and call(length=100, pad=100) == 1001  # L <= 200
    assert call(first=1) == 1001  # runs past the waveform
    assert call(length=1000, pad=480000, frames=3000) == 1001  # more frames than the output holds
    assert call(ws=lib.wx_log_mel_workspace_bytes(1) - 1) == 1004
    assert lib.wx_log_mel_workspace_bytes(1000) >= 4000


# A package laid out as the reference is around log_mel_spectrogram (asr.py:12 binds the name at
# import time; preprocess, :141-149, and detect_language, :245-252, call it), bodies reduced to
# the calls: this repository's own restatement, as in test_install.py.
STANDIN = {
    "__init__.py": "",
    "audio.py": """
        SAMPLE_RATE = 16000
        N_SAMPLES = 480000

        def load_audio(file, sr=SAMPLE_RATE): raise NotImplementedError("stand-in for the reference")
        def log_mel_spectrogram(audio, n_mels, padding=0, device=None): raise NotImplementedError("stand-in for the reference")
    """,
    "asr.py": """
        from .audio import N_SAMPLES, SAMPLE_RATE, load_audio, log_mel_spectrogram

        class FasterWhisperPipeline:
            def preprocess(self, audio):
                return log_mel_spectrogram(audio, n_mels=80, padding=N_SAMPLES - audio.shape[0])

            def detect_language(self, audio):
                return log_mel_spectrogram(audio[:N_SAMPLES], n_mels=80,
                                           padding=0 if audio.shape[0] >= N_SAMPLES else N_SAMPLES - audio.shape[0])
    """,
}

SCRIPT = textwrap.dedent(r'''
    import sys
    import numpy as np, torch
    sys.path.insert(0, sys.argv[1])   # the directory that holds the whisperx package
    sys.path.insert(0, sys.argv[2])   # this repo
    import whisperx, whisperx.audio, whisperx.asr
    assert whisperx.asr.log_mel_spectrogram is whisperx.audio.log_mel_spectrogram   # before: the reference's
    import whisperx_amd
    from whisperx_amd import audio as amd_audio
    rebound = whisperx_amd.install(whisperx)
    assert ("whisperx.asr", "log_mel_spectrogram") in rebound and ("whisperx.audio", "log_mel_spectrogram") in rebound
    assert whisperx_amd.integration.installed(whisperx)
    assert whisperx.asr.log_mel_spectrogram is amd_audio.drop_in_log_mel_spectrogram
    assert whisperx.audio.log_mel_spectrogram is amd_audio.drop_in_log_mel_spectrogram
    pipe = whisperx.asr.FasterWhisperPipeline
    assert pipe.preprocess.__globals__["log_mel_spectrogram"] is amd_audio.drop_in_log_mel_spectrogram
    assert pipe.detect_language.__globals__["log_mel_spectrogram"] is amd_audio.drop_in_log_mel_spectrogram
    if not torch.cuda.is_available():   # the call sites, end to end on the host route
        x = (np.random.default_rng(0).standard_normal(20000) * 0.1).astype(np.float32)
        got = pipe().preprocess(x)
        assert got.device.type == "cpu" and tuple(got.shape) == (80, 3000)
        assert torch.equal(got, amd_audio.log_mel_spectrogram(x, 80, padding=480000 - 20000))
        assert torch.equal(pipe().detect_language(x), got)
    print("rebound", len(rebound))
''')


def test_install_rebinds_log_mel_spectrogram(tmp_path):
    pkg = os.path.join(str(tmp_path), "whisperx")
    os.makedirs(pkg)
    for name, text in STANDIN.items():
        with open(os.path.join(pkg, name), "w") as f:
            f.write(textwrap.dedent(text))
    r = subprocess.run([sys.executable, "-c", SCRIPT, str(tmp_path), ROOT], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "rebound" in r.stdout

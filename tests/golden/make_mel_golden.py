"""Golden cases of the reference's log_mel_spectrogram (whisperx/audio.py:112-159).

TEST INFRASTRUCTURE ONLY — run by hand where a reference checkout is present, never on the GPU
machine, never imported by the package or by the tests.  WHISPERX_ROOT names the directory that
holds the reference's `whisperx` package.  Its audio.py is loaded on its own (behind a bare
package object, so that `from .utils import exact_div` resolves without running the reference's
__init__.py), fed seeded signals, and only data is written:

  mel_filters.npz   a copy of the reference's data asset (assets/mel_filters.npz)
  mel_cases.npz     per case cNN: the input (16-bit PCM: x = cNN_x / 32768 in fp32, exactly what
                    load_audio yields; cNN_x_of = MM instead where case MM has the same input),
                    n_mels, padding, the frames stored, the reference's fp32 output at those
                    frames (cNN_ref) and an fp64 evaluation of the same formula by
                    log_mel_f64 below (the reference's function does not take fp64), stored as
                    cNN_d64 = (f64 - ref) * 2**24 in fp16: f64 = ref + d64 / 2**24 to within
                    2**-11 |f64 - ref| < 2e-8, three orders below the tolerance.
                    ref_err = max |ref - f64| over every value of every case; tol = 4 * ref_err.

Which frames are stored (the file has to stay under 1 MB): every frame of the short cases; of a
case padded to 30 s the frames up to two past the last frame that touches audio, the rest being
pinned by cNN_floor, the one value every later frame has (the generator asserts it has); of the
three longest (3.1 s, 7 s, N_SAMPLES) the first and last 66 frames of that range and every 8th,
8th and 64th in between.  ref_err covers all frames, stored or not.

    WHISPERX_ROOT=/path/to/checkout python tests/golden/make_mel_golden.py
"""
import importlib.util
import os
import shutil
import sys
import types
from importlib.machinery import ModuleSpec

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N_SAMPLES, HOP, N_FFT = 480000, 160, 400


def load_reference_audio():
    root = os.environ.get("WHISPERX_ROOT")
    if not root:
        raise SystemExit("set WHISPERX_ROOT to the directory that holds the reference's whisperx package")
    pkg_dir = os.path.join(root, "whisperx")
    pkg = types.ModuleType("ref_whisperx")
    pkg.__path__ = [pkg_dir]
    pkg.__spec__ = ModuleSpec("ref_whisperx", None, is_package=True)
    sys.modules["ref_whisperx"] = pkg
    spec = importlib.util.spec_from_file_location("ref_whisperx.audio", os.path.join(pkg_dir, "audio.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_whisperx.audio"] = mod
    spec.loader.exec_module(mod)
    return mod, os.path.join(pkg_dir, "assets", "mel_filters.npz")


def log_mel_f64(x, n_mels, padding, filters):
    """audio.py:147-159 in fp64: the fp32 samples and the fp32 filterbank are the inputs, every
    operation on them (window, DFT, power, projection, log10, floor, affine) is fp64."""
    x = np.concatenate([np.asarray(x, dtype=np.float64), np.zeros(padding)])
    L = len(x)
    xp = np.pad(x, N_FFT // 2, mode="reflect")  # torch.stft(center=True, pad_mode="reflect")
    n = np.arange(N_FFT)
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)  # periodic Hann
    frames = xp[HOP * np.arange(L // HOP)[:, None] + n[None, :]]  # the last STFT frame is dropped
    power = np.abs(np.fft.rfft(frames * window, axis=1)) ** 2
    mel = filters.astype(np.float64) @ power.T
    log_spec = np.log10(np.maximum(mel, 1e-10))
    log_spec = np.maximum(log_spec, log_spec.max() - 8.0)
    return (log_spec + 4.0) / 4.0


def pcm(v):
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def noise(seed, n, scale=500.0):
    return pcm(np.random.default_rng(seed).standard_normal(n) * scale)


def am_noise(seed, n):
    """Amplitude-modulated noise from a small alphabet (keeps the file small): +-3 times a gain of
    2**k that changes every quarter second."""
    rng = np.random.default_rng(seed)
    base = rng.integers(-3, 4, n)
    gain = 2 ** rng.integers(0, 9, n // 4000 + 1)
    return pcm(base * np.repeat(gain, 4000)[:n])


def periodic_noise(seed, n):
    """A 4001-sample pattern repeated, its gain doubling every second over a 7 s cycle."""
    rng = np.random.default_rng(seed)
    base = np.tile(rng.integers(-7, 8, 4001), n // 4001 + 1)[:n]
    gain = 2 ** ((np.arange(n) // 16000) % 7)
    return pcm(base * gain)


def cases():
    out = []
    small = [201, 4959, 4960, 5120, 5280, 10079, 10240, 10401]
    for L in small:  # the right-hand reflection mirrors audio
        out.append((f"noise_{L}_pad0", noise(100 + L, L), 80, 0))
    for L in small:  # ... mirrors zeros
        out.append((f"noise_{L}_pad333", noise(100 + L, L), 80, 333))
    for sec, seed in ((0.7, 7), (3.1, 31), (7.0, 70)):
        n = int(round(sec * 16000))
        out.append((f"am_{sec}s_to30s", am_noise(seed, n), 80, N_SAMPLES - n))
    out.append(("periodic_30s_pad0", periodic_noise(30, N_SAMPLES), 80, 0))  # frame 2999 reaches the reflection
    out.append(("zeros", np.zeros(1000, np.int16), 80, 2000))
    edges = np.zeros(4000, np.int16)
    edges[:100] = noise(1, 100)
    edges[-100:] = noise(2, 100)
    out.append(("edges_only", edges, 80, 0))
    t = np.arange(4000) / 16000.0
    tone = np.concatenate([pcm(0.8 * 32768 * np.sin(2 * np.pi * 440.0 * t)), np.zeros(5600, np.int16),
                           noise(3, 6400, 1e-4 * 32768)])
    out.append(("tone_silence_faint_noise", tone, 80, 0))
    # four of them at 128 mels
    out.append(("noise_201_pad0_128", noise(100 + 201, 201), 128, 0))
    out.append(("noise_4959_pad333_128", noise(100 + 4959, 4959), 128, 333))
    out.append(("noise_10401_pad0_128", noise(100 + 10401, 10401), 128, 0))
    out.append(("zeros_128", np.zeros(1000, np.int16), 128, 2000))
    return out


def stored_frames(name, n_audio, F):
    """(indices stored, first frame pinned by the floor value or F)."""
    last_audio = -(-(n_audio + N_FFT // 2) // HOP) - 1  # the last frame with a sample of audio in it
    end = min(F, last_audio + 3)
    idx = np.arange(end)
    step = {"am_3.1s_to30s": 8, "am_7.0s_to30s": 8, "periodic_30s_pad0": 64}.get(name)
    if step:
        keep = (idx < 66) | (idx >= end - 66) | (idx % step == 0)
        idx = idx[keep]
    return idx.astype(np.int32), end


def main():
    ref, asset = load_reference_audio()
    shutil.copyfile(asset, os.path.join(HERE, "mel_filters.npz"))
    filt = {n: np.load(asset)[f"mel_{n}"] for n in (80, 128)}
    data, names, ref_err, inputs = {}, [], 0.0, {}
    for i, (name, x16, n_mels, padding) in enumerate(cases()):
        x = x16.astype(np.float32) / 32768.0
        got = ref.log_mel_spectrogram(x, n_mels, padding=padding).numpy()
        f64 = log_mel_f64(x, n_mels, padding, filt[n_mels])
        F = (len(x) + padding) // HOP
        assert got.dtype == np.float32 and got.shape == f64.shape == (n_mels, F), (name, got.shape, f64.shape)
        err = float(np.abs(got.astype(np.float64) - f64).max())
        ref_err = max(ref_err, err)
        idx, end = stored_frames(name, len(x), F)
        p = f"c{i:02d}_"
        same = inputs.setdefault(x16.tobytes(), i)
        if same == i:
            data[p + "x"] = x16
        else:
            data[p + "x_of"] = np.int32(same)
        data[p + "n_mels"] = np.int32(n_mels)
        data[p + "padding"] = np.int64(padding)
        data[p + "frames"] = idx
        data[p + "ref"] = np.ascontiguousarray(got[:, idx])
        d64 = ((f64[:, idx] - got[:, idx].astype(np.float64)) * 2.0 ** 24).astype(np.float16)
        assert np.isfinite(d64).all()
        data[p + "d64"] = d64
        data[p + "floor_from"] = np.int32(end)
        if end < F:  # every later frame has one value, the floor (or -1.5 where nothing is above it)
            assert np.all(got[:, end:] == got[0, end]) and np.all(f64[:, end:] == f64[0, end]), name
            data[p + "floor_ref"] = np.float32(got[0, end])
            data[p + "floor_f64"] = np.float64(f64[0, end])
        names.append(name)
        print(f"{name:28s} n_mels {n_mels:3d} frames {F:4d} stored {len(idx):4d} |ref - f64| {err:.3e}")
    if "zeros" in names:
        z = names.index("zeros")
        assert np.all(data[f"c{z:02d}_ref"] == -1.5)
    tol = 4.0 * ref_err
    # past the spacing of fp16 in [0.5, 1) the reference's default compute_type="float16" consumer
    # cannot tell results apart: the bound may not reach it
    assert tol < 2.0 ** -11, f"TOL = 4 * {ref_err} reaches the fp16 spacing 2**-11"
    data["names"] = np.array(names)
    data["n_cases"] = np.int32(len(names))
    data["ref_err"] = np.float64(ref_err)
    data["tol"] = np.float64(tol)
    # the constants and pad_or_trim, as the reference has them
    const = ["SAMPLE_RATE", "N_FFT", "HOP_LENGTH", "CHUNK_LENGTH", "N_SAMPLES", "N_FRAMES", "N_SAMPLES_PER_TOKEN",
             "FRAMES_PER_SECOND", "TOKENS_PER_SECOND"]
    data["const_names"] = np.array(const)
    data["const_values"] = np.array([int(getattr(ref, c)) for c in const], dtype=np.int64)
    a = np.arange(10, dtype=np.float32).reshape(2, 5)
    data["pot_in"] = a
    data["pot_trim3"] = ref.pad_or_trim(a, 3)
    data["pot_pad8"] = ref.pad_or_trim(a, 8)
    data["pot_pad4_axis0"] = ref.pad_or_trim(a, 4, axis=0)
    data["pot_tensor_pad8"] = ref.pad_or_trim(torch.from_numpy(a), 8).numpy()
    data["pot_tensor_trim1_axis0"] = ref.pad_or_trim(torch.from_numpy(a), 1, axis=0).numpy()
    data["pot_default_len"] = np.int64(ref.pad_or_trim(np.zeros(7, np.float32)).shape[0])
    path = os.path.join(HERE, "mel_cases.npz")
    np.savez_compressed(path, **data)
    size = os.path.getsize(path)
    print(len(names), "cases,", size, "bytes; ref_err", ref_err, "tol", tol)
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()

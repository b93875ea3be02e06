"""The reference's audio module (whisperx/audio.py): constants, the loader align() uses
(:25-65, ffmpeg decode to 16 kHz mono float32 in a subprocess — the same process boundary as
the reference), pad_or_trim (:68-91), mel_filters (:94-109) and Whisper's input features,
log_mel_spectrogram (:112-159).

The features of a 1-D float32 waveform on a HIP device come from wx_log_mel (one fused kernel:
frame gather, windowed DFT and mel projection on the f32 MFMA, log10; include/wx_align.h), and
log_mel_chunks computes every VAD chunk of a file in one launch.  Everything else — batched
input, a CPU tensor, no GPU — takes the host route, this module's torch restatement of the
reference's formula."""
from __future__ import annotations

import os
import subprocess
import threading
from typing import Optional, Union

import numpy as np
import torch
import torch.nn.functional as F

# audio.py:13-22
SAMPLE_RATE = 16000
N_FFT = 400
HOP_LENGTH = 160
CHUNK_LENGTH = 30
N_SAMPLES = CHUNK_LENGTH * SAMPLE_RATE  # 480000 samples in a 30-second chunk
N_FRAMES = N_SAMPLES // HOP_LENGTH  # 3000 frames in a mel spectrogram input
N_SAMPLES_PER_TOKEN = HOP_LENGTH * 2  # the initial convolutions have stride 2
FRAMES_PER_SECOND = SAMPLE_RATE // HOP_LENGTH  # 10 ms per audio frame
TOKENS_PER_SECOND = SAMPLE_RATE // N_SAMPLES_PER_TOKEN  # 20 ms per audio token


def load_audio(file: str, sr: int = SAMPLE_RATE) -> np.ndarray:
    try:
        cmd = ["ffmpeg", "-nostdin", "-threads", "0", "-i", file, "-f", "s16le", "-ac", "1",
               "-acodec", "pcm_s16le", "-ar", str(sr), "-"]
        out = subprocess.run(cmd, capture_output=True, check=True).stdout
    except FileNotFoundError as e:
        raise RuntimeError("ffmpeg is required to decode audio files; pass a waveform array instead") from e
    except subprocess.CalledProcessError as e:
        raise RuntimeError(f"Failed to load audio: {e.stderr.decode()}") from e
    return np.frombuffer(out, np.int16).flatten().astype(np.float32) / 32768.0


def pad_or_trim(array, length: int = N_SAMPLES, *, axis: int = -1):
    """Pad with zeros or trim `array` (numpy or tensor) to `length` along `axis` (audio.py:68-91)."""
    if torch.is_tensor(array):
        if array.shape[axis] > length:
            array = array.index_select(dim=axis, index=torch.arange(length, device=array.device))
        if array.shape[axis] < length:
            pad_widths = [(0, 0)] * array.ndim
            pad_widths[axis] = (0, length - array.shape[axis])
            array = F.pad(array, [pad for sizes in pad_widths[::-1] for pad in sizes])
    else:
        if array.shape[axis] > length:
            array = array.take(indices=range(length), axis=axis)
        if array.shape[axis] < length:
            pad_widths = [(0, 0)] * array.ndim
            pad_widths[axis] = (0, length - array.shape[axis])
            array = np.pad(array, pad_widths)
    return array


# ------------------------------------------------------------------------------ mel filterbank
def _hz_to_mel(f):
    """Slaney's scale: linear below 1 kHz (200 / 3 Hz per mel), logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def _mel_filters_host(n_mels: int) -> np.ndarray:
    """The [n_mels, 201] Slaney-normalised triangular mel filterbank of a 400-point FFT at 16 kHz
    (what the reference ships as assets/mel_filters.npz: librosa.filters.mel(sr=16000, n_fft=400,
    n_mels=n_mels)): computed in fp64, stored into an fp32 array, the area normalisation applied to
    the stored values."""
    fftfreqs = np.fft.rfftfreq(n=N_FFT, d=1.0 / SAMPLE_RATE)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(SAMPLE_RATE / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    weights = np.zeros((n_mels, 1 + N_FFT // 2), dtype=np.float32)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    weights *= enorm[:, np.newaxis]
    return weights


_filters: dict = {}
_filters_mu = threading.Lock()


def mel_filters(device, n_mels: int) -> torch.Tensor:
    """The mel filterbank matrix [n_mels, 201] on `device` (audio.py:94-109), computed from the
    Slaney formula (bit-equal to the reference's asset) and cached per (device, n_mels)."""
    assert n_mels in [80, 128], f"Unsupported n_mels: {n_mels}"
    key = (str(torch.device(device)), int(n_mels))
    with _filters_mu:
        t = _filters.get(key)
        if t is None:
            host = _filters.get(("host", int(n_mels)))
            if host is None:
                host = _filters[("host", int(n_mels))] = _mel_filters_host(int(n_mels))
            t = _filters[key] = torch.from_numpy(host.copy()).to(device)
        return t


# ------------------------------------------------------------------------------ features
def _log_mel_host(audio: torch.Tensor, n_mels: int, padding: int = 0) -> torch.Tensor:
    """The host route: audio.py:147-159 in torch ops on the tensor's device."""
    if padding > 0:
        audio = F.pad(audio, (0, padding))
    window = torch.hann_window(N_FFT).to(audio.device)
    stft = torch.stft(audio, N_FFT, HOP_LENGTH, window=window, return_complex=True)
    magnitudes = stft[..., :-1].abs() ** 2
    mel_spec = mel_filters(audio.device, n_mels) @ magnitudes
    log_spec = torch.clamp(mel_spec, min=1e-10).log10()
    log_spec = torch.maximum(log_spec, log_spec.max() - 8.0)
    return (log_spec + 4.0) / 4.0


def _kernel_takes(audio: torch.Tensor, padding: int) -> bool:
    return audio.dim() == 1 and audio.is_cuda and audio.dtype == torch.float32 \
        and audio.shape[0] + padding > N_FFT // 2  # (shorter: torch's reflect padding refuses it, on the host route)


def _as_tensor(audio) -> torch.Tensor:
    if not torch.is_tensor(audio):
        if isinstance(audio, str):
            audio = load_audio(audio)
        audio = torch.from_numpy(audio)
    return audio


def log_mel_spectrogram(audio: Union[str, np.ndarray, torch.Tensor], n_mels: int, padding: int = 0,
                        device: Optional[Union[str, torch.device]] = None) -> torch.Tensor:
    """The log-Mel spectrogram of a 16 kHz waveform (audio.py:112-159): a path, a numpy array or
    a tensor; `padding` zero samples are appended; the tensor is moved to `device` when given.
    Returns [n_mels, n_frames] (n_mels 80 or 128) on the tensor's device.

    A 1-D float32 signal that ends up on a HIP device is computed by wx_log_mel (B = 1); anything
    else (batched input, a CPU tensor, no GPU) takes the host route, the same formula in torch
    ops.  The two agree to fp32 tolerance, not bit for bit.  Non-finite samples are out of scope
    (the kernel's maximum ignores NaN where torch's propagates it)."""
    audio = _as_tensor(audio)
    if device is not None:
        audio = audio.to(device)
    padding = int(padding)
    if _kernel_takes(audio, padding):
        from . import _lib

        n = int(audio.shape[0])
        return _lib.log_mel(audio.contiguous(), [0], [n], [padding], mel_filters(audio.device, n_mels))[0]
    return _log_mel_host(audio, n_mels, padding)


def drop_in_log_mel_spectrogram(audio, n_mels: int, padding: int = 0, device=None) -> torch.Tensor:
    """What install() binds as whisperx.audio / whisperx.asr log_mel_spectrogram (asr.py:12,
    called per VAD chunk at :141-149 and by detect_language at :245-252): computed on the GPU when
    one is visible, returned on the device the reference would have returned it on (preprocess
    feeds numpy and stacks CPU tensors).  The host route is taken inside a DataLoader worker
    process (a forked worker must not open the GPU) and when WX_MEL_HOST=1 is set."""
    if torch.utils.data.get_worker_info() is not None or os.environ.get("WX_MEL_HOST") == "1" \
            or not torch.cuda.is_available():
        audio = _as_tensor(audio)
        if device is not None:
            audio = audio.to(device)
        return _log_mel_host(audio, n_mels, int(padding))
    audio = _as_tensor(audio)
    home = torch.device(device) if device is not None else audio.device
    out = log_mel_spectrogram(audio, n_mels, padding, home if home.type == "cuda" else "cuda")
    return out.to(home)


def _chunk_bounds(segments, n: int):
    """(first, length) int64 arrays of the chunks: dicts with 'start' / 'end' in seconds sliced as
    asr.py:179-184 does (audio[int(start * 16000) : int(end * 16000)]), or an (n, 2) integer
    array of sample bounds, sliced the same way."""
    if len(segments) and isinstance(segments[0], dict):
        b = [(int(s["start"] * SAMPLE_RATE), int(s["end"] * SAMPLE_RATE)) for s in segments]
    else:
        b = np.asarray(segments)
        if b.size and (b.ndim != 2 or b.shape[1] != 2 or not np.issubdtype(b.dtype, np.integer)):
            raise ValueError("segments must be merge_chunks' dicts or an (n, 2) integer array of sample bounds")
    b = np.asarray(b, dtype=np.int64).reshape(-1, 2)
    if (b < 0).any():
        raise ValueError("segments: negative chunk bounds")
    first = np.minimum(b[:, 0], n)
    last = np.minimum(np.maximum(b[:, 1], first), n)
    return first, last - first


def log_mel_chunks(audio, segments, n_mels: int = 80, device=None) -> torch.Tensor:
    """Whisper's input features of every chunk of one file: `audio` is the whole file (numpy, CPU
    tensor or device tensor), `segments` merge_chunks' output (dicts with 'start' / 'end' in
    seconds) or an (n, 2) integer array of sample bounds.  Returns [B, n_mels, 3000]: chunk b is
    log_mel_spectrogram(audio[f1:f2], n_mels, padding=N_SAMPLES - (f2 - f1)), what
    FasterWhisperPipeline.preprocess computes per chunk (asr.py:141-149).  On a HIP device
    (`device`, else the audio's, else the current one) the waveform is uploaded at most once and
    all chunks come from one wx_log_mel launch; without a GPU the chunks take the host route one
    by one.  An empty chunk is all -1.5; a chunk longer than N_SAMPLES raises ValueError."""
    assert n_mels in [80, 128], f"Unsupported n_mels: {n_mels}"
    if not torch.is_tensor(audio):
        audio = torch.from_numpy(np.ascontiguousarray(audio))
    if audio.dim() != 1:
        raise ValueError("log_mel_chunks: audio must be one 1-D waveform")
    first, length = _chunk_bounds(segments, int(audio.shape[0]))
    for i, n in enumerate(length):
        if n > N_SAMPLES:
            raise ValueError(f"chunk {i} has {int(n)} samples ({int(n) / SAMPLE_RATE:.2f} s): more than "
                             f"N_SAMPLES = {N_SAMPLES} ({CHUNK_LENGTH} s)")
    if device is not None:
        dev = torch.device(device)
    elif audio.is_cuda or torch.cuda.is_available():
        dev = audio.device if audio.is_cuda else torch.device("cuda", torch.cuda.current_device())
    else:
        dev = torch.device("cpu")
    audio = audio.to(device=dev, dtype=torch.float32)
    if dev.type == "cuda":
        from . import _lib

        return _lib.log_mel(audio.contiguous(), first, length, N_SAMPLES - length, mel_filters(dev, n_mels),
                            n_frames_max=N_FRAMES)
    out = torch.empty((len(length), n_mels, N_FRAMES), dtype=torch.float32)
    for i, (a, n) in enumerate(zip(first, length)):
        out[i] = _log_mel_host(audio[int(a):int(a + n)], n_mels, N_SAMPLES - int(n))
    return out

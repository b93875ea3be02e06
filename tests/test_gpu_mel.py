"""wx_log_mel on the GPU: the golden cases against the fp64 column, the all-zero-frame skip, the
batched entry against single calls and the host route, output bounds, and streams.

Figures of the run that DESIGN.md cites (27 cases): kernel max |got - fp64| is printed by
test_every_golden_case_within_tol_of_fp64 next to ref_err and TOL = 4 x ref_err."""
import numpy as np
import pytest
import torch

from mel_helpers import MelCases, check_against_f64

pytestmark = pytest.mark.gpu

OFFSETS = [0, 1, 16001, 123457, 300003]
LENGTHS = [0, 201, 77777, 480000, 31999]
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def cases():
    return MelCases()


def _kernel(x, n_mels, padding, first=0, length=None):
    """One chunk of the device waveform x through wx_log_mel: [n_mels, (length + padding) // 160]."""
    from whisperx_amd import _lib, audio

    length = int(x.shape[0]) - first if length is None else length
    return _lib.log_mel(x, [first], [length], [padding], audio.mel_filters(x.device, n_mels))[0]


def test_every_golden_case_within_tol_of_fp64(cases):
    worst = 0.0
    for i in range(len(cases)):
        c = cases[i]
        got = _kernel(torch.from_numpy(c["x"]).cuda(), c["n_mels"], c["padding"])
        err = check_against_f64(got.cpu().numpy(), c, cases.tol)
        print(f"{c['name']:28s} |kernel - fp64| {err:.3e}")
        worst = max(worst, err)
    print(f"wx_log_mel: max |got - fp64| = {worst:.3e} (ref_err {cases.ref_err:.3e}, TOL {cases.tol:.3e})")


def test_public_entry_uses_the_kernel_and_matches_it(cases):
    from whisperx_amd import audio

    c = cases[cases.names.index("noise_10401_pad333")]
    x = torch.from_numpy(c["x"]).cuda()
    want = _kernel(x, 80, 333)
    assert torch.equal(audio.log_mel_spectrogram(c["x"], 80, padding=333, device="cuda"), want)
    assert torch.equal(audio.log_mel_spectrogram(x, 80, padding=333), want)
    got = audio.drop_in_log_mel_spectrogram(c["x"], n_mels=80, padding=333)  # numpy in: a CPU tensor out
    assert got.device.type == "cpu" and torch.equal(got, want.cpu())
    # batched input takes the host route (torch ops on the device), within tolerance of the kernel
    both = audio.log_mel_spectrogram(torch.stack([x, x]), 80, padding=333)
    assert tuple(both.shape) == (2, 80, want.shape[1]) and float((both[1] - want).abs().max()) <= 2 * cases.tol


def test_zero_frame_skip_is_bit_equal(cases, monkeypatch):
    padded = [i for i in range(len(cases)) if cases.names[i].endswith("_to30s") or cases.names[i].startswith("zeros")]
    assert len(padded) == 5
    for i in padded:
        c = cases[i]
        x = torch.from_numpy(c["x"]).cuda()
        monkeypatch.delenv("WX_NO_MEL_SKIP", raising=False)
        skipped = _kernel(x, c["n_mels"], c["padding"])
        monkeypatch.setenv("WX_NO_MEL_SKIP", "1")
        full = _kernel(x, c["n_mels"], c["padding"])
        monkeypatch.delenv("WX_NO_MEL_SKIP")
        assert torch.equal(skipped.view(torch.int32), full.view(torch.int32)), c["name"]
        check_against_f64(full.cpu().numpy(), c, cases.tol)


@pytest.fixture(scope="module")
def forty_seconds():
    rng = np.random.default_rng(40)
    gain = np.repeat(rng.uniform(0.002, 0.6, 40), 16000)  # another level every second: distinct chunk maxima
    return (rng.standard_normal(40 * 16000) * gain).astype(np.float32)


def test_batched_chunks_match_single_calls_and_the_host_route(cases, forty_seconds):
    from whisperx_amd import _lib, audio

    wav = torch.from_numpy(forty_seconds).cuda()
    bounds = np.array([[a, a + n] for a, n in zip(OFFSETS, LENGTHS)], dtype=np.int64)
    got = audio.log_mel_chunks(wav, bounds, n_mels=80)
    assert tuple(got.shape) == (5, 80, audio.N_FRAMES) and got.is_cuda
    assert torch.equal(got, audio.log_mel_chunks(forty_seconds, bounds, n_mels=80, device="cuda"))  # numpy in
    host = audio.log_mel_chunks(forty_seconds, bounds, n_mels=80, device="cpu")
    for b, (a, n) in enumerate(zip(OFFSETS, LENGTHS)):
        single = _kernel(wav, 80, audio.N_SAMPLES - n, first=a, length=n)
        assert torch.equal(got[b].view(torch.int32), single.view(torch.int32)), b
        err = float((got[b].cpu().double() - host[b].double()).abs().max())
        print(f"chunk {b}: |kernel - host route| {err:.3e}")
        assert err <= cases.tol, (b, err)
    assert torch.all(got[0] == -1.5)  # the empty chunk
    assert len({float(got[b].max()) for b in range(5)}) == 5  # separate maxima
    # dict segments are sliced as asr.py:179-184 slices them
    segs = [{"start": 1.000081, "end": 5.8612}, {"start": 7.7160625, "end": 37.7160625}]
    by_dict = audio.log_mel_chunks(wav, segs)
    for b, s in enumerate(segs):
        f1, f2 = int(s["start"] * 16000), int(s["end"] * 16000)
        assert torch.equal(by_dict[b], _kernel(wav, 80, audio.N_SAMPLES - (f2 - f1), first=f1, length=f2 - f1))

    # rows of a sentinel-filled parent: the float before and the float after each row stay
    for n_mels in (80, 128):
        parent = torch.full((5, n_mels, audio.N_FRAMES + 2), SENTINEL, dtype=torch.float32, device="cuda")
        out = parent[:, :, 1:audio.N_FRAMES + 1]
        _lib.log_mel(wav, OFFSETS, LENGTHS, [audio.N_SAMPLES - n for n in LENGTHS], audio.mel_filters(wav.device, n_mels),
                     out=out)
        assert torch.all(parent[:, :, 0] == SENTINEL) and torch.all(parent[:, :, -1] == SENTINEL)
        if n_mels == 80:
            assert torch.equal(out, got)
    # frames a shorter chunk does not have are not written either
    parent = torch.full((2, 80, 70), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.log_mel(wav, [5, 77], [10401, 4959], [0, 333], audio.mel_filters(wav.device, 80), out=parent[:, :, 1:69])
    assert torch.all(parent[0, :, 66:] == SENTINEL) and torch.all(parent[1, :, 34:] == SENTINEL)
    assert torch.all(parent[:, :, 0] == SENTINEL) and torch.all(parent[:, :, 1:34] != SENTINEL)


def test_streams(forty_seconds):
    from whisperx_amd import audio

    wav = torch.from_numpy(forty_seconds).cuda()
    b1 = np.array([[a, a + n] for a, n in zip(OFFSETS, LENGTHS)], dtype=np.int64)
    b2 = np.array([[160000, 400000], [3, 160003], [600000, 640000]], dtype=np.int64)
    want1, want2 = audio.log_mel_chunks(wav, b1), audio.log_mel_chunks(wav, b2, n_mels=128)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        alone = audio.log_mel_chunks(wav, b1)
    s1.synchronize()
    assert torch.equal(alone, want1)
    got1, got2 = [], []
    for _ in range(3):  # interleaved: each stream has its own workspace
        with torch.cuda.stream(s1):
            got1.append(audio.log_mel_chunks(wav, b1))
        with torch.cuda.stream(s2):
            got2.append(audio.log_mel_chunks(wav, b2, n_mels=128))
    s1.synchronize()
    s2.synchronize()
    for g in got1:
        assert torch.equal(g, want1)
    for g in got2:
        assert torch.equal(g, want2)

"""tests/mel_probes.py without a GPU: the reference's fp32 formula and the package's host route pass
every probe set (the host route for the first time at right paddings 0 < pad < 200), a direct-DFT fp32
restatement of wx_log_mel's arithmetic passes them too, and the same restatement with one defect
switched on is rejected, each defect by the set named beside it."""
import numpy as np
import pytest
import torch

import mel_probes as mp

N_SAMPLES = 480000
TRAIN_128_STARTS = (0, 39, 40, 159)


def _sets(n_mels):
    for name, build in mp.SETS.items():
        yield build(n_mels, TRAIN_128_STARTS) if (name, n_mels) == ("impulse_train", 128) else build(n_mels)


@pytest.mark.parametrize("n_mels", [80, 128])
def test_reference_f32_passes_every_probe(n_mels):
    for st in _sets(n_mels):
        st.check(mp.per_chunk(mp.reference_f32), "reference_f32")  # (ref_err is this figure: a quarter of the bound)
    assert mp.check_poison_outside(mp.per_chunk(mp.reference_f32), n_mels) > 0
    assert mp.check_poison_neighbour(mp.per_chunk(mp.reference_f32), n_mels) > 0


def _host(x, n_mels, padding, filt):
    """(the filterbank is the package's own: _host_run sees to it that it is the probe's)"""
    from whisperx_amd import audio

    return audio.log_mel_spectrogram(x, n_mels, padding=padding, device="cpu").numpy()


def _with_filters(p):
    """The package's filterbank cache holding the probe's own filterbank (the edge-bin probes')."""
    if p.filt is mp.filters(p.n_mels):
        return None
    return {("cpu", p.n_mels): torch.from_numpy(p.filt.copy())}


def _host_run(p, monkeypatch):
    from whisperx_amd import audio

    swap = _with_filters(p)
    if swap is None:
        assert np.array_equal(audio.mel_filters("cpu", p.n_mels).numpy(), p.filt)
        return mp.per_chunk(_host)(p)
    with monkeypatch.context() as m:
        m.setattr(audio, "_filters", swap)
        return mp.per_chunk(_host)(p)


@pytest.mark.parametrize("n_mels", [80, 128])
def test_host_route_passes_every_probe(n_mels, monkeypatch):
    for st in _sets(n_mels):
        st.check(lambda p: _host_run(p, monkeypatch), "host route")


def _host_chunks(p):
    from whisperx_amd import audio

    bounds = np.stack([p.first, p.first + p.length], axis=1)
    out = audio.log_mel_chunks(p.wave, bounds, n_mels=p.n_mels, device="cpu")
    assert tuple(out.shape) == (p.B, p.n_mels, audio.N_FRAMES)
    return list(out.numpy())


def _to_30s(st, pick=None):
    """The set's shared-waveform calls as log_mel_chunks makes them: every chunk padded to 30 s."""
    probes = [(p if pick is None else p.select(pick)).padded_to(N_SAMPLES) for p in st.probes]
    return mp.ProbeSet(st.name + "_to30s", probes)


def test_log_mel_chunks_host_route_on_the_shared_waveforms():
    """log_mel_chunks pads every chunk to 30 s, so the shared-waveform sets are restated with that
    padding (a bound of their own, measured the same way); of the impulse train the chunks at
    s = 0, 39, 40, 159."""
    edge = mp.edge_impulses(80)
    abutting = mp.ProbeSet("edge_abutting_to30s", [edge.probes[1].padded_to(N_SAMPLES)])
    for st in (_to_30s(mp.impulse_train(80), TRAIN_128_STARTS), abutting, _to_30s(mp.maxima(80)), _to_30s(mp.skip_boundary(80))):
        st.check(_host_chunks, "log_mel_chunks")
    assert mp.check_poison_outside(lambda p: _host_chunks(p.padded_to(N_SAMPLES)), 80) > 0
    assert mp.check_poison_neighbour(lambda p: _host_chunks(p.padded_to(N_SAMPLES)), 80) > 0


# --------------------------------------------------------------------------- the restatement
DEFECTS = {
    # defect: (the set that must reject it, what the restatement then does)
    "tap_7_dropped": ("impulse_train", "row 7 of the windowed basis is zero"),
    "symmetric_hann": ("impulse_train", "the window is hann(400, periodic=False)"),
    "slot_64_one_late": ("impulse_train", "the first frame of every later block of 64 reads one sample late"),
    "three_hops": ("impulse_train", "frame f holds frame f + 3's samples"),
    "reflect_about_L": ("edge_impulses", "the right reflection is j -> 2 L - j"),
    "reflect_about_audio_end": ("edge_impulses", "the audio is reflected at its own end, then padded with zeros"),
    "bin_200_dropped": ("edge_bins", "the power of bin 200 is zero"),
    "filter_columns_shifted": ("even_tones", "bin k meets filterbank column k - 1"),
    "batch_maximum": ("maxima", "one maximum for all the chunks of a call"),
    "maximum_of_first_block": ("maxima", "a chunk's maximum is taken over its first 64 frames"),
    "len_ignored": ("edge_impulses", "the waveform beyond the chunk is read in place of the zero padding"),
}


@pytest.fixture(scope="module")
def bases():
    n = np.arange(mp.N_FFT)
    ang = 2.0 * np.pi * ((n[:, None] * np.arange(mp.BINS)[None, :]) % mp.N_FFT) / mp.N_FFT
    out = {}
    for sym in (False, True):
        win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / (mp.N_FFT - 1 if sym else mp.N_FFT))
        out[sym] = ((win[:, None] * np.cos(ang)).astype(np.float32), (win[:, None] * np.sin(ang)).astype(np.float32))
    return out


def restated(p, bases, defect=None):
    """wx_log_mel's arithmetic as a direct DFT in fp32 numpy: per-sample reflection and padding as the
    kernel's staging resolves them, the Hann window folded into a [400 x 201] cosine and sine basis
    (rounded from fp64), power, projection, log10, the chunk's own floor."""
    assert defect is None or defect in DEFECTS
    cosb, sinb = (b.copy() for b in bases[defect == "symmetric_hann"])
    if defect == "tap_7_dropped":
        cosb[7] = sinb[7] = 0.0
    filt = p.filt
    if defect == "filter_columns_shifted":
        filt = np.roll(filt, 1, axis=1)
    n, n_wave, logs = np.arange(mp.N_FFT), len(p.wave), []
    for b in range(p.B):
        first, ln = int(p.first[b]), int(p.length[b])
        L = ln + int(p.pad[b])
        f = np.arange(L // mp.HOP)
        i = mp.HOP * (f + 3 if defect == "three_hops" else f)[:, None] - mp.N_FFT // 2 + n[None, :]
        if defect == "slot_64_one_late":
            i[(f % mp.BLOCK == 0) & (f > 0)] += 1
        j = np.abs(i)
        if defect == "reflect_about_audio_end":
            ok = j < ln + mp.N_FFT // 2
            j = np.where(j >= ln, 2 * (ln - 1) - j, j)
        else:
            ok = i < L + mp.N_FFT // 2
            j = np.where(j >= L, (2 * L if defect == "reflect_about_L" else 2 * (L - 1)) - j, j)
        ok &= (j >= 0) & (first + j < n_wave)
        if defect != "len_ignored":
            ok &= j < ln
        x = np.where(ok, p.wave[np.clip(first + j, 0, n_wave - 1)], np.float32(0.0)).astype(np.float32)
        re, im = x @ cosb, x @ sinb
        power = re * re + im * im
        if defect == "bin_200_dropped":
            power[:, 200] = 0.0
        logs.append(np.log10(np.maximum(filt @ power.T, np.float32(1e-10))))
        assert logs[-1].dtype == np.float32
    outs = []
    for lg in logs:
        mx = lg.max()
        if defect == "batch_maximum":
            mx = max(v.max() for v in logs)
        elif defect == "maximum_of_first_block":
            mx = lg[:, :mp.BLOCK].max()
        outs.append((np.maximum(lg, mx - np.float32(8.0)) + np.float32(4.0)) / np.float32(4.0))
    return outs


@pytest.mark.parametrize("n_mels", [80, 128])
def test_restatement_passes_every_probe(n_mels, bases):
    for st in _sets(n_mels):
        st.check(lambda p: restated(p, bases), "restatement")
    assert mp.check_poison_outside(lambda p: restated(p, bases), n_mels) > 0
    assert mp.check_poison_neighbour(lambda p: restated(p, bases), n_mels) > 0


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_every_defect_is_rejected_by_its_probe(defect, bases):
    st = mp.SETS[DEFECTS[defect][0]](80)
    with pytest.raises(AssertionError, match="4 x ref_err") as e:
        st.check(lambda p: restated(p, bases, defect), defect)
    print(e.value)


def test_reading_past_a_chunk_is_also_caught_by_the_poison_probe(bases):
    with pytest.raises(AssertionError, match="poison"):
        mp.check_poison_outside(lambda p: restated(p, bases, "len_ignored"), 80)


def test_taps_1_and_399_and_filter_columns_0_and_200_are_unobservable():
    """What the module docstring states: the impulse train counts taps 2 .. 398, and Whisper's
    filterbank gives bins 0 and 200 no weight (hence the edge-bin set's moved columns)."""
    st = mp.impulse_train(80)
    assert st.pairs == 64 * 397
    for n_mels in (80, 128):
        w = mp.filters(n_mels)
        assert not w[:, 0].any() and not w[:, 200].any() and w[:, 1].any() and w[:, 199].any()
        assert mp.edge_bins(n_mels).entries > 0

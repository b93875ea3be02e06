"""Probes for Whisper's input features (wx_log_mel and the host route; numpy and CPU torch only, nothing
from the package): inputs built so that one wrong tap, frame slot, bin, filter entry, reflected sample
or chunk maximum moves an output by far more than the bound, which noise-like signals at the same bound
only do in probability.

A probe is one call log_mel(wave, first[], length[], pad[], filters) -> [B, n_mels, F]: chunk b is the
reference's log_mel_spectrogram(wave[first[b] : first[b] + length[b]], n_mels, padding=pad[b]).  A set is
a list of such calls with one bound, 4 x ref_err(set): ref_err is the largest distance of reference_f32
(the reference's formula, audio.py:147-159, in fp32 torch with torch.stft) from reference_f64 (the same
formula in numpy fp64 on the fp32 samples and the fp32 filterbank) over every value of every chunk of
the set.  It is measured when the set is built, measures the reference and never the code under test,
and is per set because per-chunk reference errors go down to one output ulp.  Every set asserts
4 x ref_err < 2**-11 (fp16's spacing in [0.5, 1), the criterion of tests/golden/make_mel_golden.py) and
its own coverage condition from the fp64 reference alone.

  impulse train   one waveform, an impulse every 480 samples (amplitudes 1 + (m % 7) / 8: neighbours
                  differ, so a frame displaced by whole hops fails); chunk s is wave[s : s + 32000],
                  s = 0 .. 159, 200 frames.  No frame sees two impulses; an interior frame f sees its
                  impulse at tap n = p + 200 - 160 f, and as the tap residue has period 3 frames (coprime
                  to 64) every pair (frame slot f % 64, tap 2 .. 398), 25,408 pairs, occurs in an interior
                  frame all of whose n_mels values lie above the chunk's floor (asserted).  Tap 0 has
                  window weight 0, and taps 1 and 399 (weight 6.2e-5, power 3.8e-9) lie more than 8
                  decades under the chunk's best frame: every frame that holds its impulse there is at
                  the floor (asserted), so no log-mel input can observe those two taps.
  edge impulses   lengths 4959 and 10277 x right padding 0, 1, 37, 159, 160, 199, 200, 201, impulses of
                  amplitude 1 + i / 8 at samples 0, 1, 199, 200, len - 201, len - 200, len - 2, len - 1:
                  once with zeros between the chunks, once back to back (a chunk's reflection then has a
                  neighbour's impulse one sample beyond its end).  Skip boundary: audio of 10039, 10040,
                  10041 samples padded to 30720 with an impulse at the last sample; the second block of
                  64 frames stages from padded position 160 * 64 - 200 = 10040.
  even tones      0.5 cos(2 pi k n / 400), 10401 samples, every k = 0 .. 200 (phase 0 and
                  len = 1 (mod 200) make both reflections seamless: every frame holds bins k - 1, k, k + 1
                  and nothing else).  Every nonzero filterbank entry filt[m][k] (391 at 80 mels, 394 at
                  128) lies at least 0.25, one decade, above the floor in the output of tone k
                  (asserted).  94 - 99 % of a tone's outputs are at the floor: that is what a tone is.
  edge bins       columns 0 and 200 of Whisper's filterbank are zero, so through it no input observes
                  bins 0 and 200 (nor the kernel's guard on the last bin tile).  Tones 198 .. 200 are
                  run through the filterbank with its columns moved up by one bin (bin 200 carries
                  column 199), tones 0 .. 2 with the columns moved down by one (bin 0 carries column 1).
  two-level tones even tones k1 and k2, k2 40, 60 and 70 dB down: the weak bins carry the absolute
                  rounding error of the strong ones.
  tilted noise    noise through four 8-tap box filters (peak 0.3) plus white noise 40, 60, 75 dB down.
  maxima          a loud chunk (amplitude 64, maximum in frame 0), a quiet one (2**-10: its log maximum
                  is negative, its floor under -10), a silent one (all -1.5) and a second loud one
                  (maximum in the last frame of a partial second block), in one call.
  poison          what a call must not depend on holds zeros in one run and NaN in the other.

Every checker returns its figure and raises AssertionError (a NaN fails every comparison here)."""
import functools
import os

import numpy as np
import torch

N_FFT, HOP, BINS, BLOCK = 400, 160, 201, 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP16_SPACING = 2.0 ** -11


@functools.lru_cache(maxsize=None)
def filters(n_mels):
    """Whisper's [n_mels, 201] fp32 filterbank (tests/golden/mel_filters.npz)."""
    with np.load(os.path.join(GOLDEN, "mel_filters.npz")) as f:
        w = np.ascontiguousarray(f[f"mel_{n_mels}"], dtype=np.float32)
    assert w.shape == (n_mels, BINS)
    return w


def rolled_filters(n_mels, by):
    """The filterbank with its columns moved by `by` bins (the column that leaves is zero)."""
    w = filters(n_mels)
    assert not w[:, -1 if by > 0 else 0].any()
    return np.ascontiguousarray(np.roll(w, by, axis=1))


# ------------------------------------------------------------------------------------ references
def reference_f64(x, n_mels, padding, filt, with_floor=False):
    """audio.py:147-159 in fp64: the fp32 samples and the fp32 filterbank are the inputs, every
    operation on them (window, DFT, power, projection, log10, floor, affine) is fp64.  with_floor: also
    the value that an output held up by the floor max(., max - 8) has (-1.5, the clamp, where the floor
    lies under it)."""
    assert filt.shape == (n_mels, BINS) and filt.dtype == np.float32
    x = np.concatenate([np.asarray(x, dtype=np.float64), np.zeros(int(padding))])
    L = len(x)
    xp = np.pad(x, N_FFT // 2, mode="reflect")  # torch.stft(center=True, pad_mode="reflect")
    n = np.arange(N_FFT)
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)  # periodic Hann
    frames = xp[HOP * np.arange(L // HOP)[:, None] + n[None, :]]  # the last STFT frame is dropped
    power = np.abs(np.fft.rfft(frames * window, axis=1)) ** 2
    mel = filt.astype(np.float64) @ power.T
    log_spec = np.log10(np.maximum(mel, 1e-10))
    floor = max(float(log_spec.max()) - 8.0, float(np.log10(1e-10)))
    log_spec = np.maximum(log_spec, log_spec.max() - 8.0)
    out = (log_spec + 4.0) / 4.0
    return (out, (floor + 4.0) / 4.0) if with_floor else out


def reference_f32(x, n_mels, padding, filt):
    """The same lines in fp32 torch, as the reference has them."""
    audio = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if padding > 0:
        audio = torch.nn.functional.pad(audio, (0, int(padding)))
    window = torch.hann_window(N_FFT)
    stft = torch.stft(audio, N_FFT, HOP, window=window, return_complex=True)
    magnitudes = stft[..., :-1].abs() ** 2
    mel_spec = torch.from_numpy(filt) @ magnitudes
    log_spec = torch.clamp(mel_spec, min=1e-10).log10()
    log_spec = torch.maximum(log_spec, log_spec.max() - 8.0)
    return ((log_spec + 4.0) / 4.0).numpy()


# ------------------------------------------------------------------------------------ probes and sets
class Probe:
    """One call: a waveform, the chunks' first sample / length / right zero padding, a filterbank."""

    def __init__(self, name, wave, first, length, pad, n_mels, filt=None):
        self.name, self.n_mels = name, int(n_mels)
        self.wave = np.ascontiguousarray(wave, dtype=np.float32)
        self.first, self.length, self.pad = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (first, length, pad))
        self.filt = filters(n_mels) if filt is None else filt
        self.B = len(self.first)
        assert self.B == len(self.length) == len(self.pad) and self.B > 0
        assert (self.first >= 0).all() and (self.first + self.length <= len(self.wave)).all()
        assert (self.length + self.pad > N_FFT // 2).all()  # torch's reflect padding needs it

    def frames(self, b):
        return int(self.length[b] + self.pad[b]) // HOP

    def chunk(self, b):
        return self.wave[int(self.first[b]):int(self.first[b] + self.length[b])]

    def covered(self):
        """Which samples of the waveform belong to a chunk."""
        m = np.zeros(len(self.wave), dtype=bool)
        for b in range(self.B):
            m[int(self.first[b]):int(self.first[b] + self.length[b])] = True
        return m

    def with_wave(self, wave, name=None):
        return Probe(name or self.name, wave, self.first, self.length, self.pad, self.n_mels, self.filt)

    def padded_to(self, n):
        """The same chunks, each padded with zeros to n samples."""
        return Probe(f"{self.name}_to{n}", self.wave, self.first, self.length, n - self.length, self.n_mels, self.filt)

    def select(self, idx):
        idx = list(idx)
        return Probe(self.name, self.wave, self.first[idx], self.length[idx], self.pad[idx], self.n_mels, self.filt)


def per_chunk(fn):
    """A runner that calls fn(x, n_mels, padding, filt) -> [n_mels, F] on every chunk by itself."""
    return lambda p: [np.asarray(fn(p.chunk(b), p.n_mels, int(p.pad[b]), p.filt)) for b in range(p.B)]


class ProbeSet:
    """Calls under one bound.  want[i][b] is chunk b of call i in fp64, floor[i][b] its floor value."""

    def __init__(self, name, probes):
        self.name, self.probes = name, list(probes)
        both = [[reference_f64(p.chunk(b), p.n_mels, int(p.pad[b]), p.filt, with_floor=True) for b in range(p.B)]
                for p in self.probes]
        self.want = [[w for w, _ in call] for call in both]
        self.floor = [[f for _, f in call] for call in both]
        self.ref_err = 0.0
        for p, want in zip(self.probes, self.want):
            for b, r in enumerate(per_chunk(reference_f32)(p)):
                assert r.dtype == np.float32 and r.shape == want[b].shape == (p.n_mels, p.frames(b))
                self.ref_err = max(self.ref_err, float(np.abs(r.astype(np.float64) - want[b]).max()))
        self.bound = 4.0 * self.ref_err
        assert 0.0 < self.bound < FP16_SPACING, f"{name}: 4 x ref_err = {self.bound:.3e} reaches fp16's spacing 2**-11"
        self.values = sum(w.size for want in self.want for w in want)

    def errors(self, outs):
        """(largest |out - fp64|, where): outs[i][b] is [n_mels, >= frames] of chunk b of call i."""
        worst, where = 0.0, None
        assert len(outs) == len(self.probes)
        for i, (p, want) in enumerate(zip(self.probes, self.want)):
            assert len(outs[i]) == p.B, (self.name, p.name, len(outs[i]))
            for b, w in enumerate(want):
                got = np.asarray(outs[i][b])
                assert got.dtype == np.float32 and got.shape[0] == p.n_mels and got.shape[1] >= w.shape[1], \
                    (self.name, p.name, b, got.dtype, got.shape)
                e = np.abs(got[:, :w.shape[1]].astype(np.float64) - w)
                e = np.where(np.isfinite(e), e, np.inf)
                if e.size and float(e.max()) >= worst:
                    m, f = np.unravel_index(int(e.argmax()), e.shape)
                    worst = float(e.max())
                    where = (f"call {p.name} chunk {b} (first {int(p.first[b])}, len {int(p.length[b])}, pad "
                             f"{int(p.pad[b])}) mel {int(m)} frame {int(f)} (slot {int(f) % BLOCK}): got "
                             f"{float(got[m, f])!r}, fp64 {float(w[m, f])!r}")
        return worst, where

    def check(self, run, label):
        """`run(probe)` -> the chunks' outputs.  max |out - fp64| <= 4 x ref_err(set); prints and returns it."""
        err, where = self.errors([run(p) for p in self.probes])
        print(f"{self.name:24s} {label:14s} |out - fp64| {err:.3e}  ref_err {self.ref_err:.3e}  bound {self.bound:.3e}  "
              f"ratio to ref_err {err / self.ref_err:.2f}  ({self.values} values)")
        if not err <= self.bound:
            raise AssertionError(f"{self.name} ({label}): |out - fp64| {err:.3e} > 4 x ref_err {self.bound:.3e}; worst at {where}")
        return err


def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


# ------------------------------------------------------------------------------------ impulse train
TRAIN_PERIOD, TRAIN_FRAMES, TRAIN_STARTS = 480, 200, 160


def _train_tap(s, f):
    """The tap at which frame f of the chunk that starts at sample s sees its impulse (or -1): the
    frame covers chunk samples 160 f - 200 .. 160 f + 199."""
    lo = s + HOP * f - N_FFT // 2
    p = -(-lo // TRAIN_PERIOD) * TRAIN_PERIOD  # the first impulse at or after lo
    return p - lo if p - lo < N_FFT else -1


@functools.lru_cache(maxsize=None)
def impulse_train(n_mels=80, starts=tuple(range(TRAIN_STARTS))):
    n = HOP * TRAIN_FRAMES
    wave = np.zeros(TRAIN_STARTS - 1 + n, dtype=np.float32)
    pos = np.arange(0, len(wave), TRAIN_PERIOD)
    wave[pos] = 1.0 + ((pos // TRAIN_PERIOD) % 7) / 8.0
    assert TRAIN_PERIOD >= N_FFT  # no frame sees two impulses
    st = ProbeSet(f"impulse_train_{n_mels}", [Probe("train", wave, list(starts), [n] * len(starts), [0] * len(starts), n_mels)])
    seen = np.zeros((BLOCK, N_FFT), dtype=bool)
    for b, s in enumerate(starts):
        want, floor = st.want[0][b], st.floor[0][b]
        for f in range(2, (n - N_FFT // 2) // HOP + 1):  # interior: no reflected sample in the frame
            assert HOP * f - N_FFT // 2 >= 0 and HOP * f + N_FFT // 2 - 1 < n
            tap = _train_tap(s, f)
            if tap in (1, N_FFT - 1):
                assert np.all(want[:, f] == floor), (s, f, tap)  # more than 8 decades down: unobservable
            elif tap >= 2 and float(want[:, f].min()) > floor:
                seen[f % BLOCK, tap] = True
    st.pairs = int(seen[:, 2:N_FFT - 1].sum())
    if starts == tuple(range(TRAIN_STARTS)):
        assert st.pairs == BLOCK * (N_FFT - 3) == 25408, st.pairs  # every (slot, tap 2 .. 398)
    return st


# ------------------------------------------------------------------------------------ edge impulses
EDGE_LENS = (4959, 10277)
EDGE_PADS = (0, 1, 37, 159, 160, 199, 200, 201)
EDGE_GAP = 512


def _edge_chunk(n):
    x = np.zeros(n, dtype=np.float32)
    for i, p in enumerate((0, 1, 199, 200, n - 201, n - 200, n - 2, n - 1)):
        x[p] = 1.0 + i / 8.0
    return x


@functools.lru_cache(maxsize=None)
def edge_impulses(n_mels=80):
    cases = [(n, pad) for n in EDGE_LENS for pad in EDGE_PADS]
    probes = []
    for name, gap in (("apart", EDGE_GAP), ("abutting", 0)):
        parts, first = [], []
        for n, _ in cases:
            first.append(sum(len(v) for v in parts))
            parts += [_edge_chunk(n), np.zeros(gap, dtype=np.float32)]
        wave = np.concatenate(parts)
        probes.append(Probe(name, wave, first, [n for n, _ in cases], [pad for _, pad in cases], n_mels))
        if not gap:  # the sample past a chunk's end is the next chunk's first impulse
            assert all(wave[f + n] == 1.0 for f, (n, _) in list(zip(first, cases))[:-1])
    st = ProbeSet(f"edge_impulses_{n_mels}", probes)
    for want, floors in zip(st.want, st.floor):
        for w, fl in zip(want, floors):  # the impulses at both ends are seen: the first and the last frame lie above the floor
            assert float(w[:, 0].min()) > fl and float(w[:, -1].min()) > fl
    return st


SKIP_LENS = (10039, 10040, 10041)
SKIP_PADDED = 30720


@functools.lru_cache(maxsize=None)
def skip_boundary(n_mels=80):
    """The any-audio decision of the second block of 64 frames, one sample either side."""
    assert BLOCK * HOP - N_FFT // 2 == SKIP_LENS[1]
    parts, first = [], []
    for n in SKIP_LENS:
        first.append(sum(len(v) for v in parts))
        x = np.zeros(n, dtype=np.float32)
        x[-1] = 1.0
        parts.append(x)
    return ProbeSet(f"skip_boundary_{n_mels}", [Probe("skip", np.concatenate(parts), first, SKIP_LENS,
                                                      [SKIP_PADDED - n for n in SKIP_LENS], n_mels)])


# ------------------------------------------------------------------------------------ tones
TONE_LEN = 10401
FILTER_MARGIN = 0.25  # one decade, in output units


def _tone(k, n=TONE_LEN, amp=0.5):
    return amp * np.cos(2.0 * np.pi * ((k * np.arange(n)) % N_FFT) / N_FFT)


def _tones_probe(name, tones, n_mels, filt=None):
    wave = np.concatenate([np.asarray(t, dtype=np.float32) for t in tones])
    lens = [len(t) for t in tones]
    return Probe(name, wave, np.cumsum([0] + lens[:-1]), lens, [0] * len(lens), n_mels, filt)


def _assert_filter_entries_seen(st, probe_i, ks, filt):
    """Every nonzero filt[m][k] lies at least a decade above the floor in every frame of tone k."""
    n = 0
    for b, k in enumerate(ks):
        w = st.want[probe_i][b]
        for m in np.nonzero(filt[:, k])[0]:
            assert float(w[m].min()) >= st.floor[probe_i][b] + FILTER_MARGIN, (st.name, k, int(m))
            n += 1
    return n


@functools.lru_cache(maxsize=None)
def even_tones(n_mels=80):
    assert TONE_LEN % 200 == 1
    ks = list(range(BINS))
    st = ProbeSet(f"even_tones_{n_mels}", [_tones_probe("tones", [_tone(k) for k in ks], n_mels)])
    st.entries = _assert_filter_entries_seen(st, 0, ks, filters(n_mels))
    assert st.entries == int(np.count_nonzero(filters(n_mels))) == {80: 391, 128: 394}[n_mels]
    values = np.concatenate([(w == fl).ravel() for w, fl in zip(st.want[0], st.floor[0])])
    st.at_floor = float(values.mean())
    assert 0.94 <= st.at_floor <= 0.99, st.at_floor
    return st


@functools.lru_cache(maxsize=None)
def edge_bins(n_mels=80):
    """Bins 0 and 200 through filterbanks in which they carry a weight."""
    up, down = rolled_filters(n_mels, 1), rolled_filters(n_mels, -1)
    assert up[:, 200].any() and down[:, 0].any()
    hi, lo = [198, 199, 200], [0, 1, 2]
    st = ProbeSet(f"edge_bins_{n_mels}", [_tones_probe("columns_up", [_tone(k) for k in hi], n_mels, up),
                                          _tones_probe("columns_down", [_tone(k) for k in lo], n_mels, down)])
    st.entries = _assert_filter_entries_seen(st, 0, hi, up) + _assert_filter_entries_seen(st, 1, lo, down)
    return st


TWO_LEVEL_PAIRS = ((10, 150), (150, 10), (3, 199), (100, 121), (60, 64))
TWO_LEVEL_DB = (40, 60, 70)


@functools.lru_cache(maxsize=None)
def two_level_tones(n_mels=80):
    tones = [_tone(k1) + _tone(k2, amp=0.5 * 10.0 ** (-db / 20.0)) for k1, k2 in TWO_LEVEL_PAIRS for db in TWO_LEVEL_DB]
    return ProbeSet(f"two_level_tones_{n_mels}", [_tones_probe("two_level", tones, n_mels)])


TILT_FRAMES = 66
TILT_DB = (40, 60, 75)


@functools.lru_cache(maxsize=None)
def tilted_noise(n_mels=80):
    n = TILT_FRAMES * HOP
    chunks = []
    for i, db in enumerate(TILT_DB):
        g = _rng(7, i)
        low = g.standard_normal(n + 28)
        for _ in range(4):
            low = np.convolve(low, np.full(8, 0.125), mode="valid")
        low *= 0.3 / np.abs(low).max()
        white = g.standard_normal(n)
        chunks.append(low + white * (np.sqrt(np.mean(low ** 2) / np.mean(white ** 2)) * 10.0 ** (-db / 20.0)))
    return ProbeSet(f"tilted_noise_{n_mels}", [_tones_probe("tilted", chunks, n_mels)])


# ------------------------------------------------------------------------------------ maxima
@functools.lru_cache(maxsize=None)
def maxima(n_mels=80):
    g = _rng(11)
    loud0 = 16.0 * g.uniform(-1, 1, 10401)
    loud0[:40] *= 4.0  # amplitude 64 at the very start: the maximum lies in frame 0
    loud0[3000:6000] = 0.0  # frames of silence: they sit on the floor, which follows the chunk's own maximum
    quiet = 2.0 ** -10 * g.uniform(-1, 1, 10401)
    quiet[4000:6000] = 0.0
    silent = np.zeros(5000)
    loud1 = 16.0 * g.uniform(-1, 1, 100 * HOP)
    loud1[-200:] *= 4.0  # ... in frame 99, the last of the partial second block (centred 160 samples before the end)
    loud1[3000:6000] = 0.0
    st = ProbeSet(f"maxima_{n_mels}", [_tones_probe("maxima", [loud0, quiet, silent, loud1], n_mels)])
    w = st.want[0]
    assert int(np.unravel_index(w[0].argmax(), w[0].shape)[1]) == 0
    assert int(np.unravel_index(w[3].argmax(), w[3].shape)[1]) == 99 and w[3].shape[1] == 99 + 1 > BLOCK
    assert float(w[3][:, :BLOCK].max()) < float(w[3].max()) - 0.125  # the first block alone gives another floor
    assert float(w[1].max()) < 0.5 and float(w[1].min()) == -1.5  # log maximum < -2: the floor lies under the clamp
    assert np.all(w[2] == -1.5)
    for b in (0, 3):
        assert float(w[b].min()) == st.floor[0][b] > float(w[1].max())  # a loud chunk's floor would flatten the quiet one
    return st


# ------------------------------------------------------------------------------------ poison
POISON_FILLS = (0.0, float("nan"))


def _noise_layout(n_mels, seed):
    """Noise chunks with a lead, gaps and a tail around them; pads that put the reflection and the
    zero padding next to what lies outside."""
    g = _rng(13, seed)
    lens, pads, gaps = [4959, 10401, 201, 5120, 10277], [0, 37, 333, 0, 199], [7, 1, 300, 3, 64, 129]
    wave, first = [np.zeros(gaps[0])], []
    for n, gap in zip(lens, gaps[1:]):
        first.append(sum(len(v) for v in wave))
        wave += [0.1 * g.standard_normal(n), np.zeros(gap)]
    return Probe("poison", np.concatenate(wave), first, lens, pads, n_mels)


def _bit_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _trim(p, outs):
    return [np.asarray(outs[b])[:, :p.frames(b)] for b in range(p.B)]


def check_poison_outside(run, n_mels=80):
    """Every sample that belongs to no chunk (lead, gaps, tail) holds zeros in one run and NaN in the
    other: the outputs are finite and equal bit for bit.  Returns the number of values compared."""
    p = _noise_layout(n_mels, 0)
    outs = []
    for fill in POISON_FILLS:
        wave = p.wave.copy()
        wave[~p.covered()] = fill
        outs.append(_trim(p, run(p.with_wave(wave))))
    n = 0
    for b, (clean, dirty) in enumerate(zip(*outs)):
        if not np.isfinite(clean).all():
            raise AssertionError(f"poison: chunk {b} over zeros is not finite")
        if not np.isfinite(dirty).all():
            raise AssertionError(f"poison: chunk {b} is not finite when the samples outside the chunks hold NaN")
        if not _bit_equal(clean, dirty):
            raise AssertionError(f"poison: {int((clean != dirty).sum())} values of chunk {b} depend on samples outside it")
        n += clean.size
    return n


def check_poison_neighbour(run, n_mels=80, bad=2):
    """A NaN sample inside chunk `bad` (whose own output is out of scope) leaves every other chunk of
    the call bit-equal to the call without it.  Returns the number of values compared."""
    p = _noise_layout(n_mels, 1)
    clean = _trim(p, run(p))
    wave = p.wave.copy()
    wave[int(p.first[bad]) + int(p.length[bad]) // 2] = np.nan
    dirty = _trim(p, run(p.with_wave(wave)))
    n = 0
    for b in range(p.B):
        if b == bad:
            continue
        if not np.isfinite(clean[b]).all() or not _bit_equal(clean[b], dirty[b]):
            raise AssertionError(f"poison: chunk {b} changes when chunk {bad} of the same call holds a NaN sample")
        n += clean[b].size
    return n


def check_bit_equal(p, a, b, label):
    """Two runs of one probe agree bit for bit on every valid frame."""
    for i, (x, y) in enumerate(zip(_trim(p, a), _trim(p, b))):
        if not _bit_equal(x, y):
            raise AssertionError(f"{label}: chunk {i} differs in {int((x != y).sum())} values")


SETS = {"impulse_train": impulse_train, "edge_impulses": edge_impulses, "skip_boundary": skip_boundary,
        "even_tones": even_tones, "edge_bins": edge_bins, "two_level_tones": two_level_tones,
        "tilted_noise": tilted_noise, "maxima": maxima}

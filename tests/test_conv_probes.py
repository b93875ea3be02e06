"""The conv / LSTM / norm probes' own conditions (tests/conv_probes.py), without a GPU: torch's fp32
CPU convolution passes every integer probe bit for bit at every shape the GPU tests use, the exactness
preconditions hold there, and each faulty restatement of the convolution below, the kind of mistake a
HIP kernel or its weight packer could make, is rejected at every shape at which it applies."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_probes as cp

POSCONV_CASES = [(96, 2), (128, 2)]  # Cg 48 and Cg 64


def _rejected(check, o):
    with pytest.raises(AssertionError):
        check(o)


# ------------------------------------------------------- faults on the weight side (any convolution)
def drop_last_tap(w):
    w = w.clone()
    w[..., -1] = 0
    return w


def swap_taps(w):
    """taps j and j ^ 1 exchanged (where both exist)"""
    K = w.shape[-1]
    j = torch.arange(K)
    return w[..., torch.where((j ^ 1) < K, j ^ 1, j)]


def drop_channel_4_of_16(w):
    w = w.clone()
    w[:, torch.arange(w.shape[1]) % 16 == 4] = 0
    return w


def swap_channels_4_7_with_8_11(w):
    """input channels 4..7 and 8..11 of every 16 exchanged in the (zero-padded) weights only: a packer
    that disagrees with the kernel"""
    Cin = w.shape[1]
    i = torch.arange(-(-Cin // 16) * 16)
    src = torch.where((i % 16 >= 4) & (i % 16 < 8), i + 4, torch.where((i % 16 >= 8) & (i % 16 < 12), i - 4, i))
    return F.pad(w, (0, 0, 0, len(i) - Cin))[:, src][:, :Cin].contiguous()


WEIGHT_FAULTS = [drop_last_tap, swap_taps]
CHANNEL_FAULTS = [drop_channel_4_of_16, swap_channels_4_7_with_8_11]  # (need more than 4 input channels)


def _tile_starts_from_row_before(true, shifted, tile):
    """the output frames at every `tile`-frame tile start taken from `shifted` (frame t computed one
    input row earlier); frames on the second last axis"""
    out = true.clone()
    out[..., ::tile, :] = shifted[..., ::tile, :]
    return out


def _last_frame_missing(o):
    o = o.clone()
    o[..., -1, :] = 0
    return o


# ----------------------------------------------------------------------------------- positional conv
def _posconv32(p, w=None, neighbour=False, tile_shift=False):
    w = p.w if w is None else w
    if neighbour:  # one convolution over all the packed rows: a segment's padding is its neighbours' rows
        y = F.gelu(F.conv1d(p.h.t()[None], w, p.bias, padding=64, groups=p.G)[0, :, :-1].t())
        return y + p.h if p.residual else y
    out = cp.posconv_reference(p.h, w, p.bias, p.G, p.lengths, p.residual)
    if tile_shift:
        off = cp.offsets(p.lengths)
        for a, b in zip(off[:-1], off[1:]):
            if b > a:
                seg = p.h[a:b]
                y = F.gelu(F.conv1d(F.pad(seg.t(), (65, 63))[None], w, p.bias, groups=p.G)[0, :, :b - a].t())
                out[a:b] = _tile_starts_from_row_before(out[a:b], y + seg if p.residual else y, 128)
    return out


@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("D,G", POSCONV_CASES)
def test_posconv_integer_probe(D, G, residual):
    p = cp.PosConvInt(D, G, residual)
    print(f"posconv D {D} G {G}: bound {p.bound:.0f}, largest pre-activation {p.pre_max:.0f}")
    assert p.bound < 2 ** 24 and p.pre_max <= p.bound and float(p.want.min()) >= 8
    assert p.lengths == [0, 1, 64, 65, 127, 128, 129, 0, 0, 191, 193, 257, 0]
    good = _posconv32(p)
    assert p.check(good) == p.rows * D
    faulty = [_posconv32(p, f(p.w)) for f in WEIGHT_FAULTS + CHANNEL_FAULTS]
    faulty += [_posconv32(p, neighbour=True), _posconv32(p, tile_shift=True), good[:-1], _last_frame_missing(good)]
    for o in faulty:
        _rejected(p.check, o)
    # the first wrong output is named by segment and frame
    bad = good.clone()
    bad[cp.offsets(p.lengths)[5] + 3, 7] += 1
    with pytest.raises(AssertionError, match=r"1 of \d+ rows wrong; first at segment 5 \(length 128\), frame 3, channel 7"):
        p.check(bad)


def test_posconv_packing_by_the_documented_layout():
    w = torch.arange(96 * 48 * 128, dtype=torch.float32).reshape(96, 48, 128)
    wp = cp.pack_posconv_weight(w, 2)
    assert wp.shape == (2, 128, 12, 48, 4)
    for g, j, i, o in [(0, 0, 0, 0), (1, 127, 47, 47), (1, 5, 9, 33), (0, 64, 6, 17)]:
        assert wp[g, j, i // 4, o, i % 4] == w[g * 48 + o, i, j]


# --------------------------------------------------------------------------------- k = 5 convolution
def _taps32(p, w=None, tile_shift=False):
    w = p.w if w is None else w
    out = cp.taps_reference(p.x, w, p.bias)
    if tile_shift:
        out = _tile_starts_from_row_before(out, cp.taps_reference(F.pad(p.x, (0, 0, 1, 0)), w, p.bias)[:, :-1], 128)
    return out


@pytest.mark.parametrize("L", cp.TAPS_LENGTHS)
@pytest.mark.parametrize("Cin,Cout", cp.TAPS_CHANNELS)
def test_taps_integer_probe(Cin, Cout, L):
    for with_bias in (True, False):
        p = cp.TapsInt(Cin, Cout, L, with_bias)
        assert p.bound < 2 ** 24 and float(p.want.abs().max()) <= p.bound
        assert p.want.shape == (3, L - 4, Cout) and (p.bias is None) == (not with_bias)
        good = _taps32(p)
        p.check(good)
        faults = WEIGHT_FAULTS + (CHANNEL_FAULTS if Cin > 4 else [])
        faulty = [_taps32(p, f(p.w)) for f in faults] + [_taps32(p, tile_shift=True), _last_frame_missing(good)]
        faulty += [good[:, :-1], torch.cat([good, good[:, -1:]], 1)]
        for o in faulty:
            _rejected(p.check, o)


# ---------------------------------------------------------------------------------- sinc filterbank
def _sinc32(p, w=None, tile_shift=False, window_stride=None):
    w = p.w if w is None else w
    out = cp.sinc_reference(p.x, w, p.S)
    if tile_shift:
        out = _tile_starts_from_row_before(out, cp.sinc_reference(F.pad(p.x, (p.S, 0)), w, p.S)[:-1], 256)
    if window_stride is not None:
        # every block of 256 rows computed from a window of 256 window_stride + 260 samples, zeros behind it
        for t0 in range(0, p.rows, 256):
            win = torch.zeros(256 * p.S + cp.SINC_KP)
            have = p.x[t0 * p.S:t0 * p.S + min(256 * window_stride + cp.SINC_KP, len(win))]
            win[:len(have)] = have
            out[t0:t0 + 256] = cp.sinc_reference(win, w, p.S)[:256][:p.rows - t0]
    return out


@pytest.mark.parametrize("S", cp.SINC_STRIDES)
def test_sinc_integer_probe(S):
    assert [(n - 251) // S + 1 for n in cp.sinc_spans(S)] == [256, 257, 262]
    assert (cp.sinc_spans(S)[2] - 251) % S == S - 1  # (samples left over behind the last row)
    for n in cp.sinc_spans(S):
        p = cp.SincInt(S, n)
        assert p.bound < 2 ** 24 and float(p.want.abs().max()) <= p.bound
        assert p.w_padded.shape == (260, 80) and not bool(p.w_padded[251:].any())
        good = _sinc32(p)
        p.check(good)
        p.check(_sinc32(p, window_stride=16))  # (the window the kernel has)
        faulty = [_sinc32(p, f(p.w)) for f in WEIGHT_FAULTS] + [_sinc32(p, tile_shift=True), _last_frame_missing(good)]
        faulty += [good[:-1], torch.cat([good, good[-1:]])]
        if S > 10:
            faulty.append(_sinc32(p, window_stride=10))
        else:
            p.check(_sinc32(p, window_stride=10))
        for o in faulty:
            _rejected(p.check, o)


# ------------------------------------------------------------------------------------- Whisper stem
def _stem32(p, w1=None, w2=None, neighbour=False, tile_shift=False):
    w1 = p.w1 if w1 is None else w1
    w2 = p.w2 if w2 is None else w2
    if neighbour:  # the chunks back to back in time: a chunk's padding is its neighbour's frames
        B = p.x.shape[0]
        x = p.x.transpose(0, 1).reshape(1, p.M, B * p.Tin)
        y = cp.stem_reference(x, w1, p.b1, w2, p.b2, p.pos.repeat(B, 1))
        return y.reshape(B, p.Tin // 2, p.D)
    out = cp.stem_reference(p.x, w1, p.b1, w2, p.b2, p.pos)
    if tile_shift:  # output row u from conv1 rows 2 u - 3 .. 2 u - 1
        a1 = F.pad(F.gelu(F.conv1d(p.x, w1, p.b1, padding=1)), (2, 0))
        y = F.gelu(F.conv1d(a1, w2, p.b2, stride=2, padding=1)).transpose(1, 2)[:, :p.Tin // 2] + p.pos
        out = _tile_starts_from_row_before(out, y, 64)
    return out


@pytest.mark.parametrize("Tin", cp.STEM_TINS)
@pytest.mark.parametrize("M", [80, 128])
def test_stem_integer_probe(M, Tin):
    p = cp.StemInt(M, Tin)
    print(f"stem n_mels {M} Tin {Tin}: bound {p.bound:.0f}, largest pre-activation {p.pre_max:.0f}")
    assert p.bound < 2 ** 24 and p.pre_max <= p.bound and p.want.shape == (3, Tin // 2, 64)
    good = _stem32(p)
    p.check(good)
    faulty = [_stem32(p, w1=f(p.w1)) for f in WEIGHT_FAULTS + CHANNEL_FAULTS]
    faulty += [_stem32(p, w2=f(p.w2)) for f in WEIGHT_FAULTS + CHANNEL_FAULTS]
    faulty += [_stem32(p, neighbour=True), _stem32(p, tile_shift=True), _last_frame_missing(good)]
    if Tin > 2:
        faulty.append(good[:, :-1])
    for o in faulty:
        _rejected(p.check, o)


def test_stem_bound_at_the_widest_geometry():
    assert cp.stem_worst_case(128, 1280) == 2979856 < 2 ** 24


def test_gelu_is_the_identity_on_integers_from_6():
    v = torch.arange(6, 80001, dtype=torch.float32)
    assert torch.equal(F.gelu(v), v)
    assert torch.equal(0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752)), v)
    big = torch.tensor([2979856.0, 2.0 ** 24 - 1])
    assert torch.equal(F.gelu(big), big)


# ------------------------------------------------------------------------------------ shared checks
def test_checks_reject_nan():
    for p in (cp.PosConvInt(96, 2, True, lengths=[3, 0, 130]), cp.TapsInt(8, 4, 9, True), cp.SincInt(3, 260),
              cp.StemInt(80, 4)):
        good = p.want.float().contiguous()
        p.check(good)
        bad = good.clone()
        bad.view(-1)[-1] = math.nan
        _rejected(p.check, bad)
        _rejected(p.check, torch.full_like(good, math.nan))
    for b in (cp.taps_random(8, 4, 9, True)[-1], cp.LstmLayout(2, 2).bounded, cp.channel_norm_offset(50, 8, True)[-1]):
        _rejected(b.check, torch.full(b.want.shape, math.nan))


def test_check_poison_is_the_attention_probes():
    import attention_probes as ap

    assert cp.check_poison is ap.check_poison


# -------------------------------------------------------------------------- fp64 with a measured bound
def test_bounded_probe_accepts_fp32_torch_and_rejects_a_lost_digit():
    x, w, bias, b = cp.taps_random(60, 60, 132, True)
    assert b.ref_err > 0
    good = cp.taps_reference(x, w, bias)
    assert b.check(good, "fp32 torch") == b.ref_err
    _rejected(b.check, good + 5 * b.ref_err)
    _rejected(b.check, cp.taps_reference(x.bfloat16().float(), w, bias))
    with pytest.raises(AssertionError):  # (ref_err > 0 is part of the probe)
        cp.Bounded("exact", torch.ones(3, dtype=torch.float64), [torch.ones(3)])


@pytest.mark.parametrize("scale", ["init", "unit"])
def test_posconv_random_probe(scale):
    h, w, bias, b = cp.posconv_random(96, 2, True, scale, lengths=[0, 5, 130, 0])
    b.check(cp.posconv_reference(h, w, bias, 2, [0, 5, 130, 0], True), "fp32 torch")
    _rejected(b.check, cp.posconv_reference(h, drop_last_tap(w), bias, 2, [0, 5, 130, 0], True))


@pytest.mark.parametrize("scale", [1, 8])
def test_lstm_probe(scale):
    """The fp32 recurrence with the kernel's sigmoid / tanh formulas is within the bound it helps to
    set; a recurrence that runs direction 1 forwards, or reads the gates in another order, is not."""
    p = cp.LstmBounded(3, 12, scale)
    b = p.bounded
    assert len(b.ref_errs) == 2 and min(b.ref_errs) > 0
    b.check(cp.lstm_recurrence(p.xp, p.whh, cp.sigmoid_rcp, cp.tanh_rcp), "fp32 restatement")
    b.check(cp.lstm_recurrence(p.xp, p.whh), "fp32 recurrence")
    flipped = cp.lstm_recurrence(p.xp.flip(1), p.whh).flip(1)  # both directions reversed in time
    _rejected(b.check, flipped)
    gates = p.xp.view(3, 12, 2, 4, 128)[:, :, :, [0, 2, 1, 3]].reshape(p.xp.shape)
    _rejected(b.check, cp.lstm_recurrence(gates, p.whh))


def test_lstm_layout_probe():
    p = cp.LstmLayout()
    assert p.xp.shape == (17, 3, 2, 512) and not bool(p.whh.any()) and float(p.xp.abs().max()) <= 4
    b = p.bounded
    b.check(cp.lstm_recurrence(p.xp, p.whh), "fp32 recurrence")
    b.check(cp.lstm_recurrence(p.xp, p.whh, cp.sigmoid_rcp, cp.tanh_rcp), "fp32 restatement")
    # the first step of each direction is sigmoid(o) tanh(sigmoid(i) tanh(g)) of its own xp
    xd = p.xp.double()
    for d, t in ((0, 0), (1, 2)):
        i, f, g, o = xd[:, t, d].split(128, dim=1)
        first = torch.sigmoid(o) * torch.tanh(torch.sigmoid(i) * torch.tanh(g))
        assert torch.equal(b.want[:, t, d * 128:(d + 1) * 128], first)
    _rejected(b.check, cp.lstm_recurrence(p.xp.flip(0), p.whh))               # batch
    _rejected(b.check, cp.lstm_recurrence(p.xp.flip(2), p.whh))               # direction
    _rejected(b.check, cp.lstm_recurrence(p.xp, p.whh).roll(1, dims=2))       # unit
    _rejected(b.check, cp.lstm_recurrence(p.xp, p.whh).flip(1))               # time


def test_offset_probes_have_every_mean_class():
    x, gamma, beta, eps, b = cp.channel_norm_offset(1000, 72, True)
    m = x.mean(0)
    assert float((m - cp.channel_means(72)).abs().max()) < 0.2 and float((x.std(0) - 1).abs().max()) < 0.1
    assert sorted(set(cp.channel_means(72).tolist())) == [-200.0, -100.0, 0.0, 100.0, 200.0]
    b.check(cp.group_norm_reference(x, gamma, beta, eps, True), "fp32 torch")
    x, w, bias, gamma, beta, eps, b = cp.conv0_offset(5005, 10, 5, 64, True)
    conv = F.conv1d(x.double()[None, None], w.double()[:, None], bias.double(), stride=5)[0]
    assert float((conv.mean(1) - bias - cp.channel_means(64)).abs().max()) < 1.0
    assert float((w.sum(1) - (cp.mean_classes(64) - 2)).abs().max()) < 1e-5
    x, gamma, beta, eps, b = cp.sincnet_stage_offset(2, 300, 60, False)
    b.check(cp.sincnet_stage_reference(x, False, gamma, beta, eps), "fp32 torch")

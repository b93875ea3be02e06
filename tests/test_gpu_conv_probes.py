"""The convolution, LSTM and normalising kernels under the probes of tests/conv_probes.py (-m gpu):
wx_posconv_packed, wx_conv1d_taps_tm, wx_sinc_filterbank and wx_whisper_stem on integer operands
whose result is exact (bit for bit, no tolerance); the first three and wx_lstm_bidir_layer with NaN
against zeros in all the memory a call must not depend on; the positional conv, the k = 5 conv and
the LSTM against fp64 on the CPU within 4 x ref_err (ref_err: fp32 torch on the CPU for the same
inputs, printed); and wx_channel_norm, wx_conv0_channel_norm and wx_sincnet_stage on channels whose
mean is up to 200 times their spread, and on digital silence, under the same rule.

Every input is built on the CPU from a seeded generator and every comparison is made on the CPU in
fp64: no result computed by torch on the GPU is a reference here."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_probes as cp

pytestmark = pytest.mark.gpu

SENTINEL = 1e4


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _slice_of(fill, shape, lead, tail=64):
    """A contiguous tensor of `shape` that is a slice of a larger buffer full of `fill`, `lead` floats
    into it."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((lead + n + tail,), fill, device="cuda")
    view = buf[lead:lead + n].view(shape)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * lead
    return view


# ------------------------------------------------------------------------------- positional conv
class _SamePad(torch.nn.Module):
    num_pad_remove = 1


class _PosConvStandIn(torch.nn.Module):
    """The positional conv embedding as emission._posconv_weights recognises it, without weight-norm:
    the effective weight is the tensor given."""

    def __init__(self, w, bias, G):
        super().__init__()
        D = w.shape[0]
        self.conv = torch.nn.Conv1d(D, D, 128, padding=64, groups=G)
        with torch.no_grad():
            self.conv.weight.copy_(w)
            self.conv.bias.copy_(bias)
        self.padding = _SamePad()
        self.activation = torch.nn.GELU()


def _posconv_packed_weights(w, bias, G):
    """The weights through emission's own packer, which must agree with the documented layout."""
    from whisperx_amd import emission

    pce = _PosConvStandIn(w, bias, G).cuda().eval()
    pc = emission._posconv_weights(pce)
    assert pc is not None and pc[2] == G and pc[3] == 128
    assert torch.equal(pc[0].cpu(), cp.pack_posconv_weight(w, G)), "emission._posconv_weights: not the layout of wx_align.h"
    assert torch.equal(pc[1].detach().cpu(), bias)
    return pc[0], pc[1].detach()


def _posconv(h_dev, w, bias, G, lengths, residual):
    from whisperx_amd import _lib

    wp, b = _posconv_packed_weights(w, bias, G)
    segs = _lib.PackedSegments(lengths)
    out = _lib.posconv_packed(h_dev, wp, b, G, 128, segs, residual=residual)
    assert out.shape == h_dev.shape
    return out.cpu()


@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("D,G", [(96, 2), (128, 2)])
def test_posconv_integer(D, G, residual):
    p = cp.PosConvInt(D, G, residual)
    n = p.check(_posconv(p.h.cuda(), p.w, p.bias, G, p.lengths, residual))
    print(f"posconv_packed integer D {D} G {G} residual {residual}: {n} outputs exact, largest sum {p.pre_max:.0f}")


@pytest.mark.parametrize("targets", [1, 0])
@pytest.mark.parametrize("D,G", [(96, 2), (128, 2)])
def test_posconv_poison(D, G, targets):
    """Segments of one parity are the targets, the others hold NaN against zeros, and h is a 16-byte
    aligned slice of a buffer that holds the same: every zero a window needs is the kernel's own."""
    h, w, bias, _ = cp.posconv_random(D, G, True, "init")
    lengths = cp.POSCONV_LENGTHS
    off = cp.offsets(lengths)
    keep = torch.zeros(sum(lengths), dtype=torch.bool)
    for s, (a, b) in enumerate(zip(off[:-1], off[1:])):
        keep[a:b] = s % 2 == targets
    assert bool(keep.any()) and not bool(keep.all())

    def run(fill):
        hv = _slice_of(fill, tuple(h.shape), 4 * 67)
        assert hv.data_ptr() % 16 == 0
        hv.copy_(torch.where(keep[:, None], h, torch.full_like(h, fill)))
        return _posconv(hv, w, bias, G, lengths, True)[keep]

    cp.check_poison(run)


@pytest.mark.parametrize("scale", ["init", "unit"])
@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("D,G", [(96, 2), (128, 2)])
def test_posconv_against_fp64(D, G, residual, scale):
    h, w, bias, b = cp.posconv_random(D, G, residual, scale)
    b.check(_posconv(h.cuda(), w, bias, G, cp.POSCONV_LENGTHS, residual), "posconv_packed")


# ------------------------------------------------------------------------------- k = 5 convolution
def _conv_taps(x_tm_dev, w, bias, monkeypatch):
    """vad_model.conv1d_batched on a device batch; fails unless the call reached wx_conv1d_taps_tm once."""
    from whisperx_amd import _lib, vad_model

    calls = []
    kernel = _lib.conv1d_taps_tm

    def spy(*args, **kwargs):
        calls.append(args)
        return kernel(*args, **kwargs)

    with monkeypatch.context() as m:
        m.setattr(_lib, "conv1d_taps_tm", spy)
        m.delenv("WX_NO_CONV_KERNEL", raising=False)
        y = vad_model.conv1d_batched(x_tm_dev.transpose(1, 2), w.cuda(), None if bias is None else bias.cuda(), 1)
    assert len(calls) == 1, f"conv1d_batched made {len(calls)} calls of conv1d_taps_tm"
    return y.transpose(1, 2).cpu()


@pytest.mark.parametrize("L", cp.TAPS_LENGTHS)
@pytest.mark.parametrize("Cin,Cout", cp.TAPS_CHANNELS)
def test_conv_taps_integer(Cin, Cout, L, monkeypatch):
    for with_bias in (True, False):
        p = cp.TapsInt(Cin, Cout, L, with_bias)
        n = p.check(_conv_taps(p.x.cuda(), p.w, p.bias, monkeypatch))
        print(f"{p.label}: {n} outputs exact")


@pytest.mark.parametrize("Cin,Cout,L", [(60, 60, 133), (68, 60, 132), (80, 60, 260), (4, 1, 5)])
def test_conv_taps_poison(Cin, Cout, L, monkeypatch):
    """Window 1 of 3 is the target; windows 0 and 2 and the buffer around the batch hold NaN against zeros."""
    x, w, bias, _ = cp.taps_random(Cin, Cout, L, True)

    def run(fill):
        xv = _slice_of(fill, tuple(x.shape), 4 * 33)
        xv.fill_(fill)
        xv[1].copy_(x[1])
        return _conv_taps(xv, w, bias, monkeypatch)[1]

    cp.check_poison(run)


@pytest.mark.parametrize("L", cp.TAPS_LENGTHS)
@pytest.mark.parametrize("Cin,Cout", cp.TAPS_CHANNELS)
def test_conv_taps_against_fp64(Cin, Cout, L, monkeypatch):
    for with_bias in (True, False):
        x, w, bias, b = cp.taps_random(Cin, Cout, L, with_bias)
        b.check(_conv_taps(x.cuda(), w, bias, monkeypatch), "conv1d_taps_tm")


# --------------------------------------------------------------------------------- sinc filterbank
@pytest.mark.parametrize("S", cp.SINC_STRIDES)
def test_sinc_filterbank_integer(S):
    from whisperx_amd import _lib

    for n in cp.sinc_spans(S):
        p = cp.SincInt(S, n)
        got = _lib.sinc_filterbank(p.x.cuda(), p.w_padded.cuda(), cp.SINC_K, S)
        print(f"sinc_filterbank integer stride {S} n {n}: {p.check(got.cpu())} outputs exact ({p.rows} rows)")


@pytest.mark.parametrize("S", cp.SINC_STRIDES)
def test_sinc_filterbank_poison(S):
    """The span is a slice of a buffer of NaN against zeros, 3 samples (12 bytes) into it."""
    from whisperx_amd import _lib

    n = cp.sinc_spans(S)[2]
    g = torch.Generator().manual_seed(S)
    x = torch.randn(n, generator=g) * 0.1
    w = F.pad(torch.randn(cp.SINC_C, cp.SINC_K, generator=g) * 0.05, (0, 9)).t().contiguous().cuda()

    def run(fill):
        xv = _slice_of(fill, (n,), 3, tail=6000)
        assert xv.data_ptr() % 16 != 0
        xv.copy_(x)
        return _lib.sinc_filterbank(xv, w, cp.SINC_K, S).cpu()

    cp.check_poison(run)


# ------------------------------------------------------------------------------------ Whisper stem
@pytest.mark.parametrize("Tin", cp.STEM_TINS)
@pytest.mark.parametrize("M", [80, 128])
def test_whisper_stem_integer(M, Tin):
    from whisperx_amd import _lib

    p = cp.StemInt(M, Tin)
    B = p.x.shape[0]
    wide = torch.full((B + 1, M + 3, Tin + 37), SENTINEL, device="cuda")
    xv = wide[:B, :M, 5:5 + Tin]  # a strided view, as log_mel's output is read
    xv.copy_(p.x)
    assert not xv.is_contiguous()
    w1p, w2p = _lib.pack_conv3_weight(p.w1.cuda()), _lib.pack_conv3_weight(p.w2.cuda())
    got = _lib.whisper_stem(xv, w1p, p.b1.cuda(), w2p, p.b2.cuda(), p.pos.cuda())
    print(f"whisper_stem integer n_mels {M} Tin {Tin}: {p.check(got.cpu())} outputs exact, largest sum {p.pre_max:.0f}")


# --------------------------------------------------------------------------------------------- LSTM
def _lstm_layer(xp_dev, whh_dev, B, T, y=None):
    from whisperx_amd import _lib

    if y is None:
        return _lib.lstm_bidir_layer(xp_dev, whh_dev, B, T).cpu()
    lib = _lib.load()  # (the wrapper allocates y itself: the sentinel probe hands the C entry point its own)
    assert y.is_contiguous() and tuple(y.shape) == (B, T, 256) and xp_dev.is_contiguous() and whh_dev.is_contiguous()
    with torch.cuda.device(xp_dev.device):
        _lib._check(lib.wx_lstm_bidir_layer(_lib._ptr(xp_dev), _lib._ptr(whh_dev), _lib._ptr(y), B, T, 128,
                                            _lib._stream(xp_dev.device)))
    return y.cpu()


@functools.lru_cache(maxsize=None)
def _lstm_probe(B, T, scale):
    return cp.LstmBounded(B, T, scale)


@pytest.mark.parametrize("scale", [1, 8])
@pytest.mark.parametrize("B,T", cp.LSTM_SHAPES)
def test_lstm_against_fp64(B, T, scale):
    """wx_lstm_bidir_layer on an input projection computed on the CPU, against fp64 torch.nn.LSTM; at
    scale 8 (every parameter times 8) the gates saturate as a trained model's do."""
    p = _lstm_probe(B, T, scale)
    p.bounded.check(_lstm_layer(p.xp.cuda(), p.whh.cuda(), B, T), "lstm_bidir_layer")


def test_lstm_layout():
    p = cp.LstmLayout()
    p.bounded.check(_lstm_layer(p.xp.cuda(), p.whh.cuda(), p.B, p.T), "lstm_bidir_layer")


def test_lstm_poison():
    """B 17: the second workgroup carries one real sequence and fifteen clamped ones.  xp and whh are
    slices of buffers of NaN against zeros; y is a slice of a sentinel-filled buffer whose rows outside
    [0, B) keep the sentinel."""
    B, T = 17, 7
    p = _lstm_probe(B, 40, 1)
    xp = p.xp[:, :T].contiguous()

    def run(fill):
        xv = _slice_of(fill, tuple(xp.shape), 3)
        wv = _slice_of(fill, tuple(p.whh.shape), 4 * 5)
        xv.copy_(xp)
        wv.copy_(p.whh)
        full = torch.full((B + 32, T, 256), SENTINEL, device="cuda")
        got = _lstm_layer(xv, wv, B, T, y=full[16:16 + B])
        assert bool((full[:16] == SENTINEL).all()) and bool((full[16 + B:] == SENTINEL).all())
        return got

    cp.check_poison(run)


# ------------------------------------------------------------------ normalising kernels, means away from 0
@pytest.mark.parametrize("gelu", [True, False])
@pytest.mark.parametrize("C", [64, 72])
def test_channel_norm_offset(C, gelu):
    from whisperx_amd import _lib

    x, gamma, beta, eps, b = cp.channel_norm_offset(1000, C, gelu)
    b.check(_lib.channel_norm(x.cuda(), gamma.cuda(), beta.cuda(), eps, gelu).cpu(), "channel_norm")


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("S,K,stride", [(5005, 10, 5), (2001, 3, 2)])
@pytest.mark.parametrize("C", [64, 72])
def test_conv0_channel_norm_offset(C, S, K, stride, with_bias):
    from whisperx_amd import _lib

    x, w, bias, gamma, beta, eps, b = cp.conv0_offset(S, K, stride, C, with_bias)
    got = _lib.conv0_channel_norm(x.cuda(), w.cuda(), None if bias is None else bias.cuda(), stride, gamma.cuda(),
                                  beta.cuda(), eps, True)
    b.check(got.cpu(), "conv0_channel_norm")


@pytest.mark.parametrize("do_abs", [False, True])
@pytest.mark.parametrize("C", [60, 80])
def test_sincnet_stage_offset(C, do_abs):
    from whisperx_amd import _lib

    x, gamma, beta, eps, b = cp.sincnet_stage_offset(2, 3000, C, do_abs)
    b.check(_lib.sincnet_stage(x.cuda(), do_abs, gamma.cuda(), beta.cuda(), eps).cpu(), "sincnet_stage")


def _silence_check(label, got, want, refs32, constant=None):
    """`constant`: the channels whose input is constant; their outputs are act(beta) within the bound."""
    b = cp.Bounded(label, want, refs32, need_ref_err=constant is not None)
    b.check(got, label.split()[0])
    if constant is not None:
        err = float((got.double() - want)[:, constant].abs().max())
        print(f"{label}: constant channels |kernel - fp64| {err:.3e}")


@pytest.mark.parametrize("C", [64, 72])
def test_channel_norm_silence(C):
    """An all-zero [L, C] (variance exactly 0): finite and act(beta) within 4 x ref_err; and one constant
    channel among random ones."""
    from whisperx_amd import _lib

    g = torch.Generator().manual_seed(C)
    gamma, beta = torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g) * 0.1
    eps = 1e-5
    for mixed in (False, True):
        x = torch.zeros((1000, C))
        if mixed:
            x = torch.randn((1000, C), generator=g)
            x[:, 5] = 0.0
            x[:, 9] = 0.75
        want = cp.group_norm_reference(x.double(), gamma.double(), beta.double(), eps, True)
        const = [5, 9] if mixed else list(range(C))
        assert float((want[:, const] - F.gelu(beta.double())[const]).abs().max()) < 1e-12
        got = _lib.channel_norm(x.cuda(), gamma.cuda(), beta.cuda(), eps, True).cpu()
        _silence_check(f"channel_norm silence C {C} mixed {mixed}", got, want,
                       [cp.group_norm_reference(x, gamma, beta, eps, True)], const if mixed else None)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("S,K,stride", [(5005, 10, 5), (2001, 3, 2)])
def test_conv0_channel_norm_silence(S, K, stride, with_bias):
    """All-zero samples (every conv output is the channel's bias: variance exactly 0), and a waveform of
    noise into filters of which two are all zero."""
    from whisperx_amd import _lib

    C = 72
    g = torch.Generator().manual_seed(S + with_bias)
    w = torch.randn((C, K), generator=g) * 0.3
    bias = torch.randn(C, generator=g) if with_bias else None
    gamma, beta = torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g) * 0.1
    eps = 1e-5
    for mixed in (False, True):
        x = torch.zeros(S)
        if mixed:
            x = torch.randn(S, generator=g) * 0.1
            w = w.clone()
            w[[5, 9]] = 0.0
        bd = None if bias is None else bias.double()
        want = cp.conv0_reference(x.double(), w.double(), bd, stride, gamma.double(), beta.double(), eps, True)
        const = [5, 9] if mixed else list(range(C))
        assert float((want[:, const] - F.gelu(beta.double())[const]).abs().max()) < 1e-12
        got = _lib.conv0_channel_norm(x.cuda(), w.cuda(), None if bias is None else bias.cuda(), stride, gamma.cuda(),
                                      beta.cuda(), eps, True).cpu()
        _silence_check(f"conv0_channel_norm silence K {K} stride {stride} bias {with_bias} mixed {mixed}", got, want,
                       [cp.conv0_reference(x, w, bias, stride, gamma, beta, eps, True)], const if mixed else None)

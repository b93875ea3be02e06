"""Probes for the convolution, LSTM and normalising kernels (plain torch, CPU tensors; the layout
follows tests/attention_probes.py): inputs whose result is known exactly, or whose error has a bound
that the probe measures, so that a kernel that is wrong in one tap, one channel group, one tile edge
or one padded row fails, which random inputs at a hand-picked tolerance only do in probability.

  integer   the operands are small integers held in fp32, chosen so that every partial sum, in any
            order, is an integer below 2^24 (asserted from the operands' absolute sums): an fp32 fma
            chain is then exact whatever its order, and the kernel equals the fp64 convolution bit
            for bit.  Where a GELU follows (positional conv, Whisper stem) inputs and weights are
            non-negative and the bias is 8: every pre-activation is an integer >= 8, where
            0.5 v (1 + erff(v / sqrt 2)) returns v exactly (erff is 1 from about 4 upwards), so the
            output is the integer itself.
  bounded   random inputs against the fp64 evaluation of the same operation within 4 x ref_err,
            ref_err being torch's fp32 evaluation on the CPU against the same fp64 (asserted > 0,
            both printed): the error of the chosen arithmetic in fp32, times the project's margin for
            another summation order.
  poison    attention_probes.check_poison: what a call must not depend on holds zeros in one run and
            NaN in the other; the valid outputs are finite and equal bit for bit.
Every check raises AssertionError (a NaN fails every comparison here)."""
import math

import torch
import torch.nn.functional as F

from attention_probes import check_poison  # noqa: F401  (the isolation probes' check, shared)

EXACT = 2 ** 24
GELU_FLOOR = 8


def _gen(*seed):
    s = 0
    for x in seed:
        s = (s * 1000003 + int(x) + 1) % (2 ** 62)
    return torch.Generator().manual_seed(s)


def _ints(g, lo, hi, shape):
    """Integers lo .. hi (inclusive) as fp32."""
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def check_exact(got, want, label, names):
    """`got` (fp32) equals the integers `want` (fp64) bit for bit; the last axis is the channel, the
    others are named by `names`.  Returns the number of outputs compared."""
    assert tuple(got.shape) == tuple(want.shape), f"{label}: shape {tuple(got.shape)}, want {tuple(want.shape)}"
    assert got.dtype == torch.float32
    ok = got.double() == want  # (a NaN compares unequal)
    if not bool(ok.all()):
        idx = [int(x) for x in (~ok).nonzero()[0]]
        rows = int((~ok).any(-1).sum())
        where = ", ".join(f"{n} {i}" for n, i in zip(list(names) + ["channel"], idx))
        raise AssertionError(f"{label}: {rows} of {ok[..., 0].numel()} rows wrong; first at {where}: got "
                             f"{float(got[tuple(idx)])!r}, want {float(want[tuple(idx)])!r}")
    return ok.numel()


def _assert_gelu_identity(pre):
    """Every pre-activation is an integer >= 8 on which fp32 erf GELU is the identity."""
    assert float(pre.min()) >= GELU_FLOOR and bool((pre == pre.round()).all())
    p32 = pre.float()
    assert torch.equal(F.gelu(p32), p32)


# ---------------------------------------------------------------- positional conv (packed segments)
POSCONV_LENGTHS = [0, 1, 64, 65, 127, 128, 129, 0, 0, 191, 193, 257, 0]
POSCONV_K = 128


def offsets(lengths):
    out = [0]
    for t in lengths:
        out.append(out[-1] + int(t))
    return out


def posconv_reference(h, w, bias, G, lengths, residual, gelu=True):
    """wav2vec2's positional conv embedding on every segment of the packed rows h [rows, D] alone:
    Conv1d(D, D, 128, padding 64, groups G) with the last output dropped, erf GELU, (+ h); in the
    inputs' precision."""
    out = torch.empty_like(h)
    off = offsets(lengths)
    for a, b in zip(off[:-1], off[1:]):
        if b == a:
            continue
        y = F.conv1d(h[a:b].t()[None], w, bias, padding=POSCONV_K // 2, groups=G)[0, :, :-1].t()
        if gelu:
            y = F.gelu(y)
        out[a:b] = y + h[a:b] if residual else y
    return out


def pack_posconv_weight(w, G):
    """include/wx_align.h: w_packed [G][K][Cg / 4][Cg][4], w_packed[g][j][i / 4][o][i % 4] =
    weight[g Cg + o][i][j], written out index by index."""
    D, Cg, K = (int(v) for v in w.shape)
    assert D == G * Cg and Cg % 4 == 0
    wp = torch.empty((G, K, Cg // 4, Cg, 4), dtype=w.dtype)
    for g in range(G):
        for i in range(Cg):
            wp[g, :, i // 4, :, i % 4] = w[g * Cg:(g + 1) * Cg, i, :].t()  # [K, o]
    return wp


class PosConvInt:
    """h in 0..3, weights in 0..3, bias 8: out[t, c] = 8 + the integer convolution (+ h[t, c])."""

    def __init__(self, D, G, residual, lengths=POSCONV_LENGTHS, seed=0):
        g = _gen(11, D, G, seed)
        Cg = D // G
        self.D, self.G, self.residual, self.lengths = D, G, bool(residual), list(lengths)
        self.rows = sum(lengths)
        self.h = _ints(g, 0, 3, (self.rows, D))
        self.w = _ints(g, 0, 3, (D, Cg, POSCONV_K))
        self.bias = torch.full((D,), float(GELU_FLOOR))
        self.bound = float(self.bias.abs().max() + self.w.abs().sum((1, 2)).max() * self.h.abs().max() + self.h.abs().max())
        assert self.bound < EXACT
        pre = posconv_reference(self.h.double(), self.w.double(), self.bias.double(), G, lengths, False, gelu=False)
        _assert_gelu_identity(pre)
        self.pre_max = float(pre.max()) if self.rows else 0.0
        self.want = pre + self.h.double() if self.residual else pre
        off = offsets(lengths)
        self.seg_of_row = torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths))
        self.seg_start = torch.tensor(off[:-1])

    def check(self, out):
        """out [rows, D] fp32, bit for bit."""
        label = f"posconv D {self.D} G {self.G} residual {self.residual}"
        assert tuple(out.shape) == tuple(self.want.shape), f"{label}: shape {tuple(out.shape)}"
        ok = out.double() == self.want
        if not bool(ok.all()):
            r, c = (int(x) for x in (~ok).nonzero()[0])
            s = int(self.seg_of_row[r])
            raise AssertionError(f"{label}: {int((~ok).any(-1).sum())} of {self.rows} rows wrong; first at segment {s} "
                                 f"(length {self.lengths[s]}), frame {r - int(self.seg_start[s])}, channel {c}: got "
                                 f"{float(out[r, c])!r}, want {float(self.want[r, c])!r}")
        return ok.numel()


# -------------------------------------------------------------------------------- k = 5 convolution
TAPS_CHANNELS = [(4, 1), (60, 60), (64, 64), (68, 60), (80, 60)]
TAPS_LENGTHS = [5, 132, 133, 260]
TAPS_B = 3


def taps_reference(x_tm, w, bias):
    """Conv1d(Cin, Cout, 5) (no padding) of time-major windows x_tm [B, L, Cin] -> [B, L - 4, Cout]."""
    return F.conv1d(x_tm.transpose(1, 2), w, bias).transpose(1, 2).contiguous()


class TapsInt:
    """x, w and the bias signed integers in -8..8."""

    def __init__(self, Cin, Cout, L, with_bias, B=TAPS_B, seed=0):
        g = _gen(12, Cin, Cout, L, with_bias, seed)
        self.x = _ints(g, -8, 8, (B, L, Cin))
        self.w = _ints(g, -8, 8, (Cout, Cin, 5))
        self.bias = _ints(g, -8, 8, (Cout,)) if with_bias else None
        self.bound = float((8 if with_bias else 0) + self.w.abs().sum((1, 2)).max() * self.x.abs().max())
        assert self.bound < EXACT
        self.want = taps_reference(self.x.double(), self.w.double(), None if self.bias is None else self.bias.double())
        self.label = f"conv taps Cin {Cin} Cout {Cout} L {L} bias {bool(with_bias)}"

    def check(self, y):
        """y [B, L - 4, Cout] fp32 time-major."""
        return check_exact(y, self.want, self.label, ("window", "frame"))


# --------------------------------------------------------------------------------- sinc filterbank
SINC_STRIDES = [1, 3, 10, 16]
SINC_K, SINC_KP, SINC_C = 251, 260, 80


def sinc_spans(S):
    """Sample counts that give 256, 257 and 262 output rows, the last with samples left over."""
    return [SINC_K + S * 255, SINC_K + S * 256, SINC_K + S * 261 + (S - 1)]


def sinc_reference(x, w, S):
    """The bias-free strided filterbank conv of the span x [n] with w [C, K] -> [rows, C]."""
    return F.conv1d(x[None, None], w[:, None], stride=S)[0].t().contiguous()


class SincInt:
    def __init__(self, S, n, seed=0):
        g = _gen(13, S, n, seed)
        self.S, self.n = S, n
        self.x = _ints(g, -8, 8, (n,))
        self.w = _ints(g, -8, 8, (SINC_C, SINC_K))
        self.w_padded = F.pad(self.w, (0, SINC_KP - SINC_K)).t().contiguous()  # [KP, C]
        self.bound = float(self.w.abs().sum(1).max() * self.x.abs().max())
        assert self.bound < EXACT
        self.want = sinc_reference(self.x.double(), self.w.double(), S)
        self.rows = (n - SINC_K) // S + 1
        assert self.want.shape == (self.rows, SINC_C)

    def check(self, y):
        return check_exact(y, self.want, f"sinc filterbank stride {self.S} n {self.n}", ("frame",))


# ------------------------------------------------------------------------------------ Whisper stem
STEM_TINS = [2, 126, 128, 130, 258]
STEM_B = 3


def stem_reference(x, w1, b1, w2, b2, pos, gelu=True):
    """gelu(conv2(gelu(conv1(x)))) + pos, time-major [B, Tin / 2, D], for x [B, n_mels, Tin]."""
    act = F.gelu if gelu else (lambda v: v)
    a1 = act(F.conv1d(x, w1, b1, padding=1))
    return act(F.conv1d(a1, w2, b2, stride=2, padding=1)).transpose(1, 2) + pos


def stem_worst_case(M, D):
    """The largest partial sum these ranges allow: every x 2, every weight 1, biases and pos 8."""
    return GELU_FLOOR + 3 * D * (GELU_FLOOR + 3 * M * 2) + 8


class StemInt:
    """x in 0..2, both weights in 0..1, both biases 8, positional rows signed integers in -8..8."""

    def __init__(self, M, Tin, D=64, B=STEM_B, seed=0):
        g = _gen(14, M, Tin, D, seed)
        self.M, self.Tin, self.D = M, Tin, D
        self.x = _ints(g, 0, 2, (B, M, Tin))
        self.w1 = _ints(g, 0, 1, (D, M, 3))
        self.w2 = _ints(g, 0, 1, (D, D, 3))
        self.b1 = torch.full((D,), float(GELU_FLOOR))
        self.b2 = torch.full((D,), float(GELU_FLOOR))
        self.pos = _ints(g, -8, 8, (Tin // 2, D))
        a1_max = float(GELU_FLOOR + self.w1.abs().sum((1, 2)).max() * self.x.abs().max())
        self.bound = float(GELU_FLOOR + self.w2.abs().sum((1, 2)).max() * a1_max + self.pos.abs().max())
        assert self.bound <= stem_worst_case(M, D) < EXACT
        xd, w1d, w2d = self.x.double(), self.w1.double(), self.w2.double()
        a1 = F.conv1d(xd, w1d, self.b1.double(), padding=1)
        _assert_gelu_identity(a1)
        pre = F.conv1d(a1, w2d, self.b2.double(), stride=2, padding=1)
        _assert_gelu_identity(pre)
        self.pre_max = float(pre.max())
        self.want = pre.transpose(1, 2) + self.pos.double()

    def check(self, out):
        """out [B, Tin / 2, D] fp32."""
        return check_exact(out, self.want, f"whisper stem n_mels {self.M} Tin {self.Tin}", ("chunk", "frame"))


# ----------------------------------------------------------------------------- fp64 with a measured bound
class Bounded:
    """`want`: the fp64 evaluation; `refs32`: one or more fp32 CPU evaluations of the same inputs,
    ref_err the largest of their errors.  `classes` (optional, int64, broadcastable to want with the
    last axis the channel): the error is printed per class."""

    def __init__(self, label, want, refs32, classes=None, class_names=None, need_ref_err=True):
        assert want.dtype == torch.float64 and bool(torch.isfinite(want).all())
        self.label, self.want = label, want
        self.ref_errs = []
        for r in refs32:
            assert r.dtype == torch.float32 and r.shape == want.shape and bool(torch.isfinite(r).all())
            self.ref_errs.append(float((r.double() - want).abs().max()) if want.numel() else 0.0)
        self.ref_err = max(self.ref_errs)
        if need_ref_err:
            assert self.ref_err > 0, label
        self.classes, self.class_names = classes, class_names

    def error(self, got):
        assert tuple(got.shape) == tuple(self.want.shape) and got.dtype == torch.float32, (self.label, tuple(got.shape))
        if not bool(torch.isfinite(got).all()):
            return float("nan"), (got.double() - self.want).abs()
        e = (got.double() - self.want).abs()
        return (float(e.max()) if e.numel() else 0.0), e

    def check(self, got, who="kernel"):
        """max |got - fp64| <= 4 x ref_err; prints both and returns the error."""
        err, e = self.error(got)
        line = (f"{self.label}: |{who} - fp64| {err:.3e}, ref_err {self.ref_err:.3e} "
                f"({', '.join(f'{x:.2e}' for x in self.ref_errs)}), bound {4 * self.ref_err:.3e}")
        if self.classes is not None and not math.isnan(err):
            cls = self.classes.expand(e.shape)
            line += "; by class " + ", ".join(
                f"{n}: {float(e[cls == c].max()):.2e}" for c, n in enumerate(self.class_names) if bool((cls == c).any()))
        print(line)
        if not err <= 4 * self.ref_err:
            raise AssertionError(line)
        return err


def posconv_random(D, G, residual, scale, lengths=POSCONV_LENGTHS, seed=0):
    """Random normal h; `scale` "init": transformers' initialisation of the positional conv (weights
    N(0, 2 sqrt(1 / (128 D))), bias 0), "unit": weights and bias N(0, 1).  Returns (h, w, bias, Bounded)."""
    g = _gen(21, D, G, residual, scale == "unit", seed)
    rows = sum(lengths)
    h = torch.randn((rows, D), generator=g)
    w = torch.randn((D, D // G, POSCONV_K), generator=g)
    if scale == "init":
        w = w * (2.0 * math.sqrt(1.0 / (POSCONV_K * D)))
        bias = torch.zeros(D)
    else:
        bias = torch.randn(D, generator=g)
    want = posconv_reference(h.double(), w.double(), bias.double(), G, lengths, residual)
    ref32 = posconv_reference(h, w, bias, G, lengths, residual)
    return h, w, bias, Bounded(f"posconv D {D} G {G} residual {bool(residual)} {scale} scale", want, [ref32])


def taps_random(Cin, Cout, L, with_bias, B=TAPS_B, seed=0):
    """Random normal x, weights N(0, 0.1), bias N(0, 1) (the existing test's scales)."""
    g = _gen(22, Cin, Cout, L, with_bias, seed)
    x = torch.randn((B, L, Cin), generator=g)
    w = torch.randn((Cout, Cin, 5), generator=g) * 0.1
    bias = torch.randn(Cout, generator=g) if with_bias else None
    want = taps_reference(x.double(), w.double(), None if bias is None else bias.double())
    return x, w, bias, Bounded(f"conv taps Cin {Cin} Cout {Cout} L {L} bias {bool(with_bias)}", want,
                               [taps_reference(x, w, bias)])


# --------------------------------------------------------------------------------------------- LSTM
LSTM_IN, LSTM_H = 60, 128
LSTM_SHAPES = [(17, 40), (1, 1), (3, 293)]


def sigmoid_rcp(x):
    """The kernel's sigmoid: 1 / (1 + exp(-x))."""
    return 1.0 / (1.0 + torch.exp(-x))


def tanh_rcp(x):
    """The kernel's tanh: 2 sigmoid(2 x) - 1."""
    return 2.0 * sigmoid_rcp(2.0 * x) - 1.0


def lstm_recurrence(xp, whh, sigmoid=torch.sigmoid, tanh=torch.tanh):
    """One bidirectional LSTM layer from its input projections, in the inputs' precision: xp
    [B, T, 2, 4H] (gate order i, f, g, o), whh [2, 4H, H] -> y [B, T, 2H]; h0 = c0 = 0, direction 1
    runs from the last step to the first."""
    B, T = xp.shape[:2]
    H = whh.shape[-1]
    y = torch.empty((B, T, 2 * H), dtype=xp.dtype)
    for d in range(2):
        h = torch.zeros((B, H), dtype=xp.dtype)
        c = torch.zeros((B, H), dtype=xp.dtype)
        wt = whh[d].t().contiguous()
        for s in range(T):
            t = T - 1 - s if d else s
            gates = xp[:, t, d] + h @ wt
            i, f, g, o = gates.split(H, dim=1)
            c = sigmoid(f) * c + sigmoid(i) * tanh(g)
            h = sigmoid(o) * tanh(c)
            y[:, t, d * H:(d + 1) * H] = h
    return y


def lstm_input_projection(lstm, x):
    """xp [B, T, 2, 4H] of layer 0 in x's precision: x W_ih^T + b_ih + b_hh per direction."""
    ws = [getattr(lstm, "weight_ih_l0" + s) for s in ("", "_reverse")]
    bs = [getattr(lstm, "bias_ih_l0" + s) + getattr(lstm, "bias_hh_l0" + s) for s in ("", "_reverse")]
    return torch.stack([x @ w.t() + b for w, b in zip(ws, bs)], dim=2).contiguous()


class LstmBounded:
    """One bidirectional layer (60 -> 128) at torch's default initialisation times `scale`, against
    fp64 torch.nn.LSTM.  xp is computed on the CPU in fp32.  ref_err: the larger of stock fp32
    torch.nn.LSTM's error and that of the fp32 recurrence with the kernel's sigmoid / tanh formulas."""

    def __init__(self, B, T, scale, seed=0):
        g = _gen(23, B, T, scale, seed)
        lstm = torch.nn.LSTM(LSTM_IN, LSTM_H, num_layers=1, bidirectional=True, batch_first=True).eval()
        with torch.no_grad():
            for p in lstm.parameters():
                k = 1.0 / math.sqrt(LSTM_H)
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * k * scale)
            x = torch.randn((B, T, LSTM_IN), generator=g)
            self.xp = lstm_input_projection(lstm, x)
            self.whh = torch.stack([lstm.weight_hh_l0, lstm.weight_hh_l0_reverse]).contiguous()
            stock32 = lstm(x)[0]
            restated32 = lstm_recurrence(self.xp, self.whh, sigmoid_rcp, tanh_rcp)
            want = lstm.double()(x.double())[0]
        self.B, self.T = B, T
        self.bounded = Bounded(f"lstm B {B} T {T} scale {scale}", want, [stock32, restated32])


class LstmLayout:
    """whh = 0, xp uniform in +-4: every output is an elementwise function of xp[b, :, d] — at the
    first step of a direction y = sigmoid(o) tanh(sigmoid(i) tanh(g)), later steps add the cell carried
    through the forget gate (c = sigmoid(f) c + sigmoid(i) tanh(g); with whh = 0 still elementwise) —
    which pins batch, time (reversed for direction 1), direction, gate and unit indexing."""

    def __init__(self, B=17, T=3, seed=0):
        g = _gen(24, B, T, seed)
        self.B, self.T = B, T
        self.xp = (torch.rand((B, T, 2, 4 * LSTM_H), generator=g) * 8 - 4)
        self.whh = torch.zeros((2, 4 * LSTM_H, LSTM_H))
        want = self._elementwise(self.xp.double(), torch.sigmoid, torch.tanh)
        refs = [self._elementwise(self.xp, torch.sigmoid, torch.tanh), self._elementwise(self.xp, sigmoid_rcp, tanh_rcp)]
        self.bounded = Bounded(f"lstm layout B {B} T {T}", want, refs)

    @staticmethod
    def _elementwise(xp, sigmoid, tanh):
        B, T = xp.shape[:2]
        H = LSTM_H
        y = torch.empty((B, T, 2 * H), dtype=xp.dtype)
        for d in range(2):
            c = torch.zeros((B, H), dtype=xp.dtype)
            for s in range(T):
                t = T - 1 - s if d else s
                i, f, g, o = xp[:, t, d].split(H, dim=1)
                c = sigmoid(f) * c + sigmoid(i) * tanh(g)
                y[:, t, d * H:(d + 1) * H] = sigmoid(o) * tanh(c)
        return y


# ------------------------------------------------------------------ normalising kernels, means away from 0
MEAN_CLASS_NAMES = ("-200", "-100", "0", "+100", "+200")  # class c % 5: mean 100 (c % 5 - 2)


def mean_classes(C):
    return torch.arange(C) % 5


def channel_means(C):
    return 100.0 * (mean_classes(C) - 2).float()


def _affine(g, C):
    return torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g) * 0.1


def group_norm_reference(x_tm, gamma, beta, eps, gelu):
    """GroupNorm with one group per channel over time-major x [L, C] (+ erf GELU), in x's precision."""
    C = x_tm.shape[1]
    y = F.group_norm(x_tm.t()[None], C, gamma, beta, eps)[0].t()
    return (F.gelu(y) if gelu else y).contiguous()


def channel_norm_offset(L, C, gelu, seed=0):
    """x [L, C]: spread 1 around a mean of 100 (c % 5 - 2).  Returns (x, gamma, beta, eps, Bounded)."""
    g = _gen(31, L, C, gelu, seed)
    x = torch.randn((L, C), generator=g) + channel_means(C)
    gamma, beta = _affine(g, C)
    eps = 1e-5
    want = group_norm_reference(x.double(), gamma.double(), beta.double(), eps, gelu)
    ref32 = group_norm_reference(x, gamma, beta, eps, gelu)
    return x, gamma, beta, eps, Bounded(f"channel_norm offset L {L} C {C} gelu {gelu}", want, [ref32],
                                        mean_classes(C), MEAN_CLASS_NAMES)


def conv0_reference(x, w, bias, stride, gamma, beta, eps, gelu):
    """Conv1d(1, C, K, stride) -> GroupNorm(C, C) -> erf GELU, time-major [Lout, C]."""
    C = w.shape[0]
    y = F.group_norm(F.conv1d(x[None, None], w[:, None], bias, stride=stride), C, gamma, beta, eps)
    return (F.gelu(y) if gelu else y)[0].t().contiguous()


def conv0_offset(S, K, stride, C, with_bias, seed=0):
    """A waveform of spread 1 around a DC offset of 100, filters whose taps sum to about c % 5 - 2
    (one class of them to about 1): the conv output's channel means are 0, +-100 and +-200 side by side.
    Returns (x, w, bias, gamma, beta, eps, Bounded)."""
    g = _gen(32, S, K, stride, C, with_bias, seed)
    x = torch.randn(S, generator=g) + 100.0
    w = torch.randn((C, K), generator=g) * 0.3
    w = w - w.mean(1, keepdim=True) + ((mean_classes(C) - 2).float() / K)[:, None]
    bias = torch.randn(C, generator=g) if with_bias else None
    gamma, beta = _affine(g, C)
    eps = 1e-5
    want = conv0_reference(x.double(), w.double(), None if bias is None else bias.double(), stride, gamma.double(),
                           beta.double(), eps, True)
    ref32 = conv0_reference(x, w, bias, stride, gamma, beta, eps, True)
    return x, w, bias, gamma, beta, eps, Bounded(f"conv0_channel_norm offset S {S} K {K} stride {stride} C {C} bias "
                                                 f"{bool(with_bias)}", want, [ref32], mean_classes(C), MEAN_CLASS_NAMES)


def sincnet_stage_reference(x_tm, do_abs, gamma, beta, eps, slope=0.01):
    """leaky_relu(InstanceNorm1d(MaxPool1d(3, 3)(|x|?))) of time-major windows x [B, L, C] -> [B, L // 3, C]."""
    xc = x_tm.transpose(1, 2)
    p = F.max_pool1d(xc.abs() if do_abs else xc, 3, 3)
    y = F.instance_norm(p, weight=gamma, bias=beta, eps=eps)
    return F.leaky_relu(y, slope).transpose(1, 2).contiguous()


def sincnet_stage_offset(B, L, C, do_abs, seed=0):
    g = _gen(33, B, L, C, do_abs, seed)
    x = torch.randn((B, L, C), generator=g) + channel_means(C)
    gamma, beta = _affine(g, C)
    eps = 1e-5
    want = sincnet_stage_reference(x.double(), do_abs, gamma.double(), beta.double(), eps)
    ref32 = sincnet_stage_reference(x, do_abs, gamma, beta, eps)
    return x, gamma, beta, eps, Bounded(f"sincnet_stage offset B {B} L {L} C {C} abs {bool(do_abs)}", want, [ref32],
                                        mean_classes(C), MEAN_CLASS_NAMES)

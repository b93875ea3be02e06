"""Probes for `layer_norm(a + b)` over rows of D floats (wx_add_layernorm, wx_add_layernorm_h16 and
wx_add_layernorm_h16_dual): inputs on which every intermediate value of a two-pass fp32 LayerNorm is
exact, so that the expected bits come from plain fp32 arithmetic on the CPU and a kernel that reads
gamma or beta at another column, leaves eps out, misses a column of the mean or lets another row's
data in fails at zero tolerance.  CPU tensors only; the tests move them to the device.

With v = a + b, d = v - mean and y = d * rstd * gamma + beta (products first, in this order):
  balanced  row r holds s_j c_r, c_r a power of two from 2^-3 to 2^6 and s_j = +-1 with D / 2 entries
            of each sign in an order of the row's own.  Every partial sum is an integer multiple of
            c_r below 2^24 c_r: the mean is 0, sum d^2 / D = c_r^2, and with eps = 0 rstd = 1 / c_r, so
            d * rstd = s_j and y = fl(s_j gamma_j + beta_j): one rounding.
  eps       the same with c = 1 and eps = 3: rstd = 1 / sqrt(4) = 0.5, y = fl(s_j gamma_j / 2 + beta_j).
            Without eps rstd is 1.
  offset    v = c0 + s_j with c0 = 1024 or 4096: the partial sums are integers below 2^24 (1280 x 4097),
            the mean is c0, d = s_j, the variance 1, and (eps = 0) y = fl(s_j gamma_j + beta_j).  A mean
            that misses a column is no longer c0, and E[v^2] - mean^2 in fp32 is not 1: 4097^2 is no
            fp32 number.
Each probe comes in the splits of v between a and b that the entry points allow: (v, 0), (0, v) and,
for offset, (c0, s) and (s, c0).  Where b is exact in fp16 and bf16 (powers of two up to 4096, +-1, 0:
every split but offset's (0, v)) the same tensors serve the 16-bit entries (`splits16`), and (v, no b)
is run there too.  gamma is 1 + 0.1 randn and
beta 0.1 randn, different in every column.

The bounded check: a = 50 + 2 randn (a mean 25 standard deviations from 0, where a one-pass variance
loses 3 digits), b = randn; against fp64 within 4 x ref_err, ref_err = max |torch fp32 layer_norm - fp64|.

On an MI355X (test_gpu_layernorm_probes.py): every exact probe holds bit for bit in all three entry
points; the bounded check's |y - fp64| is 2.4e-6 .. 5.1e-6 against ref_err 2.6e-6 .. 4.4e-6, at most
0.33 (fp32 entry, D 512), 0.27 (fp16 b, D 768) and 0.34 (bf16 b, D 768) of the 4 x ref_err allowed.
"""
import functools

import torch
import torch.nn.functional as F

WIDTHS = (256, 384, 512, 768, 1024, 1280)
ROWS = (1, 5, 67)
KINDS = ("balanced", "eps", "offset1024", "offset4096")
FAULTS = ("gamma_shifted_in_float4", "eps_dropped", "mean_over_d_minus_4", "d384_lanes_96_127", "one_pass_variance")


def _gen(*seed):
    s = 0
    for x in seed:
        s = (s * 1000003 + int(x) + 1) % (2 ** 62)
    return torch.Generator().manual_seed(s)


def _signs(rows: int, D: int, g):
    """[rows, D] of +-1, D / 2 of each per row, in an order of the row's own."""
    half = torch.cat([torch.ones(D // 2), -torch.ones(D // 2)])
    return torch.stack([half[torch.randperm(D, generator=g)] for _ in range(rows)])


class Exact:
    """One probe: `splits` [(label, a, b)] in fp32 (`splits16`: those with b exact in fp16 and bf16),
    gamma, beta, eps, and the expected fp32 `y` and `sum`, bit for bit."""

    def __init__(self, kind: str, D: int, rows: int):
        assert kind in KINDS and D in WIDTHS
        g = _gen(31, KINDS.index(kind), D, rows)
        s = _signs(rows, D, g)
        self.gamma = 1 + 0.1 * torch.randn(D, generator=g)
        self.beta = 0.1 * torch.randn(D, generator=g)
        zero = torch.zeros((rows, D))
        if kind in ("balanced", "eps"):
            c = torch.ones(rows) if kind == "eps" else 2.0 ** ((torch.arange(rows) * 7 + D // 128) % 10 - 3).float()
            assert kind == "eps" or rows < 5 or len(set(c.tolist())) >= 5
            v = s * c[:, None]
            self.eps = 3.0 if kind == "eps" else 0.0
            rstd = 0.5 / c if kind == "eps" else 1.0 / c
            self.splits = [("a = v, b = 0", v, zero), ("a = 0, b = v", zero, v)]
            self.mean = torch.zeros(rows)
        else:
            c0 = float(kind[len("offset"):])
            base = torch.full((rows, D), c0)
            v = base + s
            assert D * (c0 + 1) < 2 ** 24
            self.eps = 0.0
            rstd = torch.ones(rows)
            self.splits = [("a = c0, b = s", base, s), ("a = s, b = c0", s, base), ("a = v, b = 0", v, zero),
                           ("a = 0, b = v", zero, v)]
            self.mean = torch.full((rows,), c0)
        for _, a, b in self.splits:
            assert torch.equal(a + b, v)
        # the splits whose b both 16-bit types hold exactly: all but offset's (0, v) (1025 is no bf16 number)
        self.splits16 = [x for x in self.splits if torch.equal(x[2].half().float(), x[2]) and
                         torch.equal(x[2].bfloat16().float(), x[2])]
        assert len(self.splits16) == len(self.splits) - kind.startswith("offset")
        # plain fp32 arithmetic, one operation at a time, in the kernel's order
        d = v - self.mean[:, None]
        assert torch.equal(d, s * (v[:, :1] - self.mean[:, None]).abs())
        self.y = d * rstd[:, None] * self.gamma + self.beta
        self.sum = v
        self.kind, self.D, self.rows = kind, D, rows

    def check(self, y32=None, y16=None, s=None, label=""):
        """the outputs a call produced (CPU tensors) are the expected bits; y16: the rounding of y"""
        for name, got, want in (("y32", y32, self.y), ("y16", y16, None if y16 is None else self.y.to(y16.dtype)),
                                ("sum", s, self.sum)):
            if got is None:
                continue
            assert got.shape == want.shape and got.dtype == want.dtype, (name, label)
            bits = torch.int32 if got.element_size() == 4 else torch.int16
            bad = got.contiguous().view(bits) != want.contiguous().view(bits)
            if bool(bad.any()):
                r, j = (int(x) for x in bad.nonzero()[0])
                raise AssertionError(f"{self.kind} D {self.D} rows {self.rows} ({label}): {name} differs in "
                                     f"{int(bad.sum())} of {bad.numel()} elements; first [{r}, {j}] = "
                                     f"{float(got[r, j])!r}, want {float(want[r, j])!r}")


@functools.lru_cache(maxsize=None)
def exact(kind: str, D: int, rows: int) -> Exact:
    return Exact(kind, D, rows)


def strided(t, fill):
    """t [rows, D] as a view of a [rows + 1, D + 8] buffer that holds `fill` everywhere else: padding
    between the rows and a whole row behind the last (16-byte aligned rows in fp32 and in 16 bit)."""
    rows, D = t.shape
    wide = torch.full((rows + 1, D + 8), fill, dtype=t.dtype, device=t.device)
    view = wide[:rows, :D]
    view.copy_(t)
    return view


@functools.lru_cache(maxsize=None)
def bounded(D: int, rows: int, dtype=None):
    """(a, b, gamma, beta, eps, fp64 reference, ref_err): b rounded to `dtype` (None: fp32)."""
    g = _gen(32, D, rows)
    a = 50.0 + 2.0 * torch.randn((rows, D), generator=g)
    b = torch.randn((rows, D), generator=g)
    if dtype is not None:
        b = b.to(dtype).float()
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    eps = 1e-5
    want = F.layer_norm(a.double() + b.double(), (D,), gamma.double(), beta.double(), eps)
    ref_err = float((F.layer_norm(a + b, (D,), gamma, beta, eps).double() - want).abs().max())
    assert ref_err > 0
    return a, b, gamma, beta, eps, want, ref_err


# ------------------------------------------------------------------- a restatement, and faulty ones
def layernorm_f32(a, b, gamma, beta, eps: float, fault=None):
    """A two-pass fp32 LayerNorm of a + b (rows x D, CPU), one fp32 operation at a time: (y, a + b).
    `fault`: one of FAULTS, the mistake the kernel could make."""
    assert fault is None or fault in FAULTS
    rows, D = a.shape
    v = a + b
    total, n = v.sum(-1), D
    if fault == "mean_over_d_minus_4":
        total = v[:, :D - 4].sum(-1)
    leak = None
    if fault == "d384_lanes_96_127" and D == 384:  # float4 96 .. 127 of the row's address: the next row's first 128 floats
        leak = torch.roll(v, -1, 0)[:, :128]
        total = total + leak.sum(-1)
    mean = total / float(n)
    if fault == "one_pass_variance":
        var = (v * v).sum(-1) / float(D) - mean * mean
    else:
        d = v - mean[:, None]
        q = (d * d).sum(-1)
        if leak is not None:
            dl = leak - mean[:, None]
            q = q + (dl * dl).sum(-1)
        var = q / float(D)
    if fault != "eps_dropped":
        var = var + torch.tensor(eps, dtype=torch.float32)
    rstd = 1.0 / torch.sqrt(var)
    if fault == "gamma_shifted_in_float4":
        j = torch.arange(D)
        gamma = gamma[(j & ~3) | ((j + 1) & 3)]
    return (v - mean[:, None]) * rstd[:, None] * gamma + beta, v

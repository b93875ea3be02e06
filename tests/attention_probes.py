"""Probes for an attention `attend(q, k, v) -> o` with q [N, Tq, 64], k / v [N, L, 64] and o
[N, Tq, 64] (plain torch, CPU tensors, softmax scale 0.125): inputs whose result is known in closed
form or whose error has a stated bound, so that a kernel that is wrong in one key, one tile or one
range of scores fails, which random inputs at a max-abs tolerance only do in probability.

  permutation  query i is 15 x key pi(i) with |k|^2 = 64: the target's score is 120 (e^120 overflows
               fp32), every other score is lower by `margin` >= 40, so the target's weight is 1 and
               o[i] = v[pi(i)].  Every key is the target of exactly one query: a dropped key, or a
               weight that meets another key's value row, fails at that query.
  uniform      q = 0, v in the integers -8..-1, 1..8: every weight is 1 / L, every partial sum an
               integer below 2^24 (exact in fp32 in any order), o = sum(v) / L.  One key too few or
               too many moves an output by at least 1 / L.
  range        random q / k / v with head dim 63 reserved: q[i, 63] in (150, -150, 30, -30, 0) and
               k[j, 63] = 8 (offset) or 8 (1 + j / L) (ramp) shift every query's scores by up to
               +-150, or let them rise / fall towards the last key by up to +-300.  Against an fp64
               softmax within 4 x ref_err, ref_err being the same formula in fp32 torch.
  poison       what a call must not depend on holds zeros in one run and NaN in the other: the valid
               outputs are finite and equal bit for bit.
Every check returns its figures and raises AssertionError (a NaN fails every comparison here)."""
import math

import torch

SCALE = 0.125
D = 64
Q_CLASSES = (150.0, -150.0, 30.0, -30.0, 0.0)
MIN_MARGIN = 40.0
KINDS = ("random", "identity", "reversal")


def reference(q, k, v):
    """softmax(SCALE q k^T) v in the inputs' precision."""
    return torch.softmax(SCALE * (q @ k.transpose(-1, -2)), -1) @ v


def reference_deferred(q, k, v):
    """The same attention normalised at the end, as every kernel here does: (e^(s - max) v) / sum.
    (The uniform probe's bound is for this form; softmax's weights, each rounded to fl(1 / L), and
    their rounded products with v are further from sum(v) / L than its 2^-22.)"""
    s = SCALE * (q @ k.transpose(-1, -2))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return (p @ v) / p.sum(-1, keepdim=True)


def _gen(*seed):
    s = 0
    for x in seed:
        s = (s * 1000003 + int(x) + 1) % (2 ** 62)
    return torch.Generator().manual_seed(s)


# ------------------------------------------------------------------------------ permutation
class Permutation:
    def __init__(self, N: int, L: int, kind: str, seed: int = 0):
        g = _gen(1, N, L, KINDS.index(kind), seed)
        k = torch.randn((N, L, D), generator=g, dtype=torch.float64)
        self.k = (k * (8.0 / k.norm(dim=-1, keepdim=True))).float()
        if kind == "random":
            self.pi = torch.stack([torch.randperm(L, generator=g) for _ in range(N)])
        elif kind == "identity":
            self.pi = torch.arange(L).repeat(N, 1)
        else:
            self.pi = torch.arange(L - 1, -1, -1).repeat(N, 1)
        idx = self.pi[:, :, None].expand(N, L, D)
        self.q = 15.0 * self.k.gather(1, idx)  # (x 15: exact up to one rounding of the fp32 key)
        self.v = torch.randn((N, L, D), generator=g)
        self.want = self.v.gather(1, idx)
        self.N, self.L, self.kind = N, L, kind
        # the distance of every query's target score from its next one, in fp64, head by head
        self.margin = math.inf
        for n in range(N):
            s = SCALE * (self.q[n].double() @ self.k[n].double().t())
            target = s.gather(1, self.pi[n][:, None])[:, 0]
            assert float((target - 120.0).abs().max()) < 1e-3
            if L > 1:
                rest = s.scatter(1, self.pi[n][:, None], -math.inf).max(1).values
                self.margin = min(self.margin, float((target - rest).min()))
        assert self.margin >= MIN_MARGIN, (self.margin, N, L, kind)
        assert L * math.exp(-MIN_MARGIN) < 1e-14

    def check(self, o):
        """|o - v[pi]| <= 2^-24 |v[pi]| + 1e-12 elementwise; returns the largest |o - v[pi]|."""
        assert o.shape == self.want.shape and o.dtype == torch.float32
        err = (o.double() - self.want.double()).abs()
        tol = 2.0 ** -24 * self.want.double().abs() + 1e-12
        ok = err <= tol
        if not bool(ok.all()):
            n, i, d = (int(x) for x in (~ok).nonzero()[0])
            raise AssertionError(f"permutation ({self.kind}, L {self.L}): {int((~ok).any(-1).sum())} bad rows; first "
                                 f"o[{n}, {i}, {d}] = {float(o[n, i, d])!r}, want v[{int(self.pi[n, i])}] = "
                                 f"{float(self.want[n, i, d])!r}")
        return float(err.max())


# ---------------------------------------------------------------------------------- uniform
class Uniform:
    def __init__(self, N: int, Tq: int, L: int, seed: int = 0, values=None):
        """`values`: integer v [N, L, 64] in place of the drawn ones (the probe's own test)."""
        g = _gen(2, N, Tq, L, seed)
        mag = torch.randint(1, 9, (N, L, D), generator=g)
        sign = torch.randint(0, 2, (N, L, D), generator=g) * 2 - 1
        vi = mag * sign
        assert int(vi.abs().min()) >= 1 and int(vi.abs().max()) <= 8
        if values is not None:
            vi = values.long()
        assert int(vi.abs().sum(1).max()) < 2 ** 24  # (every partial sum in any order is exact in fp32)
        self.q = torch.zeros((N, Tq, D))
        self.k = 2.0 * torch.randn((N, L, D), generator=g)
        self.v = vi.float()
        self.sum = vi.sum(1)  # int64 [N, D]
        self.want = (self.sum.double() / L)[:, None, :].expand(N, Tq, D)
        self.N, self.Tq, self.L = N, Tq, L

    def check(self, o):
        """relative error <= 2^-22 (one rounding of sum / L, or two of sum x (1 / l)); exactly 0
        where the sum is 0.  Returns the largest relative error."""
        assert o.shape == self.want.shape and o.dtype == torch.float32
        od = o.double()
        zero = (self.want == 0)
        err = (od - self.want).abs()
        ok = torch.where(zero, od == 0, err <= 2.0 ** -22 * self.want.abs())
        if not bool(ok.all()):
            n, i, d = (int(x) for x in (~ok).nonzero()[0])
            raise AssertionError(f"uniform (L {self.L}): {int((~ok).any(-1).sum())} bad rows; first o[{n}, {i}, {d}] = "
                                 f"{float(o[n, i, d])!r}, want {int(self.sum[n, d])} / {self.L} = "
                                 f"{float(self.want[n, i, d])!r}")
        rel = err / self.want.abs().clamp_min(1e-300)
        return float(rel[~zero].max()) if bool((~zero).any()) else 0.0


# ------------------------------------------------------------------------------------ range
class Range:
    """`scales`: the factors on the random q, k and v (the self-attention tests': 2, 2, 2; the decode
    tests': 1, 3, 1).  Query (n, i) has class (n + i) mod 5, so five consecutive queries, and five
    consecutive rows of a decode batch, hold every class."""

    def __init__(self, N: int, Tq: int, L: int, variant: str, scales=(2.0, 2.0, 2.0), seed: int = 0):
        assert variant in ("offset", "ramp")
        g = _gen(3, N, Tq, L, variant == "ramp", seed)
        self.q = scales[0] * torch.randn((N, Tq, D), generator=g)
        self.k = scales[1] * torch.randn((N, L, D), generator=g)
        self.v = scales[2] * torch.randn((N, L, D), generator=g)
        self.cls = (torch.arange(N)[:, None] + torch.arange(Tq)[None, :]) % 5  # [N, Tq]
        self.q[:, :, D - 1] = torch.tensor(Q_CLASSES)[self.cls]
        j = torch.arange(L, dtype=torch.float64)
        self.k[:, :, D - 1] = (8.0 * (1.0 + j / L) if variant == "ramp" else torch.full_like(j, 8.0)).float()
        self.want = reference(self.q.double(), self.k.double(), self.v.double())
        ref32 = reference(self.q, self.k, self.v)
        assert bool(torch.isfinite(ref32).all()) and bool(torch.isfinite(self.want).all())
        self.ref_err = float((ref32.double() - self.want).abs().max())
        # (one key: the softmax is exactly 1 in every precision, o = v, and the bound is equality)
        assert self.ref_err > 0 or L == 1
        self.N, self.Tq, self.L, self.variant = N, Tq, L, variant

    def errors(self, o):
        """max |o - fp64| of every query class, in Q_CLASSES' order (NaN where o is not finite)."""
        assert o.shape == self.want.shape and o.dtype == torch.float32
        e = (o.double() - self.want).abs().amax(-1)
        out = []
        for c in range(5):
            x = e[self.cls == c]
            out.append(float("nan") if not bool(torch.isfinite(x).all()) else float(x.max()) if x.numel() else 0.0)
        return out

    def check(self, o, label=""):
        """max |o - fp64| <= 4 x ref_err; prints and returns the error."""
        by_class = self.errors(o)
        err = float("nan") if any(math.isnan(x) for x in by_class) else max(by_class)
        print(f"range {self.variant} {label} L {self.L}: |o - fp64| {err:.3e}, ref_err {self.ref_err:.3e}, bound "
              f"{4 * self.ref_err:.3e}; by class " +
              ", ".join(f"{int(c):+d}: {x:.2e}" for c, x in zip(Q_CLASSES, by_class)))
        if not err <= 4 * self.ref_err:
            raise AssertionError(f"range ({self.variant}, L {self.L}): |o - fp64| {err:.3e} > 4 x ref_err "
                                 f"{4 * self.ref_err:.3e}; by class {by_class}")
        return err


# ----------------------------------------------------------------------------------- poison
POISON_FILLS = (0.0, float("nan"))


def random_inputs(N: int, Tq: int, L: int, scales=(2.0, 2.0, 2.0), seed: int = 0):
    """Random normal q [N, Tq, 64] and k, v [N, L, 64] at the existing tests' scales."""
    g = _gen(4, N, Tq, L, seed)
    return (scales[0] * torch.randn((N, Tq, D), generator=g), scales[1] * torch.randn((N, L, D), generator=g),
            scales[2] * torch.randn((N, L, D), generator=g))


def check_poison(run):
    """`run(fill)` returns the valid output rows of a call in which everything the call must not
    depend on holds `fill`: with zeros and with NaN they are finite and equal as bit patterns."""
    clean, dirty = (run(f) for f in POISON_FILLS)
    assert clean.shape == dirty.shape and clean.dtype == dirty.dtype == torch.float32
    if not bool(torch.isfinite(clean).all()):
        raise AssertionError("poison: the run over zeros is not finite")
    if not bool(torch.isfinite(dirty).all()):
        bad = ~torch.isfinite(dirty).reshape(-1, dirty.shape[-1]).all(-1)
        raise AssertionError(f"poison: {int(bad.sum())} of {bad.numel()} valid output rows are not finite when the "
                             f"memory around the inputs holds NaN (first row {int(bad.nonzero()[0])})")
    if not torch.equal(clean.contiguous().view(torch.int32), dirty.contiguous().view(torch.int32)):
        raise AssertionError(f"poison: {int((clean != dirty).sum())} valid outputs depend on memory outside the inputs")

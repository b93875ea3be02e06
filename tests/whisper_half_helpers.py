"""Shared by the tests of WhisperEncoder's half route (float16 / bfloat16): the oracles of
wx_attention_h16 and of the whole encoder, and attention probes whose inputs are exactly
representable in the 16-bit type.  Everything here is computed once on the CPU and shared; the tests
leave it unchanged.

Attention.  Inputs: q randn, k 3 x randn, v randn, rounded to dtype (a peaked softmax at scale
0.125).  The reference is fp64 softmax(q k^T / 8) v on the rounded inputs, and
    ref_err = max |torch CPU scaled_dot_product_attention in dtype - fp64|
(9.9e-4 .. 1.1e-3 in fp16 and 7.7e-3 .. 8.5e-3 in bf16 at T 33 .. 1500; 0 at T = 1, where the
softmax is exactly 1).  The project's rule: the code under test is within 4 x ref_err of fp64.

Encoder.  ref_err_half = max |transformers' WhisperEncoder cast to dtype, on the CPU - its fp64
output| on whisper_helpers.case's weights and features: what simply casting the stock model costs.
The half route rounds a strict subset of what that model rounds (not the stream, the norms or the
stem), and must be within 2 x ref_err_half of fp64 (a CPU emulation of the route sits at 0.53 .. 0.70 x;
the factor leaves room for the GEMM library's summation orders and for rounding flips, and still
rejects a route that is worse than casting the stock model)."""
import copy
import functools
import math

import torch
import torch.nn.functional as F

from whisper_helpers import case

SCALE = 0.125
DTYPES = (torch.float16, torch.bfloat16)
# the relative error bound of one rounding to nearest: 2^-(p) for p bits of precision (11 / 8)
HALF_ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
MIN_MARGIN = 40.0


def name(dtype) -> str:
    return str(dtype).replace("torch.", "")


def _gen(*seed):
    s = 0
    for x in seed:
        s = (s * 1000003 + int(x) + 1) % (2 ** 62)
    return torch.Generator().manual_seed(s)


def attention_ref64(q, k, v):
    """softmax(SCALE q k^T) v in fp64 for [B, H, T, 64] inputs -> [B, T, H, 64] (the kernel's layout)."""
    q, k, v = (t.double() for t in (q, k, v))
    return (torch.softmax(SCALE * (q @ k.transpose(-1, -2)), -1) @ v).transpose(1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def attention_case(dtype, B: int, H: int, T: int):
    """(q, k, v [B, H, T, 64] in dtype, fp64 reference [B, T, H, 64], ref_err)."""
    g = _gen(11, DTYPES.index(dtype), B, H, T)
    q = torch.randn((B, H, T, 64), generator=g).to(dtype)
    k = (3.0 * torch.randn((B, H, T, 64), generator=g)).to(dtype)
    v = torch.randn((B, H, T, 64), generator=g).to(dtype)
    want = attention_ref64(q, k, v)
    ref = F.scaled_dot_product_attention(q, k, v, scale=SCALE).transpose(1, 2)
    assert ref.dtype == dtype
    ref_err = float((ref.double() - want).abs().max())
    assert ref_err > 0 or T == 1
    return q, k, v, want, ref_err


def fused_views(q, k, v, rows_behind: int = 0, pad: int = 0, fill: float = 0.0):
    """q / k / v [B, H, T, 64] copied into one [B, T + rows_behind, 3 * 64 H + pad] buffer of their
    dtype (the q/k/v GEMM's output layout; everything that is not q, k or v holds `fill`) and the
    three [B, H, T, 64] views of it: strides {(T + rows_behind) W, 64, W}, W = 3 * 64 H + pad."""
    B, H, T, _ = q.shape
    D = 64 * H
    buf = torch.full((B, T + rows_behind, 3 * D + pad), fill, dtype=q.dtype, device=q.device)
    views = []
    for j, t in enumerate((q, k, v)):
        view = buf[:, :T, j * D:(j + 1) * D].view(B, T, H, 64).transpose(1, 2)
        view.copy_(t)
        views.append(view)
    return buf, views


# ------------------------------------------------------------------------------ permutation
class Permutation:
    """tests/attention_probes.py's permutation probe with inputs that dtype holds exactly: the keys
    are rounded to dtype first, query i is 16 x key pi(i) (a power of two: exact), |k|^2 ~ 64, so the
    target's score is ~128 and every other score is lower by at least MIN_MARGIN (checked in fp64 on
    the rounded inputs).  The target's probability is exactly 1; another key's is at most e^-40,
    which fp16 rounds to 0 and which, in bf16, is below 2^-24 of any value it is added to.  So
    o[i] = v[pi(i)] exactly, and a V operand read at other keys than the probabilities' fails."""

    def __init__(self, dtype, N: int, L: int, kind: str):
        kinds = ("random", "identity", "reversal")
        g = _gen(12, DTYPES.index(dtype), N, L, kinds.index(kind))
        k = torch.randn((N, L, 64), generator=g, dtype=torch.float64)
        self.k = (k * (8.0 / k.norm(dim=-1, keepdim=True))).float().to(dtype)
        if kind == "random":
            self.pi = torch.stack([torch.randperm(L, generator=g) for _ in range(N)])
        elif kind == "identity":
            self.pi = torch.arange(L).repeat(N, 1)
        else:
            self.pi = torch.arange(L - 1, -1, -1).repeat(N, 1)
        idx = self.pi[:, :, None].expand(N, L, 64)
        q = 16.0 * self.k.float().gather(1, idx)
        self.q = q.to(dtype)
        assert torch.equal(self.q.float(), q)  # exactly representable
        v = torch.randn((N, L, 64), generator=g)
        self.v = torch.where(v < 0, -1.0, 1.0).mul(v.abs().clamp_min(2.0 ** -10)).to(dtype)  # |v| >= 2^-10
        self.want = self.v.gather(1, idx)
        assert float(self.want.float().abs().min()) >= 2.0 ** -10  # (L e^-40 max|v| is far below 2^-24 of it)
        self.margin = math.inf
        for n in range(N):
            s = SCALE * (self.q[n].double() @ self.k[n].double().t())
            target = s.gather(1, self.pi[n][:, None])[:, 0]
            if L > 1:
                rest = s.scatter(1, self.pi[n][:, None], -math.inf).max(1).values
                self.margin = min(self.margin, float((target - rest).min()))
        assert self.margin >= MIN_MARGIN, (self.margin, N, L, kind)


# ---------------------------------------------------------------------------------- uniform
class Uniform:
    """q = 0 and v in the integers -2 .. 2 (exact in both types): every probability is exactly 1,
    every partial sum an integer (exact in fp32 in any order), o = round(sum(v) / L).  The sums
    stay below 2^8 in magnitude (asserted), so with L a power of two the mean has at most 8
    significant bits and is exactly representable in both types."""

    def __init__(self, dtype, N: int, L: int):
        g = _gen(13, DTYPES.index(dtype), N, L)
        vi = torch.randint(-2, 3, (N, L, 64), generator=g)
        self.q = torch.zeros((N, L, 64), dtype=dtype)
        self.k = (2.0 * torch.randn((N, L, 64), generator=g)).to(dtype)
        self.v = vi.to(dtype)
        self.sum = vi.sum(1)  # [N, 64]
        assert int(self.sum.abs().max()) < 2 ** 8
        self.want = (self.sum.double() / L)[:, None, :].expand(N, L, 64)
        self.exact = L & (L - 1) == 0
        if self.exact:
            assert torch.equal(self.want.to(dtype).double(), self.want)


# ---------------------------------------------------------------------------------- encoder
@functools.lru_cache(maxsize=None)
def encoder_case(dtype, D: int, layers: int, P: int, B: int):
    """(encoder, features, HF fp64 output, ref_err_half) of one geometry (whisper_helpers.case's
    weights and features)."""
    enc, x, y64, _ = case(D, layers, P, B)
    with torch.no_grad():
        y16 = copy.deepcopy(enc).to(dtype)(x.to(dtype)).last_hidden_state
    assert y16.dtype == dtype
    ref_err_half = float((y16.double() - y64).abs().max())
    assert ref_err_half > 0
    return enc, x, y64, ref_err_half

"""Probes for the f16 / bf16 MFMA attention (wx_attention_h16 and wx_attention_h16_packed): an
elementwise error bound derived from the kernel's contract, a CPU emulation of that contract with
switches for the mistakes the kernel could make, and the inputs (random, flat, score range,
fp16 subnormals) the bound is applied to.  CPU tensors only, [N, T, 64] in the 16-bit type;
computed once and shared, the tests leave them unchanged.

The bound.  On the rounded inputs, in fp64: p_j = exp(s_j - max s), o = sum p_j v_j / sum p_j.  The
kernel multiplies V with p~_j = p_j (1 + d_j) + e_j, |d_j| <= u (one rounding of p to the type:
u = 2^-11 in fp16, 2^-8 in bf16), |e_j| <= e (half the fp16 subnormal spacing, 2^-25; 0 in bf16,
whose exponent range is fp32's), and normalises by the sum of the same p~.  Since
sum p_j (v_j - o) = 0,
    o~ - o = sum (p_j d_j + e_j) (v_j - o) / sum p~_j,
so, per output element,
    bound_P = (u sum_j p_j |v_j - o| + e sum_j |v_j - o|) / ((1 - u) sum_j p_j - L e)
    bound   = u |o| + e + bound_P + 4 ref_err32
(the rounding of the output to the type, normal or subnormal; the weights; the fp32 arithmetic, by
the project's rule: ref_err32 = max |fp32 torch softmax attention on the same inputs - fp64|, one
number per case).  Nothing in it is fitted to the kernel.

The emulation (`emulate`) restates the contract in torch on the CPU: fp32 scores taken through
scale x log2(e) and exp2, 32-key tiles of which wave w of 4 takes w, w + 4, ..., P rounded to the
type with the running sum over the rounded P, fp32 accumulation, the merge of the four waves'
(max, sum, O) in the kernel's order, the output rounded to the type.  It is not bit-equal to the
kernel (the MFMA's and torch's summation orders differ); it shows that the contract meets the
bound, and, through `fault=`, which mistakes each probe rejects (test_attention_h16_probes.py).
On the CPU it sits at err / bound <= 0.96 (fp16 and bf16, T 1 .. 300, every input kind below); on
test_gpu_attention_h16.py's random inputs the bound's largest element is about 2 x below that
test's 4 x ref_err(dtype), and it is far below it on small elements.

On an MI355X (test_gpu_attention_h16_probes.py; the largest err / bound over all cases of a probe,
err against the fp64 reference; the figure is near 1 by nature, u |o| being the rounding of the
output itself):
                                   fp16            bf16
    random, T 1 .. 257             0.948 (T 2)     0.949 (T 2)
    flat, T 1 .. 257               0.820 (T 2)     0.833 (T 2)
    range offset, T 33 .. 257      0.877 (T 33)    0.929 (T 161)
    range ramp, T 33 .. 257        0.921 (T 97)    0.948 (T 161)
    range ramp, T 1500             0.726           0.899
    subnormal v, T 33 / 97 / 161   0.927 (T 97)
    subnormal k, T 33 / 97 / 161   0.383 (T 33)
    packed range segments          0.921           0.948  (the dense launch's bits)
The 4 x ref_err32 term is 3e-5 .. 1e-4 of a bound of 2e-3 (fp16) or 2e-2 (bf16) on the range probes:
no term for the size of the scores was needed.
"""
import functools
import math

import torch

import attention_probes as ap
import whisper_half_helpers as hh

SCALE = hh.SCALE
U = hh.HALF_ULP
E = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}
# the kernel's scale_log2 = scale * 1.4426950408889634f (a power of two times the fp32 constant: exact)
SCALE_LOG2 = SCALE * float(torch.tensor(1.4426950408889634, dtype=torch.float32))
RANGE_SCALES = (1.0, 3.0, 1.0)  # the half attention tests' q, 3 x k, v
FP16_MIN_NORMAL = 2.0 ** -14

FAULTS = ("drop_last_key", "drop_key_4_of_32", "swap_weights_4_7_with_8_11", "stale_v_tile", "merge_without_wave_3",
          "no_rescale", "max_from_0", "flush_subnormal_v", "flush_subnormal_k")


def _gen(*seed):
    s = 0
    for x in seed:
        s = (s * 1000003 + int(x) + 1) % (2 ** 62)
    return torch.Generator().manual_seed(s)


# ------------------------------------------------------------------------------------ bound
class Case:
    """q / k / v [N, T, 64] in one 16-bit type, the fp64 attention `want` on them and the elementwise
    `bound` of the module docstring with its terms."""

    def __init__(self, label: str, q, k, v, chunk_elems: int = 1 << 22):
        dtype = q.dtype
        assert dtype in hh.DTYPES and k.dtype == dtype and v.dtype == dtype
        u, e = U[dtype], E[dtype]
        N, T, _ = q.shape
        L = k.shape[1]
        qd, kd, vd = q.double(), k.double(), v.double()
        self.want = torch.empty((N, T, 64), dtype=torch.float64)
        self.bound_p = torch.empty((N, T, 64), dtype=torch.float64)
        step = max(1, chunk_elems // (N * L * 64))  # (no [T, L, 64] tensor at once)
        for i in range(0, T, step):
            s = SCALE * (qd[:, i:i + step] @ kd.transpose(-1, -2))
            p = torch.exp(s - s.amax(-1, keepdim=True))
            psum = p.sum(-1, keepdim=True)
            o = (p @ vd) / psum
            dev = (vd[:, None] - o[:, :, None]).abs()  # [N, step, L, 64]
            self.want[:, i:i + step] = o
            self.bound_p[:, i:i + step] = (u * torch.einsum("ncl,ncld->ncd", p, dev) + e * dev.sum(2)) / \
                ((1 - u) * psum - L * e)
        ref32 = ap.reference(q.float(), k.float(), v.float())
        assert bool(torch.isfinite(ref32).all()) and bool(torch.isfinite(self.want).all())
        self.ref_err32 = float((ref32.double() - self.want).abs().max())
        assert self.ref_err32 > 0 or L == 1
        self.bound_round = u * self.want.abs() + e
        self.bound = self.bound_round + self.bound_p + 4 * self.ref_err32
        self.q, self.k, self.v, self.label, self.dtype = q, k, v, label, dtype

    def ratio(self, o) -> float:
        """the largest |o - fp64| / bound (NaN where o is not finite)"""
        assert o.shape == self.want.shape and o.dtype == self.dtype
        od = o.double()
        if not bool(torch.isfinite(od).all()):
            return math.nan
        err = (od - self.want).abs()
        # (one key: bound and error are both 0 where v = 0)
        return float(torch.where(err == 0, torch.zeros_like(err), err / self.bound.clamp_min(1e-300)).max())

    def check(self, o, who: str = "") -> float:
        """|o - fp64| <= bound elementwise; prints and returns the largest err / bound."""
        r = self.ratio(o)
        print(f"{who} {self.label}: largest err / bound {r:.3f} (ref_err32 {self.ref_err32:.2e}, largest bound "
              f"{float(self.bound.max()):.2e})")
        if not r <= 1.0:
            msg = "the output is not finite"
            if not math.isnan(r):
                err = (o.double() - self.want).abs()
                rel = err / self.bound.clamp_min(1e-300)
                n, i, d = (int(x) for x in (rel == rel.max()).nonzero()[0])
                msg = (f"o[{n}, {i}, {d}] = {float(o[n, i, d])!r}, fp64 {float(self.want[n, i, d])!r}: err "
                       f"{float(err[n, i, d]):.3e} > bound {float(self.bound[n, i, d]):.3e} = output rounding "
                       f"{float(self.bound_round[n, i, d]):.3e} + P rounding {float(self.bound_p[n, i, d]):.3e} + "
                       f"4 x ref_err32 {4 * self.ref_err32:.3e}")
            raise AssertionError(f"{who} {self.label}: err / bound {r:.3f}; {msg}")
        return r


@functools.lru_cache(maxsize=None)
def random_case(dtype, N: int, T: int, kind: str) -> Case:
    """kind "random": q randn, k 3 x randn, v randn (a peaked softmax); "flat": q 0.25 x randn."""
    g = _gen(21, hh.DTYPES.index(dtype), N, T, ("random", "flat").index(kind))
    q = ((1.0 if kind == "random" else 0.25) * torch.randn((N, T, 64), generator=g)).to(dtype)
    k = (3.0 * torch.randn((N, T, 64), generator=g)).to(dtype)
    v = torch.randn((N, T, 64), generator=g).to(dtype)
    return Case(f"{kind} {hh.name(dtype)} N {N} T {T}", q, k, v)


@functools.lru_cache(maxsize=None)
def range_case(dtype, N: int, T: int, variant: str) -> Case:
    """attention_probes.Range's q / k / v rounded to dtype (the class values +-150, +-30 and 0 and
    the offset's 8 are exact in both types); reference and bound are taken on the rounded inputs."""
    r = ap.Range(N, T, T, variant, RANGE_SCALES, seed=T)
    q, k, v = r.q.to(dtype), r.k.to(dtype), r.v.to(dtype)
    assert torch.equal(q[:, :, 63].float(), torch.tensor(ap.Q_CLASSES)[r.cls])
    if variant == "offset":
        assert bool((k[:, :, 63] == 8).all())
    elif T > 1:
        assert float(k[0, -1, 63]) > float(k[0, 0, 63])
    c = Case(f"range {variant} {hh.name(dtype)} N {N} T {T}", q, k, v)
    c.cls = r.cls
    return c


def share_subnormal(t) -> float:
    return float(((t.float().abs() < FP16_MIN_NORMAL) & (t != 0)).float().mean())


@functools.lru_cache(maxsize=None)
def subnormal_case(N: int, T: int, which: str) -> Case:
    """fp16.  "v": the random case's v x 2^-14, most values subnormal (|x| < 1: 68 % of a normal),
    and so are the outputs.  "k": k = 3 randn x 2^-14 (|3 x| < 1: 26 % subnormal) against
    q = randn x 2^10 and a normal v: the scores are the random case's / 16, spread about 0.19, so
    that keys flushed to zero would move the weights by some 20 %."""
    dtype = torch.float16
    g = _gen(22, N, T, ("v", "k").index(which))
    q = torch.randn((N, T, 64), generator=g)
    k = 3.0 * torch.randn((N, T, 64), generator=g)
    v = torch.randn((N, T, 64), generator=g)
    if which == "v":
        v = v * 2.0 ** -14
    else:
        q, k = q * 2.0 ** 10, k * 2.0 ** -14
    c = Case(f"subnormal {which} float16 N {N} T {T}", q.to(dtype), k.to(dtype), v.to(dtype))
    c.share = share_subnormal(c.v if which == "v" else c.k)
    return c


# -------------------------------------------------------------------------------- emulation
def emulate(q, k, v, fault=None):
    """The kernel's contract on [N, T, 64] / [N, L, 64] CPU tensors of one 16-bit type (module
    docstring); `fault`: one of FAULTS, the contract with that mistake."""
    assert fault is None or fault in FAULTS
    dtype = q.dtype
    assert dtype in hh.DTYPES
    qf, kf, vf = q.float(), k.float(), v.float()
    if fault == "flush_subnormal_v":
        vf = torch.where(vf.abs() < FP16_MIN_NORMAL, torch.zeros_like(vf), vf)
    if fault == "flush_subnormal_k":
        kf = torch.where(kf.abs() < FP16_MIN_NORMAL, torch.zeros_like(kf), kf)
    if fault == "drop_last_key":
        kf, vf = kf[:, :-1], vf[:, :-1]
    N, T, _ = qf.shape
    L = kf.shape[1]
    s = (qf @ kf.transpose(-1, -2)) * SCALE_LOG2  # fp32, log2 domain
    if fault == "drop_key_4_of_32":
        s = s.masked_fill(torch.arange(L) % 32 == 4, -math.inf)
    states = []
    for w in range(4):
        m = torch.full((N, T, 1), 0.0 if fault == "max_from_0" else -math.inf)
        l = torch.zeros((N, T, 1))
        o = torch.zeros((N, T, 64))
        first_v = None
        for k0 in range(32 * w, L, 128):
            st = s[:, :, k0:k0 + 32]
            n = st.shape[-1]
            mn = torch.maximum(m, st.amax(-1, keepdim=True))
            alpha = torch.exp2(m - mn)
            p = torch.exp2(st - mn).to(dtype).float()  # rounded to the type: the MFMA's operand
            l = l * alpha + p.sum(-1, keepdim=True)    # ... and what the row is normalised by
            vt = vf[:, k0:k0 + 32]
            if first_v is None:
                first_v = vt
            elif fault == "stale_v_tile":
                vt = first_v[:, :n]
            if fault == "swap_weights_4_7_with_8_11":
                j = torch.arange(n)
                src = torch.where((j >= 4) & (j < 8) & (j + 4 < n), j + 4, j)
                src = torch.where((j >= 8) & (j < 12), j - 4, src)
                p = p[..., src]
            if fault != "no_rescale":
                o = o * alpha
            o = o + p @ vt
            m = mn
        states.append((m, l, o))
    if fault == "merge_without_wave_3":
        states = states[:3]
    mt = states[0][0]
    for m, _, _ in states[1:]:
        mt = torch.maximum(mt, m)
    m, l, o = states[0]
    c = torch.exp2(m - mt)
    l, o = l * c, o * c
    for m, lx, ox in states[1:]:
        c = torch.exp2(m - mt)  # (a wave without keys: 0)
        l = l + lx * c
        o = o + ox * c
    return (o * (1.0 / l)).to(dtype)

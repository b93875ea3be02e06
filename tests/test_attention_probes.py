"""The attention probes' own conditions (tests/attention_probes.py), without a GPU: the fp32 torch
attention passes every probe (the uniform probe in the form that normalises at the end, see
attention_probes.reference_deferred), and each faulty restatement of attention below, the kind of mistake
the HIP kernels could make, is rejected by the probe named for it."""
import math

import pytest
import torch

import attention_probes as ap

LENGTHS = [1, 2, 31, 33, 129, 257, 1500]


def _attention(q, k, v, keep=None, weights=None):
    """fp32 attention normalised at the end; `keep`: a key mask; `weights`: a map of the [N, Tq, L]
    unnormalised weights on their way to v."""
    s = ap.SCALE * (q @ k.transpose(-1, -2))
    if keep is not None:
        s = s.masked_fill(~keep, -math.inf)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return ((p if weights is None else weights(p)) @ v) / p.sum(-1, keepdim=True)


# ----------------------------------------------------------- the faulty restatements
def drop_last_key(q, k, v):
    return ap.reference_deferred(q, k[:, :-1], v[:, :-1])


def drop_key_4_of_32(q, k, v):
    return _attention(q, k, v, keep=torch.arange(k.shape[1]) % 32 != 4)


def last_key_twice(q, k, v):
    return ap.reference_deferred(q, torch.cat([k, k[:, -1:]], 1), torch.cat([v, v[:, -1:]], 1))


def swap_weights_4_7_with_8_11(q, k, v):
    """the weights of keys 4..7 of every 32-key tile meet value rows 8..11 and back (where both exist)"""
    L = k.shape[1]
    j = torch.arange(L)
    src = torch.where((j % 32 >= 4) & (j % 32 < 8) & (j + 4 < L), j + 4, j)
    src = torch.where((j % 32 >= 8) & (j % 32 < 12), j - 4, src)
    return _attention(q, k, v, weights=lambda w: w[..., src])


def exp_without_max(q, k, v):
    w = torch.exp(ap.SCALE * (q @ k.transpose(-1, -2)))
    return (w @ v) / w.sum(-1, keepdim=True)


def max_floored_at_0(q, k, v):
    """online softmax over 32-key tiles whose running maximum starts at 0 instead of -inf"""
    N, Tq = q.shape[:2]
    m = torch.zeros((N, Tq, 1))
    l = torch.zeros((N, Tq, 1))
    o = torch.zeros((N, Tq, ap.D))
    for k0 in range(0, k.shape[1], 32):
        s = ap.SCALE * (q @ k[:, k0:k0 + 32].transpose(-1, -2))
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        p = torch.exp(s - mn)
        alpha = torch.exp(m - mn)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p @ v[:, k0:k0 + 32]
        m = mn
    return o / l


def padded_weights(q, k, v_padded):
    """the weights padded with zeros to a multiple of 32 keys, times value rows that include the
    padding: `v_padded` [N, 32 ceil(L / 32), 64]"""
    w = torch.softmax(ap.SCALE * (q @ k.transpose(-1, -2)), -1)
    w = torch.nn.functional.pad(w, (0, v_padded.shape[1] - w.shape[-1]))
    return w @ v_padded


def _rejected(check, o):
    with pytest.raises(AssertionError):
        check(o)


# ------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("kind", ap.KINDS)
def test_permutation_probe(L, kind):
    p = ap.Permutation(2, L, kind, seed=L)
    print(f"permutation {kind} L {L}: margin {p.margin:.1f}")
    assert p.margin >= 40
    assert all(sorted(p.pi[n].tolist()) == list(range(L)) for n in range(p.N))
    o = ap.reference(p.q, p.k, p.v)
    assert p.check(o) <= 1e-12
    assert torch.equal(o, p.want)  # (bit for bit)
    p.check(ap.reference_deferred(p.q, p.k, p.v))
    faults = [exp_without_max]
    if L >= 2:
        faults.append(drop_last_key)
    if L >= 5:
        faults.append(drop_key_4_of_32)
    if L >= 9:
        faults.append(swap_weights_4_7_with_8_11)
    for f in faults:
        _rejected(p.check, f(p.q, p.k, p.v))


@pytest.mark.parametrize("L", LENGTHS)
def test_uniform_probe(L):
    p = ap.Uniform(2, 3, L, seed=L)
    assert int(p.v.abs().sum(1).max()) < 2 ** 24 and float(p.v.abs().min()) >= 1
    assert p.check(ap.reference_deferred(p.q, p.k, p.v)) <= 2.0 ** -22
    faults = []
    if L >= 2:  # (with one key, counting it twice is the same attention)
        faults += [last_key_twice, drop_last_key]
    if L >= 5:
        faults.append(drop_key_4_of_32)
    for f in faults:
        _rejected(p.check, f(p.q, p.k, p.v))
    # an exact zero sum must come out as exactly zero
    vi = p.v.long()
    vi[0, :, 0] = 0
    if L > 1:
        vi[0, 0, 0], vi[0, -1, 0] = 3, -3
    z = ap.Uniform(2, 3, L, seed=L, values=vi)
    assert int(z.sum[0, 0]) == 0
    o = ap.reference_deferred(z.q, z.k, z.v)
    z.check(o)
    o[0, 1, 0] = 1e-30
    _rejected(z.check, o)


@pytest.mark.parametrize("variant", ["offset", "ramp"])
@pytest.mark.parametrize("L,Tq,scales", [(33, 33, (2, 2, 2)), (129, 129, (2, 2, 2)), (1500, 1500, (2, 2, 2)),
                                          (65, 1, (1, 3, 1)), (1500, 1, (1, 3, 1))])
def test_range_probe(L, Tq, scales, variant):
    N = 4 if Tq > 1 else 10
    p = ap.Range(N, Tq, L, variant, scales, seed=L)
    assert p.ref_err > 0 and bool(torch.isfinite(ap.reference(p.q, p.k, p.v)).all())
    assert sorted(set(p.cls.flatten().tolist())) == [0, 1, 2, 3, 4]
    s = ap.SCALE * (p.q.double() @ p.k.double().transpose(-1, -2))
    print(f"scores in [{float(s.min()):.0f}, {float(s.max()):.0f}]")
    assert float(s.max()) > 100 and float(s.min()) < -100  # (exp overflows above 88.7, flushes below -103.3)
    err = p.check(ap.reference(p.q, p.k, p.v), "fp32 torch")
    assert err == p.ref_err
    p.check(ap.reference_deferred(p.q, p.k, p.v), "fp32 torch, normalised last")
    _rejected(p.check, exp_without_max(p.q, p.k, p.v))
    _rejected(p.check, max_floored_at_0(p.q, p.k, p.v))


@pytest.mark.parametrize("L", [1, 33, 97, 1500])
def test_poison_probe(L):
    q, k, v = ap.random_inputs(2, L, L, seed=L)
    pad = -L % 32

    def padded(fill):
        return torch.cat([v, torch.full((2, pad, ap.D), fill)], 1)

    ap.check_poison(lambda fill: ap.reference(q, k, padded(fill)[:, :L]))
    _rejected(ap.check_poison, lambda fill: padded_weights(q, k, padded(fill)))
    # outputs that differ without a NaN are rejected too
    _rejected(ap.check_poison, lambda fill: ap.reference(q, k, v) + (0.0 if fill == 0 else 1e-6))


def test_checks_reject_nan():
    p = ap.Permutation(1, 33, "random")
    _rejected(p.check, torch.full_like(p.want, math.nan))
    u = ap.Uniform(1, 2, 33)
    _rejected(u.check, torch.full((1, 2, ap.D), math.nan))
    r = ap.Range(5, 1, 33, "offset")
    _rejected(r.check, torch.full((5, 1, ap.D), math.nan))

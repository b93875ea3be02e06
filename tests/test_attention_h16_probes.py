"""The half attention probes' own conditions (tests/attention_h16_probes.py), without a GPU: the CPU
emulation of wx_attention_h16's contract stays within the derived bound on every input kind, returns
whisper_half_helpers' exact probes bit for bit, and each faulty variant of it, the kind of mistake the
MFMA kernel could make, is rejected by the probe named for it at the smallest T at which the fault
can act (and is the clean emulation, bit for bit, one key below that T)."""
import pytest
import torch

import attention_h16_probes as hp
import whisper_half_helpers as hh

DTYPES = [pytest.param(d, id=hh.name(d)) for d in hh.DTYPES]
N = 2
# one wave; two; three; the first T at which all four have a tile; the first restaged V tile of wave 0
# and of wave 1; every wave with more than two tiles
LENGTHS = (1, 33, 65, 97, 129, 161, 300)


def _case(dtype, T, kind):
    return hp.random_case(dtype, N, T, kind) if kind in ("random", "flat") else hp.range_case(dtype, N, T, kind)


def _rejected(case, o):
    with pytest.raises(AssertionError):
        case.check(o, "faulty")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("kind", ["random", "flat", "offset", "ramp"])
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_emulation_is_within_the_bound(dtype, T, kind):
    c = _case(dtype, T, kind)
    o = hp.emulate(c.q, c.k, c.v)
    assert c.check(o, "emulation") <= 1.0
    if T == 1:  # one key: the softmax is exactly 1
        assert _same(o, c.v)
    elif kind == "random":  # test_gpu_attention_h16.py's inputs: the bound is tighter than its 4 x ref_err(dtype)
        ref = torch.nn.functional.scaled_dot_product_attention(c.q[:, None], c.k[:, None], c.v[:, None], scale=hp.SCALE)[:, 0]
        ref_err = float((ref.double() - c.want).abs().max())
        print(f"largest bound {float(c.bound.max()):.2e}, 4 x ref_err({hh.name(dtype)}) {4 * ref_err:.2e}")
        assert float(c.bound.max()) < 4 * ref_err


@pytest.mark.parametrize("T", [1, 2, 33, 129, 300])
@pytest.mark.parametrize("which", ["v", "k"])
def test_subnormal_cases(which, T):
    c = hp.subnormal_case(4, T, which)
    print(f"subnormal {which} T {T}: share {c.share:.2f}")
    assert c.share > (0.6 if which == "v" else 0.2)
    o = hp.emulate(c.q, c.k, c.v)
    assert c.check(o, "emulation") <= 1.0 and bool((o != 0).any())
    if which == "v":
        assert hp.share_subnormal(o) > 0.6
        _rejected(c, hp.emulate(c.q, c.k, c.v, fault="flush_subnormal_v"))  # (acts from T = 1)
    elif T == 1:
        assert _same(hp.emulate(c.q, c.k, c.v, fault="flush_subnormal_k"), o)  # (one key: its weight is 1)
    else:
        s = hp.SCALE * (c.q.double() @ c.k.double().transpose(-1, -2))
        assert 0.1 < float(s.std()) < 0.3
        _rejected(c, hp.emulate(c.q, c.k, c.v, fault="flush_subnormal_k"))


# (the fault, the smallest T at which it acts)
PERMUTATION_FAULTS = (("drop_last_key", 2), ("drop_key_4_of_32", 5), ("swap_weights_4_7_with_8_11", 9),
                      ("merge_without_wave_3", 97), ("stale_v_tile", 129))


@pytest.mark.parametrize("kind", ["identity", "reversal", "random"])
@pytest.mark.parametrize("T", [1, 2, 4, 5, 8, 9, 33, 65, 96, 97, 128, 129, 160, 161, 257])
@pytest.mark.parametrize("dtype", DTYPES)
def test_permutation_probe(dtype, T, kind):
    p = hh.Permutation(dtype, N, T, kind)
    o = hp.emulate(p.q, p.k, p.v)
    assert _same(o, p.want)
    for fault, first in PERMUTATION_FAULTS:
        if T == 1 and fault == "drop_last_key":
            continue  # (no key left)
        bad = hp.emulate(p.q, p.k, p.v, fault=fault)
        if T >= first:
            assert not _same(bad, p.want), fault
        else:
            assert _same(bad, o), fault
    # scaled values stay exact (the GPU test's variant)
    big = (p.v.float().clamp(-3.5, 3.5) * (2.0 ** 14 if dtype == torch.float16 else 2.0 ** 100)).to(dtype)
    assert bool(torch.isfinite(big).all())
    assert _same(hp.emulate(p.q, p.k, big), big.gather(1, p.pi[:, :, None].expand(N, T, 64)))


@pytest.mark.parametrize("L", [32, 64, 128, 256, 1024])
@pytest.mark.parametrize("dtype", DTYPES)
def test_uniform_probe(dtype, L):
    u = hh.Uniform(dtype, N, L)
    assert u.exact
    want = u.want.to(dtype)
    assert _same(hp.emulate(u.q, u.k, u.v), want)
    faults = ["drop_last_key", "drop_key_4_of_32"] + (["merge_without_wave_3"] if L >= 97 else [])
    for fault in faults:
        assert not _same(hp.emulate(u.q, u.k, u.v, fault=fault), want), fault
    if dtype == torch.float16:  # subnormal values and means
        tiny = (u.v.double() * 2.0 ** -22).to(dtype)
        assert torch.equal(tiny.double(), u.v.double() * 2.0 ** -22) and hp.share_subnormal(tiny) > 0.7
        want = (u.want * 2.0 ** -22).to(dtype)
        assert bool((want != 0).any())
        assert _same(hp.emulate(u.q, u.k, tiny), want)
        flushed = hp.emulate(u.q, u.k, tiny, fault="flush_subnormal_v")
        assert bool((flushed == 0).all()) and not _same(flushed, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_range_probes_reject_a_wrong_running_maximum(dtype):
    # O not rescaled when the maximum rises: needs a wave's second key tile, and scores that rise
    below, first = hp.range_case(dtype, N, 128, "ramp"), hp.range_case(dtype, N, 129, "ramp")
    assert _same(hp.emulate(below.q, below.k, below.v, fault="no_rescale"), hp.emulate(below.q, below.k, below.v))
    _rejected(first, hp.emulate(first.q, first.k, first.v, fault="no_rescale"))
    # the running maximum started at 0: scores near -150 leave no weight at all
    for T in (1, 33):
        c = hp.range_case(dtype, N, T, "offset")
        assert 1 in c.cls.flatten().tolist()
        _rejected(c, hp.emulate(c.q, c.k, c.v, fault="max_from_0"))


def test_checks_reject_nan():
    c = hp.random_case(torch.float16, N, 33, "random")
    _rejected(c, torch.full_like(c.q, float("nan")))
    o = hp.emulate(c.q, c.k, c.v)
    o[1, 2, 3] = float("inf")
    _rejected(c, o)

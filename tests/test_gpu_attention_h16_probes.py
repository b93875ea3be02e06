"""wx_attention_h16 and wx_attention_h16_packed on the GPU under the probes of
attention_h16_probes.py, fp16 and bf16: the derived elementwise bound against fp64 on random, flat,
score-range and fp16-subnormal inputs, and whisper_half_helpers' exact probes at the tile
configurations test_gpu_attention_h16.py leaves out: wave 3 without keys (T 65 .. 96), the first T at
which every wave has a tile (97), the first restaged V tile of wave 0 (129) and of wave 1 (161)."""
import pytest
import torch

import attention_h16_probes as hp
import whisper_half_helpers as hh

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(d, id=hh.name(d)) for d in hh.DTYPES]
N = 4
BOUND_TS = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 160, 161, 257)
RANGE_TS = (33, 97, 129, 161, 257)
PERMUTATION_TS = (65, 96, 97, 128, 129, 160, 161, 257)


def _attend(q, k, v):
    """[N, T, 64] CPU -> [N, T, 64] CPU through one head per batch entry."""
    from whisperx_amd import _lib

    o = _lib.attention_h16(q.cuda().unsqueeze(1), k.cuda().unsqueeze(1), v.cuda().unsqueeze(1), hh.SCALE)
    return o[:, :, 0].cpu()


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("kind", ["random", "flat"])
@pytest.mark.parametrize("T", BOUND_TS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bound(dtype, T, kind):
    c = hp.random_case(dtype, N, T, kind)
    o = _attend(c.q, c.k, c.v)
    c.check(o, "wx_attention_h16")
    if T == 1:
        assert torch.equal(_bits(o), _bits(c.v))


@pytest.mark.parametrize("variant", ["offset", "ramp"])
@pytest.mark.parametrize("T", RANGE_TS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bound_over_the_score_range(dtype, T, variant):
    """Scores shifted by +-150, or rising / falling by up to 300 towards the last key: on the ramp
    the running maximum of a rising query grows with every key tile (alpha != 1)."""
    c = hp.range_case(dtype, N, T, variant)
    c.check(_attend(c.q, c.k, c.v), "wx_attention_h16")


@pytest.mark.parametrize("dtype", DTYPES)
def test_bound_on_the_ramp_at_1500(dtype):
    c = hp.range_case(dtype, 1, 1500, "ramp")
    c.check(_attend(c.q, c.k, c.v), "wx_attention_h16")


@pytest.mark.parametrize("kind", ["identity", "reversal", "random"])
@pytest.mark.parametrize("T", PERMUTATION_TS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_permutation_probe(dtype, T, kind):
    p = hh.Permutation(dtype, N, T, kind)
    o = _attend(p.q, p.k, p.v)
    bad = (_bits(o) != _bits(p.want)).any(-1)
    assert not bool(bad.any()), (f"{int(bad.sum())} of {bad.numel()} queries do not return their target's value row; "
                                 f"first (n, i) = {tuple(int(x) for x in bad.nonzero()[0])}, margin {p.margin:.1f}")


@pytest.mark.parametrize("T", PERMUTATION_TS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_permutation_probe_with_large_values(dtype, T):
    """v x 2^14 (fp16, up to 57344) or x 2^100 (bf16): still o[i] = v[pi(i)] exactly.  (|v| is
    clamped to 3.5 first: 4 x 2^14 is past fp16's largest number.)"""
    p = hh.Permutation(dtype, N, T, "random")
    v = (p.v.float().clamp(-3.5, 3.5) * (2.0 ** 14 if dtype == torch.float16 else 2.0 ** 100)).to(dtype)
    assert bool(torch.isfinite(v).all()) and float(v.float().abs().min()) >= 16
    want = v.gather(1, p.pi[:, :, None].expand(N, T, 64))
    assert torch.equal(_bits(_attend(p.q, p.k, v)), _bits(want))


@pytest.mark.parametrize("L", [128, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_uniform_probe(dtype, L):
    u = hh.Uniform(dtype, N, L)
    assert u.exact
    assert torch.equal(_bits(_attend(u.q, u.k, u.v)), _bits(u.want.to(dtype)))


@pytest.mark.parametrize("L", [32, 64, 1024])
def test_uniform_probe_on_subnormal_values(L):
    """fp16, v x 2^-22: the values and their means are subnormal; o is torch's rounding of the exact mean."""
    dtype = torch.float16
    u = hh.Uniform(dtype, N, L)
    assert u.exact
    tiny = (u.v.double() * 2.0 ** -22).to(dtype)
    assert torch.equal(tiny.double(), u.v.double() * 2.0 ** -22) and hp.share_subnormal(tiny) > 0.7
    want = (u.want * 2.0 ** -22).to(dtype)
    assert bool((want != 0).any())
    assert torch.equal(_bits(_attend(u.q, u.k, tiny)), _bits(want))


@pytest.mark.parametrize("T", [33, 97, 161])
@pytest.mark.parametrize("which", ["v", "k"])
def test_subnormal_inputs(which, T):
    """fp16 subnormal values (and outputs), and subnormal keys whose flushing would move the weights
    by some 20 %: within the bound, which has no allowance for either."""
    c = hp.subnormal_case(N, T, which)
    assert c.share > (0.6 if which == "v" else 0.2)
    o = _attend(c.q, c.k, c.v)
    c.check(o, "wx_attention_h16")
    assert bool((o != 0).any())
    if which == "v":
        assert hp.share_subnormal(o) > 0.6


@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_range_segments_equal_the_dense_launch(dtype):
    """One pack of score-range segments (H = 4 heads: a case's N): each segment's rows are the dense
    launch's, bit for bit, and within the bound."""
    from whisperx_amd import _lib

    H = N
    cases = [hp.range_case(dtype, H, T, variant) for T, variant in ((33, "offset"), (97, "ramp"), (161, "ramp"))]
    segs = _lib.PackedSegments([c.q.shape[1] for c in cases])
    D = 64 * H
    buf = torch.full((segs.rows + 32, 3 * D + 8), float("nan"), dtype=dtype)
    for pos, c in enumerate(cases):
        a, b = segs.offsets[pos], segs.offsets[pos + 1]
        for j, t in enumerate((c.q, c.k, c.v)):
            buf[a:b, j * D:(j + 1) * D] = t.transpose(0, 1).reshape(b - a, D)
    buf = buf.cuda()
    q, k, v = (buf[None, :segs.rows, j * D:(j + 1) * D].view(1, segs.rows, H, 64).transpose(1, 2) for j in range(3))
    o = _lib.attention_h16_packed(q, k, v, hh.SCALE, segs)[0].cpu()
    for pos, c in enumerate(cases):
        got = o[segs.offsets[pos]: segs.offsets[pos + 1]].transpose(0, 1)  # [H, T, 64]
        assert torch.equal(_bits(got), _bits(_attend(c.q, c.k, c.v))), c.label
        c.check(got, "wx_attention_h16_packed")

"""The LayerNorm probes' own conditions (tests/layernorm_probes.py), without a GPU: a plain fp32
two-pass restatement returns every exact probe's expected bits in every split, torch's own layer_norm
agrees to rounding, and each faulty restatement, the kind of mistake the kernel could make, is rejected
by the probe named for it."""
import pytest
import torch
import torch.nn.functional as F

import layernorm_probes as lp


def _run(p, fault=None):
    """the restatement on every split of p; raises AssertionError at the first output that differs"""
    for label, a, b in p.splits:
        y, s = lp.layernorm_f32(a, b, p.gamma, p.beta, p.eps, fault)
        p.check(y32=y, s=s, label=label)
        for dtype in (torch.float16, torch.bfloat16):
            p.check(y16=y.to(dtype), label=label)


def _rejected(p, fault):
    with pytest.raises(AssertionError):
        _run(p, fault)


@pytest.mark.parametrize("rows", lp.ROWS)
@pytest.mark.parametrize("D", lp.WIDTHS)
@pytest.mark.parametrize("kind", lp.KINDS)
def test_exact_probes(kind, D, rows):
    p = lp.exact(kind, D, rows)
    _run(p)
    # the expected values are a LayerNorm's: torch's (Welford, other roundings) agrees closely
    for _, a, b in p.splits:
        ref = F.layer_norm((a + b).double(), (D,), p.gamma.double(), p.beta.double(), p.eps)
        assert float((p.y.double() - ref).abs().max()) < 1e-6
    assert bool(((a + b).sum(-1) == p.mean * D).all())
    # every probe reads gamma and beta at its own column
    _rejected(p, "gamma_shifted_in_float4")
    # eps: only the probe made for it tells
    if kind == "eps":
        _rejected(p, "eps_dropped")
    else:
        _run(p, "eps_dropped")
    if kind.startswith("offset"):
        _rejected(p, "mean_over_d_minus_4")
        if D == 384:
            _rejected(p, "d384_lanes_96_127")
    if kind == "offset4096":
        _rejected(p, "one_pass_variance")
    if D != 384:
        _run(p, "d384_lanes_96_127")  # (the fault of the partial-width path only)


@pytest.mark.parametrize("D", lp.WIDTHS)
def test_balanced_rows_differ(D):
    p = lp.exact("balanced", D, 67)
    v = p.sum
    assert len({float(x) for x in v.abs()[:, 0]}) == 10 and float(v.abs().min()) == 2.0 ** -3 and float(v.abs().max()) == 64
    assert bool(((v > 0).sum(-1) == D // 2).all())
    assert len({tuple((r > 0).tolist()) for r in v}) == 67
    # another row's data in a D = 384 row is seen by the balanced probe too (rows of other magnitudes)
    if D == 384:
        _rejected(p, "d384_lanes_96_127")


@pytest.mark.parametrize("D", lp.WIDTHS)
def test_bounded_check(D):
    a, b, gamma, beta, eps, want, ref_err = lp.bounded(D, 67)
    assert 49 < float(a.mean()) < 51 and 1.8 < float(a.std()) < 2.2
    y, _ = lp.layernorm_f32(a, b, gamma, beta, eps)
    err = float((y.double() - want).abs().max())
    print(f"D {D}: restatement |y - fp64| {err:.2e}, ref_err {ref_err:.2e}")
    assert err <= 4 * ref_err
    for fault in ("gamma_shifted_in_float4", "mean_over_d_minus_4", "one_pass_variance"):
        bad, _ = lp.layernorm_f32(a, b, gamma, beta, eps, fault)
        assert float((bad.double() - want).abs().max()) > 4 * ref_err, fault

"""whisper._chain without a GPU: the fused route (every residual add fused with the norm after it),
driven by a torch stand-in for wx_add_layernorm, against the plain route, and the calls it issues."""
import pytest
import torch
import torch.nn.functional as F

D = 64


def _case(n_stages: int):
    """Rows [5, 64], `n_stages` stages (norm, fixed linear map) and a final norm."""
    g = torch.Generator().manual_seed(7)

    def norm():
        return 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)

    def linear():
        w, b = torch.randn((D, D), generator=g) / D ** 0.5, 0.1 * torch.randn(D, generator=g)
        return lambda y: F.linear(y, w, b)

    h = torch.randn((5, D), generator=g)
    return h, [(norm(), linear()) for _ in range(n_stages)], norm()


@pytest.mark.parametrize("n_stages", [0, 1, 3])
def test_fused_route_equals_the_plain_one_and_issues_the_expected_calls(n_stages):
    from whisperx_amd.whisper import _chain

    h, stages, final = _case(n_stages)
    calls = []

    def add_layernorm(a, b, gamma, beta, eps, want_sum=False):
        calls.append(((gamma, beta), want_sum))
        s = a + b
        y = F.layer_norm(s, (D,), gamma, beta, eps)
        return (y, s) if want_sum else y

    before = h.clone()
    plain = _chain(h, stages, final)
    fused = _chain(h, stages, final, add_layernorm)
    assert torch.equal(h, before)  # the stream that came in is not written
    assert plain.shape == (5, D) and torch.equal(fused, plain)
    # by hand, to hold the plain route to something: h = h + fn(LN(h)) per stage, then the final norm
    want = h
    for (w, b), fn in stages:
        want = want + fn(F.layer_norm(want, (D,), w, b, 1e-5))
    assert torch.equal(plain, F.layer_norm(want, (D,), *final, 1e-5))
    # one fused call per stage, each with the norm of the stage after it (the final one at the end),
    # and only the last without a sum to keep
    assert len(calls) == n_stages
    norms = [ln for ln, _ in stages[1:]] + [final]
    for (got, want_sum), ln, last in zip(calls, norms, [False] * (n_stages - 1) + [True]):
        assert got[0] is ln[0] and got[1] is ln[1]
        assert want_sum is not last

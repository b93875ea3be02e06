"""wx_sample_token and wx_beam_topk on the GPU under the probes of selection_probes.py: planted
winners on every column of a slice and its tail and on one lane's 16 registers, ties across lanes,
waves, slices and beams, constant rows, one bit per pair of columns of the generator, whole waves and
slices of -inf, V = 2G and about every wave and slice edge, and 67 slices (the second trip of the
merge loops).  Rows are strided with NaN in the padding; the sample probes also hold the logits'
bytes and the sum / done state on every row."""
import math

import pytest
import torch

import selection_probes as sp

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _padded(x):
    """x [R, V] on the device with a row stride of V + 3 and NaN in the padding (the buffer, the view)."""
    R, V = x.shape
    wide = torch.full((R, V + 3), math.nan, device="cuda")
    wide[:, :V] = x.cuda()
    return wide, wide[:, :V]


# ------------------------------------------------------------------------------ wx_sample_token
def _sample(p):
    """One launch of probe p on the current stream: (token, logprob, sums before, sums after, done) on
    the host and whether the logits kept their bytes."""
    from whisperx_amd import _lib

    buf, view = _padded(p.x)
    before = buf.clone()
    sums0 = torch.randn(p.R, generator=torch.Generator().manual_seed(p.R + p.V)) - 3
    sums_d, done_d = sums0.cuda(), torch.zeros(p.R, dtype=torch.bool, device="cuda")
    step_d = torch.tensor([p.step], dtype=torch.int64, device="cuda")
    tok, lp = _lib.sample_token(view, step_d, p.eot, done_d, p.temperature, sp.SEED,
                                None if p.suppress is None else p.suppress.cuda(), sums_d)
    torch.cuda.current_stream().synchronize()
    same = torch.equal(_bits(buf), _bits(before))
    return tok.cpu(), lp.cpu(), sums0, sums_d.cpu(), done_d.cpu(), same


def _check_sample(p) -> float:
    tok, lp, sums0, sums, done, same = _sample(p)
    assert same, f"{p.label}: the logits were written"
    ratio = p.check((tok, lp), "wx_sample_token")
    # the state, on every row (each is scored): one fp32 addition of the logprob; done where the token is eot
    assert torch.equal(_bits(sums), _bits(sums0 + lp)), p.label
    assert torch.equal(done, tok == p.eot), p.label
    keep = torch.from_numpy(p.keep)
    assert torch.equal(done[keep], torch.from_numpy(p.done)[keep]), p.label
    return ratio


@pytest.mark.parametrize("temperature", [0.0, 1.0])
def test_every_column_wins(temperature):
    p = sp.every_column_wins(temperature)
    _check_sample(p)
    assert int(p.done.sum()) == 1  # (row V - 1 takes eot)


def test_sample_ties():
    _check_sample(sp.tie_rows())


@pytest.mark.parametrize("V", [1, 5, 1025, sp.N_EDGE])
def test_sample_constant_rows(V):
    for masked in (False, True) if V > 3 else (False,):
        _check_sample(sp.constant_row(V, masked))


@pytest.mark.parametrize("step", [0, 7])
@pytest.mark.parametrize("temperature", [0.2, 1.0])
def test_pair_rows(temperature, step):
    _check_sample(sp.pair_rows(temperature, step))


@pytest.mark.parametrize("via", ["mask", "logits"])
@pytest.mark.parametrize("unit", sp.UNITS)
def test_sample_masked_units(unit, via):
    for temperature in (0.0, 0.7):
        _check_sample(sp.masked_units(unit, via, temperature))


@pytest.mark.parametrize("temperature", [0.0, 0.7])
def test_sample_more_than_64_slices(temperature):
    p = sp.many_slices(temperature)
    _check_sample(p)
    if temperature == 0:
        assert p.token.tolist() == p.cols  # the plants; the tie of slice 0 and slice 64 goes to slice 0


def test_sample_on_a_side_stream():
    """The same inputs on a non-default stream: the same bits."""
    side = torch.cuda.Stream()
    for p in (sp.many_slices(0.7), sp.masked_units("slice 1", "mask", 0.7), sp.pair_rows(1.0, 7)):
        want = _sample(p)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = _sample(p)
        side.synchronize()
        assert got[5] and torch.equal(got[0], want[0]) and torch.equal(got[4], want[4]), p.label
        assert torch.equal(_bits(got[1]), _bits(want[1])) and torch.equal(_bits(got[3]), _bits(want[3])), p.label


# --------------------------------------------------------------------------------- wx_beam_topk
def _topk(p):
    from whisperx_amd import _lib

    buf, view = _padded(p.x)
    s, i = _lib.beam_topk(view, p.cum.cuda(), p.G)
    torch.cuda.current_stream().synchronize()
    assert tuple(s.shape) == tuple(i.shape) == (p.B, p.K) and i.dtype == torch.int32 and s.dtype == torch.float32
    return s.cpu(), i.cpu()


def _check_topk(p) -> float:
    return p.check(_topk(p), "wx_beam_topk")


@pytest.mark.parametrize("G", [1, 5, 8])
def test_concentrated_winners(G):
    _check_topk(sp.concentrated_winners(G))


@pytest.mark.parametrize("G", [1, 5, 8])
def test_topk_ties(G):
    p = sp.topk_constant_rows(G)
    _check_topk(p)
    s, i = _topk(p)
    assert i[0].tolist() == list(range(2 * G)) and bool(torch.isfinite(s).all()) and len(set(_bits(s)[0].tolist())) == 1
    for span in sp.TIE_SPANS:
        _check_topk(sp.topk_equal_maxima(G, span))
    _check_topk(sp.topk_identical_beams(max(G, 2)))


@pytest.mark.parametrize("G", sp.EDGE_G)
def test_topk_smallest_and_edge_v(G):
    worst = max(_check_topk(sp.topk_edge_v(G, V)) for V in sp.edge_v(G))
    print(f"edge V, G {G}: largest |score - fp64| / bound {worst:.3f}")


@pytest.mark.parametrize("G", [5, 8])
def test_topk_masked_units(G):
    p = sp.topk_masked_units(G)
    _check_topk(p)
    s, _ = _topk(p)
    assert not bool(torch.isnan(s).any()) and bool((s[1, 3:] == -math.inf).all()) and bool(torch.isfinite(s[1, :3]).all())


@pytest.mark.parametrize("kind", sp.MANY_KINDS)
def test_topk_more_than_64_slices(kind):
    _check_topk(sp.topk_many_slices(kind))


def test_topk_on_a_side_stream():
    """The same inputs on a non-default stream: the same bits."""
    side = torch.cuda.Stream()
    for p in (sp.topk_many_slices("tie"), sp.topk_masked_units(5), sp.concentrated_winners(8)):
        want = _topk(p)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = _topk(p)
        side.synchronize()
        assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(got[1], want[1]), p.label

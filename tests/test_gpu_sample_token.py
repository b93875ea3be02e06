"""wx_sample_token on the GPU against the fp64 evaluation of its definition (sample_helpers): tokens
wherever the definition's top-2 margin exceeds the derived eps (exactly, ties included, at
temperature 0), log-probabilities within the derived fp32 bound, the sum / done state, rows that
are done or fully masked, independence of R, logits left as they were, and every refusal."""
import ctypes

import pytest
import torch

from sample_helpers import SLICE, check_margins, definition, eps_tokens, kernel_case, logprob_bound

pytestmark = pytest.mark.gpu

WX_OK, WX_E_INVALID, WX_E_WORKSPACE = 0, 1001, 1004
# (R, V, row_stride)
SHAPES = [(1, 1, 1), (3, 96, 96), (5, 257, 300), (7, SLICE - 1, SLICE - 1), (7, SLICE, SLICE), (7, SLICE + 1, SLICE + 1),
          (80, 2 * SLICE + 3, 2 * SLICE + 3), (2, 51865, 51865)]
STEPS = [0, 7, 2 ** 32 + 1]
SEED = (3 << 32) + 12345  # both key words in use


def _run(x, stride, suppress, done, eot, temperature, step, sums, seed=SEED):
    """One launch on a strided copy of x (NaN between the rows).  Returns (token, logprob, sums, done)
    on the host and whether the logits buffer kept its bytes."""
    from whisperx_amd import _lib

    R, V = x.shape
    buf = torch.full((R, stride), float("nan"), device="cuda")
    buf[:, :V] = x.cuda()
    before = buf.clone()
    done_d, sums_d = done.cuda(), sums.cuda()
    step_d = torch.tensor([step], dtype=torch.int64, device="cuda")
    tok, lp = _lib.sample_token(buf[:, :V], step_d, eot, done_d, temperature, seed, None if suppress is None else suppress.cuda(),
                                sums_d)
    torch.cuda.synchronize()
    same = torch.equal(buf.view(torch.int32), before.view(torch.int32))
    return tok.cpu(), lp.cpu(), sums_d.cpu(), done_d.cpu(), same


@pytest.mark.parametrize("temperature", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("R,V,stride", SHAPES)
def test_against_the_definition(R, V, stride, temperature):
    x, suppress, done, eot = kernel_case(R, V)
    finite = x[torch.isfinite(x)]
    top = float(finite.abs().max())
    sums0 = torch.randn(R, generator=torch.Generator().manual_seed(R + V)) - 3
    for step in STEPS:
        label = f"R {R} V {V} T {temperature} step {step}"
        sel = definition(x, suppress, temperature, SEED, step, done, eot)
        keep = check_margins(sel, eps_tokens(top, temperature), label)  # (on the CPU, before the GPU is asked)
        tok, lp, sums, done1, same = _run(x, stride, suppress, done, eot, temperature, step, sums0)
        assert same, f"{label}: the logits were written"
        want_tok = torch.from_numpy(sel.token)
        assert torch.equal(tok[keep], want_tok[keep]), (label, (tok != want_tok).nonzero().flatten().tolist())
        agree = (tok == want_tok).numpy()
        err = (lp.double() - torch.from_numpy(sel.logprob)).abs()[agree]
        bound = logprob_bound(top, V)
        print(f"{label}: {int(agree.sum())} of {R} tokens equal; |logprob - fp64| max {float(err.max()):.3e}, bound {bound:.3e}")
        assert float(err.max()) <= bound
        # the state: a scored row's sum moved by its logprob in one fp32 addition, the others' bits are
        # left alone (so is logprob 0 and the token eot); done as the definition says
        scored = torch.from_numpy(sel.scored)
        assert torch.equal(sums[scored], (sums0 + lp)[scored])
        assert torch.equal(sums[~scored].view(torch.int32), sums0[~scored].view(torch.int32))
        assert bool((lp[~scored] == 0).all()) and bool((tok[~scored] == eot).all())
        assert torch.equal(done1[agree], torch.from_numpy(sel.done)[agree])
        assert bool(done1[done].all())
        if temperature == 0 and V >= 8:  # the exact tie of row 0: the lower id
            tie = (x[0] == 9.5).nonzero().flatten().tolist()
            assert len(tie) == 2 and int(tok[0]) == tie[0]
        if R >= 3:
            assert int(tok[1]) == eot and bool(done1[1]) and float(lp[1]) == 0  # the fully masked row


def test_no_mask_and_no_sum():
    """suppress and sum_logprob may be NULL."""
    from whisperx_amd import _lib

    R, V = 4, 300
    x, _, _, eot = kernel_case(R, V)
    done = torch.zeros(R, dtype=torch.bool, device="cuda")
    step = torch.tensor([5], dtype=torch.int64, device="cuda")
    tok, lp = _lib.sample_token(x.cuda(), step, eot, done, 0.7, SEED)
    sel = definition(x, None, 0.7, SEED, 5, torch.zeros(R, dtype=torch.bool), eot)
    keep = check_margins(sel, eps_tokens(float(x[torch.isfinite(x)].abs().max()), 0.7), "no mask")
    assert torch.equal(tok.cpu()[keep], torch.from_numpy(sel.token)[keep])
    assert torch.equal(done.cpu(), torch.from_numpy(sel.done))


@pytest.mark.parametrize("temperature", [0.0, 0.6])
def test_a_row_depends_on_neither_the_other_rows_nor_r(temperature):
    """Row 0 of 80 rows and the same row alone: token and logprob bit for bit (the generator counts
    rows from 0, so row 0 is the row both launches share), also with the other rows replaced."""
    R, V = 80, 2 * SLICE + 3
    x, suppress, done, eot = kernel_case(R, V)
    sums0 = torch.zeros(R)
    got = []
    other = x.clone()
    other[1:] = torch.randn((R - 1, V), generator=torch.Generator().manual_seed(8))
    for rows, d in ((x, done), (x[:1], done[:1]), (other, torch.zeros(R, dtype=torch.bool))):
        tok, lp, sums, _, _ = _run(rows, V + 5, suppress, d, eot, temperature, 7, sums0[:rows.shape[0]])
        got.append((int(tok[0]), int(lp[:1].view(torch.int32)), int(sums[:1].view(torch.int32))))
    assert got[0] == got[1] == got[2], got


def test_refusals():
    """Every refusal of the header, in its order, before anything is enqueued: the outputs keep their
    bytes.  The pointers handed over are real buffers of the right size throughout."""
    from whisperx_amd import _lib

    lib = _lib.load()
    R, V = 3, 100
    lg = torch.zeros((R, V), device="cuda")
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    done = torch.zeros(R, dtype=torch.uint8, device="cuda")
    tok = torch.full((R,), -7, dtype=torch.int64, device="cuda")
    lp = torch.full((R,), -7.0, device="cuda")
    sums = torch.full((R,), -7.0, device="cuda")
    wsb = lib.wx_sample_token_workspace_bytes(R, V)
    ws = torch.zeros(wsb + 16, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0 and wsb > 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(R=R, V=V, stride=V, T=0.5, eot=4, logits=p(lg), step_=p(step), done_=p(done), token=p(tok), logprob=p(lp),
             sum_=p(sums), work=p(ws), nbytes=wsb):
        return lib.wx_sample_token(logits, stride, R, V, None, T, 1, step_, eot, done_, token, logprob, sum_, work, nbytes, None)

    for kw in (dict(R=-1), dict(V=0), dict(V=(1 << 24) + 1, stride=(1 << 24) + 1), dict(stride=V - 1), dict(T=-0.5),
               dict(T=float("nan")), dict(T=float("inf")), dict(eot=-1), dict(eot=V)):
        assert call(**kw) == WX_E_INVALID, kw
    assert call(R=0, logits=None, token=None, work=None) == WX_OK  # R == 0 comes before the pointer checks ...
    assert call(R=0, V=0) == WX_E_INVALID  # ... and after the scalar ones
    for name in ("logits", "step_", "done_", "token", "logprob", "work"):
        assert call(**{name: None}) == WX_E_INVALID, name
    assert call(work=ctypes.c_void_p(ws.data_ptr() + 8)) == WX_E_INVALID
    assert call(nbytes=wsb - 1) == WX_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((tok == -7).all()) and bool((lp == -7).all()) and bool((sums == -7).all()) and not bool(done.any())
    assert not bool(ws.any())
    # R above a grid dimension: refused on the sizes alone
    big = 65536
    bytes_big = lib.wx_sample_token_workspace_bytes(big, 8)
    b_lg, b_done = torch.zeros((big, 8), device="cuda"), torch.zeros(big, dtype=torch.uint8, device="cuda")
    b_tok, b_lp = torch.full((big,), -7, dtype=torch.int64, device="cuda"), torch.full((big,), -7.0, device="cuda")
    b_ws = torch.zeros(bytes_big, dtype=torch.uint8, device="cuda")
    assert call(R=big, V=8, stride=8, logits=p(b_lg), done_=p(b_done), token=p(b_tok), logprob=p(b_lp), sum_=None,
                work=p(b_ws), nbytes=bytes_big) == WX_E_INVALID
    torch.cuda.synchronize()
    assert bool((b_tok == -7).all()) and not bool(b_ws.any())
    # and the wrapper's own checks
    with pytest.raises(_lib.WXError):
        _lib.sample_token(lg, step, 4, done[:2], 0.5, 1)
    with pytest.raises(_lib.WXError):
        _lib.sample_token(lg, step.to(torch.int32), 4, done, 0.5, 1)
    with pytest.raises(_lib.WXError):
        _lib.sample_token(lg, step, 4, done, -1.0, 1)

"""wx_penalize_logits on the device: every probe of penalty_probes bit-equal to the numpy definition,
in both history layouts and on logits whose row stride exceeds V; a row's result alone and among
five rows; a captured launch replayed while the count grows on the device; every error code."""
import ctypes

import numpy as np
import pytest
import torch

from penalty_probes import MAX_HISTORY, definition, length, probes, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WX_OK, WX_E_INVALID = 0, 1001


def _run(p, row_major, rows=None):
    """The probe (or its rows `rows`) through _lib.penalize_logits -> the whole [R, stride] buffer."""
    from whisperx_amd import _lib

    logits, hist = (p.logits, p.hist) if rows is None else (p.logits[rows], p.hist[rows])
    buf = torch.from_numpy(logits.copy()).to(DEV)
    h = torch.from_numpy(hist.copy()).to(DEV)
    if not row_major:
        h = h.t().contiguous()  # [cap, R]: the selection's record
    count = torch.tensor([p.count], dtype=torch.int64, device=DEV)
    out = _lib.penalize_logits(buf[:, :p.V], h, count, p.offset, p.max_history, p.rho, p.n, row_major=row_major)
    assert out.data_ptr() == buf.data_ptr()
    return buf.cpu().numpy()


@pytest.mark.parametrize("row_major", [False, True], ids=["step-major", "row-major"])
def test_probes_are_bit_equal_to_the_definition(row_major):
    ps = probes()
    for p in ps:
        L = length(p.count, p.offset, p.max_history)
        want = definition(p.logits, p.V, p.hist, L, p.rho, p.n)
        got = _run(p, row_major)
        assert same_bits(got, want), (p.name, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:8].tolist())
    assert any(length(p.count, p.offset, p.max_history) == MAX_HISTORY for p in ps)


def test_a_row_alone_is_the_row_among_five():
    ran = 0
    for p in probes():
        if p.logits.shape[0] != 5:
            continue
        whole = _run(p, False)
        for r in range(5):
            assert same_bits(_run(p, False, rows=[r])[0], whole[r]), (p.name, r)
        ran += 1
    assert ran >= 10


def test_a_captured_launch_reads_the_count_at_every_replay():
    from whisperx_amd import _lib
    from whisperx_amd.whisper import WhisperDecoder

    rng = np.random.default_rng(5)
    R, V, stride, offset, rho, n = 3, 40, 43, 2, 1.3, 2
    hist = rng.integers(0, 6, (R, 20))  # few ids: bigrams repeat
    x = (4 * rng.standard_normal((R, stride))).astype(np.float32)
    src, h = torch.from_numpy(x).to(DEV), torch.from_numpy(hist).to(DEV).t().contiguous()
    first = 9
    direct = []
    for i in range(3):
        buf = src.clone()
        _lib.penalize_logits(buf[:, :V], h, torch.tensor([first + i], dtype=torch.int64, device=DEV), offset, 20, rho, n)
        direct.append(buf.cpu().numpy())
        assert same_bits(direct[-1], definition(x, V, hist, first + i + offset, rho, n))
    assert not same_bits(direct[0], direct[1]) and not same_bits(direct[1], direct[2])

    work, count = src.clone(), torch.tensor([first], dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (the kernel loaded before the capture)
        _lib.penalize_logits(work[:, :V], h, count, offset, 20, rho, n)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with WhisperDecoder._capturing(g):
        _lib.penalize_logits(work[:, :V], h, count, offset, 20, rho, n)
    for i in range(3):
        work.copy_(src)
        g.replay()
        assert same_bits(work.cpu().numpy(), direct[i]), i
        count.add_(1)  # on the device: the graph's argument is the pointer


def test_error_codes():
    from whisperx_amd import _lib

    lib = _lib.load()
    x = torch.zeros((2, 8), dtype=torch.float32, device=DEV)
    h = torch.zeros((4, 2), dtype=torch.int64, device=DEV)
    c = torch.ones(1, dtype=torch.int64, device=DEV)
    before = x.clone()
    X, H, C = (ctypes.c_void_p(t.data_ptr()) for t in (x, h, c))

    def call(logits=X, row_stride=8, R=2, V=8, history=H, count=C, max_history=4, rho=1.3, n=1):
        return lib.wx_penalize_logits(logits, row_stride, R, V, history, 2, 1, count, 0, max_history, rho, n, None)

    for bad in (dict(R=-1), dict(V=0), dict(V=(1 << 24) + 1, row_stride=1 << 25), dict(row_stride=7), dict(rho=float("nan")),
                dict(rho=float("inf")), dict(rho=0.0), dict(rho=-1.3), dict(n=-1), dict(max_history=-1),
                dict(max_history=MAX_HISTORY + 1)):
        assert call(**bad) == WX_E_INVALID, bad
    # nothing to do is WX_OK before the pointers are looked at
    assert call(R=0, logits=None, history=None, count=None) == WX_OK
    assert call(max_history=0, logits=None, history=None, count=None) == WX_OK
    for bad in (dict(logits=None), dict(history=None), dict(count=None), dict(R=65536)):
        assert call(**bad) == WX_E_INVALID, bad
    # ... and an invalid argument wins over "nothing to do"
    assert call(R=0, rho=0.0) == WX_E_INVALID and call(max_history=0, n=-1) == WX_E_INVALID
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    assert call() == WX_OK
    torch.cuda.synchronize()
    assert bool(torch.isneginf(x[:, 0]).all()) and torch.equal(x[:, 1:], before[:, 1:])

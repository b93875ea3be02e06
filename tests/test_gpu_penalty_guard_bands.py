"""Where wx_penalize_logits writes: the logits between guard bands (guard_bands.py) with a row
stride above V, at the two smallest and the largest shape of the probes, under a history that
holds ids outside [0, V) (-1, V, 2^40 and their like).  WX_OK, every band byte unchanged after the
stream has drained, the columns V .. row_stride of every row still fresh, and the columns below V
bit for bit the numpy definition's.  Every comparison is of bytes."""
import ctypes

import numpy as np
import pytest
import torch

import guard_bands as gb
from penalty_probes import PAD, definition, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("row_major", [False, True], ids=["step-major", "row-major"])
@pytest.mark.parametrize("R,V", [(1, 1), (3, 5), (5, 4097)])
def test_penalize_logits(R, V, row_major):
    from whisperx_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(1000 * V + R)
    L, stride = 257, V + PAD
    hist = rng.integers(0, V, (R, L))
    outside = np.array([-1, V, 1 << 40, -(1 << 40), (1 << 32) + min(V - 1, 1), V + PAD - 1, -PAD, (1 << 31) - 1])
    hist[:, ::3] = outside[rng.integers(0, len(outside), hist[:, ::3].shape)]
    hist[:, -1] = hist[:, 1]  # an in-range bigram repeats, whatever else does
    x = (4 * rng.standard_normal((R, V))).astype(np.float32)
    x[np.abs(x) < 1e-3] = 1.0

    g = gb.guarded((R, stride), torch.float32, DEV, offset=4, name=f"logits R {R} V {V}")
    h = torch.from_numpy(hist).to(DEV)
    step_stride, row_stride = (1, L) if row_major else (R, 1)
    if not row_major:
        h = h.t().contiguous()
    count = torch.tensor([L - 2], dtype=torch.int64, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    for rho, n in ((1.3, 1), (0.5, 2)):
        g.t[:, :V] = torch.from_numpy(x).to(DEV)
        rc =lib.wx_penalize_logits(ctypes.c_void_p(g.ptr), stride, R, V, ctypes.c_void_p(h.data_ptr()), step_stride,
                                    row_stride, ctypes.c_void_p(count.data_ptr()), 2, L, rho, n, stream)
        torch.cuda.synchronize()
        assert rc == 0
        gb.check(g)
        pad = g.t[:, V:].contiguous().view(torch.uint8)
        assert bool((pad == gb.FRESH).all()), "a column at or above V was written"
        x_new = definition(x, V, hist, L, rho, n)
        assert same_bits(g.t[:, :V].cpu().numpy(), x_new), (rho, n)
        assert not same_bits(x_new, x)

"""wx_add_layernorm_h16 on the GPU, fp16 and bf16: y is bit for bit the rounding of
wx_add_layernorm(a, float(b))'s y and the sum is bit-equal to its sum, at every width, with b
contiguous, row-strided or absent, and whatever lies between and behind the rows."""
import pytest
import torch

import whisper_half_helpers as hh

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(d, id=hh.name(d)) for d in hh.DTYPES]
WIDTHS = (256, 384, 512, 768, 1024, 1280)
ROWS = (1, 5, 67)


def _inputs(dtype, D, rows):
    g = torch.Generator().manual_seed(D * 100 + rows)
    a = (2.0 * torch.randn((rows, D), generator=g)).cuda()
    b = torch.randn((rows, D), generator=g).to(dtype).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(D, generator=g)).cuda(), (0.1 * torch.randn(D, generator=g)).cuda()
    return a, b, gamma, beta


def _strided(t, fill):
    """t [rows, D] as a view of a [rows + 1, D + 8] buffer that holds `fill` everywhere else: padding
    between the rows and a whole row behind the last."""
    rows, D = t.shape
    wide = torch.full((rows + 1, D + 8), fill, dtype=t.dtype, device=t.device)
    view = wide[:rows, :D]
    view.copy_(t)
    return view


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_equals_the_rounded_fp32_kernel(dtype, D, rows):
    from whisperx_amd import _lib

    a, b, gamma, beta = _inputs(dtype, D, rows)
    want_y, want_s = _lib.add_layernorm(a, b.float(), gamma, beta, 1e-5, want_sum=True)
    want_y = want_y.to(dtype)
    for label, (aa, bb) in (("contiguous", (a, b)), ("strided, zeros around", (_strided(a, 0.0), _strided(b, 0.0))),
                            ("strided, NaN around", (_strided(a, float("nan")), _strided(b, float("nan"))))):
        assert label == "contiguous" or (bb.stride(0) == D + 8 and bb.data_ptr() % 16 == 0)
        y, s = _lib.add_layernorm_h16(aa, bb, gamma, beta, 1e-5, dtype, want_sum=True)
        assert y.dtype == dtype and s.dtype == torch.float32 and y.is_contiguous() and s.is_contiguous()
        assert torch.equal(_bits(y), _bits(want_y)), label
        assert torch.equal(_bits(s), _bits(want_s)), label
        assert torch.equal(_bits(_lib.add_layernorm_h16(aa, bb, gamma, beta, 1e-5, dtype)), _bits(want_y)), label
    assert bool(torch.isfinite(want_y).all())


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_without_b(dtype, D, rows):
    from whisperx_amd import _lib

    a, _, gamma, beta = _inputs(dtype, D, rows)
    want_y, want_s = _lib.add_layernorm(a, torch.zeros_like(a), gamma, beta, 1e-5, want_sum=True)
    y, s = _lib.add_layernorm_h16(_strided(a, float("nan")), None, gamma, beta, 1e-5, dtype, want_sum=True)
    assert torch.equal(_bits(y), _bits(want_y.to(dtype)))
    assert torch.equal(_bits(s), _bits(want_s))


def test_validation():
    """wx_add_layernorm's validation order, with the dtype checked beside D; legal pointers only."""
    import ctypes

    from whisperx_amd import _lib

    lib = _lib.load()
    D, rows = 256, 4
    a = torch.zeros((rows, D), device="cuda")
    b = torch.zeros((rows, D), dtype=torch.float16, device="cuda")
    y = torch.full((rows, D), 7.0, dtype=torch.float16, device="cuda")
    g = torch.ones(D, device="cuda")
    P = {"a": a.data_ptr(), "b": b.data_ptr(), "gamma": g.data_ptr(), "beta": g.data_ptr(), "y": y.data_ptr(), "sum": 0}

    def call(rows=rows, D=D, sa=D, sb=D, dtype=1, **ptr):
        p = {k: ctypes.c_void_p(v) if v else None for k, v in {**P, **ptr}.items()}
        return lib.wx_add_layernorm_h16(p["a"], p["b"], rows, D, sa, sb, p["gamma"], p["beta"], 1e-5, dtype, p["y"],
                                        p["sum"], None)

    INVALID = 1001
    assert call(rows=-1) == INVALID and call(D=320) == INVALID and call(dtype=0) == INVALID and call(dtype=3) == INVALID
    assert call(rows=0, a=0, y=0) == 0
    for name in ("a", "gamma", "beta", "y"):
        assert call(**{name: 0}) == INVALID
    for name in ("a", "b", "gamma", "beta", "y"):
        assert call(**{name: P[name] + 8}) == INVALID
    assert call(sum=a.data_ptr() + 8) == INVALID
    assert call(sa=D - 4) == INVALID and call(sa=D + 2) == INVALID and call(sb=D - 8) == INVALID and call(sb=D + 4) == INVALID
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert call() == 0 and call(b=0) == 0

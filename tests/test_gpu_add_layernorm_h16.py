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


@pytest.mark.parametrize("entry", ("wx_add_layernorm", "wx_add_layernorm_h16", "wx_add_layernorm_h16_dual"))
def test_validation(entry):
    """The validation the three entry points share, in wx_add_layernorm's order, each with its own rules:
    wx_add_layernorm needs b (rows at a multiple of 4 floats) and y; the 16-bit ones check the dtype
    beside D, take a null b (rows at a multiple of 8 elements) and need the 16-bit y; _dual's y32 may be
    null.  Legal pointers only, and nothing is written by a refused call."""
    import ctypes

    from whisperx_amd import _lib

    lib = _lib.load()
    half, dual = entry != "wx_add_layernorm", entry == "wx_add_layernorm_h16_dual"
    outs = ("y32", "y16") if dual else ("y16",) if half else ("y32",)
    D, rows = 256, 4
    a = torch.zeros((rows, D), device="cuda")
    b = torch.zeros((rows, D), dtype=torch.float16 if half else torch.float32, device="cuda")
    y32 = torch.full((rows, D), 7.0, device="cuda")
    y16 = torch.full((rows, D), 7.0, dtype=torch.float16, device="cuda")
    s = torch.full((rows, D), 7.0, device="cuda")
    g = torch.ones(D, device="cuda")
    P = {"a": a.data_ptr(), "b": b.data_ptr(), "gamma": g.data_ptr(), "beta": g.data_ptr(), "y32": y32.data_ptr(),
         "y16": y16.data_ptr(), "sum": 0}

    def call(rows=rows, D=D, sa=D, sb=D, dtype=1, **ptr):
        p = {k: ctypes.c_void_p(v) if v else None for k, v in {**P, **ptr}.items()}
        return getattr(lib, entry)(p["a"], p["b"], rows, D, sa, sb, p["gamma"], p["beta"], 1e-5,
                                   *((dtype,) if half else ()), *(p[o] for o in outs), p["sum"], None)

    INVALID = 1001
    assert call(rows=-1) == INVALID and call(D=320) == INVALID
    if half:
        assert call(dtype=0) == INVALID and call(dtype=3) == INVALID and call(rows=0, dtype=0) == INVALID
    assert call(rows=0, a=0, **{o: 0 for o in outs}) == 0
    for name in ("a", "gamma", "beta") + (("y16",) if half else ("b", "y32")):
        assert call(**{name: 0}) == INVALID, name
    for name in ("a", "b", "gamma", "beta") + outs:
        assert call(**{name: P[name] + 8}) == INVALID, name
    assert call(sum=s.data_ptr() + 8) == INVALID
    assert call(sa=D - 4) == INVALID and call(sa=D + 2) == INVALID
    for sb in (D - 8, D + 4) if half else (D - 4, D + 2):  # too short; rows of b that are not 16-byte aligned
        assert call(sb=sb) == INVALID, sb
    torch.cuda.synchronize()
    assert bool((y32 == 7.0).all()) and bool((y16 == 7.0).all()) and bool((s == 7.0).all())
    assert call() == 0 and call(sum=s.data_ptr()) == 0
    for name in (("b",) if half else ()) + (("y32",) if dual else ()):  # the optional pointers
        assert call(**{name: 0}) == 0, name

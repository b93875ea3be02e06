"""wx_add_layernorm, wx_add_layernorm_h16 and wx_add_layernorm_h16_dual on the GPU under the probes of
layernorm_probes.py: inputs whose LayerNorm is exact in fp32, at zero tolerance (y32, its rounding y16
and the sum; every width, rows 1 / 5 / 67, every split of the row between a and b, contiguous and
row-strided with NaN between and behind the rows), and an fp64 bound on rows with a large mean."""
import pytest
import torch

import layernorm_probes as lp
import whisper_half_helpers as hh

pytestmark = pytest.mark.gpu

LAYOUTS = ("contiguous", "strided")


def _place(t, layout):
    t = t.cuda()
    return t if layout == "contiguous" else lp.strided(t, float("nan"))


@pytest.mark.parametrize("rows", lp.ROWS)
@pytest.mark.parametrize("D", lp.WIDTHS)
@pytest.mark.parametrize("kind", lp.KINDS)
def test_exact_probes(kind, D, rows):
    from whisperx_amd import _lib

    p = lp.exact(kind, D, rows)
    gamma, beta = p.gamma.cuda(), p.beta.cuda()
    for layout in LAYOUTS:
        for label, a, b in p.splits:
            label = f"{label}, {layout}"
            ad, bd = _place(a, layout), _place(b, layout)
            assert layout == "contiguous" or (ad.stride(0) == D + 8 and bool(torch.isnan(ad._base).any()))
            y, s = _lib.add_layernorm(ad, bd, gamma, beta, p.eps, want_sum=True)
            p.check(y32=y.cpu(), s=s.cpu(), label="wx_add_layernorm, " + label)
        for dtype in hh.DTYPES:
            runs = [(lb, a, b.to(dtype)) for lb, a, b in p.splits16] + [("a = v, no b", p.sum, None)]
            for label, a, b in runs:
                label = f"{hh.name(dtype)}, {label}, {layout}"
                ad, bd = _place(a, layout), None if b is None else _place(b, layout)
                y16, s = _lib.add_layernorm_h16(ad, bd, gamma, beta, p.eps, dtype, want_sum=True)
                p.check(y16=y16.cpu(), s=s.cpu(), label="wx_add_layernorm_h16, " + label)
                y32, y16, s = _lib.add_layernorm_h16_dual(ad, bd, gamma, beta, p.eps, dtype, want_sum=True)
                p.check(y32=y32.cpu(), y16=y16.cpu(), s=s.cpu(), label="wx_add_layernorm_h16_dual, " + label)
                none, y16 = _lib.add_layernorm_h16_dual(ad, bd, gamma, beta, p.eps, dtype, want_y32=False)
                assert none is None
                p.check(y16=y16.cpu(), label="wx_add_layernorm_h16_dual without y32, " + label)


@pytest.mark.parametrize("entry", ["f32", "float16", "bfloat16"])
@pytest.mark.parametrize("D", lp.WIDTHS)
def test_bounded_check(D, entry):
    """a = 50 + 2 randn: |y - fp64| <= 4 x ref_err (torch's fp32 layer_norm on the CPU); the 16-bit
    entries' fp32 y on their own b."""
    from whisperx_amd import _lib

    dtype = None if entry == "f32" else getattr(torch, entry)
    a, b, gamma, beta, eps, want, ref_err = lp.bounded(D, 67, dtype)
    ad, gd, td = a.cuda(), gamma.cuda(), beta.cuda()
    if dtype is None:
        y = _lib.add_layernorm(ad, b.cuda(), gd, td, eps)
    else:
        y, y16 = _lib.add_layernorm_h16_dual(ad, b.to(dtype).cuda(), gd, td, eps, dtype)
        assert torch.equal(y16, y.to(dtype))
    err = float((y.cpu().double() - want).abs().max())
    print(f"add_layernorm {entry} D {D}: |kernel - fp64| {err:.3e}, ref_err {ref_err:.3e}, err / (4 x ref_err) "
          f"{err / (4 * ref_err):.3f}")
    assert err <= 4 * ref_err

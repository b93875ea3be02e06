"""The two elementwise kernels of the emission producer's half route at zero tolerance against the
entries they extend: wx_add_layernorm_h16_dual (both forms of one norm) against wx_add_layernorm
and wx_add_layernorm_h16, wx_conv0_channel_norm_h16 against the rounding of wx_conv0_channel_norm."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("with_b", [True, False], ids=["b", "null_b"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_add_layernorm_dual(dtype, with_b):
    from whisperx_amd import _lib
    from whisperx_amd.emission import _ADDLN_WIDTHS

    for D in _ADDLN_WIDTHS:
        for rows in (1, 5, 97):
            g = torch.Generator().manual_seed(1000 * D + rows)
            a = (2.0 * torch.randn((rows, D), generator=g) + 0.5).cuda()
            b = torch.randn((rows, D), generator=g).to(dtype).cuda() if with_b else None
            gamma = (1.0 + 0.1 * torch.randn(D, generator=g)).cuda()
            beta = (0.1 * torch.randn(D, generator=g)).cuda()
            b32 = b.float() if with_b else torch.zeros_like(a)
            want32, want_sum = _lib.add_layernorm(a, b32, gamma, beta, 1e-5, want_sum=True)
            want16 = _lib.add_layernorm_h16(a, b, gamma, beta, 1e-5, dtype)
            y32, y16, s = _lib.add_layernorm_h16_dual(a, b, gamma, beta, 1e-5, dtype, want_sum=True)
            assert y32.dtype == torch.float32 and y16.dtype == dtype and s.dtype == torch.float32
            assert torch.equal(_bits(y32), _bits(want32)), (D, rows)
            assert torch.equal(_bits(s), _bits(want_sum)), (D, rows)
            assert torch.equal(_bits(y16), _bits(want16)), (D, rows)
            assert torch.equal(_bits(y16), _bits(want32.to(dtype))), (D, rows)  # (its rounding to nearest even)
            none32, only16 = _lib.add_layernorm_h16_dual(a, b, gamma, beta, 1e-5, dtype, want_y32=False)
            assert none32 is None and torch.equal(_bits(only16), _bits(want16)), (D, rows)


def test_add_layernorm_dual_validation():
    from whisperx_amd import _lib

    a = torch.randn((4, 320), device="cuda")
    w = torch.ones(320, device="cuda")
    with pytest.raises(_lib.WXError):  # a width the kernels do not take
        _lib.add_layernorm_h16_dual(a, None, w, w, 1e-5, torch.float16)
    a = torch.randn((4, 256), device="cuda")
    w = torch.ones(256, device="cuda")
    with pytest.raises(_lib.WXError):
        _lib.add_layernorm_h16_dual(a, None, w, w, 1e-5, torch.float32)
    with pytest.raises(_lib.WXError):
        _lib.add_layernorm_h16_dual(a, a.to(torch.bfloat16), w, w, 1e-5, torch.float16)
    y32, y16 = _lib.add_layernorm_h16_dual(a[:0], None, w, w, 1e-5, torch.float16)
    assert y32.shape == (0, 256) and y16.shape == (0, 256)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("S,C", [(400, 8), (405, 512), (16123, 512)])
def test_conv0_channel_norm_h16(S, C, dtype):
    """K 10, stride 5 (wav2vec2's layer 0), with and without bias and GELU: the fp32 entry's output
    rounded to the type, bit for bit."""
    from whisperx_amd import _lib

    g = torch.Generator().manual_seed(S + C)
    x = (0.1 * torch.randn(S, generator=g)).cuda()
    w = (0.3 * torch.randn((C, 1, 10), generator=g)).cuda()
    bias = torch.randn(C, generator=g).cuda()
    gamma = (1.0 + 0.1 * torch.randn(C, generator=g)).cuda()
    beta = (0.1 * torch.randn(C, generator=g)).cuda()
    L = (S - 10) // 5 + 1
    for b in (bias, None):
        for gelu in (True, False):
            want = _lib.conv0_channel_norm(x, w, b, 5, gamma, beta, 1e-5, gelu)
            got = _lib.conv0_channel_norm_h16(x, w, b, 5, gamma, beta, 1e-5, gelu, dtype)
            assert got.shape == (L, C) and got.dtype == dtype
            assert torch.equal(_bits(got), _bits(want.to(dtype))), (b is not None, gelu)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_conv0_channel_norm_h16_other_geometry(dtype):
    """Another (K, stride) takes the generic kernels: the same contract."""
    from whisperx_amd import _lib

    g = torch.Generator().manual_seed(5)
    S, C, K, st = 1003, 12, 7, 3
    x = (0.1 * torch.randn(S, generator=g)).cuda()
    w = (0.3 * torch.randn((C, 1, K), generator=g)).cuda()
    gamma = (1.0 + 0.1 * torch.randn(C, generator=g)).cuda()
    beta = (0.1 * torch.randn(C, generator=g)).cuda()
    want = _lib.conv0_channel_norm(x, w, None, st, gamma, beta, 1e-5, True)
    got = _lib.conv0_channel_norm_h16(x, w, None, st, gamma, beta, 1e-5, True, dtype)
    assert torch.equal(_bits(got), _bits(want.to(dtype)))
    with pytest.raises(_lib.WXError):
        _lib.conv0_channel_norm_h16(x, w, None, st, gamma, beta, 1e-5, True, torch.float32)

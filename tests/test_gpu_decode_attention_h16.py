"""wx_decode_attention_h16 and wx_decode_attention_h16_grouped on the GPU, fp16 and bf16.

The kernels' contract is that o equals wx_decode_attention_f32 on the widened inputs, rounded once to
the type, bit for bit, and that the grouped kernel has the ungrouped one's bits for every query: the
fp32 kernels (probed by test_gpu_whisper_decoder.py / test_gpu_whisper_beam.py) are a zero-tolerance
oracle.  Beside it: an fp64 bound on the rounded inputs,
    |o - o64| <= HALF_ULP[dtype] |o64| + 4 ref_err32 + 2^-25
(one rounding; the fp32 kernel's rule with ref_err32 = max|torch fp32 CPU attention - fp64| on the
same inputs; half an fp16 subnormal step), the exact probes of whisper_half_helpers, NaN where the
kernels must not read, independence of the batch and of the other beams, and the argument checks."""
import ctypes

import pytest
import torch

import attention_probes as ap
import whisper_half_helpers as hh
from whisper_decoder_helpers import attention_inputs, attention_ref

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 257, 448, 1500]
GROUPED_LENGTHS = [1, 2, 127, 128, 129, 257, 1500]
GROUPS = [1, 2, 5, 8]
SHAPES = [(1, 1), (3, 6), (2, 20)]
WX_E_INVALID, WX_E_WORKSPACE = 1001, 1004
CODE = {torch.float16: 1, torch.bfloat16: 2}


def _bits(t):
    return t.contiguous().view(torch.int16)


def _inputs(dtype, B, H, L, kv_scale=1.0):
    q, k, v = attention_inputs(B, H, L)
    return q.to(dtype), (k * kv_scale).to(dtype), (v * kv_scale).to(dtype)


def _cache_views(k, v, L, fill=0.0):
    """k / v [B, H, L, 64] as views [B, H, L + 5, 64] of wider buffers full of `fill` (the rows at and
    past L and the 8 columns of padding of every row too): batch, head and row strides all differ
    from the packed ones and are multiples of 8."""
    B, H = k.shape[:2]
    views = []
    for t in (k, v):
        wide = torch.full((B + 1, H + 1, L + 7, 72), fill, dtype=t.dtype, device="cuda")
        view = wide[:B, :H, 1:6 + L, 8:72]
        view[:, :, :L] = t.cuda()
        assert view.stride(-1) == 1 and view.stride(2) == 72 and not view.is_contiguous()
        views.append(view)
    return views


def _cross_views(k, v, L):
    """k / v as the two halves of one [B, L, 2 H 64] tensor: row stride 2 H 64, head stride 64."""
    B, H = k.shape[:2]
    kv = torch.cat([k.transpose(1, 2).reshape(B, L, H * 64), v.transpose(1, 2).reshape(B, L, H * 64)], -1).cuda()
    return [kv[:, :, j * H * 64:(j + 1) * H * 64].view(B, L, H, 64).transpose(1, 2) for j in range(2)]


def _strided(q, fill=0.0):
    """q [..., H, 64] as a view of rows 72 elements apart with `fill` between them."""
    shape = list(q.shape)
    wide = torch.full(shape[:-2] + [shape[-2] + 1, 72], fill, dtype=q.dtype, device="cuda")
    view = wide[..., :shape[-2], 8:72]
    view.copy_(q.cuda())
    assert view.stride(-1) == 1 and view.stride(-2) == 72
    return view


def _f32_rounded(q, k, v, L, dtype):
    """The oracle: the fp32 kernel on the widened views, rounded to dtype."""
    from whisperx_amd import _lib

    return _lib.decode_attention_f32(q.float(), k.float(), v.float(), hh.SCALE, L=L).to(dtype)


@pytest.mark.parametrize("B,H", SHAPES)
@pytest.mark.parametrize("layout", ["cache", "cross"])
@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
def test_equals_the_fp32_kernel_and_is_near_fp64(dtype, layout, B, H):
    from whisperx_amd import _lib

    for L in LENGTHS:
        q, k, v = _inputs(dtype, B, H, L)
        kv_, vv_ = _cache_views(k, v, L, 1e4) if layout == "cache" else _cross_views(k, v, L)
        full = torch.full((B + 2, H, 64), 1e4, dtype=dtype, device="cuda")
        got = _lib.decode_attention_h16(q.cuda(), kv_, vv_, hh.SCALE, L=L, out=full[1:B + 1])
        want = _f32_rounded(q.cuda(), kv_, vv_, L, dtype)
        torch.cuda.synchronize()
        assert got.data_ptr() == full[1].data_ptr() and got.dtype == dtype
        assert bool((full[0] == 1e4).all()) and bool((full[B + 1] == 1e4).all())
        assert torch.equal(_bits(got), _bits(want)), L
        # fp64 on the rounded inputs
        o64 = attention_ref(q.double(), k.double(), v.double())
        ref_err32 = float((attention_ref(q.float(), k.float(), v.float()).double() - o64).abs().max())
        err = (got.cpu().double() - o64).abs()
        bound = hh.HALF_ULP[dtype] * o64.abs() + 4 * ref_err32 + 2.0 ** -25
        print(f"decode h16 {hh.name(dtype)} {layout} B {B} H {H} L {L}: |kernel - fp64| max {float(err.max()):.3e}, "
              f"ref_err32 {ref_err32:.3e}, largest err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), L


@pytest.mark.parametrize("B,H", SHAPES)
def test_subnormal_keys_and_values_fp16(B, H):
    """k and v scaled by 2^-14: most of them are fp16 subnormals, and so are the outputs."""
    from whisperx_amd import _lib

    dtype = torch.float16
    for L in LENGTHS:
        q, k, v = _inputs(dtype, B, H, L, 2.0 ** -14)
        sub = [float(((t.float().abs() < 2.0 ** -14) & (t != 0)).float().mean()) for t in (k, v)]
        assert sub[0] > 0.2 and sub[1] > 0.6 or L < 63, sub # (|3 x| < 1: 26 %, |x| < 1: 68 % of a normal)
        kv_, vv_ = _cross_views(k, v, L)
        got = _lib.decode_attention_h16(q.cuda(), kv_, vv_, hh.SCALE, L=L)
        want = _f32_rounded(q.cuda(), kv_, vv_, L, dtype)
        assert torch.equal(_bits(got), _bits(want)), L
        assert bool((got != 0).any())


@pytest.mark.parametrize("L", [1, 2, 128, 129, 1500])
@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
def test_permutation(dtype, L):
    """The L queries are batch entries over one k / v (batch stride 0), H = 1: o[i] = v[pi(i)] exactly."""
    from whisperx_amd import _lib

    for kind in ("random", "reversal"):
        p = hh.Permutation(dtype, 1, L, kind)
        for layout in ("cache", "cross"):
            views = _cache_views(p.k[None], p.v[None], L, 1e4) if layout == "cache" else _cross_views(p.k[None], p.v[None], L)
            kv_, vv_ = (t.expand(L, -1, -1, -1) for t in views)
            assert kv_.stride(0) == 0 or L == 1
            got = _lib.decode_attention_h16(p.q[0][:, None].contiguous().cuda(), kv_, vv_, hh.SCALE, L=L)
            assert torch.equal(_bits(got.cpu()[:, 0]), _bits(p.want[0])), (kind, layout)
        print(f"decode h16 permutation {hh.name(dtype)} {kind} L {L}: margin {p.margin:.1f}")


@pytest.mark.parametrize("L", [64, 128, 256, 1024])
@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
def test_uniform(dtype, L):
    """q = 0, integer v: o is the exact mean; in fp16 once more with v x 2^-22 (subnormal values and
    means), against torch's rounding of the exact mean."""
    from whisperx_amd import _lib

    N = 3
    u = hh.Uniform(dtype, N, L)
    assert u.exact
    q, k, v = u.q[:, :1].cuda(), u.k[:, None].cuda(), u.v[:, None].cuda()
    got = _lib.decode_attention_h16(q, k, v, hh.SCALE)
    assert torch.equal(_bits(got.cpu()[:, 0]), _bits(u.want[:, 0].to(dtype)))
    if dtype == torch.float16:
        tiny = (u.v.double() * 2.0 ** -22).to(dtype)
        assert torch.equal(tiny.double(), u.v.double() * 2.0 ** -22)  # exact
        got = _lib.decode_attention_h16(q, k, tiny[:, None].cuda(), hh.SCALE)
        assert torch.equal(_bits(got.cpu()[:, 0]), _bits((u.want[:, 0] * 2.0 ** -22).to(dtype)))


@pytest.mark.parametrize("L", [1, 127, 128, 129, 300])
@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
def test_poison(dtype, L):
    """NaN against zeros in the cache rows at and past L, in the padding of the 72-element rows and
    between the strided query rows: the outputs are finite and equal bit for bit."""
    from whisperx_amd import _lib

    B, G, H = 2, 5, 3
    q, k, v = _inputs(dtype, B, H, L)
    qg = torch.randn((B, G, H, 64), generator=torch.Generator().manual_seed(L)).to(dtype)

    def run(fill):
        kv_, vv_ = _cache_views(k, v, L, fill)
        return _lib.decode_attention_h16(_strided(q, fill), kv_, vv_, hh.SCALE, L=L).cpu().float()

    def run_grouped(fill):
        kv_, vv_ = _cache_views(k, v, L, fill)
        return _lib.decode_attention_h16_grouped(_strided(qg, fill), kv_, vv_, hh.SCALE, L=L).cpu().float().view(B * G, H, 64)

    ap.check_poison(run)
    ap.check_poison(run_grouped)


@pytest.mark.parametrize("L", [1500, 65])
@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
def test_a_row_does_not_depend_on_the_batch(dtype, L):
    from whisperx_amd import _lib

    q, k, v = (t.cuda() for t in _inputs(dtype, 3, 6, L))
    both = _lib.decode_attention_h16(q, k, v, hh.SCALE)
    for b, h in ((0, 0), (1, 3), (2, 5)):
        alone = _lib.decode_attention_h16(q[b:b + 1, h:h + 1].contiguous(), k[b:b + 1, h:h + 1].contiguous(),
                                          v[b:b + 1, h:h + 1].contiguous(), hh.SCALE)
        assert torch.equal(_bits(alone[0, 0]), _bits(both[b, h])), (b, h)
    assert bool(torch.isfinite(both).all())


def _queries(dtype, B, G, H, L):
    g = torch.Generator().manual_seed(7 + 1000 * L + 10 * H + B + 100000 * G)
    q = torch.randn((B, G, H, 64), generator=g)
    q[:, 0] = attention_inputs(B, H, L)[0]
    return _strided(q.to(dtype))


@pytest.mark.parametrize("B,H", SHAPES)
@pytest.mark.parametrize("layout", ["cache", "cross"])
@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
def test_grouped_equals_the_ungrouped_kernel_per_beam(dtype, layout, B, H):
    from whisperx_amd import _lib

    for L in GROUPED_LENGTHS:
        _, k, v = _inputs(dtype, B, H, L)
        kv_, vv_ = _cache_views(k, v, L, 1e4) if layout == "cache" else _cross_views(k, v, L)
        for G in GROUPS:
            q = _queries(dtype, B, G, H, L)
            full = torch.full((B + 2, G, H, 64), 1e4, dtype=dtype, device="cuda")
            got = _lib.decode_attention_h16_grouped(q, kv_, vv_, hh.SCALE, L=L, out=full[1:B + 1])
            want = torch.stack([_lib.decode_attention_h16(q[:, g].contiguous(), kv_, vv_, hh.SCALE, L=L)
                                for g in range(G)], 1)
            torch.cuda.synchronize()
            assert got.data_ptr() == full[1].data_ptr()
            assert bool((full[0] == 1e4).all()) and bool((full[B + 1] == 1e4).all())
            assert bool(torch.isfinite(got).all())
            assert torch.equal(_bits(got), _bits(want)), (L, G)


@pytest.mark.parametrize("L", [129, 1500, 65])
@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
def test_a_grouped_row_depends_on_neither_the_other_beams_nor_the_batch(dtype, L):
    from whisperx_amd import _lib

    B, G, H = 3, 5, 6
    _, k, v = (t.cuda() for t in _inputs(dtype, B, H, L))
    q = _queries(dtype, B, G, H, L)
    both = _lib.decode_attention_h16_grouped(q, k, v, hh.SCALE)
    other = q.clone()
    other[:, 1:] = (5.0 * torch.randn((B, G - 1, H, 64), generator=torch.Generator().manual_seed(L))).to(dtype).cuda()
    got = _lib.decode_attention_h16_grouped(other, k, v, hh.SCALE)
    assert torch.equal(_bits(got[:, 0]), _bits(both[:, 0])) and not torch.equal(got[:, 1:], both[:, 1:])
    for b in range(B):  # the chunk alone, and one beam of it alone
        alone = _lib.decode_attention_h16_grouped(q[b:b + 1], k[b:b + 1], v[b:b + 1], hh.SCALE)
        assert torch.equal(_bits(alone[0]), _bits(both[b]))
        one = _lib.decode_attention_h16_grouped(q[b:b + 1, 3:4], k[b:b + 1], v[b:b + 1], hh.SCALE)
        assert torch.equal(_bits(one[0, 0]), _bits(both[b, 3]))


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("grouped", [False, True], ids=["ungrouped", "grouped"])
def test_argument_checks(grouped):
    """Every refusal, in the header's order (a refusal of an earlier step wins over a later one's
    cause), with o and the workspace left untouched; B == 0; then the accepted call."""
    from whisperx_amd import _lib

    lib = _lib.load()
    B, G, H, L = 2, 5, 3, 300
    dtype = torch.float16
    q, k, v = (t.cuda() for t in _inputs(dtype, B, H, L))
    if grouped:
        q = q[:, None].expand(B, G, H, 64).contiguous()
        need = lib.wx_decode_attention_grouped_workspace_bytes(B, G, H, L)
    else:
        need = lib.wx_decode_attention_workspace_bytes(B, H, L)
    nq = q.dim() - 1
    o = torch.empty_like(q)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = [(ctypes.c_int64 * n)(*t.stride()[:n]) for t, n in ((q, nq), (k, 3), (v, 3))]

    def arr(a, i, x):
        vals = list(a)
        vals[i] = x
        return (ctypes.c_int64 * len(vals))(*vals)

    def call(B=B, G=G, H=H, L=L, D=64, code=1, qp=_P(q), kp=_P(k), vp=_P(v), op=_P(o), qs=st[0], ks=st[1], vs=st[2],
             wp=_P(ws), wsb=need, stream=None):
        if grouped:
            return lib.wx_decode_attention_h16_grouped(qp, kp, vp, op, B, G, H, L, D, qs, ks, vs, 0.125, code, wp, wsb, stream)
        return lib.wx_decode_attention_h16(qp, kp, vp, op, B, H, L, D, qs, ks, vs, 0.125, code, wp, wsb, stream)

    o.fill_(7.0)
    ws.fill_(9)
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)  # noqa: E731
    # 1: the sizes, the head dim and the dtype, before B == 0
    first = [dict(B=-1), dict(H=0), dict(L=0), dict(D=32), dict(code=0), dict(code=3)]
    if grouped:
        first += [dict(G=0), dict(G=9)]
    for bad in first:
        assert call(**bad) == WX_E_INVALID, bad
        assert call(B=0, **{k_: v_ for k_, v_ in bad.items() if k_ != "B"}) == (WX_E_INVALID if "B" not in bad else 0), bad
    # 2: B == 0 is WX_OK whatever the pointers are
    assert call(B=0, qp=None, kp=None, vp=None, op=None, wp=None, wsb=0) == 0
    # 3: pointers, strides and grid limits, before the workspace size
    third = [dict(qp=None), dict(kp=None), dict(vp=None), dict(op=None), dict(wp=None), dict(qs=None), dict(ks=None),
             dict(vs=None), dict(qp=off(q, 8)), dict(kp=off(k, 8)), dict(vp=off(v, 8)), dict(op=off(o, 8)),
             dict(wp=off(ws, 8)), dict(B=65536), dict(H=65536)]
    third += [dict(qs=arr(st[0], i, st[0][i] + 4)) for i in range(nq)]
    third += [dict(ks=arr(st[1], i, st[1][i] + 4)) for i in range(3)] + [dict(vs=arr(st[2], i, st[2][i] + 4)) for i in range(3)]
    for bad in third:
        assert call(**bad) == WX_E_INVALID, bad
        assert call(wsb=0, **bad) == WX_E_INVALID, bad
    # 4: a short workspace
    assert call(wsb=need - 1) == WX_E_WORKSPACE and call(wsb=0) == WX_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((ws == 9).all())  # nothing was enqueued
    fn = _lib.decode_attention_h16_grouped if grouped else _lib.decode_attention_h16
    want = fn(q, k, v, 0.125)
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(o), _bits(want))
    # a batch stride of 0 (shared k / v) is legal
    assert call(ks=arr(st[1], 0, 0), vs=arr(st[2], 0, 0)) == 0
    torch.cuda.synchronize()
    shared = fn(q, k[:1].expand(B, -1, -1, -1), v[:1].expand(B, -1, -1, -1), 0.125)
    assert torch.equal(_bits(o), _bits(shared)) and torch.equal(_bits(o[0]), _bits(want[0]))
    # the wrappers refuse what the entry points cannot take
    with pytest.raises(_lib.WXError):
        fn(q.float(), k.float(), v.float(), 0.125)
    with pytest.raises(_lib.WXError):
        fn(q, k.to(torch.bfloat16), v, 0.125)


@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
def test_side_stream_gives_the_same_result(dtype):
    from whisperx_amd import _lib

    q, k, v = (t.cuda() for t in _inputs(dtype, 2, 8, 300))
    qg = _queries(dtype, 2, 5, 8, 300)
    want, want_g = _lib.decode_attention_h16(q, k, v, hh.SCALE), _lib.decode_attention_h16_grouped(qg, k, v, hh.SCALE)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, got_g = _lib.decode_attention_h16(q, k, v, hh.SCALE), _lib.decode_attention_h16_grouped(qg, k, v, hh.SCALE)
    side.synchronize()
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(got_g), _bits(want_g))

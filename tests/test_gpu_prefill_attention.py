"""wx_prefill_attention_f32 / wx_prefill_attention_h16 on the GPU.

Accuracy against fp64 over the covering set of prefill_helpers (4 x ref_err, every output finite), on
both layouts the decoder reads in place; the independence the header promises, at zero tolerance (a
row depends on its query, on causal + i and on the K / V rows below that, and on nothing else); the
closed-form probes of attention_probes, the uniform one under the mask; the h16 entry against the
f32 entry on the widened inputs, bit for bit; every refusal."""
import ctypes

import pytest
import torch

import attention_probes as ap
import prefill_helpers as ph
import whisper_half_helpers as hh

pytestmark = pytest.mark.gpu

WX_E_INVALID = 1001
LAYOUTS = ["cache", "cross"]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _q_view(q, fill=0.0):
    """q [B, H, Tq, 64] as the q slice of a fused [B, Tq, 3 H 64] GEMM output whose k and v slots hold `fill`."""
    B, H, Tq, _ = q.shape
    fused = torch.full((B, Tq, 3, H, 64), fill, dtype=q.dtype, device="cuda")
    fused[:, :, 0] = q.transpose(1, 2).cuda()
    return fused[:, :, 0].transpose(1, 2)


def _cache_views(k, v, Tk, fill=0.0):
    """k / v [B, H, Tk, 64] as views [B, H, Tk + 5, 64] of wider buffers full of `fill`: the rows at
    and past Tk and the 8 columns of padding of every row too; no stride is the packed one."""
    B, H = k.shape[:2]
    views = []
    for t in (k, v):
        wide = torch.full((B + 1, H + 1, Tk + 7, 72), fill, dtype=t.dtype, device="cuda")
        view = wide[:B, :H, 1:6 + Tk, 8:72]
        view[:, :, :Tk] = t[:, :, :Tk].cuda()
        views.append(view)
    return views


def _cross_views(k, v, Tk, fill=0.0):
    """k / v as halves of [B, Tk, 2 H 64] tensors (row stride 2 H 64, head stride 64): k the first
    half of one whose other half holds `fill`, v the second half of another."""
    B, H = k.shape[:2]
    views = []
    for j, t in enumerate((k, v)):
        kv = torch.full((B, Tk, 2, H, 64), fill, dtype=t.dtype, device="cuda")
        kv[:, :, j] = t[:, :, :Tk].transpose(1, 2).cuda()
        views.append(kv[:, :, j].transpose(1, 2))
    return views


def _views(layout, k, v, Tk, fill=0.0):
    return _cache_views(k, v, Tk, fill) if layout == "cache" else _cross_views(k, v, Tk, fill)


def _split(t, B, H):
    return t.view(B, H, *t.shape[1:])


def _rows(o):
    """[B, Tq, H, 64] -> [B H, Tq, 64] on the CPU, fp32."""
    B, Tq, H, D = o.shape
    return o.permute(0, 2, 1, 3).reshape(B * H, Tq, D).cpu().float()


def _attend(layout, q, k, v, causal, Tk, B, H, dtype=torch.float32, fill=0.0, kv_scale=1.0):
    """The entry point of `dtype` on [B H, T, 64] CPU inputs through the layout's views -> device o [B, Tq, H, 64]."""
    from whisperx_amd import _lib

    q, k, v = _split(q, B, H).to(dtype), _split(k * kv_scale, B, H).to(dtype), _split(v * kv_scale, B, H).to(dtype)
    kv_, vv_ = _views(layout, k, v, Tk, fill)
    fn = _lib.prefill_attention_f32 if dtype == torch.float32 else _lib.prefill_attention_h16
    return fn(_q_view(q, fill), kv_, vv_, ph.SCALE, causal=causal, Tk=Tk)


# --------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("layout", LAYOUTS)
def test_accuracy_against_fp64(layout):
    for B, H, Tq, Tk, causal in ph.covering():
        q, k, v, want, ref_err = ph.case(B * H, Tq, Tk, causal)
        o = _attend(layout, q, k, v, causal, Tk, B, H)
        assert tuple(o.shape) == (B, Tq, H, 64) and o.is_contiguous()
        ph.check_accuracy(_rows(o), want, ref_err, f"prefill f32 {layout} B {B} H {H} Tq {Tq} Tk {Tk} causal {causal}")


# ----------------------------------------------------------------------- independence
def _direct(q, k, v, causal, Tk=None):
    from whisperx_amd import _lib

    return _lib.prefill_attention_f32(q, k, v, ph.SCALE, causal=causal, Tk=Tk)


@pytest.mark.parametrize("causal", [0, 5, 33])
def test_a_prefix_of_the_queries_gives_the_same_rows(causal):
    B, H, n = 2, 3, 70
    q, k, v = (_split(t, B, H).cuda() for t in ap.random_inputs(B * H, n, causal + n, seed=causal))
    full = _direct(q, k, v, causal)
    assert bool(torch.isfinite(full).all())
    for i in (0, 30, 31, 32, n - 2):
        part = _direct(q[:, :, :i + 1], k, v, causal, Tk=causal + i + 1)
        assert torch.equal(_bits(part), _bits(full[:, :i + 1])), i
        # Tk beyond the row's last key changes nothing either
        assert torch.equal(_bits(_direct(q[:, :, :i + 1], k, v, causal)), _bits(part)), i


@pytest.mark.parametrize("p", [3, 31, 32, 40, 64, 100])
def test_a_position_does_not_depend_on_how_it_is_split(p):
    B, H = 2, 3
    q, k, v = (_split(t, B, H).cuda() for t in ap.random_inputs(B * H, p + 1, p + 1, seed=p))
    a = _direct(q, k, v, 0)[:, p]
    b = _direct(q[:, :, p - 3:], k, v, p - 3)[:, 3]
    assert torch.equal(_bits(a), _bits(b))
    c = _direct(q[:, :, p:], k, v, p)[:, 0]  # and as a single query
    assert torch.equal(_bits(a), _bits(c))


@pytest.mark.parametrize("causal,n", [(5, 33), (0, 65), (33, 40)])
def test_keys_above_a_rows_diagonal_do_not_reach_it(causal, n):
    B, H = 2, 3
    q, k, v = (_split(t, B, H).cuda() for t in ap.random_inputs(B * H, n, causal + n, seed=n))
    full = _direct(q, k, v, causal)
    for i in (0, 1, 26, 27, 31, 32, n - 2):
        if i >= n - 1:
            continue
        k2, v2 = k.clone(), v.clone()
        k2[:, :, causal + i + 1:] = 7.0 * torch.randn_like(k2[:, :, causal + i + 1:])
        v2[:, :, causal + i + 1:] = -3.0 * torch.randn_like(v2[:, :, causal + i + 1:])
        other = _direct(q, k2, v2, causal)
        assert torch.equal(_bits(other[:, :i + 1]), _bits(full[:, :i + 1])), i
        assert not torch.equal(other[:, i + 1:], full[:, i + 1:])


@pytest.mark.parametrize("Tq,Tk,causal", [(33, 38, 5), (65, 98, 33), (1, 1, 0), (33, 78, 5), (2, 133, 100), (33, 129, None),
                                          (65, 1500, None)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_poison(layout, Tq, Tk, causal):
    """NaN against zeros in the K / V rows at and past min(Tk, causal + Tq) (inside Tk and past it),
    in the padding between strided rows, in the other half of the cross tensors and in the k / v
    slots of the fused q/k/v tensor: the outputs are finite and equal bit for bit."""
    B, H = 2, 3
    q, k, v, _, _ = ph.case(B * H, Tq, Tk, causal)
    end = Tk if causal is None else min(Tk, causal + Tq)

    def run(fill):
        k2, v2 = k.clone(), v.clone()
        k2[:, end:], v2[:, end:] = fill, fill
        return _rows(_attend(layout, q, k2, v2, causal, Tk, B, H, fill=fill))

    ap.check_poison(run)


def test_a_row_does_not_depend_on_the_batch():
    B, H, Tq, causal = 3, 6, 40, 5
    q, k, v = (_split(t, B, H).cuda() for t in ap.random_inputs(B * H, Tq, causal + Tq))
    for c in (causal, None):
        both = _direct(q, k, v, c)
        for b, h in ((0, 0), (1, 3), (2, 5)):
            alone = _direct(q[b:b + 1, h:h + 1], k[b:b + 1, h:h + 1], v[b:b + 1, h:h + 1], c)
            assert torch.equal(_bits(alone[0, :, 0]), _bits(both[b, :, h])), (b, h)
        # every G-th row of a cache: a batch stride of 2 rows
        wide = _direct(q[::2], k[::2], v[::2], c)
        assert torch.equal(_bits(wide), _bits(both[::2]))


# ----------------------------------------------------------------------------- probes
@pytest.mark.parametrize("Tq,causal,Tk", [(33, 5, None), (65, 33, None), (1, 0, None), (65, 0, None), (33, 5, 78),
                                          (32, 100, None), (31, 1, None), (2, 31, None), (33, 32, None)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_uniform_under_the_mask(layout, Tq, causal, Tk):
    B, H = 2, 3
    u = ph.MaskedUniform(B * H, Tq, causal, Tk)
    o = _rows(_attend(layout, u.q, u.k, u.v, causal, u.Tk, B, H))
    print(f"uniform {layout} Tq {Tq} causal {causal} Tk {u.Tk}: relative error {u.check(o):.3e}")


@pytest.mark.parametrize("L", [33, 129])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_permutation(layout, L):
    B, H = 2, 2
    for kind in ("random", "reversal"):
        p = ap.Permutation(B * H, L, kind, seed=L)
        err = p.check(_rows(_attend(layout, p.q, p.k, p.v, None, L, B, H)))
        print(f"permutation {layout} {kind} L {L}: margin {p.margin:.1f}, |o - v[pi]| {err:.3e}")


@pytest.mark.parametrize("variant", ["offset", "ramp"])
def test_range(variant):
    B, H, Tq, Tk = 2, 2, 33, 1500
    r = ap.Range(B * H, Tq, Tk, variant, seed=Tk)
    r.check(_rows(_attend("cross", r.q, r.k, r.v, None, Tk, B, H)), "prefill f32")


# -------------------------------------------------------------------------------- h16
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
def test_h16_equals_the_rounded_f32_entry(dtype, layout):
    for B, H, Tq, Tk, causal in ph.covering():
        q, k, v, _, _ = ph.case(B * H, Tq, Tk, causal)
        got = _attend(layout, q, k, v, causal, Tk, B, H, dtype, fill=1e4)
        widened = [t.to(dtype).float() for t in (q, k, v)]
        want = _attend(layout, *widened, causal, Tk, B, H, fill=1e4).to(dtype)
        assert got.dtype == dtype and bool(torch.isfinite(got).all())
        assert torch.equal(_bits(got), _bits(want)), (B, H, Tq, Tk, causal)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_h16_subnormal_keys_and_values_fp16(layout):
    dtype, s = torch.float16, 2.0 ** -14
    nonzero = False
    for B, H, Tq, Tk, causal in ph.covering():
        q, k, v, _, _ = ph.case(B * H, Tq, Tk, causal)
        got = _attend(layout, q, k, v, causal, Tk, B, H, dtype, kv_scale=s)
        widened = [q.to(dtype).float(), (k * s).to(dtype).float(), (v * s).to(dtype).float()]
        want = _attend(layout, *widened, causal, Tk, B, H).to(dtype)
        assert torch.equal(_bits(got), _bits(want)), (B, H, Tq, Tk, causal)
        nonzero = nonzero or bool((got != 0).any())
    assert nonzero


# -------------------------------------------------------------------------- refusals
def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("half", [False, True], ids=["f32", "h16"])
def test_argument_checks(half):
    """Every refusal in the header's order (an earlier step's refusal wins over a later one's cause),
    with o untouched; B == 0; then the accepted call."""
    from whisperx_amd import _lib

    lib = _lib.load()
    dtype = torch.float16 if half else torch.float32
    B, H, Tq, Tk, causal = 2, 3, 40, 45, 5
    mult = 8 if half else 4
    q, k, v = (_split(t, B, H).to(dtype).cuda() for t in ap.random_inputs(B * H, Tq, Tk))
    o = torch.empty((B, Tq, H, 64), dtype=dtype, device="cuda")
    st = [(ctypes.c_int64 * 3)(*t.stride()[:3]) for t in (q, k, v)]

    def arr(a, i, x):
        vals = list(a)
        vals[i] = x
        return (ctypes.c_int64 * 3)(*vals)

    def call(B=B, H=H, Tq=Tq, Tk=Tk, causal=causal, D=64, code=1, qp=_P(q), kp=_P(k), vp=_P(v), op=_P(o), qs=st[0],
             ks=st[1], vs=st[2], stream=None):
        if half:
            return lib.wx_prefill_attention_h16(qp, kp, vp, op, B, H, Tq, Tk, causal, D, qs, ks, vs, 0.125, code, stream)
        return lib.wx_prefill_attention_f32(qp, kp, vp, op, B, H, Tq, Tk, causal, D, qs, ks, vs, 0.125, stream)

    o.fill_(7.0)
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)  # noqa: E731
    # 1: the sizes, the head dim and the dtype, before B == 0
    first = [dict(B=-1), dict(H=0), dict(Tq=0), dict(Tk=0), dict(Tq=-1), dict(Tk=-1), dict(D=32)]
    if half:
        first += [dict(code=0), dict(code=3)]
    for bad in first:
        assert call(**bad) == WX_E_INVALID, bad
        assert call(B=0, **{k_: v_ for k_, v_ in bad.items() if k_ != "B"}) == (WX_E_INVALID if "B" not in bad else 0), bad
    # 2: B == 0 is WX_OK whatever the pointers are
    assert call(B=0, qp=None, kp=None, vp=None, op=None, qs=None) == 0
    # 3: pointers, strides and the grid limit
    third = [dict(qp=None), dict(kp=None), dict(vp=None), dict(op=None), dict(qs=None), dict(ks=None), dict(vs=None),
             dict(qp=off(q, 8)), dict(kp=off(k, 8)), dict(vp=off(v, 8)), dict(op=off(o, 8))]
    for i in range(3):
        third += [dict(qs=arr(st[0], i, st[0][i] + mult // 2)), dict(ks=arr(st[1], i, st[1][i] + mult // 2)),
                  dict(vs=arr(st[2], i, st[2][i] + mult // 2))]
    third += [dict(ks=arr(st[1], 2, -64)), dict(vs=arr(st[2], 2, -64)), dict(ks=arr(st[1], 2, 2 ** 23 + 64)),
              dict(vs=arr(st[2], 2, 2 ** 23 + 64))]
    third += [dict(B=2 ** 20, H=2 ** 11, Tq=1), dict(B=2 ** 16, H=2 ** 14, Tq=33)]  # 2^31 workgroups
    for bad in third:
        assert call(**bad) == WX_E_INVALID, bad
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())  # nothing was enqueued
    fn = _lib.prefill_attention_h16 if half else _lib.prefill_attention_f32
    want = fn(q, k, v, 0.125, causal=causal)
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(o), _bits(want))
    # any negative causal is "no mask"; a batch stride of 0 (shared k / v) is legal
    assert call(causal=-7) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(o), _bits(fn(q, k, v, 0.125)))
    assert call(ks=arr(st[1], 0, 0), vs=arr(st[2], 0, 0)) == 0
    torch.cuda.synchronize()
    shared = fn(q, k[:1].expand(B, -1, -1, -1), v[:1].expand(B, -1, -1, -1), 0.125, causal=causal)
    assert torch.equal(_bits(o), _bits(shared)) and torch.equal(_bits(o[0]), _bits(want[0]))
    # the wrappers refuse what the entry points cannot take
    other = torch.float32 if half else torch.float16
    for bad in ((q.to(other), k.to(other), v.to(other)), (q, k.to(torch.bfloat16), v), (q[0], k, v), (q, k[:, :, :, :32], v),
                (q, k, v[:1]), (q.cpu(), k, v)):
        with pytest.raises(_lib.WXError):
            fn(*bad, 0.125)
    for kw in (dict(Tk=0), dict(Tk=Tk + 1), dict(causal=-2)):
        with pytest.raises(_lib.WXError):
            fn(q, k, v, 0.125, **kw)


def test_side_stream_gives_the_same_result():
    B, H, Tq, causal = 2, 8, 70, 5
    q, k, v = (_split(t, B, H).cuda() for t in ap.random_inputs(B * H, Tq, causal + Tq))
    want = _direct(q, k, v, causal)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _direct(q, k, v, causal)
    side.synchronize()
    assert torch.equal(_bits(got), _bits(want))

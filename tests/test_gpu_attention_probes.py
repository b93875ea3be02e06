"""The three attention entry points under the probes of tests/attention_probes.py (-m gpu):
wx_attention_f32, wx_attention_f32_packed (every wave split) and wx_decode_attention_f32 (both
layouts) against closed-form expectations (permutation: o[i] = v[pi(i)]; uniform: o = sum(v) / L),
against an fp64 softmax at scores up to +-300 within 4 x ref_err (ref_err: fp32 torch on the same
inputs, printed), and with NaN against zeros in all the memory a call must not depend on.

Self-attention reads q, k and v as views of one fused [B, T + 32, 3 H 64] projection buffer whose 32
spare rows per batch entry are the poison area: a read past the last key lands in the test's own
tensor."""
import functools

import pytest
import torch

import attention_probes as ap

pytestmark = pytest.mark.gpu

SENTINEL = 1e4
HD = ap.D


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


# -------------------------------------------------------------------------- wx_attention_f32
def _fused_views(B, H, T, fill):
    """q, k, v [B, H, T, 64] views of one [B, T + 32, 3 H 64] buffer full of `fill`."""
    buf = torch.full((B, T + 32, 3 * H * HD), fill, device="cuda")
    return [buf[:, :T, i * H * HD:(i + 1) * H * HD].view(B, T, H, HD).transpose(1, 2) for i in range(3)]


def _self_attend(B, H, fill=0.0):
    def attend(q, k, v):
        from whisperx_amd import _lib

        T = q.shape[1]
        views = _fused_views(B, H, T, fill)
        for view, x in zip(views, (q, k, v)):
            view.copy_(x.view(B, H, T, HD))
        got = _lib.attention_f32(*views, ap.SCALE)  # [B, T, H, 64]
        assert got.shape == (B, T, H, HD)
        return got.permute(0, 2, 1, 3).reshape(B * H, T, HD).cpu()

    return attend


SELF_SHAPES = [(2, 2, T) for T in (1, 31, 32, 33, 64, 96, 127, 128, 129, 160)] + [(1, 20, 1500), (1, 6, 1500)]


@pytest.mark.parametrize("B,H,T", SELF_SHAPES)
def test_attention_f32_permutation(B, H, T):
    attend = _self_attend(B, H)
    for kind in ap.KINDS:
        p = ap.Permutation(B * H, T, kind, seed=T)
        err = p.check(attend(p.q, p.k, p.v))
        print(f"attention_f32 permutation {kind} B {B} H {H} T {T}: margin {p.margin:.1f}, |o - v[pi]| max {err:.1e}")


@pytest.mark.parametrize("B,H,T", SELF_SHAPES)
def test_attention_f32_uniform(B, H, T):
    p = ap.Uniform(B * H, T, T, seed=T)
    rel = p.check(_self_attend(B, H)(p.q, p.k, p.v))
    print(f"attention_f32 uniform B {B} H {H} T {T}: relative error {rel:.2e}, bound {2.0 ** -22:.2e}")


@pytest.mark.parametrize("variant", ["offset", "ramp"])
@pytest.mark.parametrize("T", [33, 129, 1500])
def test_attention_f32_range(T, variant):
    p = ap.Range(4, T, T, variant, seed=T)
    p.check(_self_attend(2, 2)(p.q, p.k, p.v), "attention_f32")


@pytest.mark.parametrize("T", [1, 33, 97, 1500])
def test_attention_f32_poison(T):
    """The 32 spare rows behind every batch entry's q, k and v hold NaN against zeros."""
    q, k, v = ap.random_inputs(4, T, T, seed=T)
    ap.check_poison(lambda fill: _self_attend(2, 2, fill)(q, k, v))


# ------------------------------------------------------------------- wx_attention_f32_packed
PACKED_LENGTHS = [33, 5, 97, 1, 64, 130, 1500, 32]
PACKED_H = 2
PACKED_POISONED = (1, 3, len(PACKED_LENGTHS) - 1)  # 5 rows, 1 row, and a whole tile at the end


def _packed_attend(split, poisoned=(), fill=0.0):
    """attend over the per-segment q / k / v lists ([H, T_s, 64] each): one packed call on views of a
    fused [1, rows, 3 H 64] buffer; the `poisoned` segments' rows hold `fill` in q, k and v."""

    def attend(qs, ks, vs):
        from whisperx_amd import _lib

        segs = _lib.PackedSegments(PACKED_LENGTHS)
        H, R = PACKED_H, segs.rows
        qkv = torch.empty((1, R, 3 * H * HD), device="cuda")
        views = [qkv[..., i * H * HD:(i + 1) * H * HD].view(1, R, H, HD).transpose(1, 2) for i in range(3)]
        for view, xs in zip(views, (qs, ks, vs)):
            view[0].copy_(torch.cat(xs, 1))
        for s in poisoned:
            qkv[:, segs.offsets[s]:segs.offsets[s + 1]] = fill
        got = _lib.attention_f32_packed(*views, ap.SCALE, segs, split)  # [1, rows, H, 64]
        assert got.shape == (1, R, H, HD)
        got = got[0].permute(1, 0, 2).cpu()
        return [got[:, a:b] for a, b in zip(segs.offsets[:-1], segs.offsets[1:])]

    return attend


@functools.lru_cache(maxsize=None)
def _packed_probes(which, arg=None):
    """One probe per segment, each with its own seed (and permutation), shared by the splits."""
    if which == "permutation":
        return [ap.Permutation(PACKED_H, T, arg, seed=100 + s) for s, T in enumerate(PACKED_LENGTHS)]
    if which == "uniform":
        return [ap.Uniform(PACKED_H, T, T, seed=100 + s) for s, T in enumerate(PACKED_LENGTHS)]
    return [ap.Range(PACKED_H, T, T, arg, seed=100 + s) for s, T in enumerate(PACKED_LENGTHS)]


def _run_packed(split, probes):
    return _packed_attend(split)([p.q for p in probes], [p.k for p in probes], [p.v for p in probes])


@pytest.mark.parametrize("split", [0, 1, 2, 4])
def test_attention_f32_packed_permutation(split):
    for kind in ap.KINDS:
        probes = _packed_probes("permutation", kind)
        errs = [p.check(o) for p, o in zip(probes, _run_packed(split, probes))]
        print(f"attention_f32_packed split {split} permutation {kind}: margin {min(p.margin for p in probes):.1f}, "
              f"|o - v[pi]| max {max(errs):.1e}")


@pytest.mark.parametrize("split", [0, 1, 2, 4])
def test_attention_f32_packed_uniform(split):
    probes = _packed_probes("uniform")
    rel = [p.check(o) for p, o in zip(probes, _run_packed(split, probes))]
    print(f"attention_f32_packed split {split} uniform: relative error {max(rel):.2e}, bound {2.0 ** -22:.2e}")


@pytest.mark.parametrize("variant", ["offset", "ramp"])
@pytest.mark.parametrize("split", [0, 1, 2, 4])
def test_attention_f32_packed_range(split, variant):
    probes = _packed_probes("range", variant)
    out = _run_packed(split, probes)
    failures = []
    for s, (p, o) in enumerate(zip(probes, out)):
        try:
            p.check(o, f"attention_f32_packed split {split} segment {s}")
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, failures


@pytest.mark.parametrize("split", [0, 1, 2, 4])
def test_attention_f32_packed_poison(split):
    """Segments 1, 3 and the last hold NaN against zeros in q, k and v: the other segments' rows are
    finite and bit-equal (the poisoned segments' own rows are not asserted)."""
    qkv = [ap.random_inputs(PACKED_H, T, T, seed=200 + s) for s, T in enumerate(PACKED_LENGTHS)]
    qs, ks, vs = ([x[i] for x in qkv] for i in range(3))

    def run(fill):
        out = _packed_attend(split, PACKED_POISONED, fill)(qs, ks, vs)
        return torch.cat([o for s, o in enumerate(out) if s not in PACKED_POISONED], 1)

    ap.check_poison(run)


# ------------------------------------------------------------------- wx_decode_attention_f32
DECODE_LENGTHS = [1, 2, 16, 17, 127, 128, 129, 257, 1500]
LAYOUTS = ["cache", "cross"]


def _cache_views(k, v, L, fill=SENTINEL):
    """k / v [B, H, L, 64] as views [B, H, L + 5, 64] of wider buffers full of `fill` (the rows at and
    past L too): batch, head and row strides all differ from the packed ones."""
    B, H = k.shape[:2]
    Lcap = L + 5
    views = []
    for t in (k, v):
        wide = torch.full((B + 1, H + 1, Lcap + 2, 72), fill, device="cuda")
        view = wide[:B, :H, 1:1 + Lcap, 4:68]
        view[:, :, :L] = t.cuda()
        assert view.stride(-1) == 1 and not view.is_contiguous()
        views.append(view)
    return views


def _cross_views(k, v, L):
    """k / v as the two halves of one [B, L, 2 H 64] tensor: row stride 2 H 64, head stride 64."""
    B, H = k.shape[:2]
    kv = torch.cat([k.transpose(1, 2).reshape(B, L, H * HD), v.transpose(1, 2).reshape(B, L, H * HD)], -1).cuda()
    return [kv[:, :, j * H * HD:(j + 1) * H * HD].view(B, L, H, HD).transpose(1, 2) for j in range(2)]


def _decode_views(layout, k, v, L):
    return _cache_views(k, v, L) if layout == "cache" else _cross_views(k, v, L)


def _decode_rows(layout, B, H):
    """attend for q [B H, 1, 64] and k / v [B H, L, 64]: row n is (batch n // H, head n % H)."""

    def attend(q, k, v):
        from whisperx_amd import _lib

        L = k.shape[1]
        kv_, vv_ = _decode_views(layout, k.view(B, H, L, HD), v.view(B, H, L, HD), L)
        got = _lib.decode_attention_f32(q.view(B, H, HD).cuda(), kv_, vv_, ap.SCALE, L=L)
        return got.cpu().view(B * H, 1, HD)

    return attend


@pytest.mark.parametrize("L", DECODE_LENGTHS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_attention_permutation(layout, L):
    """B = L rows over one batch entry's k / v (expanded over the batch with stride 0): row b of head
    h asks for cache row pi_h(b), so every cache row is some row's target."""
    from whisperx_amd import _lib

    H = 2
    for kind in ap.KINDS:
        p = ap.Permutation(H, L, kind, seed=L)
        kv_, vv_ = (t.expand(L, -1, -1, -1) for t in _decode_views(layout, p.k[None], p.v[None], L))
        assert L == 1 or kv_.stride(0) == vv_.stride(0) == 0
        got = _lib.decode_attention_f32(p.q.transpose(0, 1).contiguous().cuda(), kv_, vv_, ap.SCALE, L=L)  # [L, H, 64]
        err = p.check(got.cpu().transpose(0, 1).contiguous())
        print(f"decode_attention_f32 {layout} permutation {kind} L {L}: margin {p.margin:.1f}, "
              f"|o - v[pi]| max {err:.1e}")


@pytest.mark.parametrize("L", DECODE_LENGTHS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_attention_uniform(layout, L):
    p = ap.Uniform(10, 1, L, seed=L)
    rel = p.check(_decode_rows(layout, 5, 2)(p.q, p.k, p.v))
    print(f"decode_attention_f32 {layout} uniform L {L}: relative error {rel:.2e}, bound {2.0 ** -22:.2e}")


@pytest.mark.parametrize("variant", ["offset", "ramp"])
@pytest.mark.parametrize("L", [65, 129, 1500])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_attention_range(layout, L, variant):
    p = ap.Range(10, 1, L, variant, scales=(1.0, 3.0, 1.0), seed=L)
    assert sorted(set(p.cls.flatten().tolist())) == [0, 1, 2, 3, 4]
    p.check(_decode_rows(layout, 5, 2)(p.q, p.k, p.v), f"decode_attention_f32 {layout}")


@pytest.mark.parametrize("L", [1, 65, 127, 128, 129, 300])
def test_decode_attention_poison(L):
    """The cache rows at and past L and the space around the k / v views hold NaN against zeros; the
    output's neighbours stay behind their finite sentinel."""
    from whisperx_amd import _lib

    B, H = 3, 2
    q, k, v = ap.random_inputs(B * H, 1, L, scales=(1.0, 3.0, 1.0), seed=L)

    def run(fill):
        kv_, vv_ = _cache_views(k.view(B, H, L, HD), v.view(B, H, L, HD), L, fill)
        full = torch.full((B + 2, H, HD), SENTINEL, device="cuda")
        got = _lib.decode_attention_f32(q.view(B, H, HD).cuda(), kv_, vv_, ap.SCALE, L=L, out=full[1:B + 1])
        torch.cuda.synchronize()
        assert bool((full[0] == SENTINEL).all()) and bool((full[B + 1] == SENTINEL).all())
        return got.cpu()

    ap.check_poison(run)

"""Beam search on the GPU: wx_decode_attention_f32_grouped bit for bit against wx_decode_attention_f32
called per beam (both K / V layouts, independence of the other beams and of B, NaN where it must not
read, the permutation probe with another permutation per beam, the argument checks); wx_beam_topk
against an fp64 evaluation of its definition and on exact inputs (the tie order, suppressed ids,
dead beams, winners at the ends and on both sides of every slice boundary, independence of B); and
WhisperDecoder.beam_search on the kernel route against the fp64 beam search of beam_helpers."""
import ctypes
import math

import pytest
import torch

import attention_probes as ap
from beam_helpers import EOT, check_beam_search
from selection_probes import _reference
from whisper_decoder_helpers import GEOMETRIES, attention_inputs, case

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 127, 128, 129, 257, 1500]
GROUPS = [1, 2, 5, 8]
WX_E_INVALID, WX_E_WORKSPACE = 1001, 1004


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cache_views(k, v, L, fill=0.0):
    """k / v [B, H, L, 64] as views [B, H, L + 5, 64] of wider buffers full of `fill` (the rows at and
    past L too): batch, head and row strides all differ from the packed ones."""
    B, H = k.shape[:2]
    views = []
    for t in (k, v):
        wide = torch.full((B + 1, H + 1, L + 7, 72), fill, device="cuda")
        view = wide[:B, :H, 1:6 + L, 4:68]
        view[:, :, :L] = t.cuda()
        views.append(view)
    return views


def _cross_views(k, v, L):
    """k / v as the two halves of one [B, L, 2 H 64] tensor: row stride 2 H 64, head stride 64."""
    B, H = k.shape[:2]
    kv = torch.cat([k.transpose(1, 2).reshape(B, L, H * 64), v.transpose(1, 2).reshape(B, L, H * 64)], -1).cuda()
    return [kv[:, :, j * H * 64:(j + 1) * H * 64].view(B, L, H, 64).transpose(1, 2) for j in range(2)]


def _queries(B, G, H, L, fill=0.0):
    """q [B, G, H, 64] as a strided view (rows 72 floats apart, `fill` between them) on the device;
    beam 0 holds attention_inputs' query."""
    g = torch.Generator().manual_seed(7 + 1000 * L + 10 * H + B + 100000 * G)
    q = torch.randn((B, G, H, 64), generator=g)
    q[:, 0] = attention_inputs(B, H, L)[0]
    wide = torch.full((B, G + 1, H + 1, 72), fill, device="cuda")
    view = wide[:, :G, :H, 4:68]
    view.copy_(q.cuda())
    assert view.stride(-1) == 1 and view.stride(2) == 72
    return view


def _per_beam(q, kv_, vv_, L):
    from whisperx_amd import _lib

    return torch.stack([_lib.decode_attention_f32(q[:, g].contiguous(), kv_, vv_, 0.125, L=L)
                        for g in range(q.shape[1])], 1)


@pytest.mark.parametrize("B,H", [(1, 1), (3, 6), (2, 20)])
@pytest.mark.parametrize("layout", ["cache", "cross"])
def test_grouped_equals_the_ungrouped_kernel_per_beam(B, H, layout):
    from whisperx_amd import _lib

    for L in LENGTHS:
        _, k, v = attention_inputs(B, H, L)
        kv_, vv_ = _cache_views(k, v, L, 1e4) if layout == "cache" else _cross_views(k, v, L)
        for G in GROUPS:
            q = _queries(B, G, H, L)
            full = torch.full((B + 2, G, H, 64), 1e4, device="cuda")
            got = _lib.decode_attention_f32_grouped(q, kv_, vv_, 0.125, L=L, out=full[1:B + 1])
            want = _per_beam(q, kv_, vv_, L)
            torch.cuda.synchronize()
            assert got.data_ptr() == full[1].data_ptr()
            assert bool((full[0] == 1e4).all()) and bool((full[B + 1] == 1e4).all())
            assert bool(torch.isfinite(got).all())
            assert torch.equal(_bits(got), _bits(want)), (L, G)


@pytest.mark.parametrize("L", [129, 1500, 65])
def test_a_row_depends_on_neither_the_other_beams_nor_the_batch(L):
    from whisperx_amd import _lib

    B, G, H = 3, 5, 6
    _, k, v = (t.cuda() for t in attention_inputs(B, H, L))
    q = _queries(B, G, H, L)
    both = _lib.decode_attention_f32_grouped(q, k, v, 0.125)
    other = q.clone()
    other[:, 1:] = 5.0 * torch.randn((B, G - 1, H, 64), generator=torch.Generator().manual_seed(L)).cuda()
    got = _lib.decode_attention_f32_grouped(other, k, v, 0.125)
    assert torch.equal(_bits(got[:, 0]), _bits(both[:, 0])) and not torch.equal(got[:, 1:], both[:, 1:])
    for b in range(B):  # the chunk alone, and one beam of it alone
        alone = _lib.decode_attention_f32_grouped(q[b:b + 1], k[b:b + 1], v[b:b + 1], 0.125)
        assert torch.equal(_bits(alone[0]), _bits(both[b]))
        one = _lib.decode_attention_f32_grouped(q[b:b + 1, 3:4], k[b:b + 1], v[b:b + 1], 0.125)
        assert torch.equal(_bits(one[0, 0]), _bits(both[b, 3]))


@pytest.mark.parametrize("L", [1, 127, 128, 129, 300])
def test_grouped_poison(L):
    """NaN against zeros in the cache rows at and past L, around the k / v views and between the
    strided query rows: the outputs are finite and equal bit for bit."""
    from whisperx_amd import _lib

    B, G, H = 2, 5, 3
    _, k, v = attention_inputs(B, H, L)

    def run(fill):
        kv_, vv_ = _cache_views(k, v, L, fill)
        return _lib.decode_attention_f32_grouped(_queries(B, G, H, L, fill), kv_, vv_, 0.125, L=L).cpu().view(B * G, H, 64)

    ap.check_poison(run)


@pytest.mark.parametrize("L", [2, 128, 129, 1500])
@pytest.mark.parametrize("layout", ["cache", "cross"])
def test_grouped_permutation(layout, L):
    """B = L chunks over one chunk's k / v (expanded with stride 0), G beams: beam g of chunk b and
    head h asks for cache row pi_h((b + g) mod L), another permutation for every beam, and every
    cache row is the target of one chunk in every beam."""
    from whisperx_amd import _lib

    H, G = 2, 5
    for kind in ("random", "reversal"):
        p = ap.Permutation(H, L, kind, seed=L)
        views = _cache_views(p.k[None], p.v[None], L, 1e4) if layout == "cache" else _cross_views(p.k[None], p.v[None], L)
        kv_, vv_ = (t.expand(L, -1, -1, -1) for t in views)
        q = torch.stack([torch.roll(p.q, -g, 1) for g in range(G)], 0)  # [G, H, L, 64]: [g, h, b] = q[h, (b + g) % L]
        got = _lib.decode_attention_f32_grouped(q.permute(2, 0, 1, 3).contiguous().cuda(), kv_, vv_, ap.SCALE, L=L)
        for g in range(G):
            o = got[:, g].cpu().transpose(0, 1)  # [H, L, 64]: [h, b] = v[h, pi((b + g) % L)]
            err = p.check(torch.roll(o, g, 1).contiguous())
        print(f"grouped {layout} permutation {kind} L {L}: margin {p.margin:.1f}, |o - v[pi]| max {err:.1e}")


def test_grouped_argument_checks():
    from whisperx_amd import _lib

    lib = _lib.load()
    q, k, v = (t.cuda() for t in attention_inputs(2, 3, 300))
    q = q[:, None].expand(2, 5, 3, 64).contiguous()
    o = torch.empty_like(q)
    need = lib.wx_decode_attention_grouped_workspace_bytes(2, 5, 3, 300)
    assert need >= lib.wx_decode_attention_workspace_bytes(10, 3, 300) > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = [(ctypes.c_int64 * 3)(*t.stride()[:3]) for t in (q, k, v)]
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(G=5, D=64, qs=st[0], wsb=need, qp=P(q), L=300):
        return lib.wx_decode_attention_f32_grouped(qp, P(k), P(v), P(o), 2, G, 3, L, D, qs, st[1], st[2], 0.125, P(ws), wsb,
                                                   None)

    o.fill_(7.0)
    for bad in (dict(G=0), dict(G=9), dict(D=32), dict(L=0), dict(qs=(ctypes.c_int64 * 3)(960, 194, 64)),
                dict(qp=ctypes.c_void_p(q.data_ptr() + 4)), dict(qp=None)):
        assert call(**bad) == WX_E_INVALID, bad
    assert call(wsb=need - 1) == WX_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())  # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(o), _bits(_lib.decode_attention_f32_grouped(q, k, v, 0.125)))


# ------------------------------------------------------------------------------ wx_beam_topk
def _padded(x, fill=math.nan):
    """x [R, V] on the device with a row stride > V and `fill` in the padding."""
    R, V = x.shape
    wide = torch.full((R, V + 3), fill, device="cuda")
    wide[:, :V] = x.cuda()
    return wide[:, :V]


def _check_topk(x, cum, G, label):
    """wx_beam_topk on (x, cum) against the fp64 definition: the oracle's gaps among its first 2G + 1
    candidates exceed 8 x ref_err (ref_err: the largest |fp32 torch.log_softmax - fp64| on these
    rows), then equal indices and scores within 4 x ref_err."""
    from whisperx_amd import _lib

    R, V = x.shape
    B, K = R // G, 2 * G
    want_s, want_i = _reference(x, cum, G, min(K + 1, G * V))
    ref_err = float((torch.log_softmax(x, 1).double() - torch.log_softmax(x.double(), 1)).abs().max())
    gaps = (want_s[:, :-1] - want_s[:, 1:])
    got_s, got_i = _lib.beam_topk(_padded(x), cum.cuda(), G)
    assert tuple(got_s.shape) == tuple(got_i.shape) == (B, K) and got_i.dtype == torch.int32
    err = float((got_s.cpu().double() - want_s[:, :K]).abs().max())
    print(f"beam_topk {label} B {B} G {G} V {V}: smallest gap {float(gaps.min()):.3e}, ref_err {ref_err:.3e}, "
          f"8 x ref_err {8 * ref_err:.3e}; |score - fp64| {err:.3e}, bound {4 * ref_err:.3e}")
    assert ref_err > 0 and float(gaps.min()) > 8 * ref_err
    assert torch.equal(got_i.cpu().long(), want_i[:, :K])
    assert err <= 4 * ref_err
    return got_s, got_i


@pytest.mark.parametrize("B,G,V", [(1, 1, 2), (2, 5, 10), (3, 5, 96), (2, 8, 51865), (1, 3, 4099)])
def test_topk_against_the_fp64_definition(B, G, V):
    g = torch.Generator().manual_seed(1 + V + 10 * G)
    x = 4.0 * torch.randn((B * G, V), generator=g)
    cum = -2.0 * torch.rand(B * G, generator=g)  # (running sums of a few steps)
    _check_topk(x, cum, G, "randn")


def _topk(rows, cum, G):
    from whisperx_amd import _lib

    s, i = _lib.beam_topk(_padded(torch.tensor(rows, dtype=torch.float32)), torch.tensor(cum, dtype=torch.float32).cuda(), G)
    return s.cpu().tolist(), i.cpu().tolist()


def test_topk_tie_order():
    ninf = -math.inf
    # equal rows, equal sums: the scores of the three 5s tie in both beams -> lower g, then lower t
    row = [3.0, 5.0, 5.0, 1.0, 0.0, ninf, 5.0, 2.0]
    s, i = _topk([row, row], [-1.0, -1.0], 2)
    assert i == [[1, 2, 6, 8 + 1]] and len(set(s[0])) == 1 and math.isfinite(s[0][0])
    s, i = _topk([row, row], [-1.0, -0.5], 2)  # the better beam first
    assert i == [[8 + 1, 8 + 2, 8 + 6, 1]] and s[0][0] == s[0][2] > s[0][3]
    # sums of -2^26 (spacing 8) swallow x - lse for the four logits within 4 of lse = 10.44..: equal
    # scores in one beam -> higher logit first, whatever t
    row = [7.0, 9.0, 10.0, 8.0, -20.0, -20.0, -20.0, -20.0]
    big = -float(2 ** 26)
    s, i = _topk([row, row], [big, big], 2)
    assert i == [[2, 1, 3, 0]] and s == [[big] * 4]
    s, i = _topk([row, row, row], [big, big, big], 3)
    assert i == [[2, 1, 3, 0, 8 + 2, 8 + 1]] and s == [[big] * 6]


def test_topk_suppressed_ids_and_dead_beams():
    ninf = -math.inf
    # one finite logit in the row: lse is that logit and the score is the sum exactly; beam 1 is dead
    row0 = [ninf] * 9
    row0[5] = 3.5
    row1 = [float(t) for t in range(9)]
    s, i = _topk([row0, row1], [-1.25, ninf], 2)
    assert i == [[5, 0, 1, 2]]  # then -inf scores: lower g, (equal logits) lower t
    assert s == [[-1.25, ninf, ninf, ninf]]
    # dead beams 1 and 2 of 3: the live beam's six best, then -inf by g and logit
    g = torch.Generator().manual_seed(4)
    x = 4.0 * torch.randn((6, 40), generator=g)
    cum = torch.tensor([0.0, ninf, ninf, -1.0, ninf, -0.5])
    got_s, got_i = _check_topk_live(x, cum, 3)
    assert all(idx // 40 == 0 for idx in got_i[0]) and all(idx // 40 in (0, 2) for idx in got_i[1])
    # fewer than 2G finite candidates: 2 live ids in the one live beam
    x2 = torch.full((3, 40), ninf)
    x2[0, 7], x2[0, 30] = 1.0, 2.0
    x2[1], x2[2] = x[1], x[2]
    s, i = _topk(x2.tolist(), [0.0, ninf, ninf], 3)
    assert i[0][:2] == [30, 7] and all(math.isfinite(v) for v in s[0][:2]) and s[0][2:] == [ninf] * 4
    assert i[0][2:] == [0, 1, 2, 3]  # beam 0's -inf logits by t, before any candidate of beams 1 and 2


def _check_topk_live(x, cum, G):
    got_s, got_i = _check_topk(x, cum, G, "dead beams")
    assert bool(torch.isfinite(got_s).all())
    return got_s.cpu().tolist(), got_i.cpu().tolist()


def test_topk_winners_at_the_ends_and_at_every_slice_boundary():
    """V = 3 slices of 4096 and 5 columns: winners planted at column 0, at V - 1 and on both sides of
    every multiple of 1024 (a wave's columns) and of 4096 (a block's), each in some chunk's 2G."""
    from whisperx_amd import _lib

    assert _lib.BEAM_TOPK_SLICE == 4096
    B, G, V = 2, 8, 3 * 4096 + 5
    special = [0, V - 1] + [c + d for c in range(1024, V, 1024) for d in (-1, 0)]
    assert len(special) == 26
    g = torch.Generator().manual_seed(9)
    x = torch.randn((B * G, V), generator=g)
    planted = [[], []]
    for j, col in enumerate(special):
        b, r = j % 2, (j // 2) % G
        x[b * G + r, col] = 20.0 + 1.5 * j
        planted[b].append(r * V + col)
    cum = -0.37 * torch.arange(B * G, dtype=torch.float32)
    _, got_i = _check_topk(x, cum, G, "boundaries")
    for b in range(B):
        assert set(planted[b]) <= set(got_i[b].tolist()), b


def test_topk_does_not_depend_on_the_batch():
    from whisperx_amd import _lib

    G, V = 5, 4099
    g = torch.Generator().manual_seed(2)
    x = _padded(4.0 * torch.randn((3 * G, V), generator=g))
    cum = (-3.0 * torch.rand(3 * G, generator=g)).cuda()
    s, i = _lib.beam_topk(x, cum, G)
    for b in range(3):
        s1, i1 = _lib.beam_topk(x[b * G:(b + 1) * G], cum[b * G:(b + 1) * G].contiguous(), G)
        assert torch.equal(_bits(s1[0]), _bits(s[b])) and torch.equal(i1[0], i[b])


def test_topk_argument_checks():
    from whisperx_amd import _lib

    lib = _lib.load()
    x = torch.randn((10, 96), device="cuda")
    cum = torch.zeros(10, device="cuda")
    s = torch.full((2, 10), 7.0, device="cuda")
    i = torch.full((2, 10), 7, dtype=torch.int32, device="cuda")
    need = lib.wx_beam_topk_workspace_bytes(2, 5, 96)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(G=5, V=96, stride=96, wsb=need, xp=P(x)):
        return lib.wx_beam_topk(xp, stride, P(cum), 2, G, V, P(s), P(i), P(ws), wsb, None)

    for bad in (dict(G=0), dict(G=9), dict(V=9), dict(stride=95), dict(xp=None)):
        assert call(**bad) == WX_E_INVALID, bad
    assert call(wsb=need - 1) == WX_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((s == 7.0).all()) and bool((i == 7).all())  # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    ws_s, ws_i = _lib.beam_topk(x, cum, 5)
    assert torch.equal(_bits(s), _bits(ws_s)) and torch.equal(i, ws_i)


# ------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_beam_search_on_the_kernel_route_equals_the_fp64_search(geometry):
    from whisperx_amd import WhisperDecoder

    c = case(*geometry)
    dec = WhisperDecoder(c.model, device="cuda")
    got = check_beam_search(c, dec, "kernels", EOT[c.D])
    st = dec.start(c.enc, beams=5)
    assert st.kernels and all(tuple(x.shape) == (c.B, c.geometry[2], 2 * c.D) for x in st.cross)
    host = dec.beam_search(c.enc, [1, 5, 7], EOT[c.D], max_length=3 + 12, kernels=False)  # the host route on the device
    assert [[h.ids for h in hs] for hs in host] == [[h.ids for h in hs] for hs in got]


def test_beam_sizes_on_the_kernel_route():
    from whisperx_amd import WhisperDecoder

    c = case(*GEOMETRIES[2])
    dec = WhisperDecoder(c.model, device="cuda")
    for G in (2, 8):
        check_beam_search(c, dec, "kernels", EOT[c.D], G=G)
    kw = dict(max_length=3 + 12)
    assert [hs[0].ids for hs in dec.beam_search(c.enc, [1, 5, 7], EOT[c.D], beam_size=1, **kw)] == \
        dec.generate(c.enc, [1, 5, 7], EOT[c.D], **kw)

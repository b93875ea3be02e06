"""wx_attention_h16 on the GPU, fp16 and bf16: against an fp64 softmax(q k^T / 8) v within 4 x ref_err
(whisper_half_helpers: ref_err is torch's CPU attention in the same type), exact probes for the key
order between the probabilities and the V operand (permutation) and for the key count (uniform),
memory behind the tensors (poison), independence of the batch, and the argument validation.

The entry point takes one path at every size: a workgroup owns 64 queries (two MFMA tiles, the
second empty when T mod 64 is 1 .. 32) and always splits their keys over 4 waves, wave w taking the
32-key tiles w, w + 4, ...: T <= 32 leaves waves 1-3 without keys, T = 33 .. 64 waves 2-3,
T = 65 .. 96 wave 3; from T = 97 every wave has a tile, from T = 129 some have two (the
register-staged V tile is replaced in LDS); T = 1500 is Whisper's 46 full tiles + 28 keys.  The T
lists below cover each."""
import ctypes

import pytest
import torch

import whisper_half_helpers as hh

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(d, id=hh.name(d)) for d in hh.DTYPES]
TS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 257, 1500)
BHS = ((1, 1), (3, 6), (2, 20))


def _attend(q, k, v):
    """[N, T, 64] -> [N, T, 64] through one head per batch entry."""
    from whisperx_amd import _lib

    o = _lib.attention_h16(q.unsqueeze(1), k.unsqueeze(1), v.unsqueeze(1), hh.SCALE)
    return o[:, :, 0]


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_against_fp64(dtype, T):
    from whisperx_amd import _lib

    for B, H in BHS:
        q, k, v, want, ref_err = hh.attention_case(dtype, B, H, T)
        qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
        _, fused = hh.fused_views(qd, kd, vd)
        for label, (a, b, c) in (("contiguous", (qd, kd, vd)), ("fused", fused)):
            o = _lib.attention_h16(a, b, c, hh.SCALE)
            assert o.dtype == dtype and tuple(o.shape) == (B, T, H, 64) and o.is_contiguous()
            err = float((o.cpu().double() - want).abs().max())
            print(f"attention_h16 {hh.name(dtype)} B {B} H {H} T {T} {label}: |kernel - fp64| {err:.3e}, ref_err "
                  f"{ref_err:.3e}, bound {4 * ref_err:.3e}")
            if ref_err == 0:  # one key: the softmax is exactly 1
                assert T == 1 and torch.equal(o.cpu(), v.transpose(1, 2))
            else:
                assert err <= 4 * ref_err


@pytest.mark.parametrize("kind", ["identity", "reversal", "random"])
@pytest.mark.parametrize("T", [32, 33, 64, 1500])
@pytest.mark.parametrize("dtype", DTYPES)
def test_permutation_probe(dtype, T, kind):
    p = hh.Permutation(dtype, 4, T, kind)
    o = _attend(p.q.cuda(), p.k.cuda(), p.v.cuda()).cpu()
    bad = (o != p.want).any(-1)
    assert not bool(bad.any()), (f"{int(bad.sum())} of {bad.numel()} queries do not return their target's value row; "
                                 f"first (n, i) = {tuple(int(x) for x in bad.nonzero()[0])}, margin {p.margin:.1f}")


@pytest.mark.parametrize("T", [32, 33, 64, 1024, 1500])
@pytest.mark.parametrize("dtype", DTYPES)
def test_uniform_probe(dtype, T):
    u = hh.Uniform(dtype, 3, T)
    o = _attend(u.q.cuda(), u.k.cuda(), u.v.cuda()).cpu().double()
    err = (o - u.want).abs()
    worst = float((err / u.want.abs().clamp_min(1e-300))[u.want != 0].max())
    print(f"uniform {hh.name(dtype)} T {T}: largest relative error {worst:.3e}")
    if u.exact:
        assert torch.equal(o, u.want)
    else:  # one rounding to dtype of sum / T, itself two fp32 roundings from exact
        assert bool((err <= (hh.HALF_ULP[dtype] + 2.0 ** -22) * u.want.abs()).all())


@pytest.mark.parametrize("T", [1, 33, 65, 1500])
@pytest.mark.parametrize("dtype", DTYPES)
def test_memory_behind_the_tensors_is_not_read(dtype, T):
    """The 32 rows behind each batch entry of the fused buffer and 8 elements of padding behind
    every row hold zeros in one run and NaN in the other: bit-equal, finite outputs."""
    from whisperx_amd import _lib

    q, k, v, _, _ = hh.attention_case(dtype, 3, 6, T)
    outs = []
    for fill in (0.0, float("nan")):
        buf, views = hh.fused_views(q.cuda(), k.cuda(), v.cuda(), rows_behind=32, pad=8, fill=fill)
        assert bool(torch.isnan(buf).any()) == (fill != 0.0)
        outs.append(_lib.attention_h16(*views, hh.SCALE))
    assert bool(torch.isfinite(outs[0]).all()) and bool(torch.isfinite(outs[1]).all())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


@pytest.mark.parametrize("T", [33, 1500])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_does_not_depend_on_the_batch(dtype, T):
    from whisperx_amd import _lib

    q, k, v, _, _ = hh.attention_case(dtype, 3, 6, T)
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    whole = _lib.attention_h16(qd, kd, vd, hh.SCALE)
    for b, h in ((0, 0), (1, 3), (2, 5)):
        alone = _lib.attention_h16(*(t[b:b + 1, h:h + 1] for t in (qd, kd, vd)), hh.SCALE)
        assert torch.equal(alone[0, :, 0].view(torch.int16), whole[b, :, h].view(torch.int16))


def test_mixed_or_fp32_inputs_are_refused():
    from whisperx_amd import _lib

    x = torch.zeros((1, 1, 4, 64), device="cuda")
    with pytest.raises(_lib.WXError):
        _lib.attention_h16(x, x, x, hh.SCALE)
    with pytest.raises(_lib.WXError):
        _lib.attention_h16(x.half(), x.half(), x.bfloat16(), hh.SCALE)


def test_validation():
    """Every WX_E_INVALID case of the header, with legal device pointers; nothing is launched: the
    output keeps its sentinel.  B = 0 is WX_OK (before the pointers are looked at)."""
    from whisperx_amd import _lib

    lib = _lib.load()
    B, H, T = 2, 3, 40
    x = torch.zeros((3, B, H, T, 64), dtype=torch.float16, device="cuda")
    o = torch.full((B, T, H, 64), 7.0, dtype=torch.float16, device="cuda")
    good = (ctypes.c_int64 * 3)(H * T * 64, T * 64, 64)
    odd = [(ctypes.c_int64 * 3)(*(s + 4 if i == j else s for j, s in enumerate(good))) for i in range(3)]
    p = [x[i].data_ptr() for i in range(3)] + [o.data_ptr()]

    def call(ptrs=p, B=B, H=H, T=T, D=64, st=(good, good, good), dtype=1):
        return lib.wx_attention_h16(*(ctypes.c_void_p(a) if a else None for a in ptrs), B, H, T, D, *st, 0.125, dtype, None)

    INVALID = 1001
    assert call(B=-1) == INVALID and call(H=0) == INVALID and call(T=0) == INVALID and call(D=32) == INVALID
    assert call(dtype=0) == INVALID and call(dtype=3) == INVALID
    assert call(B=0) == 0 and call(B=0, ptrs=[0, 0, 0, 0]) == 0
    assert call(B=0, T=0) == INVALID  # (the sizes are checked before the empty batch)
    for i in range(4):
        assert call(ptrs=[0 if j == i else a for j, a in enumerate(p)]) == INVALID      # null
        assert call(ptrs=[a + 8 if j == i else a for j, a in enumerate(p)]) == INVALID  # inside the tensor, misaligned
    for i in range(3):
        assert call(st=tuple(None if j == i else good for j in range(3))) == INVALID
        for bad in odd:
            assert call(st=tuple(bad if j == i else good for j in range(3))) == INVALID
    assert call(B=1 << 20, H=1 << 12) == INVALID  # 2^32 workgroups
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((o == 0.0).all())

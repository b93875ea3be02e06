"""WhisperDecoder on the GPU: wx_decode_attention_f32 against an fp64 torch attention (strided
key / value views in both layouts, rows past L and the output's neighbours behind sentinels, batch
independence bit for bit), then the decoder against transformers': teacher-forced logits, greedy
decoding token for token against the fp64 greedy loop, stopping, suppression, language detection
and a side stream.

Tolerance (the encoder tests' rule): ref_err = max|fp32 reference - fp64 reference| on the same
inputs on the CPU, and max|ours - fp64| <= 4 x ref_err; both are printed."""
import pytest
import torch

from whisper_decoder_helpers import (GEOMETRIES, attention_inputs, attention_ref, case, check_detect_language,
                                     check_forced_logits, check_greedy, check_stopping, check_suppression)

pytestmark = pytest.mark.gpu

SENTINEL = 1e4


def _chunk():
    from whisperx_amd import _lib

    return _lib.DECODE_CHUNK


def _lengths():
    C = _chunk()
    return sorted({1, 2, 63, 64, 65, C - 1, C, C + 1, 2 * C + 1, 448, 1500})


def _cache_views(k, v, L):
    """k / v [B, H, L, 64] as views [B, H, Lcap, 64] of wider buffers full of the sentinel (rows >= L
    too): batch, head and row strides all differ from the packed ones."""
    B, H = k.shape[:2]
    Lcap = L + 5
    views = []
    for t in (k, v):
        wide = torch.full((B + 1, H + 1, Lcap + 2, 72), SENTINEL, device="cuda")
        view = wide[:B, :H, 1:1 + Lcap, 4:68]
        view[:, :, :L] = t.cuda()
        assert view.stride(-1) == 1 and not view.is_contiguous()
        views.append(view)
    return views


def _cross_views(k, v, L):
    """k / v as the two halves of one [B, L, 2 H 64] tensor: row stride 2 H 64, head stride 64."""
    B, H = k.shape[:2]
    kv = torch.cat([k.transpose(1, 2).reshape(B, L, H * 64), v.transpose(1, 2).reshape(B, L, H * 64)], -1).cuda()
    return [kv[:, :, j * H * 64:(j + 1) * H * 64].view(B, L, H, 64).transpose(1, 2) for j in range(2)]


@pytest.mark.parametrize("B,H", [(1, 1), (3, 6), (2, 20)])
@pytest.mark.parametrize("layout", ["cache", "cross"])
def test_kernel_against_fp64(B, H, layout):
    from whisperx_amd import _lib

    for L in _lengths():
        q, k, v = attention_inputs(B, H, L)
        want = attention_ref(q.double(), k.double(), v.double())
        ref_err = float((attention_ref(q, k, v).double() - want).abs().max())
        kv_, vv_ = _cache_views(k, v, L) if layout == "cache" else _cross_views(k, v, L)
        full = torch.full((B + 2, H, 64), SENTINEL, device="cuda")
        got = _lib.decode_attention_f32(q.cuda(), kv_, vv_, 0.125, L=L, out=full[1:B + 1])
        torch.cuda.synchronize()
        assert got.data_ptr() == full[1].data_ptr()
        assert bool((full[0] == SENTINEL).all()) and bool((full[B + 1] == SENTINEL).all())
        err = float((got.cpu().double() - want).abs().max())
        print(f"decode attention {layout} B {B} H {H} L {L}: |kernel - fp64| {err:.3e}, ref_err {ref_err:.3e}, "
              f"bound {4 * ref_err:.3e}")
        # (one key: the softmax is exactly 1 in every precision, o = v, and the bound is equality)
        assert (ref_err > 0 or L == 1) and err <= 4 * ref_err, L


@pytest.mark.parametrize("L", [1500, 65])
def test_a_row_does_not_depend_on_the_batch(L):
    """Row (b, h) computed inside B = 3 equals the same row computed alone, bit for bit."""
    from whisperx_amd import _lib

    q, k, v = (t.cuda() for t in attention_inputs(3, 6, L))
    both = _lib.decode_attention_f32(q, k, v, 0.125)
    for b, h in ((0, 0), (1, 3), (2, 5)):
        alone = _lib.decode_attention_f32(q[b:b + 1, h:h + 1].contiguous(), k[b:b + 1, h:h + 1].contiguous(),
                                          v[b:b + 1, h:h + 1].contiguous(), 0.125)
        assert torch.equal(alone[0, 0].view(torch.int32), both[b, h].view(torch.int32)), (b, h)
    assert bool(torch.isfinite(both).all())


def _device(c):
    from whisperx_amd import WhisperDecoder

    return WhisperDecoder(c.model, device="cuda")


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_teacher_forced_logits_against_the_oracle(geometry):
    c = case(*geometry)
    dec = _device(c)
    got = check_forced_logits(c, dec, "kernels")
    ids, _, ref_err = c.forced()
    host = dec.logits(c.enc, ids, kernels=False)  # the host route's arithmetic on the device
    err_host = float((got - host).abs().max())
    print(f"|kernels - host route| {err_host:.3e}, bound {8 * ref_err:.3e}")
    assert err_host <= 2 * 4 * ref_err


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_greedy_generate_equals_the_fp64_loop(geometry):
    c = case(*geometry)
    check_greedy(c, _device(c), "kernels")


def test_stopping_and_suppression():
    c = case(*GEOMETRIES[0])
    dec = _device(c)
    check_stopping(c, dec)
    check_suppression(c, dec, "kernels")


def test_detect_language():
    c = case(*GEOMETRIES[0])
    check_detect_language(c, _device(c), "kernels")


def test_side_stream_gives_the_same_result():
    from whisperx_amd import _lib

    c = case(*GEOMETRIES[2])
    ids, y64, ref_err = c.forced()
    dec = _device(c)
    q, k, v = (t.cuda() for t in attention_inputs(2, 8, 300))
    want_attn, want = _lib.decode_attention_f32(q, k, v, 0.125), dec.logits(c.enc, ids)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got_attn = _lib.decode_attention_f32(q, k, v, 0.125)
        st = dec.start(c.enc)
        got = torch.stack([dec.step(st, ids[:, i]) for i in range(ids.shape[1])], 1)
    side.synchronize()
    assert torch.equal(got_attn.view(torch.int32), want_attn.view(torch.int32))
    # (the GEMM library may pick its kernels per stream: the logits are held to the oracle's bound)
    assert float((got.cpu().double() - y64).abs().max()) <= 4 * ref_err
    assert float((got - want).abs().max()) <= 4 * ref_err

"""wx_decode_self_attention_f32 / _h16 on the GPU, zero tolerance: the self-attention of one decode
step at a position read on the device, with the cache append fused, against the existing entry
points on a copy of the cache that had the new row copied in (o bit for bit, cache row p the new
row, every other cache row untouched, NaN in every row at and above p); positions outside the cache
write nothing; and one captured launch replayed over the 128-row chunk boundary."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

LCAP = 448
POSITIONS = [0, 1, 126, 127, 128, 129, 255, 256, 383, 447]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
SENTINEL = 7.0


def _entries(dtype):
    from whisperx_amd import _lib

    if dtype == torch.float32:
        return _lib.decode_self_attention_f32, _lib.decode_attention_f32
    return _lib.decode_self_attention_h16, _lib.decode_attention_h16


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _qkv(B, H, dtype, seed):
    """One [B, 3 H 64] buffer (a q/k/v GEMM output) and its three column blocks as [B, H, 64] views:
    k 3x q's scale, so the softmax is peaked."""
    g = torch.Generator().manual_seed(seed)
    D = H * 64
    buf = torch.randn((B, 3 * D), generator=g)
    buf[:, D:2 * D] *= 3.0
    buf = buf.to(dtype).cuda()
    q, k, v = (buf[:, j * D:(j + 1) * D].view(B, H, 64) for j in range(3))
    assert not q.is_contiguous() or B == 1
    return buf, q, k, v


def _cache(B, H, p, dtype, seed):
    """k / v caches [B, H, LCAP, 64]: random rows below p, NaN at and above it."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for scale in (3.0, 1.0):
        c = scale * torch.randn((B, H, LCAP, 64), generator=g)
        c[:, :, p:] = float("nan")
        out.append(c.to(dtype).cuda())
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("B,H", [(1, 1), (3, 6), (2, 20)])
def test_equals_the_existing_entry_after_the_copy(B, H, dtype):
    fused, plain = _entries(dtype)
    for p in POSITIONS:
        _, q, k, v = _qkv(B, H, dtype, 100 * p + B)
        ck, cv = _cache(B, H, p, dtype, 7 + p)
        wk, wv = ck.clone(), cv.clone()
        wk[:, :, p], wv[:, :, p] = k, v
        want = plain(q, wk, wv, 0.125, L=p + 1)
        pos = torch.tensor([p], dtype=torch.int32, device="cuda")
        got = fused(q, k, v, ck, cv, pos, 0.125)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (B, H, 64) and got.dtype == dtype and bool(torch.isfinite(got.float()).all()), p
        assert torch.equal(_bits(got), _bits(want)), p
        for c, w, new in ((ck, wk, k), (cv, wv, v)):
            assert torch.equal(_bits(c[:, :, p]), _bits(new)), p  # the new row, bit for bit
            assert torch.equal(_bits(c), _bits(w)), p  # and every other row as it was (the NaN rows too)
        assert int(pos) == p


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_a_position_outside_the_cache_writes_nothing(dtype):
    from whisperx_amd import _lib

    fused, _ = _entries(dtype)
    B, H = 3, 6
    _, q, k, v = _qkv(B, H, dtype, 5)
    ws = _lib.decode_attention_workspace(B, H, LCAP, "cuda")
    for p in (-1, LCAP, LCAP + 128, -(2 ** 31), 2 ** 31 - 1):
        ck, cv = _cache(B, H, 200, dtype, 9)
        bk, bv = ck.clone(), cv.clone()
        out = torch.full((B + 2, H, 64), SENTINEL, dtype=dtype, device="cuda")
        ws.fill_(0x5A)
        pos = torch.tensor([p], dtype=torch.int32, device="cuda")
        fused(q, k, v, ck, cv, pos, 0.125, out=out[1:B + 1], workspace=ws)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), p
        assert torch.equal(_bits(ck), _bits(bk)) and torch.equal(_bits(cv), _bits(bv)), p
        assert bool((ws == 0x5A).all()), p  # nothing at all


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_own_workspace_and_out_are_used(dtype):
    """With `workspace` the call's partial results land in the caller's buffer (Lcap > 128 and
    p >= 128: two chunks and a merge), `out` is written in place and nothing around it."""
    from whisperx_amd import _lib

    fused, plain = _entries(dtype)
    B, H, p = 2, 3, 300
    _, q, k, v = _qkv(B, H, dtype, 3)
    ck, cv = _cache(B, H, p, dtype, 4)
    wk, wv = ck.clone(), cv.clone()
    wk[:, :, p], wv[:, :, p] = k, v
    ws = _lib.decode_attention_workspace(B, H, LCAP, "cuda")
    ws.fill_(0x5A)
    out = torch.full((B + 2, H, 64), SENTINEL, dtype=dtype, device="cuda")
    got = fused(q, k, v, ck, cv, torch.tensor([p], dtype=torch.int32, device="cuda"), 0.125, out=out[1:B + 1], workspace=ws)
    want = plain(q, wk, wv, 0.125, L=p + 1, workspace=_lib.decode_attention_workspace(B, H, p + 1, "cuda"))
    torch.cuda.synchronize()
    assert got.data_ptr() == out[1].data_ptr() and torch.equal(_bits(got), _bits(want))
    assert bool((out[0] == SENTINEL).all()) and bool((out[B + 1] == SENTINEL).all())
    assert not bool((ws == 0x5A).all())
    with pytest.raises(_lib.WXError):
        fused(q, k, v, ck, cv, torch.tensor([p], dtype=torch.int64, device="cuda"), 0.125)
    with pytest.raises(_lib.WXError):
        fused(q, k, v, ck, cv, torch.tensor([p], dtype=torch.int32), 0.125)
    with pytest.raises(_lib.WXError):
        fused(q, k, v, ck, cv, torch.tensor([p], dtype=torch.int32, device="cuda"), 0.125, workspace=ws[:64])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_a_captured_launch_follows_the_position_on_the_device(dtype):
    """One call and pos += 1 captured in a graph, replayed 130 times from p = 0 with fresh q / k / v
    copied into the static buffer: every replay's o and the final caches equal an eager loop over
    the existing entry point (copy the row in, L = p + 1)."""
    from whisperx_amd import _lib

    fused, plain = _entries(dtype)
    B, H, N = 2, 3, 130
    D = H * 64
    g = torch.Generator().manual_seed(11)
    steps = torch.randn((N, B, 3 * D), generator=g)
    steps[:, :, D:2 * D] *= 3.0
    steps = steps.to(dtype).cuda()

    buf = torch.zeros((B, 3 * D), dtype=dtype, device="cuda")
    q, k, v = (buf[:, j * D:(j + 1) * D].view(B, H, 64) for j in range(3))
    ck, cv = (torch.full((B, H, LCAP, 64), float("nan"), dtype=dtype, device="cuda") for _ in range(2))
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros((B, H, 64), dtype=dtype, device="cuda")
    ws = _lib.decode_attention_workspace(B, H, LCAP, "cuda")

    buf.copy_(steps[0])
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):  # the warm-up: idempotent without the increment
        fused(q, k, v, ck, cv, pos, 0.125, out=out, workspace=ws)
    cur.wait_stream(side)
    gc.collect()  # (no graph object of an earlier test may be freed by the collector during the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused(q, k, v, ck, cv, pos, 0.125, out=out, workspace=ws)
        pos.add_(1)
    got = []
    for i in range(N):
        buf.copy_(steps[i])
        graph.replay()
        got.append(out.clone())
    torch.cuda.synchronize()
    assert int(pos) == N

    wk, wv = (torch.full((B, H, LCAP, 64), float("nan"), dtype=dtype, device="cuda") for _ in range(2))
    for i in range(N):
        qi, ki, vi = (steps[i][:, j * D:(j + 1) * D].view(B, H, 64) for j in range(3))
        wk[:, :, i], wv[:, :, i] = ki, vi
        want = plain(qi, wk, wv, 0.125, L=i + 1)
        assert torch.equal(_bits(got[i]), _bits(want)), i
    assert torch.equal(_bits(ck), _bits(wk)) and torch.equal(_bits(cv), _bits(wv))

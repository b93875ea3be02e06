"""Where wx_sample_token writes: token, logprob, sum_logprob, done and a workspace of exactly
wx_sample_token_workspace_bytes(R, V) bytes between guard bands (guard_bands.py), at the two
smallest and the largest shape of test_gpu_sample_token.py.  As in test_gpu_guard_bands.py: WX_OK,
every band byte unchanged after the stream has drained, the outputs equal bit for bit what the _lib
wrapper returns with its ordinary allocations, and a workspace one byte short is WX_E_WORKSPACE and
leaves every output and workspace byte as it was.  Every comparison is of bytes."""
import ctypes

import pytest
import torch

import guard_bands as gb
from sample_helpers import kernel_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WX_OK, WX_E_WORKSPACE = 0, 1004
SEED = (3 << 32) + 12345


def _p(x):
    if x is None:
        return None
    return ctypes.c_void_p(x.ptr if isinstance(x, gb.Guarded) else x.data_ptr())


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("temperature", [0.0, 0.6])
@pytest.mark.parametrize("R,V", [(1, 1), (3, 96), (2, 51865)])
def test_sample_token(R, V, temperature):
    from whisperx_amd import _lib

    lib = _lib.load()
    x, suppress, done, eot = kernel_case(R, V)
    lg, sup = x.to(DEV), suppress.to(DEV)
    step = torch.tensor([7], dtype=torch.int64, device=DEV)
    sums0 = (torch.randn(R, generator=torch.Generator().manual_seed(R)) - 3).to(DEV)
    wsb = lib.wx_sample_token_workspace_bytes(R, V)
    assert wsb > 0
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    label = f"sample_token R {R} V {V} T {temperature}"

    def buffers():
        """The weakest alignments the header allows: 8 bytes for int64, 4 for fp32, none for the
        bytes of done (4 here); 16 for the workspace.  sum_logprob and done are in / out."""
        tok = gb.guarded(R, torch.int64, DEV, offset=8, name="token")
        lp = gb.guarded(R, torch.float32, DEV, offset=4, name="logprob")
        sm = gb.guarded(R, torch.float32, DEV, offset=4, name="sum_logprob")
        dn = gb.guarded(R, torch.uint8, DEV, offset=4, name="done")
        ws = gb.guarded(int(wsb), torch.uint8, DEV, offset=16, name=label + " workspace")
        sm.t.copy_(sums0)
        dn.t.copy_(done.to(DEV))
        return tok, lp, sm, dn, ws

    def call(b, nbytes):
        tok, lp, sm, dn, ws = b
        rc = lib.wx_sample_token(_p(lg), V, R, V, _p(sup), temperature, SEED, _p(step), eot, _p(dn), _p(tok), _p(lp), _p(sm),
                                 _p(ws), nbytes, stream)
        torch.cuda.synchronize()
        return rc

    b = buffers()
    assert call(b, wsb - 1) == WX_E_WORKSPACE, f"{label}: a workspace one byte short was accepted"
    gb.check(*b)
    tok, lp, sm, dn, ws = b
    assert gb.untouched(tok) and gb.untouched(lp) and gb.untouched(ws), f"{label}: written although the call was refused"
    assert torch.equal(_bytes(sm.t), _bytes(sums0)) and torch.equal(dn.t, done.to(DEV).view(torch.uint8))

    b = buffers()
    assert call(b, wsb) == WX_OK, label
    gb.check(*b)
    tok, lp, sm, dn, ws = b
    want_done, want_sum = done.to(DEV), sums0.clone()
    want_tok, want_lp = _lib.sample_token(lg, step, eot, want_done, temperature, SEED, sup, want_sum)
    torch.cuda.synchronize()
    for got, want, name in ((tok.t, want_tok, "token"), (lp.t, want_lp, "logprob"), (sm.t, want_sum, "sum_logprob"),
                            (dn.t, want_done.view(torch.uint8), "done")):
        assert torch.equal(_bytes(got), _bytes(want)), f"{label}: {name} differs from the wrapper's"
    assert not gb.untouched(tok) and not gb.untouched(lp)

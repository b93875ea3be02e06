"""The graph-replayed decode step without a GPU: wx_decode_self_attention_f32 / _h16 are declared,
exported and bound; their argument validation in the header's order (no device needed: every case
returns before anything is enqueued; dummy, aligned, never dereferenced pointers); and the refusals
of WhisperDecoder's `graph` and `sync_every` arguments off the HIP route."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from whisper_decoder_helpers import GEOMETRIES, PROMPT, case

HEADER = os.path.join(ROOT, "include", "wx_align.h")
WX_E_INVALID, WX_E_WORKSPACE = 1001, 1004
NAMES = ("wx_decode_self_attention_f32", "wx_decode_self_attention_h16")


def test_the_entry_points_are_declared_exported_and_bound():
    from whisperx_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load(require_device=False)
    for name, n in zip(NAMES, (20, 21)):
        assert re.search(rf"\bint {name}\s*\(", txt), name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n
    for name in ("decode_self_attention_f32", "decode_self_attention_h16", "decode_attention_workspace"):
        assert callable(getattr(_lib, name))


@pytest.mark.parametrize("half", [False, True], ids=["f32", "h16"])
def test_self_attention_entry_validates_before_anything_is_enqueued(half):
    from whisperx_amd import _lib

    lib = _lib.load(require_device=False)
    fn = getattr(lib, NAMES[half])
    p = ctypes.c_void_p(1 << 20)
    off4 = ctypes.c_void_p((1 << 20) + 4)
    rs = (ctypes.c_int64 * 2)(3 * 6 * 64, 64)  # the column blocks of a [B, 3 H 64] GEMM output
    cs = (ctypes.c_int64 * 3)(6 * 448 * 64, 448 * 64, 64)

    def call(B=2, H=6, Lcap=448, D=64, ws=None, q=p, kn=p, vn=p, kc=p, vc=p, o=p, pos=p, wsp=p, q_strides=rs,
             kn_strides=rs, vn_strides=rs, k_strides=cs, v_strides=cs, dtype=1):
        need = lib.wx_decode_attention_workspace_bytes(B, H, Lcap)
        return fn(q, kn, vn, kc, vc, o, B, H, Lcap, D, q_strides, kn_strides, vn_strides, k_strides, v_strides, 0.125,
                  *((dtype,) if half else ()), pos, wsp, need if ws is None else ws, None)

    # the shape (and the dtype) first, before B == 0
    for bad in (dict(B=-1), dict(H=0), dict(Lcap=0), dict(D=32), dict(B=0, D=32), dict(B=0, H=0), dict(B=0, Lcap=0)):
        assert call(**bad) == WX_E_INVALID, bad
    if half:
        for bad in (dict(dtype=0), dict(dtype=3), dict(B=0, dtype=0)):
            assert call(**bad) == WX_E_INVALID, bad
        assert call(B=0, dtype=2) == 0
    # then B == 0, whatever the pointers and the workspace are
    assert call(B=0) == 0 and call(B=0, ws=0, q=None, pos=None, wsp=None) == 0
    # then the pointers: null or misaligned, pos (4-byte aligned) included
    for name in ("q", "kn", "vn", "kc", "vc", "o", "pos", "wsp", "q_strides", "kn_strides", "vn_strides", "k_strides",
                 "v_strides"):
        assert call(**{name: None}) == WX_E_INVALID, name
    for name in ("q", "kn", "vn", "kc", "vc", "o", "wsp"):
        assert call(**{name: off4}) == WX_E_INVALID, name
    assert call(pos=off4, ws=0) == WX_E_WORKSPACE  # 4-byte aligned: legal, the next check speaks
    for off in (1, 2, 3):
        assert call(pos=ctypes.c_void_p((1 << 20) + off)) == WX_E_INVALID, off
    # ... before the workspace's size is looked at
    assert call(pos=None, ws=0) == WX_E_INVALID and call(q=off4, ws=0) == WX_E_INVALID
    # the strides: rows off 16 bytes
    for name in ("q_strides", "kn_strides", "vn_strides"):
        assert call(**{name: (ctypes.c_int64 * 2)(3 * 6 * 64 + 2, 64)}) == WX_E_INVALID, name
        # 4 elements: 16 bytes of floats (legal: the next check speaks), 8 bytes of 16-bit elements
        assert call(**{name: (ctypes.c_int64 * 2)(3 * 6 * 64 + 4, 64), "ws": 0}) == \
            (WX_E_INVALID if half else WX_E_WORKSPACE), name
    for name in ("k_strides", "v_strides"):
        assert call(**{name: (ctypes.c_int64 * 3)(6 * 448 * 64, 448 * 64, 66)}) == WX_E_INVALID, name
        if half:  # 16 bytes are 8 elements
            assert call(**{name: (ctypes.c_int64 * 3)(6 * 448 * 64, 448 * 64, 68)}) == WX_E_INVALID, name
    assert call(B=70000) == WX_E_INVALID and call(H=70000) == WX_E_INVALID
    assert call(B=70000, ws=0) == WX_E_INVALID  # the grid's limits before the workspace
    # then the workspace: wx_decode_attention_workspace_bytes(B, H, Lcap), to the byte
    need = lib.wx_decode_attention_workspace_bytes(2, 6, 448)
    assert need >= 2 * 6 * 4 * 66 * 4  # (m, l, acc[64]) per chunk of Lcap
    assert call(ws=need - 1) == WX_E_WORKSPACE and call(ws=0) == WX_E_WORKSPACE


def _host(model):
    from whisperx_amd import WhisperDecoder

    return WhisperDecoder(model, device="cpu")


def test_graph_is_refused_off_the_hip_route():
    c = case(*GEOMETRIES[0])
    dec = _host(c.model)
    for kernels in (None, False):
        with pytest.raises(ValueError, match="HIP route"):
            dec.start(c.enc, kernels=kernels, graph=True)
        with pytest.raises(ValueError, match="HIP route"):
            dec.start(c.enc, kernels=kernels, beams=3, graph=True)
        with pytest.raises(ValueError, match="HIP route"):
            dec.generate(c.enc, PROMPT, 2, kernels=kernels, graph=True)
        with pytest.raises(ValueError, match="HIP route"):
            dec.generate(c.enc, PROMPT, 2, kernels=kernels, graph=True, prefill=True)
        with pytest.raises(ValueError, match="HIP route"):
            dec.generate(c.enc, PROMPT, 2, kernels=kernels, graph=True, beam_size=3)
        with pytest.raises(ValueError, match="HIP route"):
            dec.beam_search(c.enc, PROMPT, 2, beam_size=2, kernels=kernels, graph=True)
        with pytest.raises(ValueError, match="HIP route"):
            dec.logits(c.enc, [[1, 2]] * c.B, kernels=kernels, graph=True)
    assert dec.graph_captures == 0
    dec.release_graphs()  # nothing to drop: legal


def test_sync_every_below_one_is_refused():
    c = case(*GEOMETRIES[0])
    dec = _host(c.model)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="sync_every"):
            dec.generate(c.enc, PROMPT, 2, sync_every=bad)
        with pytest.raises(ValueError, match="sync_every"):
            dec.generate(c.enc, PROMPT, 2, sync_every=bad, graph=True)
    # graph=False ignores a legal value: the default route, token for token
    assert dec.generate(c.enc, PROMPT, 95, max_length=8, sync_every=3) == dec.generate(c.enc, PROMPT, 95, max_length=8)

"""Where every entry point of include/wx_align.h writes: guard bands around outputs and workspaces.

Each case calls the C ABI directly (whisperx_amd._lib.load() and ctypes) with every output pointer
inside a guard_bands.guarded payload of exactly the size the header states, the workspace (where
there is one) a guarded payload of exactly wx_*_workspace_bytes(...) bytes, and asserts
  (a) WX_OK,
  (b) every band byte unchanged after the stream has drained,
  (c) the outputs equal, bit for bit, what the _lib wrapper returns for the same inputs with its
      ordinary allocations (the rest of the suite pins the wrapper's values),
  (d) with a workspace: workspace_bytes - 1 is WX_E_WORKSPACE and leaves every output byte and every
      workspace byte as it was.
Nothing here rests on a tolerance: every comparison is of bytes.

Payload alignment is the weakest the header allows: 4 bytes for fp32 / int32 data it asks nothing
of, 8 for fp64 / int64, 16 where it asks 16 (2-byte types only ever appear with the 16-byte rule).
A workspace gets 16: the strictest rule the header states for one, and it states none weaker.

Shapes: one below, at and one above every granularity of the launch, read from the kernels.

  entry point                      granularity                              shapes
  -------------------------------  ---------------------------------------  ----------------------------------------
  wx_column0_cumsum                kChunk = 32 rows per chunk               T 0 1 2 30 31 32 33 63 64 65 94 95; V 3
  wx_align_dp, _mode, _ex          32-row chunks; 64-lane waves x cells     every mode of MODES; V 32 and 29: segments
    (5 outputs, workspace,           per lane (buckets by N); V <= 32 /       N 1, 64, 65, 300 with T = N + 2..70 (no
    hand-off region)                 <= 64 / gathered columns                 multiple of 32) and one N > T (status 1);
                                                                              V 1000: one segment (gather route)
  wx_trellis                       the same buckets, throughput shape       the V 32 / 29 batches; trellis exactly
                                                                              sum (T + 1)(N + 1) floats
  wx_backtrack (workspace)         256 threads per segment, 32-row words    the same batches; paths of capacity sum_T
  wx_merge_repeats                 one wave per path, 64 points per pass    the same paths packed back to back, the
                                                                              segment arrays exactly the paths' length
  wx_binarize, wx_binarize_ex      64 frames per word; regions stored 64    files of 0 1 63 64 65 129 4097 frames in
    (workspace)                      at a time; scan (1024 threads) or fsm    one launch; both routes; max_duration
                                     route                                    0.05 and 30; capacity F + 1, exactly the
                                                                              count, and one fewer for each file
  wx_vad_aggregate                 256 frames per block                     n_frames 1 255 256 257; 3 chunks of 8
                                                                              frames; 1 and 3 classes
  wx_lstm_bidir_layer              kLR = 16 sequences per workgroup         (B, T) (1, 1) (15, 2) (16, 3) (17, 5)
  wx_sincnet_stage, _ex            R = 256 / (C / 4) pooled rows per pass,  C 4 (R 256): Lp 255 256 257; C 60 (4R 68):
                                     4 R per unrolled pass; one block per     Lp 67 68 69; C 80 (R 12, 4R 48): Lp 11 12
                                     window                                   13 47 48 49; L = 3 Lp + (Lp % 3); B 2
  wx_sinc_filterbank               256 output rows per block                255 256 257 262 rows; strides 1 3 10 16
  wx_conv1d_taps_tm                128 output frames per block; 64 / 80     TAPS_CHANNELS; L 5 131 132 133 (1 127 128
                                     input channels                           129 frames); B 3
  wx_posconv_packed                128 frames per block                     POSCONV_LENGTHS (0 1 64 65 127 128 129 191
                                                                              193 257); Cg 48 and 64, G 2
  wx_channel_norm (workspace)      256 float4 per block (apply); 64-channel C 4: L 1 255 256 257; C 60 64 68: L 1 5
                                     tiles                                    and 1030 (kSplit 256 x 4 waves, + 6)
  wx_conv0_channel_norm, _h16      64 rows per block (128 on the K 10 /     K 3 stride 2: L 63 64 65; K 10 stride 5:
    (workspace)                      stride 5 route); 64-channel tiles        L 127 128 129; C 8 and 68; f16 and bf16
  wx_add_layernorm, _h16,          4 rows per block (one wave per row);     rows 1 3 4 5; D 256 384 (and 1280 once);
    _h16_dual                        D / 4 float4 per row                     y alone and with the sum; b NULL (h16)
  wx_attention_f32, _packed        32-query tiles, 4 waves over 32-key      T 1 31 32 33 129; packed: POSCONV_LENGTHS
                                     tiles
  wx_attention_h16, _packed        64-query units, 32-key MFMA tiles        T 1 63 64 65 129; packed: the same lengths
  wx_prefill_attention_f32, _h16   32-query tiles                           Tq 1 31 32 33 with Tk = 40 + Tq, causal 40
  wx_log_mel (workspace)           64 frames per block                      B 1 (65 frames) and B 3 (63 64 65 frames)
  wx_whisper_stem (workspace)      64 output rows per block; 64 / 128       Tin 2 126 130; D 64 and 384; B 2
                                     channels per block
  wx_decode_attention_f32, _h16    128 keys per chunk; merge: 4 (b, h)      L 1 128 129 257; (B, H) (1, 3) (2, 2) (1, 5)
    (workspace)                      rows per block
  wx_decode_attention_*_grouped    the same, G queries per workgroup        L 1 128 129 257; G 1 5 8; B 2, H 2
    (workspace)
  wx_decode_self_attention_*       grid fixed by Lcap; row pos appended     Lcap 448; pos 0 127 128 447; the caches
    (workspace)                                                               are guarded payloads too
  wx_beam_topk (workspace)         4096 columns per slice                   V 2G 4095 4096 4097; G 1 5 8; B 2

wx_assign_speakers has no workspace, and test_gpu_diarize.py::
test_outputs_as_views_leave_their_surroundings_untouched already hands it outputs inside checked
buffers.  Every *_workspace_bytes query of the header (11, wx_align_dp_handoff_bytes among them) is
used at its exact size and at one byte fewer.
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_probes as cp
import guard_bands as gb
from oracle import oracle
from test_gpu_parity import MODES, _large_vocab_cases, _random_cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WX_OK, WX_E_WORKSPACE = 0, 1004
F16, BF16 = torch.float16, torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from whisperx_amd import _lib

    return _lib.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _p(x):
    """The device pointer of a Guarded, a tensor or None."""
    if x is None:
        return None
    return ctypes.c_void_p(x.ptr if isinstance(x, gb.Guarded) else x.data_ptr())


def _out(shape, dtype, name):
    """A guarded output at the weakest alignment its element type can have."""
    size = torch.empty(0, dtype=dtype).element_size()
    return gb.guarded(shape, dtype, DEV, offset=16 if size == 2 else max(size, 4), name=name)


def _out16(shape, dtype, name):
    """A guarded output the header wants 16-byte aligned."""
    return gb.guarded(shape, dtype, DEV, offset=16, name=name)


def _workspace(nbytes, name):
    return gb.guarded(int(nbytes), torch.uint8, DEV, offset=16, name=name + " workspace")


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _same(got, want, label):
    """Bit for bit (NaN payloads, signed zeros and all)."""
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), \
        f"{label}: {got.dtype} {tuple(got.shape)} against the wrapper's {want.dtype} {tuple(want.shape)}"
    a, b = _bits(got), _bits(want)
    if not torch.equal(a, b):
        bad = (a != b).nonzero().reshape(-1)
        size = got.element_size()
        raise AssertionError(f"{label}: differs from the wrapper's result in {int(bad.numel())} bytes, elements "
                             f"{int(bad[0]) // size}..{int(bad[-1]) // size} of {got.numel()}")


def _drive(label, make_outs, call, ws_bytes=None):
    """(d), then (a) and (b).  make_outs() -> fresh guarded outputs; call(outs, ws, nbytes) -> the
    entry point's return code (ws a Guarded or None).  Returns the outputs of the real call."""
    if ws_bytes is not None:
        assert ws_bytes > 0, f"{label}: the workspace query returned {ws_bytes}"
        outs, ws = make_outs(), _workspace(ws_bytes, label)
        rc = call(outs, ws, ws_bytes - 1)
        torch.cuda.synchronize()
        assert rc == WX_E_WORKSPACE, f"{label}: a workspace one byte short returned {rc}"
        gb.check(*outs, ws)
        for g in (*outs, ws):
            assert gb.untouched(g), f"{label}: {g.name} was written although the call refused its workspace"
    outs = make_outs()
    ws = _workspace(ws_bytes, label) if ws_bytes is not None else None
    rc = call(outs, ws, ws_bytes)
    torch.cuda.synchronize()
    assert rc == WX_OK, f"{label}: returned {rc}"
    gb.check(*outs, *(() if ws is None else (ws,)))
    return outs


def _gen(*seed):
    g = torch.Generator()
    mixed = 0
    for s in seed:
        mixed = (mixed * 1000003 + int(s)) % (2 ** 31 - 1)
    g.manual_seed(mixed)
    return g


def _randn(g, *shape, scale=1.0, dtype=torch.float32):
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


# ----------------------------------------------------------------------------- column 0
@pytest.mark.parametrize("T", [0, 1, 2, 30, 31, 32, 33, 63, 64, 65, 94, 95])
def test_column0_cumsum(lib, T):
    """S[0..T] and nothing else: the last chunk of 32 rows must not store its sums past S(T).
    While the kernel stored all 32 sums of every chunk, this failed at T = 1, 2, 33 and 65 with the
    tail band changed for 30, 29, 30 and 30 doubles past S[T] (up to S[32 ceil(T / 32) - 1]), and
    passed at T = 0, 31, 32, 63, 64 and 95: with T % 32 in {0, 31} the last chunk ends at S[T].
    T = 30 and 94 are the smallest overrun of that kind, one double."""
    from whisperx_amd import _lib

    em = _randn(_gen(1, T), max(T, 1), 3)[:T].contiguous()

    def call(outs, ws, n):
        return lib.wx_column0_cumsum(_p(em) if T else None, T, 3, _p(outs[0]), _stream())

    (S,) = _drive(f"column0_cumsum T {T}", lambda: [_out(T + 1, torch.float64, f"S (T = {T})")], call)
    _same(S.t, _lib.column0_cumsum(em), f"column0_cumsum T {T}")


# ----------------------------------------------------------------------------- alignment
def _dp_cases(V):
    rng = np.random.default_rng(1000 + V)
    if V > 64:
        return _large_vocab_cases(rng, V, 1, (150, 151), (40, 41), 30)
    cases = []
    for N in (1, 64, 65, 300):
        T = N + 2 + int(rng.integers(0, 69))
        T += 1 if T % 32 == 0 else 0
        cases += _random_cases(rng, 1, (T, T + 1), (N, N + 1), V)
    cases += _random_cases(rng, 1, (10, 11), (30, 31), V)  # N > T: backtrack fails
    return cases


_batches = {}


def _dp_batch(V):
    """The batch of _dp_cases(V), built once."""
    from whisperx_amd import _lib

    if V not in _batches:
        cases = _dp_cases(V)
        _batches[V] = _lib.Batch([torch.from_numpy(c["em"]).to(DEV) for c in cases], [c["tokens"].tolist() for c in cases],
                                 [int(c["blank"]) for c in cases], device=DEV)
    return _batches[V]


def _dp_outs(b):
    nt = b.tok_off[-1]
    return [_out(nt, torch.int32, "seg_start"), _out(nt, torch.int32, "seg_end"), _out(nt, torch.float64, "seg_score"),
            _out(b.S, torch.int32, "t_start"), _out(b.S, torch.int32, "status")]


def _dp_head(b, outs, ws, n):
    return (_p(b.em), _p(b.em_off_d), b.V, _p(b.tok), _p(b.tok_off_d), _p(b.blank), b.S, b.min_N, b.max_N, b.sum_T,
            *(_p(g) for g in outs), _p(ws), n)


def _dp_compare(b, outs, want, label):
    """Against the wrapper: t_start and status of every segment (the hand-off recovery flag aside: it
    reports a transient of the launch, not a result), spans and scores of every aligned one."""
    from whisperx_amd import _lib

    ss, se, sc, ts, st = (g.t for g in outs)
    _same(ts, want[3][:b.S], f"{label}: t_start")
    keep = ~_lib.STATUS_RECOVERED
    _same(st & keep, want[4][:b.S] & keep, f"{label}: status")
    ok = _lib.status_ok(st.cpu().numpy())
    assert ok.tolist() == [n + 2 <= t for n, t in zip(b.Ns, b.Ts)], (label, ok)  # (only the N > T segment fails)
    for s in range(b.S):
        if ok[s]:
            a, e = b.tok_off[s], b.tok_off[s + 1]
            for got, w, name in ((ss, want[0], "seg_start"), (se, want[1], "seg_end"), (sc, want[2], "seg_score")):
                _same(got[a:e], w[a:e], f"{label}: {name} of segment {s}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V", [32, 29, 1000])
def test_align_dp(lib, V, mode):
    """wx_align_dp_ex with a caller-owned hand-off region of exactly wx_align_dp_handoff_bytes (zeroed
    in the payload only), and wx_align_dp_mode, whose hand-off region lies inside the workspace."""
    from whisperx_amd import _lib

    b = _dp_batch(V)
    wsb = lib.wx_align_dp_workspace_bytes(b.S, b.sum_T, b.max_N)
    hob = lib.wx_align_dp_handoff_bytes(b.S, b.sum_T)
    assert hob > 0
    want = _lib.align_dp(b, mode)
    label = f"align_dp V {V} mode {mode}"
    ho = gb.guarded(hob, torch.uint8, DEV, offset=16, name="hand-off region").zero_()

    def call_ex(outs, ws, n):
        return lib.wx_align_dp_ex(*_dp_head(b, outs, ws, n), _p(ho), hob, mode, _stream())

    outs = _drive(label + " (_ex)", lambda: _dp_outs(b), call_ex, wsb)
    gb.check(ho)
    _dp_compare(b, outs, want, label + " (_ex)")

    # a hand-off region one byte short: refused before anything is enqueued
    fresh, ws = _dp_outs(b), _workspace(wsb, label)
    ho2 = gb.guarded(hob, torch.uint8, DEV, offset=16, name="hand-off region").zero_()
    rc = lib.wx_align_dp_ex(*_dp_head(b, fresh, ws, wsb), _p(ho2), hob - 1, mode, _stream())
    torch.cuda.synchronize()
    assert rc == WX_E_WORKSPACE, f"{label}: a hand-off region one byte short returned {rc}"
    gb.check(*fresh, ws, ho2)
    assert all(gb.untouched(g) for g in (*fresh, ws)) and not bool(ho2.payload_bytes().any())

    def call_mode(outs, ws, n):
        return lib.wx_align_dp_mode(*_dp_head(b, outs, ws, n), mode, _stream())

    outs = _drive(label + " (_mode)", lambda: _dp_outs(b), call_mode, wsb)
    _dp_compare(b, outs, want, label + " (_mode)")


@pytest.mark.parametrize("V", [32, 29])
def test_align_dp_auto(lib, V):
    from whisperx_amd import _lib

    b = _dp_batch(V)
    wsb = lib.wx_align_dp_workspace_bytes(b.S, b.sum_T, b.max_N)

    def call(outs, ws, n):
        return lib.wx_align_dp(*_dp_head(b, outs, ws, n), _stream())

    outs = _drive(f"align_dp V {V}", lambda: _dp_outs(b), call, wsb)
    _dp_compare(b, outs, _lib.align_dp(b), f"align_dp V {V}")


@pytest.mark.parametrize("V", [32, 29])
def test_trellis_backtrack_merge_repeats(lib, V):
    """The three materialised stages in a chain, each into buffers of exactly the stated capacity."""
    from whisperx_amd import _lib

    b = _dp_batch(V)
    S = b.S
    want_tr, offs = _lib.trellis(b)
    offs_d = _lib._dev_i64(offs, DEV)

    def call_tr(outs, ws, n):
        return lib.wx_trellis(_p(b.em), _p(b.em_off_d), b.V, _p(b.tok), _p(b.tok_off_d), _p(b.blank), S, b.max_N,
                              _p(outs[0]), _p(offs_d), _stream())

    (tr,) = _drive(f"trellis V {V}", lambda: [_out(offs[-1], torch.float32, "trellis")], call_tr)
    _same(tr.t, want_tr[:offs[-1]], f"trellis V {V}")

    # backtrack: paths of capacity T_s at em_off[s]
    want = _lib.backtrack(b, want_tr, offs)
    wsb = lib.wx_backtrack_workspace_bytes(S, b.sum_T, b.max_N)

    def outs_bt():
        return [_out(b.sum_T, torch.int32, "path_tok"), _out(b.sum_T, torch.int32, "path_time"),
                _out(b.sum_T, torch.float32, "path_prob"), _out(S, torch.int32, "path_len"), _out(S, torch.int32, "t_start")]

    def call_bt(outs, ws, n):
        return lib.wx_backtrack(_p(want_tr), _p(offs_d), _p(b.em), _p(b.em_off_d), b.V, _p(b.tok), _p(b.tok_off_d),
                                _p(b.blank), S, b.max_N, b.sum_T, *(_p(g) for g in outs), _p(ws), n, _stream())

    bt = _drive(f"backtrack V {V}", outs_bt, call_bt, wsb)
    _same(bt[3].t, want[3][:S], f"backtrack V {V}: path_len")
    _same(bt[4].t, want[4][:S], f"backtrack V {V}: t_start")
    plen = want[3][:S].cpu().tolist()
    assert plen[-1] == -1 and all(n > 0 for n in plen[:-1]), plen
    for s in range(S):
        a = b.em_off[s]
        for k, name in enumerate(("path_tok", "path_time", "path_prob")):
            _same(bt[k].t[a:a + max(plen[s], 0)], want[k][a:a + max(plen[s], 0)], f"backtrack V {V}: {name} of segment {s}")

    # merge_repeats: the paths packed back to back, every array exactly their total length
    lens = [max(n, 0) for n in plen]
    poff = [0]
    for n in lens:
        poff.append(poff[-1] + n)
    packed = [torch.cat([want[k][b.em_off[s]:b.em_off[s] + lens[s]] for s in range(S)]).contiguous() for k in range(3)]
    poff_d = _lib._dev_i64(poff, DEV)
    plen_d = want[3][:S].contiguous()
    wm = _lib.merge_repeats(*packed, poff_d, plen_d, DEV)
    total = poff[-1]

    def outs_mr():
        return [_out(total, torch.int32, "seg_tok"), _out(total, torch.int32, "seg_start"), _out(total, torch.int32, "seg_end"),
                _out(total, torch.float64, "seg_score"), _out(S, torch.int32, "seg_count")]

    def call_mr(outs, ws, n):
        return lib.wx_merge_repeats(*(_p(t) for t in packed), _p(poff_d), _p(plen_d), S, *(_p(g) for g in outs), _stream())

    mr = _drive(f"merge_repeats V {V}", outs_mr, call_mr)
    _same(mr[4].t, wm[4][:S], f"merge_repeats V {V}: seg_count")
    cnt = wm[4][:S].cpu().tolist()
    assert cnt[:-1] == b.Ns[:-1] and cnt[-1] == 0, cnt
    for s in range(S):
        for k, name in enumerate(("seg_tok", "seg_start", "seg_end", "seg_score")):
            _same(mr[k].t[poff[s]:poff[s] + cnt[s]], wm[k][poff[s]:poff[s] + cnt[s]], f"merge_repeats V {V}: {name} of path {s}")


# ------------------------------------------------------------------------------ binarize
BIN_LENGTHS = [0, 1, 63, 64, 65, 129, 4097]
BIN_GEOM = (0.016875, 0.0619375)
SCAN = "void wx::binarize_scan_kernel(wx::BinScanArgs)"
FSM = "void wx::binarize_fsm_kernel(wx::BinarizeArgs, wx::BinWords)"


class _BinCase:
    """Uniform noise in files of BIN_LENGTHS frames, thresholded at its median (about every other
    frame an event), with the oracle's regions per file (computed on the CPU, once per setting)."""

    def __init__(self, route, maxd):
        rng = np.random.default_rng(77)
        self.cols = [rng.random(n).astype(np.float32) for n in BIN_LENGTHS]
        med = float(np.float32(np.median(np.concatenate(self.cols))))
        self.onset, self.offset = (med, med) if route == "scan" else (med, float(np.float32(med + 0.125)))
        self.maxd = maxd
        self.starts = [0.25 * i for i in range(len(self.cols))]
        self.regions = [oracle.binarize(c, s, *BIN_GEOM, self.onset, self.offset, max_duration=maxd)
                        for c, s in zip(self.cols, self.starts)]
        self.counts = [len(r) for r in self.regions]
        self.f_off = np.concatenate([[0], np.cumsum(BIN_LENGTHS)]).astype(np.int64)
        n = len(self.cols)
        self.dev = dict(y=torch.from_numpy(np.concatenate(self.cols)).to(DEV), f_off=torch.from_numpy(self.f_off).to(DEV),
                        start=torch.tensor(self.starts, dtype=torch.float64, device=DEV),
                        step=torch.full((n,), BIN_GEOM[0], dtype=torch.float64, device=DEV),
                        dur=torch.full((n,), BIN_GEOM[1], dtype=torch.float64, device=DEV))


_bin_cases = {}


def _bin_case(route, maxd):
    if (route, maxd) not in _bin_cases:
        _bin_cases[route, maxd] = _BinCase(route, maxd)
    return _bin_cases[route, maxd]


def _binarize(lib, c, caps, two_pass, label):
    """One launch over all files with region capacities `caps`, laid back to back.  Returns
    (reg_start, reg_end, reg_count) on the host and the slot offsets."""
    n = len(caps)
    roff = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    roff_d = torch.from_numpy(roff).to(DEV)
    d = c.dev
    total = int(c.f_off[-1])

    def outs():
        return [_out(int(roff[-1]), torch.float64, "reg_start"), _out(int(roff[-1]), torch.float64, "reg_end"),
                _out(n, torch.int64, "reg_count")]

    tail = (c.onset, c.offset, float(c.maxd), 0.0, 0.0)
    if two_pass:
        def call(o, ws, nb):
            return lib.wx_binarize_ex(_p(d["y"]), _p(d["f_off"]), n, total, _p(d["start"]), _p(d["step"]), _p(d["dur"]),
                                      *tail, _p(o[0]), _p(o[1]), _p(roff_d), _p(o[2]), _p(ws), nb, _stream())
        o = _drive(label, outs, call, lib.wx_binarize_workspace_bytes(n, total))
    else:
        def call(o, ws, nb):
            return lib.wx_binarize(_p(d["y"]), _p(d["f_off"]), n, _p(d["start"]), _p(d["step"]), _p(d["dur"]), *tail,
                                   _p(o[0]), _p(o[1]), _p(roff_d), _p(o[2]), _stream())
        o = _drive(label, outs, call)
    return o, roff


def _bin_check_file(c, o, roff, f, label):
    """File f's count and regions equal the oracle's, and its slots past the count were not written."""
    rs, re, cnt = o
    k = c.counts[f]
    assert int(cnt.t[f]) == k, f"{label}: file {f} ({BIN_LENGTHS[f]} frames) has reg_count {int(cnt.t[f])}, the oracle {k}"
    a = int(roff[f])
    got = list(zip(rs.t[a:a + k].cpu().tolist(), re.t[a:a + k].cpu().tolist()))
    assert got == c.regions[f], f"{label}: regions of file {f} ({BIN_LENGTHS[f]} frames)"
    for g in (rs, re):
        assert not bool(gb.written(g)[8 * (a + k):8 * int(roff[f + 1])].any()), \
            f"{label}: {g.name} of file {f} was written past its {k} regions"


@pytest.mark.parametrize("two_pass", [True, False], ids=["binarize_ex", "binarize"])
@pytest.mark.parametrize("maxd", [0.05, 30.0])
@pytest.mark.parametrize("route", ["scan", "fsm"])
def test_binarize(lib, route, maxd, two_pass):
    from whisperx_amd import _lib

    c = _bin_case(route, maxd)
    total = int(c.f_off[-1])
    assert _lib.binarize_plan(c.onset, c.offset, total)[-1] == (SCAN if route == "scan" else FSM)
    assert c.counts[0] == 0 and c.counts[-1] > 4 * 64, c.counts  # far more than one store of 64 regions
    n = len(BIN_LENGTHS)
    label = f"{'binarize_ex' if two_pass else 'binarize'} {route} max_duration {maxd}"
    # capacity F + 1 (always suffices), then exactly the oracle's count
    for what, caps in (("F + 1", [x + 1 for x in BIN_LENGTHS]), ("the count", c.counts)):
        o, roff = _binarize(lib, c, caps, two_pass, f"{label}, capacity {what}")
        for f in range(n):
            _bin_check_file(c, o, roff, f, f"{label}, capacity {what}")
    # one slot fewer than file v needs: -1 for v alone, every other file complete, and nothing
    # written outside v's own (too few) slots, whose neighbours are the other files' regions
    for v in [f for f in range(n) if c.counts[f] > 0]:
        caps = list(c.counts)
        caps[v] -= 1
        what = f"{label}, file {v} one slot short"
        o, roff = _binarize(lib, c, caps, two_pass, what)
        assert int(o[2].t[v]) == -1, f"{what}: reg_count {int(o[2].t[v])}"
        for f in range(n):
            if f != v:
                _bin_check_file(c, o, roff, f, what)


# ----------------------------------------------------------------------------- VAD producer
@pytest.mark.parametrize("n_classes", [1, 3])
@pytest.mark.parametrize("n_frames", [1, 255, 256, 257])
def test_vad_aggregate(lib, n_frames, n_classes):
    from whisperx_amd import _lib

    K = 8
    scores = torch.rand((3, K, n_classes), generator=_gen(2, n_frames, n_classes)).to(DEV)
    sf = sorted([0, min(3, n_frames - 1), max(n_frames - 5, 0)])
    sf_d = _lib._dev_i64(sf, DEV)

    def call(outs, ws, n):
        return lib.wx_vad_aggregate(_p(scores), _p(sf_d), 3, K, n_classes, n_frames, -1.0, _p(outs[0]), _stream())

    (out,) = _drive(f"vad_aggregate n_frames {n_frames}", lambda: [_out(n_frames, torch.float32, "out")], call)
    _same(out.t, _lib.vad_aggregate(scores, sf, n_frames, missing=-1.0), f"vad_aggregate n_frames {n_frames} classes {n_classes}")


@pytest.mark.parametrize("B,T", [(1, 1), (15, 2), (16, 3), (17, 5)])
def test_lstm_bidir_layer(lib, B, T):
    from whisperx_amd import _lib

    g = _gen(3, B, T)
    xp, whh = _randn(g, B, T, 2, 512, scale=0.5), _randn(g, 2, 512, 128, scale=0.05)

    def call(outs, ws, n):
        return lib.wx_lstm_bidir_layer(_p(xp), _p(whh), _p(outs[0]), B, T, 128, _stream())

    (y,) = _drive(f"lstm B {B} T {T}", lambda: [_out16((B, T, 256), torch.float32, "y")], call)
    _same(y.t, _lib.lstm_bidir_layer(xp, whh, B, T), f"lstm B {B} T {T}")


SINCNET_SHAPES = [(4, 255), (4, 256), (4, 257), (60, 67), (60, 68), (60, 69), (80, 11), (80, 12), (80, 13), (80, 47),
                  (80, 48), (80, 49)]


@pytest.mark.parametrize("ex", [False, True], ids=["sincnet_stage", "sincnet_stage_ex"])
@pytest.mark.parametrize("C,Lp", SINCNET_SHAPES)
def test_sincnet_stage(lib, C, Lp, ex):
    """_ex: a per-window input affine and windows that overlap (a window stride of 8 rows)."""
    from whisperx_amd import _lib

    B, L = 2, 3 * Lp + Lp % 3
    g = _gen(4, C, Lp, ex)
    gamma, beta = _randn(g, C, scale=0.5) + 1, _randn(g, C, scale=0.1)
    if ex:
        base = _randn(g, 8 * (B - 1) + L, C)
        x = base.as_strided((B, L, C), (8 * C, C, 1))
        sc, sh = _randn(g, B) + 2, _randn(g, B, C)
    else:
        x, sc, sh = _randn(g, B, L, C), None, None

    def call(outs, ws, n):
        if ex:
            return lib.wx_sincnet_stage_ex(_p(x), B, L, C, x.stride(0), 1, _p(sc), _p(sh), _p(gamma), _p(beta), 1e-5, 0.01,
                                           _p(outs[0]), _stream())
        return lib.wx_sincnet_stage(_p(x), B, L, C, x.stride(0), 1, _p(gamma), _p(beta), 1e-5, 0.01, _p(outs[0]), _stream())

    label = f"sincnet_stage{'_ex' if ex else ''} C {C} Lp {Lp}"
    (y,) = _drive(label, lambda: [_out16((B, Lp, C), torch.float32, "y")], call)
    _same(y.t, _lib.sincnet_stage(x, True, gamma, beta, 1e-5, 0.01, in_scale=sc, in_shift=sh), label)


@pytest.mark.parametrize("S", cp.SINC_STRIDES)
def test_sinc_filterbank(lib, S):
    from whisperx_amd import _lib

    g = _gen(5, S)
    w = torch.nn.functional.pad(torch.randn((cp.SINC_C, cp.SINC_K), generator=g), (0, cp.SINC_KP - cp.SINC_K)).t().contiguous().to(DEV)
    for n in [cp.SINC_K + S * 254] + cp.sinc_spans(S):
        rows = (n - cp.SINC_K) // S + 1
        x = _randn(g, n)

        def call(outs, ws, nb):
            return lib.wx_sinc_filterbank(_p(x), n, S, _p(w), cp.SINC_C, cp.SINC_K, cp.SINC_KP, _p(outs[0]), _stream())

        label = f"sinc_filterbank stride {S}, {rows} rows"
        (y,) = _drive(label, lambda: [_out((rows, cp.SINC_C), torch.float32, "y")], call)
        _same(y.t, _lib.sinc_filterbank(x, w, cp.SINC_K, S), label)


@pytest.mark.parametrize("L", [5, 131, 132, 133])
@pytest.mark.parametrize("Cin,Cout", cp.TAPS_CHANNELS)
def test_conv1d_taps_tm(lib, Cin, Cout, L):
    from whisperx_amd import _lib

    B = cp.TAPS_B
    g = _gen(6, Cin, Cout, L)
    x = _randn(g, B, L, Cin)
    wp = _randn(g, 5, (64 if Cin <= 64 else 80) // 4, 64, 4, scale=0.1)  # [K][CINP / 4][64][4]: any values will do
    bias = _randn(g, Cout)

    def call(outs, ws, n):
        return lib.wx_conv1d_taps_tm(_p(x), B, L, Cin, _p(wp), _p(bias), Cout, 5, _p(outs[0]), _stream())

    label = f"conv1d_taps_tm Cin {Cin} Cout {Cout} L {L}"
    (y,) = _drive(label, lambda: [_out((B, L - 4, Cout), torch.float32, "y")], call)
    _same(y.t, _lib.conv1d_taps_tm(x, wp, bias, Cout, 5), label)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("Cg", [48, 64])
def test_posconv_packed(lib, Cg, residual):
    from whisperx_amd import _lib

    G, D = 2, 2 * Cg
    lengths = cp.POSCONV_LENGTHS
    g = _gen(7, Cg, residual)
    segs = _lib.PackedSegments(lengths)
    h = _randn(g, segs.rows, D)
    wp = _randn(g, G, 128, Cg // 4, Cg, 4, scale=0.02)
    bias = _randn(g, D)
    rows_t, tiles_t, n_tiles, _ = segs.tables(torch.device(DEV), 1, 128)

    def call(outs, ws, n):
        return lib.wx_posconv_packed(_p(h), D, _p(wp), _p(bias), G, 128, len(lengths), _p(rows_t), _p(tiles_t), n_tiles,
                                     int(residual), _p(outs[0]), _stream())

    label = f"posconv_packed Cg {Cg} residual {residual}"
    (y,) = _drive(label, lambda: [_out((segs.rows, D), torch.float32, "out")], call)
    _same(y.t, _lib.posconv_packed(h, wp, bias, G, 128, segs, residual), label)


# ------------------------------------------------------------------------- emission producer
@pytest.mark.parametrize("C,L", [(4, 1), (4, 255), (4, 256), (4, 257), (60, 1), (60, 5), (64, 5), (68, 5), (68, 1030)])
def test_channel_norm(lib, C, L):
    from whisperx_amd import _lib

    g = _gen(8, C, L)
    x, gamma, beta = _randn(g, L, C), _randn(g, C, scale=0.5) + 1, _randn(g, C, scale=0.1)
    for gelu in (0, 1):
        def call(outs, ws, n):
            return lib.wx_channel_norm(_p(x), L, C, _p(gamma), _p(beta), 1e-5, gelu, _p(outs[0]), _p(ws), n, _stream())

        label = f"channel_norm C {C} L {L} gelu {gelu}"
        (y,) = _drive(label, lambda: [_out16((L, C), torch.float32, "y")], call, lib.wx_channel_norm_workspace_bytes(C))
        _same(y.t, _lib.channel_norm(x, gamma, beta, 1e-5, bool(gelu)), label)


@pytest.mark.parametrize("dtype", [torch.float32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("C", [8, 68])
@pytest.mark.parametrize("K,stride,L", [(3, 2, 63), (3, 2, 64), (3, 2, 65), (10, 5, 127), (10, 5, 128), (10, 5, 129)])
def test_conv0_channel_norm(lib, K, stride, L, C, dtype):
    from whisperx_amd import _lib

    S = (L - 1) * stride + K + (stride - 1)  # samples left over past the last frame
    g = _gen(9, K, L, C)
    x, w = _randn(g, S), _randn(g, C, K, scale=0.3)
    gamma, beta = _randn(g, C, scale=0.5) + 1, _randn(g, C, scale=0.1)
    half = dtype != torch.float32

    def call(outs, ws, n):
        if half:
            return lib.wx_conv0_channel_norm_h16(_p(x), S, K, stride, _p(w), None, C, _p(gamma), _p(beta), 1e-5, 1,
                                                 _lib.HALF_DTYPES[dtype], _p(outs[0]), _p(ws), n, _stream())
        return lib.wx_conv0_channel_norm(_p(x), S, K, stride, _p(w), None, C, _p(gamma), _p(beta), 1e-5, 1, _p(outs[0]),
                                         _p(ws), n, _stream())

    label = f"conv0_channel_norm K {K} stride {stride} L {L} C {C} {dtype}"
    (y,) = _drive(label, lambda: [_out((L, C), dtype, "y")], call, lib.wx_conv0_channel_norm_workspace_bytes(L, C))
    want = _lib.conv0_channel_norm_h16(x, w, None, stride, gamma, beta, 1e-5, True, dtype) if half else \
        _lib.conv0_channel_norm(x, w, None, stride, gamma, beta, 1e-5, True)
    _same(y.t, want, label)


@pytest.mark.parametrize("D,rows", [(256, 1), (256, 3), (256, 4), (256, 5), (384, 1), (384, 3), (384, 4), (384, 5), (1280, 5)])
def test_add_layernorm_family(lib, D, rows):
    """wx_add_layernorm (y, then y and the sum), wx_add_layernorm_h16 (b given and NULL) and
    wx_add_layernorm_h16_dual (y32, y16 and the sum), f16 and bf16."""
    from whisperx_amd import _lib

    g = _gen(10, D, rows)
    a, b = _randn(g, rows, D), _randn(g, rows, D)
    gamma, beta = _randn(g, D, scale=0.5) + 1, _randn(g, D, scale=0.1)
    for want_sum in (False, True):
        def outs32():
            return [_out16((rows, D), torch.float32, "y")] + ([_out16((rows, D), torch.float32, "sum_out")] if want_sum else [])

        def call(outs, ws, n):
            return lib.wx_add_layernorm(_p(a), _p(b), rows, D, D, D, _p(gamma), _p(beta), 1e-5, _p(outs[0]),
                                        _p(outs[1]) if want_sum else None, _stream())

        label = f"add_layernorm D {D} rows {rows} sum {want_sum}"
        o = _drive(label, outs32, call)
        want = _lib.add_layernorm(a, b, gamma, beta, 1e-5, want_sum=True)
        for got, w in zip(o, want):
            _same(got.t, w, label)
    for dtype in (F16, BF16):
        code = _lib.HALF_DTYPES[dtype]
        for bh in (b.to(dtype), None):
            def outs16():
                return [_out16((rows, D), dtype, "y"), _out16((rows, D), torch.float32, "sum_out")]

            def call16(outs, ws, n):
                return lib.wx_add_layernorm_h16(_p(a), _p(bh), rows, D, D, D, _p(gamma), _p(beta), 1e-5, code, _p(outs[0]),
                                                _p(outs[1]), _stream())

            label = f"add_layernorm_h16 D {D} rows {rows} {dtype} b {'given' if bh is not None else 'NULL'}"
            o = _drive(label, outs16, call16)
            for got, w in zip(o, _lib.add_layernorm_h16(a, bh, gamma, beta, 1e-5, dtype, want_sum=True)):
                _same(got.t, w, label)

        def outs_dual():
            return [_out16((rows, D), torch.float32, "y32"), _out16((rows, D), dtype, "y16"),
                    _out16((rows, D), torch.float32, "sum_out")]

        bh = b.to(dtype)

        def call_dual(outs, ws, n):
            return lib.wx_add_layernorm_h16_dual(_p(a), _p(bh), rows, D, D, D, _p(gamma), _p(beta), 1e-5, code,
                                                 *(_p(x) for x in outs), _stream())

        label = f"add_layernorm_h16_dual D {D} rows {rows} {dtype}"
        o = _drive(label, outs_dual, call_dual)
        for got, w in zip(o, _lib.add_layernorm_h16_dual(a, bh, gamma, beta, 1e-5, dtype, want_y32=True, want_sum=True)):
            _same(got.t, w, label)


# ---------------------------------------------------------------------- encoder attention
def _strides(t, n):
    return (ctypes.c_int64 * n)(*(int(s) for s in t.stride()[:n]))


@pytest.mark.parametrize("dtype", [torch.float32, F16, BF16], ids=["f32", "f16", "bf16"])
def test_attention(lib, dtype):
    from whisperx_amd import _lib

    half = dtype != torch.float32
    B, H = 2, 2
    for T in (1, 63, 64, 65, 129) if half else (1, 31, 32, 33, 129):
        g = _gen(11, T, half)
        q, k, v = (_randn(g, B, H, T, 64, dtype=dtype) for _ in range(3))
        st = [_strides(t, 3) for t in (q, k, v)]

        def call(outs, ws, n):
            if half:
                return lib.wx_attention_h16(_p(q), _p(k), _p(v), _p(outs[0]), B, H, T, 64, *st, 0.125,
                                            _lib.HALF_DTYPES[dtype], _stream())
            return lib.wx_attention_f32(_p(q), _p(k), _p(v), _p(outs[0]), B, H, T, 64, *st, 0.125, _stream())

        label = f"attention {dtype} T {T}"
        (o,) = _drive(label, lambda: [_out16((B, T, H, 64), dtype, "o")], call)
        _same(o.t, (_lib.attention_h16 if half else _lib.attention_f32)(q, k, v, 0.125), label)


@pytest.mark.parametrize("dtype", [torch.float32, F16, BF16], ids=["f32", "f16", "bf16"])
def test_attention_packed(lib, dtype):
    from whisperx_amd import _lib

    half = dtype != torch.float32
    H = 2
    lengths = cp.POSCONV_LENGTHS
    segs = _lib.PackedSegments(lengths)
    R = segs.rows
    g = _gen(12, half)
    q, k, v = (_randn(g, 1, H, R, 64, dtype=dtype) for _ in range(3))
    st = [(ctypes.c_int64 * 2)(int(t.stride(1)), int(t.stride(2))) for t in (q, k, v)]
    rows_t, units_t, n_units, _ = segs.tables(torch.device(DEV), H, 64 if half else 32)

    def call(outs, ws, n):
        if half:
            return lib.wx_attention_h16_packed(_p(q), _p(k), _p(v), _p(outs[0]), len(lengths), _p(rows_t), _p(units_t),
                                               n_units, H, 64, *st, 0.125, _lib.HALF_DTYPES[dtype], _stream())
        return lib.wx_attention_f32_packed(_p(q), _p(k), _p(v), _p(outs[0]), len(lengths), _p(rows_t), _p(units_t),
                                           n_units, H, 64, *st, 0.125, 0, _stream())

    label = f"attention packed {dtype}"
    (o,) = _drive(label, lambda: [_out16((1, R, H, 64), dtype, "o")], call)
    _same(o.t, (_lib.attention_h16_packed if half else _lib.attention_f32_packed)(q, k, v, 0.125, segs), label)


@pytest.mark.parametrize("dtype", [torch.float32, F16], ids=["f32", "f16"])
def test_prefill_attention(lib, dtype):
    from whisperx_amd import _lib

    half = dtype != torch.float32
    B, H = 2, 2
    for Tq in (1, 31, 32, 33):
        Tk = 40 + Tq
        g = _gen(13, Tq, half)
        q = _randn(g, B, H, Tq, 64, dtype=dtype)
        k, v = (_randn(g, B, H, Tk, 64, dtype=dtype) for _ in range(2))
        st = [_strides(t, 3) for t in (q, k, v)]

        def call(outs, ws, n):
            if half:
                return lib.wx_prefill_attention_h16(_p(q), _p(k), _p(v), _p(outs[0]), B, H, Tq, Tk, 40, 64, *st, 0.125,
                                                    _lib.HALF_DTYPES[dtype], _stream())
            return lib.wx_prefill_attention_f32(_p(q), _p(k), _p(v), _p(outs[0]), B, H, Tq, Tk, 40, 64, *st, 0.125, _stream())

        label = f"prefill_attention {dtype} Tq {Tq}"
        (o,) = _drive(label, lambda: [_out16((B, Tq, H, 64), dtype, "o")], call)
        _same(o.t, (_lib.prefill_attention_h16 if half else _lib.prefill_attention_f32)(q, k, v, 0.125, causal=40), label)


# --------------------------------------------------------------------------------- Whisper
@pytest.mark.parametrize("frames", [(65,), (63, 64, 65)], ids=["B1", "B3"])
def test_log_mel(lib, frames):
    """Chunk b writes frames 0 .. L_b / 160 - 1 of its rows of an output of exactly B n_mels
    n_frames_max floats (row_stride = n_frames_max) and leaves the other frames unwritten."""
    from whisperx_amd import _lib

    B, n_mels = len(frames), 80
    first = [37 + 11 * i for i in range(B)]
    pad = [320 * (i % 2) for i in range(B)]
    length = [160 * f + 7 - p for f, p in zip(frames, pad)]
    g = _gen(14, B)
    wave = _randn(g, max(a + n for a, n in zip(first, length)) + 5, scale=0.1)
    filters = torch.rand((n_mels, 201), generator=g).to(DEV) * 0.02
    fmax = max(frames)
    ch = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.int64) for x in (first, length, pad)]))
    ch_d = torch.from_numpy(ch.reshape(-1)).to(DEV)
    host = [ctypes.c_void_p(ch[i].ctypes.data) for i in range(3)]
    basis = _lib.mel_basis(torch.device(DEV))

    def call(outs, ws, n):
        return lib.wx_log_mel(_p(wave), wave.numel(), *host, _p(ch_d), B, n_mels, _p(filters), _p(basis), _p(outs[0]), fmax,
                              fmax, _p(ws), n, _stream())

    label = f"log_mel B {B}"
    (out,) = _drive(label, lambda: [_out((B, n_mels, fmax), torch.float32, "out")], call, lib.wx_log_mel_workspace_bytes(B))
    want = _lib.log_mel(wave, first, length, pad, filters)
    wr = gb.written(out).reshape(B, n_mels, fmax, 4)
    for b, f in enumerate(frames):
        _same(out.t[b, :, :f], want[b, :, :f], f"{label}: chunk {b}")
        assert not bool(wr[b, :, f:].any()), f"{label}: chunk {b} was written past its {f} frames"


@pytest.mark.parametrize("D", [64, 384])
@pytest.mark.parametrize("Tin", [2, 126, 130])
def test_whisper_stem(lib, Tin, D):
    from whisperx_amd import _lib

    B, M = 2, 80
    g = _gen(15, Tin, D)
    x = _randn(g, B, M, Tin)
    w1, w2 = _randn(g, D // 16, 3, M // 16, 64, 4, scale=0.1), _randn(g, D // 16, 3, D // 16, 64, 4, scale=0.05)
    b1, b2, pos = _randn(g, D), _randn(g, D), _randn(g, Tin // 2, D)

    def call(outs, ws, n):
        return lib.wx_whisper_stem(_p(x), M * Tin, Tin, B, M, Tin, _p(w1), _p(b1), _p(w2), _p(b2), _p(pos), D, _p(outs[0]),
                                   _p(ws), n, _stream())

    label = f"whisper_stem Tin {Tin} D {D}"
    (out,) = _drive(label, lambda: [_out16((B, Tin // 2, D), torch.float32, "out")], call,
                    lib.wx_whisper_stem_workspace_bytes(B, Tin, D))
    _same(out.t, _lib.whisper_stem(x, w1, b1, w2, b2, pos), label)


@pytest.mark.parametrize("dtype", [torch.float32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("L", [1, 128, 129, 257])
def test_decode_attention(lib, L, dtype):
    from whisperx_amd import _lib

    half = dtype != torch.float32
    for B, H in ((1, 3), (2, 2), (1, 5)):
        g = _gen(16, L, B, H, half)
        q = _randn(g, B, H, 64, dtype=dtype)
        k, v = (_randn(g, B, H, L, 64, dtype=dtype) for _ in range(2))
        st = [_strides(q, 2), _strides(k, 3), _strides(v, 3)]

        def call(outs, ws, n):
            if half:
                return lib.wx_decode_attention_h16(_p(q), _p(k), _p(v), _p(outs[0]), B, H, L, 64, *st, 0.125,
                                                   _lib.HALF_DTYPES[dtype], _p(ws), n, _stream())
            return lib.wx_decode_attention_f32(_p(q), _p(k), _p(v), _p(outs[0]), B, H, L, 64, *st, 0.125, _p(ws), n, _stream())

        label = f"decode_attention {dtype} L {L} B {B} H {H}"
        (o,) = _drive(label, lambda: [_out16((B, H, 64), dtype, "o")], call, lib.wx_decode_attention_workspace_bytes(B, H, L))
        _same(o.t, (_lib.decode_attention_h16 if half else _lib.decode_attention_f32)(q, k, v, 0.125), label)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("G", [1, 5, 8])
def test_decode_attention_grouped(lib, G, dtype):
    from whisperx_amd import _lib

    half = dtype != torch.float32
    B, H = 2, 2
    for L in (1, 128, 129, 257):
        g = _gen(17, L, G, half)
        q = _randn(g, B, G, H, 64, dtype=dtype)
        k, v = (_randn(g, B, H, L, 64, dtype=dtype) for _ in range(2))
        st = [_strides(q, 3), _strides(k, 3), _strides(v, 3)]

        def call(outs, ws, n):
            if half:
                return lib.wx_decode_attention_h16_grouped(_p(q), _p(k), _p(v), _p(outs[0]), B, G, H, L, 64, *st, 0.125,
                                                           _lib.HALF_DTYPES[dtype], _p(ws), n, _stream())
            return lib.wx_decode_attention_f32_grouped(_p(q), _p(k), _p(v), _p(outs[0]), B, G, H, L, 64, *st, 0.125, _p(ws), n,
                                                       _stream())

        label = f"decode_attention_grouped {dtype} G {G} L {L}"
        (o,) = _drive(label, lambda: [_out16((B, G, H, 64), dtype, "o")], call,
                      lib.wx_decode_attention_grouped_workspace_bytes(B, G, H, L))
        _same(o.t, (_lib.decode_attention_h16_grouped if half else _lib.decode_attention_f32_grouped)(q, k, v, 0.125), label)


@pytest.mark.parametrize("dtype", [torch.float32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("pos", [0, 127, 128, 447])
def test_decode_self_attention(lib, pos, dtype):
    """The caches are outputs too (row pos is appended): each lies in a guarded payload of exactly
    [B][H][Lcap][64] elements, and afterwards differs from its earlier contents in row pos alone."""
    from whisperx_amd import _lib

    half = dtype != torch.float32
    B, H, Lcap = 1, 3, 448
    g = _gen(18, pos, half)
    q, kn, vn = (_randn(g, B, H, 64, dtype=dtype) for _ in range(3))
    k0, v0 = (_randn(g, B, H, Lcap, 64, dtype=dtype) for _ in range(2))
    pos_d = torch.tensor([pos], dtype=torch.int32, device=DEV)
    st = [_strides(q, 2), _strides(kn, 2), _strides(vn, 2), _strides(k0, 3), _strides(v0, 3)]
    wsb = lib.wx_decode_attention_workspace_bytes(B, H, Lcap)
    fn = lib.wx_decode_self_attention_h16 if half else lib.wx_decode_self_attention_f32
    label = f"decode_self_attention {dtype} pos {pos}"

    def run(nbytes):
        kc, vc = _out16((B, H, Lcap, 64), dtype, "k_cache"), _out16((B, H, Lcap, 64), dtype, "v_cache")
        kc.t.copy_(k0)
        vc.t.copy_(v0)
        o, ws = _out16((B, H, 64), dtype, "o"), _workspace(wsb, label)
        rc = fn(_p(q), _p(kn), _p(vn), _p(kc), _p(vc), _p(o), B, H, Lcap, 64, *st, 0.125,
                *((_lib.HALF_DTYPES[dtype],) if half else ()), _p(pos_d), _p(ws), nbytes, _stream())
        torch.cuda.synchronize()
        gb.check(kc, vc, o, ws)
        return rc, kc, vc, o, ws

    rc, kc, vc, o, ws = run(wsb - 1)
    assert rc == WX_E_WORKSPACE, f"{label}: a workspace one byte short returned {rc}"
    assert gb.untouched(o) and gb.untouched(ws), label
    _same(kc.t, k0, label + ": k_cache after the refused call")
    _same(vc.t, v0, label + ": v_cache after the refused call")
    rc, kc, vc, o, ws = run(wsb)
    assert rc == WX_OK, f"{label}: returned {rc}"
    k1, v1 = k0.clone(), v0.clone()
    want = (_lib.decode_self_attention_h16 if half else _lib.decode_self_attention_f32)(q, kn, vn, k1, v1, pos_d, 0.125)
    _same(o.t, want, label)
    _same(kc.t, k1, label + ": k_cache")
    _same(vc.t, v1, label + ": v_cache")
    rest = [r for r in range(Lcap) if r != pos]
    _same(kc.t[:, :, rest], k0[:, :, rest], label + ": k_cache rows other than pos")
    _same(vc.t[:, :, rest], v0[:, :, rest], label + ": v_cache rows other than pos")


@pytest.mark.parametrize("G", [1, 5, 8])
def test_beam_topk(lib, G):
    from whisperx_amd import _lib

    B = 2
    for V in (2 * G, 4095, 4096, 4097):
        g = _gen(19, G, V)
        logits, cum = _randn(g, B * G, V, scale=3.0), -torch.rand(B * G, generator=g).to(DEV) * 5

        def call(outs, ws, n):
            return lib.wx_beam_topk(_p(logits), V, _p(cum), B, G, V, _p(outs[0]), _p(outs[1]), _p(ws), n, _stream())

        label = f"beam_topk G {G} V {V}"
        o = _drive(label, lambda: [_out((B, 2 * G), torch.float32, "scores"), _out((B, 2 * G), torch.int32, "index")], call,
                   lib.wx_beam_topk_workspace_bytes(B, G, V))
        for got, w, name in zip(o, _lib.beam_topk(logits, cum, G), ("scores", "index")):
            _same(got.t, w, f"{label}: {name}")

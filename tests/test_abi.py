"""The C-ABI library loads and exports every symbol include/wx_align.h declares (CPU only:
no compute calls; argument validation paths return before any launch)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "wx_align.h")


def declared_symbols():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(wx_[a-z_0-9]+)\s*\(", txt)))


def declared_arities():
    """name -> parameter count of every wx_* prototype in the header: comments stripped, the
    top-level commas of the parameter list counted, `void` (or nothing) is 0."""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    out = {}
    for m in re.finditer(r"\b(wx_[a-z_0-9]+)\s*\(", txt):
        depth, i, commas = 1, m.end(), 0
        while depth:
            c = txt[i]
            depth += (c == "(") - (c == ")")
            commas += c == "," and depth == 1
            i += 1
        params = txt[m.end():i - 1].strip()
        assert txt[i:].lstrip().startswith(";"), f"{m.group(1)}: not a prototype"
        out[m.group(1)] = 0 if params in ("", "void") else commas + 1
    return out


@pytest.fixture(scope="module")
def lib():
    from whisperx_amd import _lib

    _lib.build()
    return _lib.load(require_device=False)


def test_header_lists_expected_entry_points():
    syms = declared_symbols()
    for s in ("wx_align_dp", "wx_trellis", "wx_backtrack", "wx_merge_repeats", "wx_binarize"):
        assert s in syms


def test_library_exports_every_declared_symbol(lib):
    from whisperx_amd import _lib

    for s in declared_symbols():
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, f"{s} not bound in _lib.SIGNATURES"


def test_bindings_have_the_declared_arity():
    """A ctypes call with an argument too few is accepted silently and reads garbage: every
    SIGNATURES entry lists as many argtypes as the header's prototype has parameters."""
    from whisperx_amd import _lib

    arity = declared_arities()
    assert sorted(arity) == declared_symbols() and len(arity) >= 34
    for name, n in arity.items():
        assert len(_lib.SIGNATURES[name][1]) == n, name


def _batch_attrs(b):
    import torch

    return {k: (v.dtype, tuple(v.shape), v.tolist()) if torch.is_tensor(v) else v for k, v in vars(b).items()}


@pytest.mark.parametrize("Ts,tokens,blanks", [([5, 0, 3], [[1, 2], [], [3]], [0, 0, 6]), ([], [], [])])
def test_batch_constructors_agree(Ts, tokens, blanks):
    """Batch(list of emissions) and Batch.from_csr(packed matrix) build the same batch: every
    attribute equal, tensors in dtype, shape and value (host tensors; no device, no library)."""
    import torch

    from whisperx_amd import _lib

    g = torch.Generator().manual_seed(3)
    ems = [torch.randn(T, 7, generator=g) for T in Ts]
    a = _lib.Batch(ems, tokens, blanks, device="cpu")
    b = _lib.Batch.from_csr(a.em, Ts, tokens, blanks)
    A, B = _batch_attrs(a), _batch_attrs(b)
    assert set(A) == set(B) >= {"S", "device", "V", "Ts", "Ns", "em_off", "tok_off", "sum_T", "em", "tok", "blank",
                                "em_off_d", "tok_off_d", "min_N", "max_N"}
    for k in A:
        assert A[k] == B[k], k
    assert a.S == len(Ts) and a.sum_T == sum(Ts) and a.em_off == [0] + [sum(Ts[:i + 1]) for i in range(len(Ts))]
    assert a.V == (7 if Ts else 1) and a.tok.tolist() == ([x for t in tokens for x in t] or [0])
    assert a.blank.tolist() == (blanks or [0]) and (a.min_N, a.max_N) == ((0, 2) if Ts else (0, 0))
    if Ts:
        assert torch.equal(a.em, torch.cat(ems, 0))


def test_version_and_errors(lib):
    assert b"gfx950" in lib.wx_version()
    assert lib.wx_strerror(0) == b"ok"
    assert b"workspace" in lib.wx_strerror(1004)


def test_workspace_queries_monotone(lib):
    a = lib.wx_align_dp_workspace_bytes(64, 64 * 1499, 500)
    b = lib.wx_align_dp_workspace_bytes(128, 128 * 1499, 500)
    assert 0 < a < b
    assert lib.wx_backtrack_workspace_bytes(4, 4000, 900) > 0


def test_argument_validation_without_device(lib):
    # S < 0 and oversized vocab/tokens are rejected before anything touches the device
    assert lib.wx_align_dp(None, None, 32, None, None, None, -1, 0, 0, 0, None, None, None, None, None,
                           None, 0, None) == 1001
    assert lib.wx_align_dp(None, None, 32, None, None, None, 0, 0, 0, 0, None, None, None, None, None,
                           None, 0, None) == 0
    dummy = ctypes.c_void_p(8)
    assert lib.wx_align_dp(dummy, dummy, 20000, dummy, dummy, dummy, 1, 1, 1, 10, dummy, dummy, dummy, dummy,
                           dummy, dummy, 1 << 30, None) == 1002
    assert lib.wx_align_dp(dummy, dummy, 32, dummy, dummy, dummy, 1, 1, 20000, 10, dummy, dummy, dummy, dummy,
                           dummy, dummy, 1 << 30, None) == 1003
    assert lib.wx_align_dp(dummy, dummy, 32, dummy, dummy, dummy, 1, 1, 10, 10, dummy, dummy, dummy, dummy,
                           dummy, dummy, 16, None) == 1004
    assert lib.wx_align_dp_mode(dummy, dummy, 32, dummy, dummy, dummy, 1, 1, 10, 10, dummy, dummy, dummy, dummy,
                                dummy, dummy, 1 << 30, 7, None) == 1001  # unknown launch shape
    assert lib.wx_binarize(None, None, -1, None, None, None, 0.5, 0.3, 1.0, 0.0, 0.0, None, None, None, None,
                           None) == 1001
    ws = lib.wx_binarize_workspace_bytes(3, 213334)
    assert ws >= 24 * (213334 // 64 + 4)
    assert lib.wx_binarize_ex(dummy, dummy, 3, 213334, dummy, dummy, dummy, 0.5, 0.3, 30.0, 0.0, 0.0, dummy, dummy,
                              dummy, dummy, dummy, ws - 1, None) == 1004
    assert lib.wx_binarize_ex(None, None, -1, 0, None, None, None, 0.5, 0.3, 1.0, 0.0, 0.0, None, None, None, None,
                              None, 0, None) == 1001


def test_launch_plan_bucket_selection(lib):
    """Host-side launch planning (wx_align_dp_plan, no device work): the kernels a batch maps
    to in each launch shape."""
    from whisperx_amd import _lib

    k = "void wx::align_dp_kernel<{}>(wx::AlignArgs)".format
    sk = "void wx::align_dp_split_kernel<{}>(wx::AlignArgs)".format
    # config 2 (64 x 30 s, N 300..500): one latency launch, each segment over 4 CUs (the
    # planner assumes 256 CUs without a device); 128 segments: one CU per segment
    assert _lib.align_dp_plan(64, 300, 500, 32) == [sk("1, 32, 4")]
    assert _lib.align_dp_plan(128, 300, 500, 32) == [k("2, 32, 7, 1")]
    assert _lib.align_dp_plan(64, 300, 500, 32, _lib.MODE_LATENCY) == [k("2, 32, 7, 1")]
    assert _lib.align_dp_plan(64, 300, 500, 32, _lib.MODE_LATENCY_1CU) == [k("2, 32, 7, 1")]
    # split over 4 CUs: one split kernel for the whole batch (the bucket of its longest segment)
    assert _lib.align_dp_plan(64, 300, 500, 32, _lib.MODE_SPLIT4) == [sk("1, 32, 4")]
    assert _lib.align_dp_plan(64, 300, 1100, 32, _lib.MODE_SPLIT4) == [sk("2, 32, 3")]
    # ... short segments a wide split bucket cannot lay out take throughput buckets beside it
    assert _lib.align_dp_plan(64, 1, 2000, 32, _lib.MODE_SPLIT4) == [sk("4, 32, 3"), k("1, 32, 1, 0")]
    # saturated batches: throughput buckets by N; V picks the LDS row width (32 / 64 / gather)
    assert _lib.align_dp_plan(4096, 300, 500, 32) == [k("6, 32, 1, 0"), k("8, 32, 1, 0")]
    assert _lib.align_dp_plan(2048, 850, 951, 40) == [k("8, 64, 2, 0")]
    assert _lib.align_dp_plan(2048, 850, 951, 1000) == [k("8, 256, 2, 0")]
    assert _lib.align_dp_plan(0, 1, 1, 32) == []


def test_product_refuses_without_device():
    import torch

    from whisperx_amd import _lib

    if torch.cuda.is_available():
        pytest.skip("a device is visible")
    with pytest.raises(_lib.WXError):
        _lib.load(require_device=True)


def test_binarize_plan_kernel_selection(lib):
    """wx_binarize_plan (no device work): offset <= onset takes the parallel scan, offset >
    onset (vad.py:146-175: a frame may both set and reset) the event-jumping state machine."""
    from whisperx_amd import _lib

    words = "void wx::binarize_words_kernel(wx::BinWordArgs)"
    scan = "void wx::binarize_scan_kernel(wx::BinScanArgs)"
    fsm = "void wx::binarize_fsm_kernel(wx::BinarizeArgs, wx::BinWords)"
    assert _lib.binarize_plan(0.5, 0.363, 1000) == [words, scan]
    assert _lib.binarize_plan(0.5, 0.5, 1000) == [words, scan]
    assert _lib.binarize_plan(0.4, 0.6, 1000) == [words, fsm]
    assert _lib.binarize_plan(0.5, 0.55, 0) == [fsm]


CSRC = os.path.join(ROOT, "whisperx_amd", "csrc")


HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))
# the DP headers also with the phase-timing macros' bodies (wx_dp_timing.h)
HEADER_BUILDS = [(h, "") for h in HEADERS] + [(h, "-DWX_PHASE_TIMING") for h in HEADERS if "_dp" in h]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not installed")
@pytest.mark.parametrize("header,flag", HEADER_BUILDS)
def test_header_compiles_on_its_own(header, flag, tmp_path):
    """Every csrc header includes what it uses: a translation unit of that one #include passes
    hipcc's syntax check for gfx950 with the build's flags."""
    from whisperx_amd import _lib

    tu = tmp_path / "tu.hip"
    tu.write_text(f'#include "{os.path.join(CSRC, header)}"\n')
    res = subprocess.run(["hipcc", *_lib.BASE_FLAGS, *flag.split(), f"-I{_lib.INCLUDE_DIR}", "-x", "hip",
                          "-fsyntax-only", str(tu)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

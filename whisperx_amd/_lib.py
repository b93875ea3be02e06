"""ctypes binding of libwxalign.so (C ABI in include/wx_align.h).

Everything in this module needs the shared object and a HIP device: if either is missing,
every entry point raises.  The package's host routes live in `audio`, `diarize` and `vad`.

Tensors are PyTorch device tensors (torch is plumbing here: device memory and streams);
the library sees raw device pointers, sizes and the current HIP stream.
"""
from __future__ import annotations

import ctypes
import glob
import os
import subprocess
import threading
from typing import Optional

import numpy as np

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WX_LIB_PATH") or os.path.join(_HERE, "libwxalign.so")
SRC_PATH = os.path.join(_HERE, "csrc", "wx_align.hip")
SRC_PATHS = [SRC_PATH, os.path.join(_HERE, "csrc", "wx_binarize.hip"), os.path.join(_HERE, "csrc", "wx_emission.hip"),
             os.path.join(_HERE, "csrc", "wx_add_layernorm.hip"),
             os.path.join(_HERE, "csrc", "wx_vad.hip"), os.path.join(_HERE, "csrc", "wx_diarize.hip"),
             os.path.join(_HERE, "csrc", "wx_mel.hip"), os.path.join(_HERE, "csrc", "wx_whisper.hip"),
             os.path.join(_HERE, "csrc", "wx_decode.hip"), os.path.join(_HERE, "csrc", "wx_beam.hip"),
             os.path.join(_HERE, "csrc", "wx_attention_h16.hip"), os.path.join(_HERE, "csrc", "wx_prefill.hip"),
             os.path.join(_HERE, "csrc", "wx_sample.hip"), os.path.join(_HERE, "csrc", "wx_penalty.hip")]
INST_PATH = os.path.join(_HERE, "csrc", "wx_align_inst.hip")
HDR_PATHS = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.h"))) + [INST_PATH]  # (a new header: a rebuild)
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

MAX_VOCAB = 16384
MAX_SEGMENT_COLUMNS = 256  # V > 64: distinct emission columns one segment may use
MAX_TOKENS = 16000
# wx_align_dp status word (include/wx_align.h): outcome in the low bits, route flags above
STATUS_MASK, STATUS_RECOVERED, STATUS_GENERIC = 15, 16, 32


def status_ok(status):
    """Aligned segments of a status array (numpy or torch): outcome 0, whatever the flags."""
    return (status & STATUS_MASK) == 0


def status_summary(status) -> dict:
    """Counts of a status array: aligned, None, and the segments the in-kernel generic
    forward computed (recovered after a lost hand-off / too many columns)."""
    st = status.cpu().numpy() if torch.is_tensor(status) else np.asarray(status)
    out = st & STATUS_MASK
    return {"aligned": int((out == 0).sum()), "none": int((out == 1).sum()),
            "not_computed": int((out >= 2).sum()),
            "recovered_segments": int(((st & STATUS_RECOVERED) != 0).sum()),
            "generic_forward_segments": int(((st & STATUS_GENERIC) != 0).sum())}

_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_f32 = ctypes.c_float
_f64 = ctypes.c_double
_sz = ctypes.c_size_t

# name -> (restype, argtypes); every symbol declared in include/wx_align.h
SIGNATURES = {
    "wx_version": (ctypes.c_char_p, []),
    "wx_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "wx_trellis": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp]),
    "wx_backtrack_workspace_bytes": (_sz, [_i32, _i64, _i64]),
    "wx_backtrack": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i64, _i64,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "wx_merge_repeats": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wx_column0_cumsum": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp]),
    "wx_align_dp_workspace_bytes": (_sz, [_i32, _i64, _i64]),
    "wx_align_dp": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _i64, _i64, _i64,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "wx_align_dp_mode": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _i64, _i64, _i64,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    "wx_align_dp_handoff_bytes": (_sz, [_i32, _i64]),
    "wx_align_dp_ex": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _i64, _i64, _i64,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _i32, _vp]),
    "wx_align_dp_plan": (ctypes.c_int, [_i32, _i64, _i64, _i32, _i32, ctypes.c_char_p, _sz]),
    "wx_channel_norm_workspace_bytes": (_sz, [_i32]),
    "wx_channel_norm": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _f32, _i32, _vp, _vp, _sz, _vp]),
    "wx_conv0_channel_norm_workspace_bytes": (_sz, [_i64, _i32]),
    "wx_conv0_channel_norm": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _f32, _i32, _vp, _vp,
                                             _sz, _vp]),
    "wx_add_layernorm": (ctypes.c_int, [_vp, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _f32, _vp, _vp, _vp]),
    "wx_sincnet_stage_ex": (ctypes.c_int, [_vp, _i64, _i64, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _f32, _f32, _vp, _vp]),
    "wx_vad_aggregate": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _i64, _f32, _vp, _vp]),
    "wx_attention_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _f32, _vp]),
    "wx_conv1d_taps_tm": (ctypes.c_int, [_vp, _i64, _i64, _i32, _vp, _vp, _i32, _i32, _vp, _vp]),
    "wx_sinc_filterbank": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp, _vp]),
    "wx_lstm_bidir_layer": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _i32, _vp]),
    "wx_posconv_packed": (ctypes.c_int, [_vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp]),
    "wx_attention_f32_packed": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp,
                                               _f32, _i32, _vp]),
    "wx_binarize": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _f32, _f32, _f64, _f64, _f64,
                                   _vp, _vp, _vp, _vp, _vp]),
    "wx_binarize_workspace_bytes": (_sz, [_i32, _i64]),
    "wx_binarize_ex": (ctypes.c_int, [_vp, _vp, _i32, _i64, _vp, _vp, _vp, _f32, _f32, _f64, _f64, _f64,
                                      _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "wx_binarize_plan": (ctypes.c_int, [_f32, _f32, _i64, ctypes.c_char_p, _sz]),
    "wx_sincnet_stage": (ctypes.c_int, [_vp, _i64, _i64, _i32, _i64, _i32, _vp, _vp, _f32, _f32, _vp, _vp]),
    "wx_assign_speakers": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i32, _i64, _i32,
                                          _vp, _vp, _vp]),
    "wx_log_mel_workspace_bytes": (_sz, [_i32]),
    "wx_log_mel": (ctypes.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i64, _i64, _vp, _sz, _vp]),
    "wx_whisper_stem_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "wx_whisper_stem": (ctypes.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _sz, _vp]),
    "wx_decode_attention_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "wx_decode_attention_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _f32, _vp, _sz, _vp]),
    "wx_decode_attention_grouped_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "wx_decode_attention_f32_grouped": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _f32,
                                                       _vp, _sz, _vp]),
    "wx_beam_topk_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "wx_beam_topk": (ctypes.c_int, [_vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "wx_attention_h16": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _f32, _i32, _vp]),
    "wx_add_layernorm_h16": (ctypes.c_int, [_vp, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _f32, _i32, _vp, _vp, _vp]),
    "wx_attention_h16_packed": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp,
                                               _f32, _i32, _vp]),
    "wx_add_layernorm_h16_dual": (ctypes.c_int, [_vp, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _f32, _i32, _vp, _vp, _vp,
                                                 _vp]),
    "wx_conv0_channel_norm_h16": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _f32, _i32, _i32, _vp,
                                                 _vp, _sz, _vp]),
    "wx_decode_attention_h16": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _f32, _i32, _vp,
                                               _sz, _vp]),
    "wx_decode_attention_h16_grouped": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _f32,
                                                       _i32, _vp, _sz, _vp]),
    "wx_prefill_attention_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _f32,
                                                _vp]),
    "wx_prefill_attention_h16": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _f32,
                                                _i32, _vp]),
    "wx_decode_self_attention_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                                    _vp, _vp, _f32, _vp, _vp, _sz, _vp]),
    "wx_decode_self_attention_h16": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                                    _vp, _vp, _f32, _i32, _vp, _vp, _sz, _vp]),
    "wx_sample_token_workspace_bytes": (_sz, [_i32, _i32]),
    "wx_sample_token": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _f32, ctypes.c_uint64, _vp, _i64, _vp, _vp, _vp, _vp,
                                       _vp, _sz, _vp]),
    "wx_penalize_logits": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _i64, _i64, _vp, _i32, _i32, _f32, _i32, _vp]),
}


class WXError(RuntimeError):
    pass


N_SHARDS = 8  # instantiation shards of csrc/wx_align_inst.hip (WX_SHARD=0..7)
BASE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall"]


def build(force: bool = False, verbose: bool = False, out: Optional[str] = None, flags=(),
          jobs: Optional[int] = None) -> str:
    """Compile the HIP sources for gfx950 into libwxalign.so (in-tree), one translation unit per
    process: the host ABI, the emission and VAD kernels, and the fused-DP instantiations split
    over N_SHARDS shards (a single TU takes ~4.5 min; the shards build in parallel).  `flags`
    adds hipcc flags (A/B variants: tools/build_variant.sh); -DWX_PHASE_TIMING builds the DP in
    one TU (its debug arrays must be a single copy)."""
    out = out or LIB_PATH
    flags = list(flags)
    if not force and out == LIB_PATH and not flags and os.path.exists(out) and \
            os.path.getmtime(out) >= _newest_source():
        return out
    phase = "-DWX_PHASE_TIMING" in flags
    tus = [(p, []) for p in SRC_PATHS]
    if not phase:
        tus += [(INST_PATH, [f"-DWX_SHARD={k}"]) for k in range(N_SHARDS)]
    objdir = os.path.join(os.path.dirname(_HERE), "build", "obj", os.path.basename(out).replace(".so", ""))
    os.makedirs(objdir, exist_ok=True)
    jobs = jobs or max(1, min(len(tus), int(os.environ.get("MAX_JOBS", "0")) or (os.cpu_count() or 4)))
    cmds, objs = [], []
    for src, extra in tus:
        tag = os.path.basename(src).replace(".hip", "") + "".join(e.split("=")[-1] for e in extra)
        obj = os.path.join(objdir, tag + ".o")
        objs.append(obj)
        cmds.append(["hipcc", *BASE_FLAGS, *flags, *extra, f"-I{INCLUDE_DIR}", "-c", src, "-o", obj])
    pending, running, failed = list(cmds), [], []
    while pending or running:
        while pending and len(running) < jobs:
            c = pending.pop(0)
            if verbose:
                print(" ".join(c), flush=True)
            running.append((c, subprocess.Popen(c, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        c, p = running.pop(0)
        log = p.communicate()[0]
        if p.returncode != 0:
            failed.append((c, log))
        elif verbose and log.strip():
            print(log)
    if failed:
        for p in [p for _, p in running]:
            p.wait()
        c, log = failed[0]
        raise WXError(f"hipcc failed: {' '.join(c)}\n{log}")
    link = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--no-undefined", "-o", out + ".tmp", *objs]
    res = subprocess.run(link, capture_output=True, text=True)
    if res.returncode != 0:
        raise WXError(f"link failed ({res.returncode}):\n{res.stderr}")
    os.replace(out + ".tmp", out)
    return out


def _newest_source() -> float:
    paths = SRC_PATHS + HDR_PATHS + [os.path.join(INCLUDE_DIR, "wx_align.h")]
    return max(os.path.getmtime(p) for p in paths if os.path.exists(p))


_lib: Optional[ctypes.CDLL] = None


def load(require_device: bool = True) -> ctypes.CDLL:
    """Load the HIP library.  Raises if it was not built or (by default) no GPU is visible."""
    global _lib
    if require_device and not torch.cuda.is_available():
        raise WXError("whisperx_amd._lib needs a HIP device (MI355X) and none is visible; the host routes live in "
                      "whisperx_amd.audio, .diarize and .vad")
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WXError(f"{LIB_PATH} is missing: run whisperx_amd._lib.build() (hipcc, gfx950)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                if os.environ.get("WX_LIB_PATH"):  # an older build under A/B (tools/satbench.py)
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _check(rc: int):
    if rc != 0:
        raise WXError(f"libwxalign error {rc}: {load(False).wx_strerror(rc).decode()}")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _h2d(x, dtype, device):
    """Host list/array -> device tensor through pinned memory.  An async copy from a
    temporary *pageable* tensor is unsafe here (the staging buffer can be recycled before
    the copy runs); the caching host allocator keeps a pinned block alive until its copy
    has completed on the stream."""
    h = torch.as_tensor(x, dtype=dtype)
    if h.dim() == 0:
        h = h.reshape(1)
    if torch.cuda.is_available():
        h = h.pin_memory()
    return h.to(device, non_blocking=True)


def _dev_i64(x, device):
    return _h2d(x, torch.int64, device)


class Scratch:
    """Grow-only device scratch buffers, one per (tag, device, stream): every user has a tag of
    its own, and calls enqueued on different streams (or from different threads) never share
    scratch, as the ABI's reentrancy allows.  A buffer is allocated with its device and stream
    current, so the caching allocator orders its reuse after that stream's pending kernels when
    a larger one replaces it.  zero=True fills it with zeros when allocated or grown (the
    hand-off region of split launches: it then holds only hand-off granules, and a launch never
    matches an earlier launch's epoch, so no per-launch memset)."""

    def __init__(self):
        self.buf: dict = {}
        self._mu = threading.Lock()

    def get(self, tag: str, device, nbytes: int, stream=None, zero: bool = False) -> torch.Tensor:
        device = torch.device(device)
        st = stream if stream is not None else torch.cuda.current_stream(device)
        key = (tag, str(device), int(st.cuda_stream))
        with self._mu:
            b = self.buf.get(key)
            if b is None or b.numel() < nbytes:
                with torch.cuda.device(device), torch.cuda.stream(st):
                    b = (torch.zeros if zero else torch.empty)(max(nbytes, 1 << 16), dtype=torch.uint8, device=device)
                self.buf[key] = b
            return b


_scratch = Scratch()


# ----------------------------------------------------------------------------------- batch
class Batch:
    """CSR packing of S segments: emissions [sum_T, V] fp32, tokens int32, blank ids."""

    def __init__(self, emissions, tokens, blank_ids, device=None):
        if len(emissions) != len(tokens) or len(tokens) != len(blank_ids):
            raise ValueError("emissions, tokens and blank_ids must have the same length")
        device = torch.device(device) if device is not None else (
            emissions[0].device if emissions and emissions[0].is_cuda else torch.device("cuda", torch.cuda.current_device()))
        Vs = {int(e.shape[1]) for e in emissions if e.dim() == 2}
        if len(Vs) > 1:
            raise ValueError("all emissions of a batch must have the same vocabulary size")
        V = Vs.pop() if Vs else 1
        if emissions:
            em = torch.cat([e.to(device=device, dtype=torch.float32).reshape(-1, V) for e in emissions], 0)
        else:
            em = torch.empty((0, V), dtype=torch.float32, device=device)
        self._init(em.contiguous(), device, [e.shape[0] for e in emissions], tokens, blank_ids)

    @classmethod
    def from_csr(cls, em: torch.Tensor, Ts, tokens, blank_ids):
        """A batch over an already packed [sum_T, V] fp32 device matrix (segment s owns rows
        sum(Ts[:s]) .. +Ts[s]), e.g. the one _emissions_csr writes log_softmax into."""
        self = cls.__new__(cls)
        if len(Ts) != len(tokens) or len(tokens) != len(blank_ids):
            raise ValueError("Ts, tokens and blank_ids must have the same length")
        if em.dim() != 2 or em.dtype != torch.float32 or not em.is_contiguous() or em.shape[0] != sum(Ts):
            raise ValueError("em must be a contiguous [sum(Ts), V] float32 tensor")
        self._init(em, em.device, Ts, tokens, blank_ids)
        return self

    def _init(self, em: torch.Tensor, device, Ts, tokens, blank_ids):
        """Both constructors end here: the offsets, the token / blank uploads and the N range of
        the packed matrix `em`."""
        self.S = len(Ts)
        self.device = device
        self.V = int(em.shape[1])
        self.Ts = [int(t) for t in Ts]
        self.Ns = [len(t) for t in tokens]
        self.em_off = [0]
        for T in self.Ts:
            self.em_off.append(self.em_off[-1] + T)
        self.tok_off = [0]
        for N in self.Ns:
            self.tok_off.append(self.tok_off[-1] + N)
        self.sum_T = self.em_off[-1]
        self.em = em
        flat = [int(x) for t in tokens for x in t]
        self.tok = _h2d(flat if flat else [0], torch.int32, device)
        self.blank = _h2d([int(b) for b in blank_ids] or [0], torch.int32, device)
        self.em_off_d = _dev_i64(self.em_off, device)
        self.tok_off_d = _dev_i64(self.tok_off, device)
        self.min_N = min(self.Ns) if self.Ns else 0
        self.max_N = max(self.Ns) if self.Ns else 0


def _validate(b: Batch):
    if b.V < 1 or b.V > MAX_VOCAB:
        raise WXError(f"vocabulary size {b.V} outside [1, {MAX_VOCAB}]")
    if b.max_N > MAX_TOKENS:
        raise WXError(f"a segment has {b.max_N} tokens; the kernel supports up to {MAX_TOKENS}")


MODE_AUTO, MODE_THROUGHPUT, MODE_LATENCY, MODE_LATENCY_1CU = -1, 0, 1, 2
MODE_SPLIT2, MODE_SPLIT3, MODE_SPLIT4 = 12, 13, 14  # latency shape over 2 / 3 / 4 CUs per segment


def _dp_outputs(b: Batch):
    """Fresh output tensors of a fused-DP call on `b`: (seg_start, seg_end, seg_score, t_start, status)."""
    dev = b.device
    nt = max(b.tok_off[-1], 1)
    return (torch.empty(nt, dtype=torch.int32, device=dev), torch.empty(nt, dtype=torch.int32, device=dev),
            torch.empty(nt, dtype=torch.float64, device=dev), torch.empty(max(b.S, 1), dtype=torch.int32, device=dev),
            torch.empty(max(b.S, 1), dtype=torch.int32, device=dev))


def _dp_args(b: Batch, outs, ws: torch.Tensor, wsb: int, ho: torch.Tensor, hob: int):
    """wx_align_dp_ex's arguments up to the hand-off size; mode and stream follow."""
    return (_ptr(b.em), _ptr(b.em_off_d), b.V, _ptr(b.tok), _ptr(b.tok_off_d), _ptr(b.blank), b.S, b.min_N, b.max_N,
            b.sum_T, *(_ptr(t) for t in outs), _ptr(ws), wsb, _ptr(ho), hob)


def align_dp(b: Batch, mode: int = MODE_AUTO):
    """Fused DP: returns device tensors (seg_start, seg_end, seg_score, t_start, status).
    `mode` picks the launch shape (WX_MODE_*); results are identical in every mode."""
    lib = load()
    _validate(b)
    dev = b.device
    outs = _dp_outputs(b)
    wsb = lib.wx_align_dp_workspace_bytes(b.S, b.sum_T, b.max_N)
    hob = lib.wx_align_dp_handoff_bytes(b.S, b.sum_T)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ws = _scratch.get("dp", dev, wsb, stream)
        ho = _scratch.get("handoff", dev, hob, stream, zero=True)  # two streams never share one
        _check(lib.wx_align_dp_ex(*_dp_args(b, outs, ws, wsb, ho, ho.numel()), int(mode),
                                  ctypes.c_void_p(stream.cuda_stream)))
    return outs


class AlignPlan:
    """Preallocated outputs + workspace for repeated wx_align_dp calls on one batch (the
    bench's timed step, and any caller that re-aligns a resident batch)."""

    def __init__(self, b: Batch, mode: int = MODE_AUTO):
        self.lib = load()
        _validate(b)
        self.b = b
        self.mode = int(mode)
        self.outs = self.seg_start, self.seg_end, self.seg_score, self.t_start, self.status = _dp_outputs(b)
        self.wsb = self.lib.wx_align_dp_workspace_bytes(b.S, b.sum_T, b.max_N)
        self.ws = torch.empty(max(self.wsb, 1), dtype=torch.uint8, device=b.device)
        # the plan's own hand-off region (zeroed once; it then holds only hand-off granules);
        # runs of one plan are serialised by the caller (one stream at a time)
        self.hob = self.lib.wx_align_dp_handoff_bytes(b.S, b.sum_T)
        self.ho = torch.zeros(max(self.hob, 1), dtype=torch.uint8, device=b.device)
        self.args = _dp_args(b, self.outs, self.ws, self.wsb, self.ho, self.hob)

    def run(self, stream=None):
        st = ctypes.c_void_p(stream if stream is not None else torch.cuda.current_stream(self.b.device).cuda_stream)
        _check(self.lib.wx_align_dp_ex(*self.args, self.mode, st))
        return self.outs


def align_dp_plan(S: int, min_N: int, max_N: int, V: int, mode: int = MODE_AUTO):
    """Kernel names (rocprof form) wx_align_dp_mode launches for such a batch."""
    lib = load(require_device=False)
    buf = ctypes.create_string_buffer(4096)
    lib.wx_align_dp_plan(S, min_N, max_N, V, mode, buf, len(buf))
    return [x for x in buf.value.decode().split(";") if x]


def trellis(b: Batch, out: Optional[torch.Tensor] = None):
    """Materialised trellises (CSR): returns (flat tensor, offsets list).  `out`: a contiguous
    float32 tensor on the batch's device with room for every trellis, written instead of a
    fresh one (a timed loop re-running the launch)."""
    lib = load()
    _validate(b)
    dev = b.device
    offs = [0]
    for T, N in zip(b.Ts, b.Ns):
        offs.append(offs[-1] + (T + 1) * (N + 1))
    if out is None:
        out = torch.empty(max(offs[-1], 1), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.device != dev or not out.is_contiguous() or out.numel() < offs[-1]:
        raise WXError(f"trellis: out must be a contiguous float32 tensor of >= {offs[-1]} elements on {dev}")
    offs_d = _dev_i64(offs, dev)  # keep referenced until the launch is enqueued
    with torch.cuda.device(dev):
        _check(lib.wx_trellis(_ptr(b.em), _ptr(b.em_off_d), b.V, _ptr(b.tok), _ptr(b.tok_off_d), _ptr(b.blank),
                              b.S, b.max_N, _ptr(out), _ptr(offs_d), _stream(dev)))
    return out, offs


def backtrack(b: Batch, tr_flat: torch.Tensor, tr_offs):
    """backtrack() from materialised trellises: (path_tok, path_time, path_prob, path_len, t_start)."""
    lib = load()
    dev = b.device
    cap = max(b.sum_T, 1)
    pt = torch.empty(cap, dtype=torch.int32, device=dev)
    pm = torch.empty(cap, dtype=torch.int32, device=dev)
    pp = torch.empty(cap, dtype=torch.float32, device=dev)
    plen = torch.empty(max(b.S, 1), dtype=torch.int32, device=dev)
    ts = torch.empty(max(b.S, 1), dtype=torch.int32, device=dev)
    wsb = lib.wx_backtrack_workspace_bytes(b.S, b.sum_T, b.max_N)
    tr_off_d = _dev_i64(tr_offs, dev)
    with torch.cuda.device(dev):
        ws = _scratch.get("backtrack", dev, wsb)
        _check(lib.wx_backtrack(_ptr(tr_flat), _ptr(tr_off_d), _ptr(b.em), _ptr(b.em_off_d), b.V,
                                _ptr(b.tok), _ptr(b.tok_off_d), _ptr(b.blank), b.S, b.max_N, b.sum_T,
                                _ptr(pt), _ptr(pm), _ptr(pp), _ptr(plen), _ptr(ts), _ptr(ws), wsb, _stream(dev)))
    return pt, pm, pp, plen, ts


def merge_repeats(path_tok, path_time, path_prob, path_off, path_len, device):
    """merge_repeats over CSR paths (device tensors): (seg_tok, seg_start, seg_end, seg_score, seg_count)."""
    lib = load()
    dev = torch.device(device)
    S = int(path_len.numel())
    cap = max(int(path_tok.numel()), 1)
    st = torch.empty(cap, dtype=torch.int32, device=dev)
    ss = torch.empty(cap, dtype=torch.int32, device=dev)
    se = torch.empty(cap, dtype=torch.int32, device=dev)
    sc = torch.empty(cap, dtype=torch.float64, device=dev)
    cnt = torch.empty(max(S, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(lib.wx_merge_repeats(_ptr(path_tok), _ptr(path_time), _ptr(path_prob), _ptr(path_off), _ptr(path_len),
                                    S, _ptr(st), _ptr(ss), _ptr(se), _ptr(sc), _ptr(cnt), _stream(dev)))
    return st, ss, se, sc, cnt


def column0_cumsum(em):
    """Column 0 of get_trellis (alignment.py:367) as the fused DP computes it: the fp64 running
    sums S(0..T) of em[:, 0] (a [T, V] fp32 device tensor), as a float64 device tensor."""
    lib = load()
    em = em.contiguous()
    T, V = int(em.shape[0]), int(em.shape[1])
    out = torch.empty(T + 1, dtype=torch.float64, device=em.device)
    with torch.cuda.device(em.device):
        _check(lib.wx_column0_cumsum(_ptr(em), T, V, _ptr(out), _stream(em.device)))
    return out


def binarize(scores_list, sw_geometry, onset: float, offset: float, max_duration: float,
             pad_onset: float = 0.0, pad_offset: float = 0.0, device=None, two_pass: bool = True):
    """Binarize score columns on the GPU.  scores_list: 1-D float32 arrays/tensors (one per
    column); sw_geometry: [(start, step, duration)] per column.  Returns [(starts, ends)]
    as float64 numpy arrays per column.  two_pass picks wx_binarize_ex (bit-word pre-pass +
    event-jumping state machine; the default) or the one-pass scan wx_binarize."""
    lib = load()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    F = [int(len(s)) for s in scores_list]
    f_off = [0]
    for n in F:
        f_off.append(f_off[-1] + n)
    r_off = [0]
    for n in F:
        r_off.append(r_off[-1] + n + 1)
    if F and all(torch.is_tensor(s) and s.is_cuda for s in scores_list):
        # scores already on the device (the VAD producer's output): no host round trip
        ys = torch.cat([s.to(device=dev, dtype=torch.float32).reshape(-1) for s in scores_list]).contiguous()
    else:
        ys = torch.cat([torch.as_tensor(s, dtype=torch.float32).reshape(-1).cpu() for s in scores_list]) \
            if F else torch.zeros(1)
        ys = _h2d(ys, torch.float32, dev)
    g = _h2d(torch.tensor(sw_geometry, dtype=torch.float64).reshape(-1, 3), torch.float64, dev)
    st0, stp, dur = g[:, 0].contiguous(), g[:, 1].contiguous(), g[:, 2].contiguous()
    rs = torch.empty(max(r_off[-1], 1), dtype=torch.float64, device=dev)
    re = torch.empty(max(r_off[-1], 1), dtype=torch.float64, device=dev)
    cnt = torch.empty(max(len(F), 1), dtype=torch.int64, device=dev)
    f_off_d, r_off_d = _dev_i64(f_off, dev), _dev_i64(r_off, dev)  # referenced until enqueued
    with torch.cuda.device(dev):
        if two_pass:
            wsb = lib.wx_binarize_workspace_bytes(len(F), f_off[-1])
            ws = _scratch.get("binarize", dev, wsb)
            _check(lib.wx_binarize_ex(_ptr(ys), _ptr(f_off_d), len(F), f_off[-1], _ptr(st0), _ptr(stp), _ptr(dur),
                                      float(np.float32(onset)), float(np.float32(offset)), float(max_duration),
                                      float(pad_onset), float(pad_offset), _ptr(rs), _ptr(re), _ptr(r_off_d),
                                      _ptr(cnt), _ptr(ws), ws.numel(), _stream(dev)))
        else:  # the one-pass event scan (wx_binarize)
            _check(lib.wx_binarize(_ptr(ys), _ptr(f_off_d), len(F), _ptr(st0), _ptr(stp), _ptr(dur),
                                   float(np.float32(onset)), float(np.float32(offset)), float(max_duration),
                                   float(pad_onset), float(pad_offset), _ptr(rs), _ptr(re), _ptr(r_off_d),
                                   _ptr(cnt), _stream(dev)))
    cnt_h = cnt.cpu().numpy()
    out = []
    for i in range(len(F)):
        n = int(cnt_h[i])
        if n < 0:
            raise WXError("binarize region buffer overflow")
        # copy back only the regions found (the buffers hold F + 1 slots per column)
        a = r_off[i]
        out.append((rs[a:a + n].cpu().numpy(), re[a:a + n].cpu().numpy()))
    return out


def binarize_plan(onset: float, offset: float, total_frames: int = 1):
    """Kernel names (rocprof form) wx_binarize_ex launches for these thresholds."""
    lib = load(require_device=False)
    buf = ctypes.create_string_buffer(512)
    lib.wx_binarize_plan(float(np.float32(onset)), float(np.float32(offset)), int(total_frames), buf, len(buf))
    return [x for x in buf.value.decode().split(";") if x]


def vad_aggregate(scores: torch.Tensor, start_frames, n_frames: int, missing: float = float("nan")):
    """wx_vad_aggregate: scores [n_chunks, K, n_classes] fp32 device tensor, start_frames
    (host ints, non-decreasing) -> [n_frames] fp32 device tensor."""
    lib = load()
    dev = scores.device
    sc = scores.to(torch.float32).contiguous()
    n_chunks, K, n_cls = (int(x) for x in sc.shape)
    sf = _dev_i64(list(start_frames) if n_chunks else [0], dev)
    out = torch.empty(max(int(n_frames), 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _check(lib.wx_vad_aggregate(_ptr(sc), _ptr(sf), n_chunks, K, n_cls, int(n_frames), float(missing),
                                    _ptr(out), _stream(dev)))
    return out[: int(n_frames)]


class SpeakerTurns:
    """Diarization turn tables of F files packed for wx_assign_speakers (host arrays, numpy
    only: the host route of whisperx_amd.diarize walks the same packing).  Per file the
    speakers are ranked by sorted label order (pandas' groupby order) and the turns
    stable-sorted by rank, so a group holds one speaker's turns in table row order:
    start / end [n_turns] fp64, turn_off [G + 1], grp_off [F + 1] int64, labels[f] = the
    file's labels by rank."""

    def __init__(self, tables):
        starts, ends, turn_off, grp_off, self.labels = [], [], [0], [0], []
        for start, end, speaker in tables:
            start = np.asarray(start, dtype=np.float64).reshape(-1)
            end = np.asarray(end, dtype=np.float64).reshape(-1)
            speaker = list(speaker)
            if not (len(start) == len(end) == len(speaker)):
                raise ValueError("a turn table's start, end and speaker columns differ in length")
            labels = sorted(set(speaker))
            rank_of = {s: r for r, s in enumerate(labels)}
            rank = np.fromiter((rank_of[s] for s in speaker), dtype=np.int64, count=len(speaker))
            order = np.argsort(rank, kind="stable")
            starts.append(start[order])
            ends.append(end[order])
            counts = np.bincount(rank, minlength=len(labels))
            for n in counts:
                turn_off.append(turn_off[-1] + int(n))
            grp_off.append(grp_off[-1] + len(labels))
            self.labels.append(labels)
        self.F = len(self.labels)
        self.start = np.concatenate(starts) if starts else np.zeros(0)
        self.end = np.concatenate(ends) if ends else np.zeros(0)
        self.turn_off = np.asarray(turn_off, dtype=np.int64)
        self.grp_off = np.asarray(grp_off, dtype=np.int64)
        self.G = int(self.grp_off[-1])
        self.n_turns = int(self.turn_off[-1])


def assign_speakers(turns: SpeakerTurns, q_start, q_end, q_off, fill_nearest: bool = False, device=None,
                    speaker_out: Optional[torch.Tensor] = None, best_out: Optional[torch.Tensor] = None):
    """wx_assign_speakers over packed turns and queries (q_start / q_end [Q] fp64 host arrays,
    q_off [F + 1]): one launch on the current stream.  Returns device tensors (speaker [Q]
    int32: rank within the file or -1; best_sum [Q] fp64).  speaker_out / best_out: contiguous
    device tensors of Q elements to write into instead of fresh ones."""
    lib = load()
    dev = torch.device(device) if device is not None else torch.device("cuda")
    if dev.type != "cuda":
        raise WXError(f"assign_speakers: {dev} is not a HIP device")
    if dev.index is None:  # "cuda": the current device, spelled as tensors report it
        dev = torch.device("cuda", torch.cuda.current_device())
    q_start = np.ascontiguousarray(q_start, dtype=np.float64).reshape(-1)
    q_end = np.ascontiguousarray(q_end, dtype=np.float64).reshape(-1)
    q_off = np.ascontiguousarray(q_off, dtype=np.int64).reshape(-1)
    Q, F, nt = int(q_start.size), turns.F, turns.n_turns
    if q_end.size != Q or q_off.size != F + 1 or int(q_off[0]) != 0 or int(q_off[-1]) != Q or np.any(np.diff(q_off) < 0):
        raise WXError("assign_speakers: q_off must be F + 1 non-decreasing offsets from 0 to len(q_start) == len(q_end)")
    speaker = speaker_out if speaker_out is not None else torch.empty(max(Q, 1), dtype=torch.int32, device=dev)[:Q]
    best = best_out if best_out is not None else torch.empty(max(Q, 1), dtype=torch.float64, device=dev)[:Q]
    for t, dt in ((speaker, torch.int32), (best, torch.float64)):
        if t.dtype != dt or t.numel() != Q or not t.is_contiguous() or t.device != dev:
            raise WXError("assign_speakers: outputs must be contiguous int32 / float64 device tensors of Q elements")
    # two uploads: the fp64 arrays and the int64 tables, each through one pinned buffer; both
    # stay referenced until the launch is enqueued
    f64 = _h2d(np.concatenate([turns.start, turns.end, q_start, q_end, np.zeros(1)]), torch.float64, dev)
    i64 = _h2d(np.concatenate([turns.turn_off, turns.grp_off, q_off]), torch.int64, dev)
    n_to, n_go = turns.turn_off.size, turns.grp_off.size
    with torch.cuda.device(dev):
        _check(lib.wx_assign_speakers(_ptr(f64[0:]), _ptr(f64[nt:]), _ptr(i64[0:]), _ptr(i64[n_to:]), turns.G, nt,
                                      _ptr(f64[2 * nt:]), _ptr(f64[2 * nt + Q:]), _ptr(i64[n_to + n_go:]), F, Q,
                                      int(bool(fill_nearest)), _ptr(speaker), _ptr(best), _stream(dev)))
    return speaker, best


MEL_BIN_TILES, MEL_TAP_GROUPS = 13, 25  # wx_log_mel's basis: [13][2][25][64][4] (include/wx_align.h)
_mel_basis: dict = {}
_mel_mu = threading.Lock()


def mel_basis_host() -> np.ndarray:
    """The windowed 400-point DFT basis packed as wx_log_mel reads it (include/wx_align.h):
    computed in fp64 (periodic Hann window times cos / sin), rounded to fp32 once."""
    bt, cs, g, lane, j = np.meshgrid(np.arange(MEL_BIN_TILES), np.arange(2), np.arange(MEL_TAP_GROUPS), np.arange(64),
                                     np.arange(4), indexing="ij")
    n = 16 * g + 4 * (lane // 16) + j
    k = 16 * bt + lane % 16
    ang = 2.0 * np.pi * ((k * n) % 400).astype(np.float64) / 400.0
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n.astype(np.float64) / 400.0)
    val = win * np.where(cs == 0, np.cos(ang), np.sin(ang))
    return np.where(k <= 200, val, 0.0).astype(np.float32)


def mel_basis(device) -> torch.Tensor:
    """mel_basis_host() on `device`, uploaded once per device."""
    key = str(torch.device(device))
    with _mel_mu:
        t = _mel_basis.get(key)
        if t is None:
            t = _mel_basis[key] = torch.from_numpy(mel_basis_host()).to(device).contiguous()
        return t


def log_mel(wave: torch.Tensor, first, length, pad, filters: torch.Tensor, out: Optional[torch.Tensor] = None,
            n_frames_max: Optional[int] = None) -> torch.Tensor:
    """wx_log_mel: the reference's log_mel_spectrogram(wave[first : first + length], n_mels, pad)
    for every chunk (first / length / pad: host int sequences of B entries) of a 1-D fp32 device
    waveform, on the current stream.  filters: [n_mels, 201] fp32 on the same device.  Returns
    `out`, a [B, n_mels, n_frames_max] fp32 device tensor (made here unless given: any batch
    stride that is a multiple of n_mels rows, any row stride, last dim contiguous); chunk b fills
    frames 0 .. (length + pad) // 160 - 1 of its rows and nothing else."""
    lib = load()
    if wave.dim() != 1 or wave.dtype != torch.float32 or not wave.is_cuda or not wave.is_contiguous():
        raise WXError("log_mel: wave must be a contiguous 1-D float32 device tensor")
    dev = wave.device
    ch = np.ascontiguousarray(np.stack([np.asarray(first, dtype=np.int64).reshape(-1),
                                        np.asarray(length, dtype=np.int64).reshape(-1),
                                        np.asarray(pad, dtype=np.int64).reshape(-1)]))
    B = int(ch.shape[1])
    n_mels = int(filters.shape[0])
    if tuple(filters.shape) != (n_mels, 201) or filters.dtype != torch.float32 or filters.device != dev \
            or not filters.is_contiguous():
        raise WXError("log_mel: filters must be a contiguous [n_mels, 201] float32 tensor on the waveform's device")
    frames = int(((ch[1] + ch[2]) // 160).max()) if B else 0
    if n_frames_max is None:
        n_frames_max = int(out.shape[2]) if out is not None else frames
    if out is None:
        out = torch.empty((B, n_mels, n_frames_max), dtype=torch.float32, device=dev)
    if out.dim() != 3 or tuple(out.shape[:2]) != (B, n_mels) or out.shape[2] < n_frames_max or out.dtype != torch.float32 \
            or out.device != dev or (out.shape[2] > 1 and out.stride(2) != 1) \
            or (B > 1 and out.stride(0) != n_mels * out.stride(1)):
        raise WXError("log_mel: out must be a float32 [B, n_mels, >= n_frames_max] device tensor with contiguous frames "
                      "and chunks n_mels rows apart")
    if B == 0:
        return out
    basis = mel_basis(dev)
    chunks_d = _dev_i64(ch.reshape(-1), dev)  # referenced until the launches are enqueued
    wsb = lib.wx_log_mel_workspace_bytes(B)
    host = [ctypes.c_void_p(ch[i].ctypes.data) for i in range(3)]  # (ch stays referenced through the call)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ws = _scratch.get("mel", dev, wsb, stream)
        _check(lib.wx_log_mel(_ptr(wave), int(wave.numel()), host[0], host[1], host[2], _ptr(chunks_d), B,
                              n_mels, _ptr(filters), _ptr(basis), _ptr(out), int(n_frames_max), int(out.stride(1)), _ptr(ws), wsb,
                              ctypes.c_void_p(stream.cuda_stream)))
    return out


def pack_conv3_weight(w: torch.Tensor) -> torch.Tensor:
    """A Conv1d(Cin, D, 3) weight [D, Cin, 3] packed as wx_whisper_stem reads it (include/wx_align.h):
    [D / 16][3][Cin / 16][64 lanes][4], entry [ot][j][g][lane][i] = w[16 ot + lane % 16][16 g + 4 (lane / 16) + i][j]."""
    D, Cin, K = (int(v) for v in w.shape)
    if K != 3 or D % 16 or Cin % 16:
        raise WXError(f"pack_conv3_weight: weight {tuple(w.shape)} is not [16 a, 16 b, 3]")
    # [ot, o16, g, q, i, j] -> [ot, j, g, q, o16, i]: lane = 16 q + o16
    return (w.detach().to(torch.float32).reshape(D // 16, 16, Cin // 16, 4, 4, 3).permute(0, 5, 2, 3, 1, 4)
            .contiguous().reshape(D // 16, 3, Cin // 16, 64, 4))


def whisper_stem(x: torch.Tensor, w1_packed: torch.Tensor, b1: torch.Tensor, w2_packed: torch.Tensor,
                 b2: torch.Tensor, pos: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wx_whisper_stem: x [B, n_mels, Tin] fp32 device features (frames contiguous, any batch / row
    stride: a slice of log_mel's output is read in place) -> [B, Tin / 2, D] time-major rows,
    gelu(conv2(gelu(conv1(x)))) + pos, on the current stream.  w*_packed: pack_conv3_weight of the
    two conv weights; pos [Tin / 2, D].  `out`: a contiguous [B, Tin / 2, D] tensor (or slice) to
    write into instead of a fresh one."""
    lib = load()
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_cuda or (x.shape[2] > 1 and x.stride(2) != 1):
        raise WXError("whisper_stem: x must be a float32 [B, n_mels, Tin] device tensor with contiguous frames")
    B, M, Tin = (int(v) for v in x.shape)
    D = int(b1.numel())
    dev = x.device
    for t in (w1_packed, b1, w2_packed, b2, pos):
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise WXError("whisper_stem: weights must be contiguous float32 tensors on the features' device")
    if w1_packed.numel() != 3 * M * D or w2_packed.numel() != 3 * D * D or b2.numel() != D \
            or tuple(pos.shape) != (Tin // 2, D):
        raise WXError(f"whisper_stem: weights do not fit n_mels {M}, D {D}, {Tin} frames")
    if out is None:
        out = torch.empty((B, Tin // 2, D), dtype=torch.float32, device=dev)
    if tuple(out.shape) != (B, Tin // 2, D) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise WXError("whisper_stem: out must be a contiguous float32 [B, Tin / 2, D] tensor on the features' device")
    wsb = lib.wx_whisper_stem_workspace_bytes(B, Tin, D)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ws = _scratch.get("whisper_stem", dev, wsb, stream)
        _check(lib.wx_whisper_stem(_ptr(x), int(x.stride(0)) if B > 1 else M * int(x.stride(1)), int(x.stride(1)),
                                   B, M, Tin, _ptr(w1_packed), _ptr(b1), _ptr(w2_packed), _ptr(b2), _ptr(pos), D,
                                   _ptr(out), _ptr(ws), ws.numel(), ctypes.c_void_p(stream.cuda_stream)))
    return out


DECODE_CHUNK = 128  # WX_DECODE_ATTENTION_CHUNK (include/wx_align.h): keys per workgroup of wx_decode_attention_f32


def decode_attention_f32(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, L: Optional[int] = None,
                         out: Optional[torch.Tensor] = None,
                         workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wx_decode_attention_f32: one query row per (batch, head), q [B, H, 64], against rows 0 .. L - 1
    of k / v [B, H, Lcap, 64] (L defaults to Lcap): fp32 device views of any batch / head / row
    stride with a contiguous head dim and 16-byte aligned rows, read in place (the self-attention
    cache, or the halves of the cross-attention [B, P, 2 H 64] GEMM output).  Returns [B, H, 64]
    contiguous (`out` when given) on the current stream."""
    return _decode_attention("decode_attention_f32", q, k, v, scale, L, out, False, False, workspace)


DECODE_MAX_GROUP = 8  # WX_DECODE_ATTENTION_MAX_GROUP: queries per (batch, head) of the grouped kernel
BEAM_TOPK_SLICE = 4096  # WX_BEAM_TOPK_SLICE: columns per workgroup of wx_beam_topk's first pass


def decode_attention_f32_grouped(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float,
                                 L: Optional[int] = None, out: Optional[torch.Tensor] = None,
                                 workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wx_decode_attention_f32_grouped: G query rows per (batch, head), q [B, G, H, 64] (the beams of
    one chunk), against rows 0 .. L - 1 of the k / v [B, H, Lcap, 64] they share, read in place
    under decode_attention_f32's stride and alignment rules.  Returns [B, G, H, 64] contiguous
    (`out` when given) on the current stream; row (b, g, h) has the bits decode_attention_f32
    gives that query on the same k / v."""
    return _decode_attention("decode_attention_f32_grouped", q, k, v, scale, L, out, False, True, workspace)


def beam_topk(logits: torch.Tensor, cum: torch.Tensor, G: int):
    """wx_beam_topk: logits [B G, V] fp32 (any row stride >= V, columns contiguous) and the beams'
    running sums cum [B G] -> (scores [B, 2G] fp32, index [B, 2G] int32 = g V + t): per chunk the 2G
    best candidates cum + log_softmax(logits), best first, ties by lower g, higher logit, lower t.
    On the current stream."""
    lib = load()
    G = int(G)
    if logits.dim() != 2 or cum.dim() != 1 or G < 1 or logits.shape[0] % G or cum.shape[0] != logits.shape[0]:
        raise WXError(f"beam_topk: logits {tuple(logits.shape)} / cum {tuple(cum.shape)} are not [B G, V] / [B G] for "
                      f"G = {G}")
    dev = logits.device
    for t in (logits, cum):
        if t.dtype != torch.float32 or not t.is_cuda or t.device != dev:
            raise WXError("beam_topk: logits and cum must be float32 tensors on one HIP device")
    if (logits.shape[1] > 1 and logits.stride(1) != 1) or not cum.is_contiguous():
        raise WXError("beam_topk: the logits' columns and cum must be contiguous")
    B, V = int(logits.shape[0]) // G, int(logits.shape[1])
    scores = torch.empty((B, 2 * G), dtype=torch.float32, device=dev)
    index = torch.empty((B, 2 * G), dtype=torch.int32, device=dev)
    wsb = lib.wx_beam_topk_workspace_bytes(B, G, V)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ws = _scratch.get("beam_topk", dev, wsb, stream)
        _check(lib.wx_beam_topk(_ptr(logits), int(logits.stride(0)) if B * G > 1 else V, _ptr(cum), B, G, V,
                                _ptr(scores), _ptr(index), _ptr(ws), ws.numel(), ctypes.c_void_p(stream.cuda_stream)))
    return scores, index


SAMPLE_TOKEN_SLICE = 4096  # WX_SAMPLE_TOKEN_SLICE: columns per workgroup of wx_sample_token's first pass


def sample_token_workspace(R: int, V: int, device) -> torch.Tensor:
    """A workspace of exactly wx_sample_token_workspace_bytes(R, V) bytes on `device` (a graph plan's own)."""
    return torch.empty(max(load().wx_sample_token_workspace_bytes(int(R), int(V)), 1), dtype=torch.uint8, device=device)


def sample_token(logits: torch.Tensor, step: torch.Tensor, eot: int, done: torch.Tensor, temperature: float = 0.0,
                 seed: int = 0, suppress: Optional[torch.Tensor] = None, sum_logprob: Optional[torch.Tensor] = None,
                 token: Optional[torch.Tensor] = None, logprob: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None):
    """wx_sample_token: logits [R, V] fp32 (any row stride >= V, columns contiguous; read only),
    `step` an int64 device tensor whose first element is the step counter (read on the device),
    `done` [R] bool or uint8 (in / out), `suppress` [V] bool or uint8 (nonzero: the id is masked) or
    None, `sum_logprob` [R] fp32 (in / out) or None -> (token [R] int64, logprob [R] fp32): per row
    the argmax (temperature 0) or the Gumbel-max sample at `temperature` keyed on (seed, row, step)
    of the masked logits and its log-probability at temperature 1; a row that is done gets `eot`
    and 0.  `token` / `logprob`: tensors to write into instead of fresh ones; `workspace`: a uint8
    tensor of at least wx_sample_token_workspace_bytes(R, V) bytes instead of the stream's scratch.
    On the current stream."""
    lib = load()
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_cuda:
        raise WXError(f"sample_token: logits must be a float32 [R, V] device tensor, got {logits.dtype} "
                      f"{tuple(logits.shape)}")
    dev = logits.device
    R, V = int(logits.shape[0]), int(logits.shape[1])
    if V > 1 and logits.stride(1) != 1:
        raise WXError("sample_token: the logits' columns must be contiguous")
    if token is None:
        token = torch.empty(R, dtype=torch.int64, device=dev)
    if logprob is None:
        logprob = torch.empty(R, dtype=torch.float32, device=dev)

    def fits(t, n, dtypes):
        return t.dtype in dtypes and tuple(t.shape) == (n,) and t.device == dev and t.is_contiguous()

    if not fits(done, R, (torch.bool, torch.uint8)) or not fits(token, R, (torch.int64,)) \
            or not fits(logprob, R, (torch.float32,)) \
            or (sum_logprob is not None and not fits(sum_logprob, R, (torch.float32,))) \
            or (suppress is not None and not fits(suppress, V, (torch.bool, torch.uint8))):
        raise WXError("sample_token: done [R] bool / uint8, token [R] int64, logprob and sum_logprob [R] float32 and "
                      "suppress [V] bool / uint8 must be contiguous tensors on the logits' device")
    if step.dtype != torch.int64 or step.device != dev or step.numel() < 1 or not step.is_contiguous():
        raise WXError("sample_token: step must be a contiguous int64 tensor on the logits' device")
    if not 0 <= int(seed) < 1 << 64:
        raise WXError(f"sample_token: seed {seed} is not an unsigned 64-bit integer")
    wsb = lib.wx_sample_token_workspace_bytes(R, V)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ws = workspace if workspace is not None else _scratch.get("sample_token", dev, wsb, stream)
        _check(lib.wx_sample_token(_ptr(logits), int(logits.stride(0)) if R > 1 else V, R, V, _ptr(suppress),
                                   float(temperature), int(seed), _ptr(step), int(eot), _ptr(done), _ptr(token),
                                   _ptr(logprob), _ptr(sum_logprob), _ptr(ws), ws.numel(),
                                   ctypes.c_void_p(stream.cuda_stream)))
    return token, logprob


PENALTY_MAX_HISTORY = 1024  # WX_PENALTY_MAX_HISTORY: the longest history wx_penalize_logits reads


def penalize_logits(logits: torch.Tensor, history: torch.Tensor, count: torch.Tensor, count_offset: int = 0,
                    max_history: Optional[int] = None, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                    row_major: bool = False) -> torch.Tensor:
    """wx_penalize_logits: logits [R, V] fp32 (any row stride >= V, columns contiguous), rewritten in
    place and returned.  `history`: an int64 tensor of two dimensions on the logits' device, any
    strides: [steps, R] (element [i, r] is id i of row r: the decoder's record), or with `row_major`
    [R, steps].  `count`: an int64 device tensor whose first element, plus `count_offset`, is the
    history's length, read on the device and clamped to [0, max_history]; `max_history` defaults
    to the steps the tensor holds, at most PENALTY_MAX_HISTORY, and may not exceed either.  Every
    distinct id of the history in [0, V) has its logit multiplied (below 0) or divided by
    `repetition_penalty`, and with n = `no_repeat_ngram_size` >= 1 every id that would repeat an
    n-gram of the history is set to -inf (include/wx_align.h states both).  On the current stream."""
    lib = load()
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_cuda:
        raise WXError(f"penalize_logits: logits must be a float32 [R, V] device tensor, got {logits.dtype} "
                      f"{tuple(logits.shape)}")
    dev = logits.device
    R, V = int(logits.shape[0]), int(logits.shape[1])
    if V > 1 and logits.stride(1) != 1:
        raise WXError("penalize_logits: the logits' columns must be contiguous")
    if history.dim() != 2 or history.dtype != torch.int64 or history.device != dev:
        raise WXError("penalize_logits: history must be an int64 tensor of two dimensions on the logits' device")
    steps_dim, rows_dim = (1, 0) if row_major else (0, 1)
    if int(history.shape[rows_dim]) != R:
        raise WXError(f"penalize_logits: history {tuple(history.shape)} does not hold {R} rows")
    steps = int(history.shape[steps_dim])
    cap = min(steps, PENALTY_MAX_HISTORY) if max_history is None else int(max_history)
    if cap > steps:
        raise WXError(f"penalize_logits: max_history {cap} is more than the {steps} steps history holds")
    if count.dtype != torch.int64 or count.device != dev or count.numel() < 1 or not count.is_contiguous():
        raise WXError("penalize_logits: count must be a contiguous int64 tensor on the logits' device")
    with torch.cuda.device(dev):
        _check(lib.wx_penalize_logits(_ptr(logits), int(logits.stride(0)) if R > 1 else V, R, V, _ptr(history),
                                      int(history.stride(steps_dim)), int(history.stride(rows_dim)), _ptr(count),
                                      int(count_offset), cap, float(repetition_penalty), int(no_repeat_ngram_size),
                                      _stream(dev)))
    return logits


def sincnet_stage(x_tm: torch.Tensor, do_abs: bool, gamma, beta, eps: float, slope: float = 0.01,
                  in_scale: Optional[torch.Tensor] = None, in_shift: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wx_sincnet_stage(_ex) on a time-major conv output x_tm [B, L, C] (row stride C, any
    window stride, windows may overlap): leaky_relu(InstanceNorm1d(MaxPool1d(3, 3)(|x'|?))) with
    x' = x * in_scale[b] + in_shift[b, c] when given, as [B, L // 3, C] contiguous."""
    lib = load()
    B, L, C = (int(v) for v in x_tm.shape)
    if x_tm.dtype != torch.float32 or x_tm.stride(2) != 1 or x_tm.stride(1) != C:
        raise WXError("sincnet_stage: x must be float32 [B, L, C] with contiguous rows")
    y = torch.empty((B, L // 3, C), dtype=torch.float32, device=x_tm.device)
    g = gamma.detach().contiguous() if gamma is not None else None
    bt = beta.detach().contiguous() if beta is not None else None
    sc = in_scale.detach().to(torch.float32).contiguous() if in_scale is not None else None
    sh = in_shift.detach().to(torch.float32).contiguous() if in_shift is not None else None
    with torch.cuda.device(x_tm.device):
        _check(lib.wx_sincnet_stage_ex(_ptr(x_tm), B, L, C, int(x_tm.stride(0)), int(bool(do_abs)), _ptr(sc), _ptr(sh),
                                       _ptr(g), _ptr(bt), float(eps), float(slope), _ptr(y), _stream(x_tm.device)))
    return y


def conv1d_taps_tm(x_tm: torch.Tensor, w_packed: torch.Tensor, bias, cout: int, k: int) -> torch.Tensor:
    """wx_conv1d_taps_tm: Conv1d(Cin, cout, k) (no padding, stride 1) of every window of a
    time-major [B, L, Cin] fp32 batch (contiguous) with the packed weights
    [k][CINP / 4][64][4]; returns [B, L - k + 1, cout] time-major."""
    lib = load()
    B, L, C = (int(v) for v in x_tm.shape)
    if not x_tm.is_contiguous() or x_tm.dtype != torch.float32:
        raise WXError("conv1d_taps_tm: x must be a contiguous fp32 [B, L, Cin] tensor")
    y = torch.empty((B, max(L - k + 1, 0), cout), dtype=torch.float32, device=x_tm.device)
    with torch.cuda.device(x_tm.device):
        _check(lib.wx_conv1d_taps_tm(_ptr(x_tm), B, L, C, _ptr(w_packed), _ptr(bias) if bias is not None else None,
                                     int(cout), int(k), _ptr(y), _stream(x_tm.device)))
    return y


def sinc_filterbank(x: torch.Tensor, w_padded: torch.Tensor, k: int, stride: int) -> torch.Tensor:
    """wx_sinc_filterbank: the strided k-tap filterbank convolution of one contiguous fp32
    waveform span x [n] with the taps zero-padded to w_padded [KP, C]; returns
    [(n - k) // stride + 1, C] time-major."""
    lib = load()
    KP, C = (int(v) for v in w_padded.shape)
    n = int(x.shape[0])
    if x.dim() != 1 or not x.is_contiguous() or x.dtype != torch.float32 or not w_padded.is_contiguous() \
            or w_padded.dtype != torch.float32 or not 0 < k <= KP:
        raise WXError("sinc_filterbank: x must be a contiguous fp32 [n] span, w_padded a contiguous fp32 [KP >= k, C]")
    F_out = (n - k) // stride + 1 if n >= k else 0
    y = torch.empty((F_out, C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib.wx_sinc_filterbank(_ptr(x), n, int(stride), _ptr(w_padded), C, int(k), KP, _ptr(y),
                                      _stream(x.device)))
    return y


def lstm_bidir_layer(xp: torch.Tensor, whh: torch.Tensor, B: int, T: int) -> torch.Tensor:
    """wx_lstm_bidir_layer: one bidirectional LSTM layer (H = 128) over B sequences of T steps
    from the input projections xp [B, T, 2, 4H] (x W_ih^T + b_ih + b_hh per direction) and
    whh [2, 4H, H]; returns the outputs [B, T, 2H] (forward then reverse direction)."""
    lib = load()
    H = int(whh.shape[-1])
    if tuple(xp.shape) != (B, T, 2, 4 * H) or tuple(whh.shape) != (2, 4 * H, H) or not xp.is_contiguous() \
            or not whh.is_contiguous() or xp.dtype != torch.float32 or whh.dtype != torch.float32:
        raise WXError(f"lstm_bidir_layer: xp {tuple(xp.shape)} / whh {tuple(whh.shape)} are not [B, T, 2, 4H] / [2, 4H, H] fp32")
    y = torch.empty((B, T, 2 * H), dtype=torch.float32, device=xp.device)
    with torch.cuda.device(xp.device):
        _check(lib.wx_lstm_bidir_layer(_ptr(xp), _ptr(whh), _ptr(y), int(B), int(T), H, _stream(xp.device)))
    return y


def channel_norm(x: torch.Tensor, gamma, beta, eps: float, gelu: bool, out: Optional[torch.Tensor] = None):
    """wx_channel_norm on a time-major [L, C] fp32 device tensor (contiguous)."""
    lib = load()
    L, C = (int(v) for v in x.shape)
    y = out if out is not None else torch.empty_like(x)
    wsb = lib.wx_channel_norm_workspace_bytes(C)
    stream = torch.cuda.current_stream(x.device)
    # one scratch per (device, stream): align() runs forwards on several streams at once
    ws = _scratch.get("channel_norm", x.device, wsb, stream)
    with torch.cuda.device(x.device):
        _check(lib.wx_channel_norm(_ptr(x), L, C, _ptr(gamma), _ptr(beta), float(eps), int(bool(gelu)), _ptr(y),
                                   _ptr(ws), ws.numel(), ctypes.c_void_p(stream.cuda_stream)))
    return y


def conv0_channel_norm(x: torch.Tensor, w: torch.Tensor, bias, stride: int, gamma, beta, eps: float, gelu: bool,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wx_conv0_channel_norm: the 1-channel conv (w [C, 1, K] or [C, K]) over the samples x [S]
    (contiguous fp32 device tensor), GroupNorm per channel, GELU; returns [Lout, C] time-major.
    (`bias` cancels in the per-channel normalisation: the kernels do not read it.)"""
    lib = load()
    S = int(x.shape[-1])
    C, K = int(w.shape[0]), int(w.shape[-1])
    w2 = w.reshape(C, K).contiguous()
    L = (S - K) // stride + 1 if S >= K else 0
    y = out if out is not None else torch.empty((L, C), dtype=torch.float32, device=x.device)
    if L == 0:
        return y
    stream = torch.cuda.current_stream(x.device)
    ws = _scratch.get("conv0", x.device, lib.wx_conv0_channel_norm_workspace_bytes(L, C), stream)
    with torch.cuda.device(x.device):
        _check(lib.wx_conv0_channel_norm(_ptr(x), S, K, int(stride), _ptr(w2), _ptr(bias) if bias is not None else None,
                                         C, _ptr(gamma), _ptr(beta), float(eps), int(bool(gelu)), _ptr(y), _ptr(ws),
                                         ws.numel(), ctypes.c_void_p(stream.cuda_stream)))
    return y


def _add_layernorm(who: str, a: torch.Tensor, b: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                   eps: float, dtype: Optional[torch.dtype], dual: bool, want_y32: bool, want_sum: bool):
    """add_layernorm (dtype None: b fp32) and add_layernorm_h16 / add_layernorm_h16_dual (b and y16 of `dtype`).
    Returns (y32, y16, a + float(b)), None for what the call does not produce."""
    lib = load()
    half = dtype is not None
    code = HALF_DTYPES.get(dtype)
    if half and (code is None or a.dtype != torch.float32 or (b is not None and b.dtype != dtype)):
        raise WXError(f"{who}: a must be float32 and b float16 / bfloat16 as `dtype` says, got {a.dtype}, "
                      f"{None if b is None else b.dtype}, dtype {dtype}")
    D = int(a.shape[-1])
    if b is not None and tuple(a.shape) != tuple(b.shape):
        raise WXError(f"{who}: shapes differ ({tuple(a.shape)}, {tuple(b.shape)})")

    # the kernel reads 16-byte vectors: 16-byte aligned rows (row stride a multiple of 4 floats / 8 halves);
    # an unaligned view is copied (contiguous) rather than refused
    def rows_of(t, mult):
        t = t.reshape(-1, D)
        return t if t.data_ptr() % 16 == 0 and (t.shape[0] <= 1 or t.stride(0) % mult == 0) and t.stride(1) == 1 \
            else t.contiguous()
    a2, b2 = rows_of(a, 4), None if b is None else rows_of(b, 8 if half else 4)
    rows = int(a2.shape[0])
    y32 = torch.empty(a.shape, dtype=torch.float32, device=a.device) if want_y32 else None
    y16 = torch.empty(a.shape, dtype=dtype, device=a.device) if half else None
    s = torch.empty(a.shape, dtype=torch.float32, device=a.device) if want_sum else None
    with torch.cuda.device(a.device):
        _check(getattr(lib, "wx_" + who)(_ptr(a2), _ptr(b2), rows, D, int(a2.stride(0)) if rows else D,
                                         int(b2.stride(0)) if rows and b2 is not None else D, _ptr(gamma), _ptr(beta),
                                         float(eps), *((code,) if half else ()),
                                         *((_ptr(y32), _ptr(y16)) if dual else (_ptr(y16 if half else y32),)), _ptr(s),
                                         _stream(a.device)))
    return y32, y16, s


def add_layernorm(a: torch.Tensor, b: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                  want_sum: bool = False):
    """wx_add_layernorm: LayerNorm(a + b) over the last dim of fp32 device tensors of one shape
    (last dim contiguous, rows at any stride the leading dims flatten to).  Returns y, or
    (y, a + b) with want_sum."""
    y, _, s = _add_layernorm("add_layernorm", a, b, gamma, beta, eps, None, False, True, want_sum)
    return (y, s) if want_sum else y


def attention_f32(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float) -> torch.Tensor:
    """wx_attention_f32: softmax(scale * q k^T) v for [B, H, T, 64] fp32 device views (head dim
    contiguous, any batch / head / time strides).  Returns [B, T, H, 64] (transformers'
    attention-interface layout) on the current stream."""
    lib = load()
    B, H, T, D = (int(x) for x in q.shape)
    if tuple(k.shape) != (B, H, T, D) or tuple(v.shape) != (B, H, T, D):
        raise WXError(f"attention_f32: q/k/v shapes differ ({tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)})")
    o = torch.empty((B, T, H, D), dtype=torch.float32, device=q.device)
    st = [(ctypes.c_int64 * 3)(*(int(x) for x in t.stride()[:3])) for t in (q, k, v)]
    with torch.cuda.device(q.device):
        _check(lib.wx_attention_f32(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, T, D, st[0], st[1], st[2],
                                    float(scale), _stream(q.device)))
    return o


# wx_attention_h16 / wx_add_layernorm_h16's dtype argument (include/wx_align.h WX_DTYPE_*)
HALF_DTYPES = {torch.float16: 1, torch.bfloat16: 2}


def attention_h16(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float) -> torch.Tensor:
    """wx_attention_h16: softmax(scale * q k^T) v for [B, H, T, 64] fp16 or bf16 device views of one
    dtype (head dim contiguous, batch / head / time strides multiples of 8, 16-byte aligned: the
    slices of a fused q/k/v GEMM output as they are).  Returns [B, T, H, 64] in that dtype on the
    current stream."""
    lib = load()
    code = HALF_DTYPES.get(q.dtype)
    if code is None or k.dtype != q.dtype or v.dtype != q.dtype:
        raise WXError(f"attention_h16: q/k/v must share one of float16 / bfloat16, got {q.dtype}, {k.dtype}, {v.dtype}")
    B, H, T, D = (int(x) for x in q.shape)
    if tuple(k.shape) != (B, H, T, D) or tuple(v.shape) != (B, H, T, D):
        raise WXError(f"attention_h16: q/k/v shapes differ ({tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)})")
    if any(t.stride(3) != 1 for t in (q, k, v)) and D > 1:
        raise WXError("attention_h16: the head dim must be contiguous")
    o = torch.empty((B, T, H, D), dtype=q.dtype, device=q.device)
    st = [(ctypes.c_int64 * 3)(*(int(x) for x in t.stride()[:3])) for t in (q, k, v)]
    with torch.cuda.device(q.device):
        _check(lib.wx_attention_h16(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, T, D, st[0], st[1], st[2],
                                    float(scale), code, _stream(q.device)))
    return o


def add_layernorm_h16(a: torch.Tensor, b: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                      dtype: torch.dtype, want_sum: bool = False):
    """wx_add_layernorm_h16: LayerNorm(a + float(b)) over the last dim, a fp32 and b of `dtype`
    (float16 / bfloat16) of one shape, or LayerNorm(a) with b None; the norm is computed in fp32
    and y is rounded to `dtype`.  Returns y, or (y, a + float(b)) with want_sum (the sum is fp32)."""
    _, y, s = _add_layernorm("add_layernorm_h16", a, b, gamma, beta, eps, dtype, False, False, want_sum)
    return (y, s) if want_sum else y


def _decode_attention(who: str, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, L: Optional[int],
                      out: Optional[torch.Tensor], half: bool, grouped: bool,
                      workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """decode_attention_f32 / _h16 (q [B, H, 64]) and their _grouped forms (q [B, G, H, 64]).
    `workspace`: the caller's own buffer (decode_attention_workspace: a captured graph's calls must
    not touch the shared scratch cache, which is keyed by stream and would allocate inside the capture)."""
    lib = load()
    qd = 4 if grouped else 3
    lead = "[B, G, H, 64]" if grouped else "[B, H, 64]"
    if q.dim() != qd or k.dim() != 4 or v.dim() != 4:
        raise WXError(f"{who}: q {tuple(q.shape)} / k {tuple(k.shape)} / v {tuple(v.shape)} are not "
                      f"{lead} / [B, H, Lcap, 64] / [B, H, Lcap, 64]")
    B, H, D = int(q.shape[0]), int(q.shape[-2]), int(q.shape[-1])
    Lcap = int(k.shape[2])
    L = Lcap if L is None else int(L)
    if tuple(k.shape) != (B, H, Lcap, D) or tuple(v.shape) != (B, H, Lcap, D) or not 1 <= L <= Lcap:
        raise WXError(f"{who}: k {tuple(k.shape)} / v {tuple(v.shape)} do not hold {L} rows for q {tuple(q.shape)}")
    dev = q.device
    code = HALF_DTYPES.get(q.dtype) if half else None
    for t in (q, k, v):
        if (code is None if half else t.dtype != torch.float32) or t.dtype != q.dtype or not t.is_cuda or \
                t.device != dev or t.stride(-1) != 1:
            raise WXError(f"{who}: q, k and v must {'share one of float16 / bfloat16' if half else 'be float32 tensors'}, "
                          "on one HIP device with a contiguous head dim")
    if out is None:
        out = torch.empty(tuple(q.shape), dtype=q.dtype, device=dev)
    if tuple(out.shape) != tuple(q.shape) or out.dtype != q.dtype or out.device != dev or not out.is_contiguous():
        raise WXError(f"{who}: out must be a contiguous {lead} tensor of the queries' dtype on their device")
    st = [(ctypes.c_int64 * n)(*(int(x) for x in t.stride()[:n])) for t, n in ((q, qd - 1), (k, 3), (v, 3))]
    dims = (B, int(q.shape[1]), H, L) if grouped else (B, H, L)
    name = "decode_attention_grouped" if grouped else "decode_attention"
    fn = getattr(lib, f"wx_decode_attention_{'h16' if half else 'f32'}{'_grouped' if grouped else ''}")
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ws = _own_workspace(who, workspace, dev) if workspace is not None else \
            _scratch.get(name, dev, getattr(lib, f"wx_{name}_workspace_bytes")(*dims), stream)
        _check(fn(_ptr(q), _ptr(k), _ptr(v), _ptr(out), *dims, D, st[0], st[1], st[2], float(scale),
                  *((code,) if half else ()), _ptr(ws), ws.numel(), ctypes.c_void_p(stream.cuda_stream)))
    return out


def _own_workspace(who: str, ws: torch.Tensor, dev) -> torch.Tensor:
    if not torch.is_tensor(ws) or ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous():
        raise WXError(f"{who}: workspace must be a contiguous uint8 tensor on the queries' device")
    return ws


def decode_attention_workspace(B: int, H: int, L: int, device, G: Optional[int] = None) -> torch.Tensor:
    """A workspace of the caller's own for the decode-attention wrappers' `workspace=` argument:
    wx_decode_attention_workspace_bytes(B, H, L) bytes, or with `G` the grouped entry points'."""
    lib = load()
    n = lib.wx_decode_attention_workspace_bytes(B, H, L) if G is None else \
        lib.wx_decode_attention_grouped_workspace_bytes(B, G, H, L)
    return torch.empty(max(int(n), 16), dtype=torch.uint8, device=device)


def _decode_self_attention(who: str, q, k_new, v_new, k_cache, v_cache, pos, scale, out, workspace, half: bool):
    """decode_self_attention_f32 and decode_self_attention_h16."""
    lib = load()
    if q.dim() != 3 or k_cache.dim() != 4 or v_cache.dim() != 4:
        raise WXError(f"{who}: q {tuple(q.shape)} / k_cache {tuple(k_cache.shape)} / v_cache {tuple(v_cache.shape)} are "
                      "not [B, H, 64] / [B, H, Lcap, 64] / [B, H, Lcap, 64]")
    B, H, D = (int(x) for x in q.shape)
    Lcap = int(k_cache.shape[2])
    if tuple(k_new.shape) != (B, H, D) or tuple(v_new.shape) != (B, H, D) or tuple(k_cache.shape) != (B, H, Lcap, D) or \
            tuple(v_cache.shape) != (B, H, Lcap, D) or Lcap < 1:
        raise WXError(f"{who}: k_new {tuple(k_new.shape)} / v_new {tuple(v_new.shape)} / k_cache {tuple(k_cache.shape)} / "
                      f"v_cache {tuple(v_cache.shape)} do not fit q {tuple(q.shape)}")
    dev = q.device
    code = HALF_DTYPES.get(q.dtype) if half else None
    for t in (q, k_new, v_new, k_cache, v_cache):
        if (code is None if half else t.dtype != torch.float32) or t.dtype != q.dtype or not t.is_cuda or \
                t.device != dev or t.stride(-1) != 1:
            raise WXError(f"{who}: q, k_new, v_new and the caches must "
                          f"{'share one of float16 / bfloat16' if half else 'be float32 tensors'}, on one HIP device with "
                          "a contiguous head dim")
    if not torch.is_tensor(pos) or pos.dtype != torch.int32 or pos.numel() != 1 or pos.device != dev:
        raise WXError(f"{who}: pos must be an int32 tensor of one element on the queries' device")
    if out is None:
        out = torch.empty((B, H, D), dtype=q.dtype, device=dev)
    if tuple(out.shape) != (B, H, D) or out.dtype != q.dtype or out.device != dev or not out.is_contiguous():
        raise WXError(f"{who}: out must be a contiguous [B, H, 64] tensor of the queries' dtype on their device")
    st = [(ctypes.c_int64 * n)(*(int(x) for x in t.stride()[:n]))
          for t, n in ((q, 2), (k_new, 2), (v_new, 2), (k_cache, 3), (v_cache, 3))]
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ws = _own_workspace(who, workspace, dev) if workspace is not None else \
            _scratch.get("decode_attention", dev, lib.wx_decode_attention_workspace_bytes(B, H, Lcap), stream)
        _check(getattr(lib, "wx_" + who)(_ptr(q), _ptr(k_new), _ptr(v_new), _ptr(k_cache), _ptr(v_cache), _ptr(out), B, H,
                                         Lcap, D, *st, float(scale), *((code,) if half else ()), _ptr(pos), _ptr(ws),
                                         ws.numel(), ctypes.c_void_p(stream.cuda_stream)))
    return out


def decode_self_attention_f32(q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor,
                              v_cache: torch.Tensor, pos: torch.Tensor, scale: float,
                              out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wx_decode_self_attention_f32: the self-attention of one decode step at the position p = pos[0]
    that the kernels read on the device (`pos`: an int32 device tensor of one element).  q / k_new /
    v_new [B, H, 64] are fp32 device views (the column blocks of the q/k/v GEMM output as they are),
    k_cache / v_cache [B, H, Lcap, 64]: row p of the caches becomes k_new / v_new, and the result
    [B, H, 64] (`out` when given) has the bits of decode_attention_f32 with L = p + 1 on the caches
    after that copy.  p outside [0, Lcap) writes nothing.  The launch does not depend on p, so a
    captured graph may replay it; pass the graph's own `workspace` (decode_attention_workspace(B, H,
    Lcap)) then.  On the current stream."""
    return _decode_self_attention("decode_self_attention_f32", q, k_new, v_new, k_cache, v_cache, pos, scale, out,
                                  workspace, False)


def decode_self_attention_h16(q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor,
                              v_cache: torch.Tensor, pos: torch.Tensor, scale: float,
                              out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wx_decode_self_attention_h16: decode_self_attention_f32 on fp16 or bf16 tensors of one dtype,
    under decode_attention_h16's stride rules; the result has decode_attention_h16's bits at L = p + 1."""
    return _decode_self_attention("decode_self_attention_h16", q, k_new, v_new, k_cache, v_cache, pos, scale, out,
                                  workspace, True)


def decode_attention_h16(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, L: Optional[int] = None,
                         out: Optional[torch.Tensor] = None,
                         workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wx_decode_attention_h16: decode_attention_f32 on fp16 or bf16 device views of one dtype: q
    [B, H, 64] against rows 0 .. L - 1 of k / v [B, H, Lcap, 64], read in place (head dim contiguous,
    every other stride a multiple of 8 elements, 16-byte aligned).  Returns [B, H, 64] contiguous in
    that dtype (`out` when given) on the current stream: decode_attention_f32 of the widened inputs,
    rounded once."""
    return _decode_attention("decode_attention_h16", q, k, v, scale, L, out, True, False, workspace)


def decode_attention_h16_grouped(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float,
                                 L: Optional[int] = None, out: Optional[torch.Tensor] = None,
                                 workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wx_decode_attention_h16_grouped: G query rows per (batch, head), q [B, G, H, 64] fp16 or bf16,
    against the k / v [B, H, Lcap, 64] they share, under decode_attention_h16's rules.  Returns
    [B, G, H, 64] contiguous in that dtype; row (b, g, h) has the bits decode_attention_h16 gives that
    query on the same k / v."""
    return _decode_attention("decode_attention_h16_grouped", q, k, v, scale, L, out, True, True, workspace)


def _prefill_attention(who: str, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, causal: Optional[int],
                       Tk: Optional[int], half: bool) -> torch.Tensor:
    """prefill_attention_f32 and prefill_attention_h16."""
    lib = load()
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise WXError(f"{who}: q {tuple(q.shape)} / k {tuple(k.shape)} / v {tuple(v.shape)} are not "
                      "[B, H, Tq, 64] / [B, H, Tkcap, 64] / [B, H, Tkcap, 64]")
    B, H, Tq, D = (int(x) for x in q.shape)
    cap = int(k.shape[2])
    Tk = cap if Tk is None else int(Tk)
    if tuple(k.shape) != (B, H, cap, D) or tuple(v.shape) != (B, H, cap, D) or not 1 <= Tk <= cap:
        raise WXError(f"{who}: k {tuple(k.shape)} / v {tuple(v.shape)} do not hold {Tk} rows for q {tuple(q.shape)}")
    causal = -1 if causal is None else int(causal)
    if causal < 0 and causal != -1 or causal > 2 ** 31 - 1:
        raise WXError(f"{who}: causal must be None or the position of query 0 (>= 0), got {causal}")
    dev = q.device
    code = HALF_DTYPES.get(q.dtype) if half else None
    for t in (q, k, v):
        if (code is None if half else t.dtype != torch.float32) or t.dtype != q.dtype or not t.is_cuda or \
                t.device != dev or t.stride(-1) != 1:
            raise WXError(f"{who}: q, k and v must {'share one of float16 / bfloat16' if half else 'be float32 tensors'}, "
                          "on one HIP device with a contiguous head dim")
    o = torch.empty((B, Tq, H, D), dtype=q.dtype, device=dev)
    st = [(ctypes.c_int64 * 3)(*(int(x) for x in t.stride()[:3])) for t in (q, k, v)]
    with torch.cuda.device(dev):
        if half:
            _check(lib.wx_prefill_attention_h16(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, Tq, Tk, causal, D, st[0], st[1],
                                                st[2], float(scale), code, _stream(dev)))
        else:
            _check(lib.wx_prefill_attention_f32(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, Tq, Tk, causal, D, st[0], st[1],
                                                st[2], float(scale), _stream(dev)))
    return o


def prefill_attention_f32(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, causal: Optional[int] = None,
                          Tk: Optional[int] = None) -> torch.Tensor:
    """wx_prefill_attention_f32: Tq query rows per (batch, head), q [B, H, Tq, 64], against rows
    0 .. Tk - 1 of k / v [B, H, Tkcap, 64] (Tk defaults to Tkcap): fp32 device views of any batch /
    head / row stride with a contiguous head dim and 16-byte aligned rows, read in place (the
    self-attention cache or a `cache[::G]` view of it, the halves of the cross-attention
    [B, P, 2 H 64] GEMM output, the q slice of a fused q/k/v GEMM output).  `causal`: None for no
    mask, or the position of query 0: query i then sees keys 0 .. causal + i.  Returns
    [B, Tq, H, 64] contiguous on the current stream."""
    return _prefill_attention("prefill_attention_f32", q, k, v, scale, causal, Tk, False)


def prefill_attention_h16(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, causal: Optional[int] = None,
                          Tk: Optional[int] = None) -> torch.Tensor:
    """wx_prefill_attention_h16: prefill_attention_f32 on fp16 or bf16 device views of one dtype
    (head dim contiguous, every other stride a multiple of 8 elements, 16-byte aligned).  Returns
    [B, Tq, H, 64] contiguous in that dtype: prefill_attention_f32 of the widened inputs, rounded
    once."""
    return _prefill_attention("prefill_attention_h16", q, k, v, scale, causal, Tk, True)


class PackedSegments:
    """Row layout of segments packed back to back (the packed encoder's batch): host lengths
    and, per device, the int32 tables wx_attention_f32_packed reads — seg_rows (row offsets) and
    seg_units (prefix of H x 32-query tiles; 64-query units for wx_attention_h16_packed), uploaded
    once per (device, H, rows per unit)."""

    def __init__(self, lengths):
        self.lengths = [int(t) for t in lengths]
        self.offsets = [0]
        for t in self.lengths:
            self.offsets.append(self.offsets[-1] + t)
        self.rows = self.offsets[-1]
        self._dev = {}

    def tables(self, device, H: int, rows_per_unit: int = 32):
        """(seg_rows, seg_units, n_units) on `device`: units of `rows_per_unit` rows, H per
        segment row-tile (attention: 32-row query tiles x heads; positional conv: 128-row
        tiles, H = 1)."""
        key = (str(device), int(H), int(rows_per_unit))
        t = self._dev.get(key)
        if t is None:
            units = [0]
            for n in self.lengths:
                units.append(units[-1] + H * ((n + rows_per_unit - 1) // rows_per_unit))
            if units[-1] > 2 ** 31 - 1 or self.rows > 2 ** 31 - 1:
                raise WXError("packed segments: more than 2^31 rows or work units")
            host = torch.tensor(self.offsets + units, dtype=torch.int32).pin_memory()
            dev = host.to(device, non_blocking=True)
            n = len(self.lengths) + 1
            t = (dev[:n], dev[n:], units[-1], host)  # (the pinned source lives as long as the copy)
            self._dev[key] = t
        return t


def attention_f32_packed(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, segs: PackedSegments,
                         split: int = 0) -> torch.Tensor:
    """wx_attention_f32_packed: per-segment softmax(scale * q k^T) v over segments packed along
    the row axis of [1, H, rows, 64] fp32 device views (head dim contiguous).  Returns
    [1, rows, H, 64] like attention_f32."""
    lib = load()
    B, H, R, D = (int(x) for x in q.shape)
    if B != 1 or R != segs.rows or tuple(k.shape) != (1, H, R, D) or tuple(v.shape) != (1, H, R, D):
        raise WXError(f"attention_f32_packed: q/k/v {tuple(q.shape)} / {tuple(k.shape)} / {tuple(v.shape)} "
                      f"do not cover the {segs.rows} packed rows")
    o = torch.empty((1, R, H, D), dtype=torch.float32, device=q.device)
    rows_t, units_t, n_units, _ = segs.tables(q.device, H)
    st = [(ctypes.c_int64 * 2)(int(t.stride(1)), int(t.stride(2))) for t in (q, k, v)]
    with torch.cuda.device(q.device):
        _check(lib.wx_attention_f32_packed(_ptr(q), _ptr(k), _ptr(v), _ptr(o), len(segs.lengths), _ptr(rows_t),
                                           _ptr(units_t), n_units, H, D, st[0], st[1], st[2], float(scale), int(split),
                                           _stream(q.device)))
    return o


def posconv_packed(h: torch.Tensor, w_packed: torch.Tensor, bias, G: int, K: int, segs: PackedSegments,
                   residual: bool) -> torch.Tensor:
    """wx_posconv_packed over h [rows, D] (or [1, rows, D]) contiguous fp32: GELU(conv + bias)
    per segment (+ h with residual), same shape as h."""
    lib = load()
    D = int(h.shape[-1])
    h2 = h.reshape(-1, D)
    if h2.shape[0] != segs.rows or not h2.is_contiguous() or h2.dtype != torch.float32:
        raise WXError(f"posconv_packed: h {tuple(h.shape)} is not the {segs.rows} packed rows (contiguous fp32)")
    out = torch.empty_like(h)
    rows_t, tiles_t, n_tiles, _ = segs.tables(h.device, 1, 128)
    with torch.cuda.device(h.device):
        _check(lib.wx_posconv_packed(_ptr(h2), D, _ptr(w_packed), _ptr(bias) if bias is not None else None, int(G),
                                     int(K), len(segs.lengths), _ptr(rows_t), _ptr(tiles_t), n_tiles,
                                     int(bool(residual)), _ptr(out), _stream(h.device)))
    return out


def attention_h16_packed(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float,
                         segs: PackedSegments) -> torch.Tensor:
    """wx_attention_h16_packed: per-segment softmax(scale * q k^T) v over segments packed along the
    row axis of [1, H, rows, 64] fp16 or bf16 device views of one dtype (head dim contiguous, head /
    row strides multiples of 8, 16-byte aligned: the slices of the fused q/k/v GEMM output as they
    are).  Returns [1, rows, H, 64] in that dtype; a segment's rows are bit for bit attention_h16's
    on that segment alone."""
    lib = load()
    code = HALF_DTYPES.get(q.dtype)
    if code is None or k.dtype != q.dtype or v.dtype != q.dtype:
        raise WXError(f"attention_h16_packed: q/k/v must share one of float16 / bfloat16, got {q.dtype}, {k.dtype}, "
                      f"{v.dtype}")
    B, H, R, D = (int(x) for x in q.shape)
    if B != 1 or R != segs.rows or tuple(k.shape) != (1, H, R, D) or tuple(v.shape) != (1, H, R, D):
        raise WXError(f"attention_h16_packed: q/k/v {tuple(q.shape)} / {tuple(k.shape)} / {tuple(v.shape)} "
                      f"do not cover the {segs.rows} packed rows")
    if any(t.stride(3) != 1 for t in (q, k, v)) and D > 1:
        raise WXError("attention_h16_packed: the head dim must be contiguous")
    o = torch.empty((1, R, H, D), dtype=q.dtype, device=q.device)
    if R == 0 and H >= 1 and D == 64:  # no unit: nothing to launch (and an empty tensor has no storage to point at)
        return o
    rows_t, units_t, n_units, _ = segs.tables(q.device, H, 64)
    st = [(ctypes.c_int64 * 2)(int(t.stride(1)), int(t.stride(2))) for t in (q, k, v)]
    with torch.cuda.device(q.device):
        _check(lib.wx_attention_h16_packed(_ptr(q), _ptr(k), _ptr(v), _ptr(o), len(segs.lengths), _ptr(rows_t),
                                           _ptr(units_t), n_units, H, D, st[0], st[1], st[2], float(scale), code,
                                           _stream(q.device)))
    return o


def add_layernorm_h16_dual(a: torch.Tensor, b: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                           eps: float, dtype: torch.dtype, want_y32: bool = True, want_sum: bool = False):
    """wx_add_layernorm_h16_dual: LayerNorm(a + float(b)) (b None: LayerNorm(a)) over the last dim in
    one pass, a fp32 and b of `dtype`.  Returns (y32, y16): the norm in fp32 (None without want_y32)
    and its rounding to `dtype`; with want_sum (y32, y16, a + float(b))."""
    y32, y16, s = _add_layernorm("add_layernorm_h16_dual", a, b, gamma, beta, eps, dtype, True, want_y32, want_sum)
    return (y32, y16, s) if want_sum else (y32, y16)


def conv0_channel_norm_h16(x: torch.Tensor, w: torch.Tensor, bias, stride: int, gamma, beta, eps: float, gelu: bool,
                           dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wx_conv0_channel_norm_h16: conv0_channel_norm on the fp32 samples x [S] with the [Lout, C]
    output stored in `dtype` (float16 / bfloat16): bit for bit the rounding of conv0_channel_norm's."""
    lib = load()
    code = HALF_DTYPES.get(dtype)
    if code is None or x.dtype != torch.float32 or (out is not None and (out.dtype != dtype or not out.is_contiguous())):
        raise WXError(f"conv0_channel_norm_h16: x must be float32 and the output contiguous float16 / bfloat16, got "
                      f"{x.dtype}, dtype {dtype}, out {None if out is None else out.dtype}")
    S = int(x.shape[-1])
    C, K = int(w.shape[0]), int(w.shape[-1])
    w2 = w.reshape(C, K).contiguous()
    L = (S - K) // stride + 1 if S >= K else 0
    if out is not None and tuple(out.shape) != (L, C):
        raise WXError(f"conv0_channel_norm_h16: out is {tuple(out.shape)}, the output is {(L, C)}")
    y = out if out is not None else torch.empty((L, C), dtype=dtype, device=x.device)
    if L == 0:
        return y
    stream = torch.cuda.current_stream(x.device)
    ws = _scratch.get("conv0", x.device, lib.wx_conv0_channel_norm_workspace_bytes(L, C), stream)
    with torch.cuda.device(x.device):
        _check(lib.wx_conv0_channel_norm_h16(_ptr(x), S, K, int(stride), _ptr(w2), _ptr(bias) if bias is not None else None,
                                             C, _ptr(gamma), _ptr(beta), float(eps), int(bool(gelu)), code, _ptr(y),
                                             _ptr(ws), ws.numel(), ctypes.c_void_p(stream.cuda_stream)))
    return y

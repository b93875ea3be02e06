#!/usr/bin/env python3
"""Times of Whisper's input features (log_mel_spectrogram) for one hour of audio (no threshold:
a record).

Workload: one hour of whisperx_amd.synthetic.waveform cut into merge_chunks-like chunks of
15-30 s at non-aligned offsets (synthetic.vad_chunks), every chunk padded to 30 s as
FasterWhisperPipeline.preprocess does (asr.py:141-149): [B, 80, 3000] features.  The waveform is
resident on the device (where the VAD producer has it) for the device arms.

Arms (--arms, comma separated), each the median of --repeat warm repetitions (with min and max,
the spread a difference has to exceed):
  chunks   (a) one whisperx_amd.log_mel_chunks call, end to end (chunk table upload, the two
           launches, synchronise)
  kernel   the two wx_log_mel launches alone on resident inputs, between device events
  torch    (b) the same chunks one by one through torch's own ops on the device (F.pad,
           torch.stft, matmul, elementwise), what a user would otherwise write
  host     (c) the host route per chunk on --threads CPU threads

The kernel arm also reports what the algorithm needs, computed from the shapes: bytes (chunk
samples read + features written, once each) over the HBM peak and FLOP (frames that touch
audio x (2 x 400 x 400 DFT + 2 x 201 x n_mels projection)) over the fp32 MFMA peak, both as
shares of the measured kernel time.  Prints one JSON line; --out writes it to a file
(profiles/mel_bench_<host>.json).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from benchlib import event_timed, timed  # noqa: E402

HBM_PEAK_BPS = 8.0e12        # MI355X HBM3E, spec
F32_MFMA_PEAK_FLOPS = 157.3e12  # MI355X v_mfma_f32_*_f32, spec


def torch_chunk(x, n_mels, padding, filters, window):
    """audio.py:147-159 in torch's own ops on x's device."""
    import torch
    import torch.nn.functional as F

    x = F.pad(x, (0, padding))
    stft = torch.stft(x, 400, 160, window=window, return_complex=True)
    mag = stft[..., :-1].abs() ** 2
    log_spec = torch.clamp(filters @ mag, min=1e-10).log10()
    log_spec = torch.maximum(log_spec, log_spec.max() - 8.0)
    return (log_spec + 4.0) / 4.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="chunks,kernel,torch,host")
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--n-mels", type=int, default=80)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20, help="launch pairs per kernel-arm repetition")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    arms = args.arms.split(",")
    import torch

    from whisperx_amd import _lib, audio, synthetic

    wav_h = synthetic.waveform(args.seed, args.seconds)
    segs = synthetic.vad_chunks(args.seed + 1, args.seconds)
    first, length = audio._chunk_bounds(segs, len(wav_h))
    B, n_mels = len(segs), args.n_mels
    audio_frames = int(np.minimum(-(-(length + 200) // 160), audio.N_FRAMES).sum())  # frames with a sample of audio
    result = {"tool": "tools/mel_bench.py", "arms": arms, "cpu": platform.processor() or platform.machine(),
              "lib": os.path.basename(_lib.LIB_PATH),
              "shape": {"audio_s": args.seconds, "chunks": B, "n_mels": n_mels, "frames_per_chunk": audio.N_FRAMES,
                        "chunk_samples": int(length.sum()), "frames_touching_audio": audio_frames}}
    need_gpu = any(a in arms for a in ("chunks", "kernel", "torch"))
    if need_gpu:
        if not torch.cuda.is_available():
            raise SystemExit("mel_bench: the chunks / kernel / torch arms need a HIP device (--arms host runs without)")
        dev = torch.device("cuda", 0)
        result["device"] = torch.cuda.get_device_name(0)
        wav = torch.from_numpy(wav_h).to(dev)
        sync = torch.cuda.synchronize
        ours = audio.log_mel_chunks(wav, segs, n_mels=n_mels)
        sync()
    if "chunks" in arms:
        result["chunks"] = timed(lambda: audio.log_mel_chunks(wav, segs, n_mels=n_mels), args.repeat, args.warmup, sync)
    if "kernel" in arms:
        lib = _lib.load()
        filt, basis = audio.mel_filters(dev, n_mels), _lib.mel_basis(dev)
        ch = np.ascontiguousarray(np.stack([first, length, audio.N_SAMPLES - length]).astype(np.int64))
        ch_d = torch.from_numpy(ch.reshape(-1)).to(dev)
        out = torch.empty((B, n_mels, audio.N_FRAMES), dtype=torch.float32, device=dev)
        wsb = lib.wx_log_mel_workspace_bytes(B)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        host = [ctypes.c_void_p(ch[i].ctypes.data) for i in range(3)]
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def launch(i=0):
            rc = lib.wx_log_mel(p(wav), wav.numel(), host[0], host[1], host[2], p(ch_d), B, n_mels, p(filt), p(basis),
                                p(out), audio.N_FRAMES, audio.N_FRAMES, p(ws), wsb, stream)
            assert rc == 0, rc

        launch()
        sync()
        assert torch.equal(out, ours)
        k = event_timed(launch, args.repeat, args.warmup, args.steps, torch)
        k["algorithmic_bytes"] = int(length.sum()) * 4 + B * n_mels * audio.N_FRAMES * 4
        k["algorithmic_flop"] = audio_frames * (2 * 400 * 400 + 2 * 201 * n_mels)
        k["hbm_time_share"] = k["algorithmic_bytes"] / HBM_PEAK_BPS / k["median_s"]
        k["f32_mfma_time_share"] = k["algorithmic_flop"] / F32_MFMA_PEAK_FLOPS / k["median_s"]
        k["bound"] = "fp32 MFMA" if k["f32_mfma_time_share"] > k["hbm_time_share"] else "HBM"
        k["peaks"] = {"hbm_bytes_per_s": HBM_PEAK_BPS, "f32_mfma_flop_per_s": F32_MFMA_PEAK_FLOPS}
        result["kernel"] = k
    if "torch" in arms:
        filt = audio.mel_filters(dev, n_mels)
        window = torch.hann_window(400, device=dev)

        def torch_arm():
            return torch.stack([torch_chunk(wav[int(a):int(a + n)], n_mels, audio.N_SAMPLES - int(n), filt, window)
                                for a, n in zip(first, length)])

        theirs = torch_arm()
        sync()
        result["torch"] = timed(torch_arm, args.repeat, args.warmup, sync)
        result["torch"]["max_abs_diff_to_chunks"] = float((theirs - ours).abs().max())
    if "host" in arms:
        torch.set_num_threads(args.threads)
        result["host"] = timed(lambda: audio.log_mel_chunks(wav_h, segs, n_mels=n_mels, device="cpu"),
                               max(5, args.repeat // 2), 1)
        result["host"]["threads"] = args.threads
    if "chunks" in arms and "torch" in arms:
        a, b = result["chunks"], result["torch"]
        result["chunks_vs_torch"] = {"speedup_median": b["median_s"] / a["median_s"],
                                     "beats_beyond_spread": bool(a["max_s"] < b["min_s"])}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

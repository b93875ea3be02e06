#!/usr/bin/env python3
"""align() on the half route (float16 / bfloat16) against the fp32 route, in one run (a record: no
threshold).  Prints one JSON line; --out writes it to a file (profiles/align_half_<host>.json).

Shapes (--shapes, comma separated): bench.py's own workloads, random weights, synthetic audio:
  base   e2e_align: 16 x 30 s, wav2vec2-base shape (12 x 768, group-norm feature encoder), V 32
  large  config 5: 8 x 60 s, wav2vec2-large-xlsr shape (24 x 1024, layer-norm feature encoder), V 40

Per shape:
  align      whisperx_amd.align() with metadata dtype absent (fp32), float16 and bfloat16: each the
             median of --repeat warm calls (with min and max, the spread a difference has to exceed),
             synchronised; the half legs compared with the fp32 leg (benchlib.beats)
  accuracy   each half leg against the fp32 leg of the same run: word-boundary MAE in ms (bench.py's
             mae_e2e measure) and the segments whose token paths (char times) differ.  Recorded, not
             asserted: the half route's log-probabilities differ from fp32's, so these are not zero.
  forward    emission.packed_logits on the shape's first pack per dtype between device events, and
             its feature encoder (emission.packed_features) alone: the encoder, projection and head
             are the difference
  kernels    per dtype, from a kernel trace of its own (not the timed calls): one process per leg,
             `rocprofv3 --kernel-trace --output-format csv -d DIR/<shape>_<dtype> -- python
             tools/align_half_bench.py --leg <shape>:<dtype>`, then `--traces DIR --out JSON` folds the
             traces into the record: the last call's kernel time per category (GEMMs told apart by their
             place in the stream; the feature encoder's tap GEMMs and the projection are one category)
  stock      the comparator: the stock model cast to the type (model.half() / .bfloat16(), sdpa), one
             unpadded forward per segment on the same device, likewise timed

Attention (--attention): wx_attention_h16_packed, wx_attention_f32_packed (on fp32 copies) and one
wx_attention_h16 launch per segment, on the same packed q/k/v: H 12, 16 x 1499 rows and H 16, 8 x 2999
rows, the three views of one fused [rows, 3 x 64 H] buffer, between device events over --steps launches.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from benchlib import beats, event_timed, timed  # noqa: E402

N_LAYERS = {"base": 12, "large": 24}


def classify(name: str, state: dict, n_layers: int) -> str:
    """A kernel of the packed forward by its name and its place in the stream (as
    tools/forward_roofline.py): GEMMs before the positional conv are the feature encoder's taps and
    the projection; after it they come per layer as q/k/v, out, FF1, FF2; then the head."""
    n = name
    if "conv0_" in n or "chan_" in n:
        return "conv0_norm_gelu"
    if "posconv" in n:
        state.update(enc=True, gemms=0)
        return "posconv"
    if "attn_" in n:
        return "attention"
    if "add_ln" in n:
        return "add_layernorm"
    if "align_dp" in n:
        return "dp"
    if "softmax" in n.lower():
        state["enc"] = False
        return "log_softmax"
    if "Cijk" in n or "gemm" in n.lower():
        if not state.get("enc"):
            return "fe_tap_gemms_and_projection"
        i = state["gemms"]
        state["gemms"] = i + 1
        return "lm_head" if i >= 4 * n_layers else ("qkv_gemm", "out_proj_gemm", "ff1_gemm", "ff2_gemm")[i % 4]
    if "gelu" in n.lower():
        return "ff_gelu" if state.get("enc") else "fe_gelu"
    if "layer_norm" in n.lower() or "layernorm" in n.lower():
        return "layer_norm_torch"
    return "glue (casts, copies, gathers)"


def summarize_trace(path: str, n_layers: int, calls: int) -> dict:
    """Kernel time per category, in ms, of the LAST align() call in a rocprofv3 --kernel-trace CSV of
    `--leg` (a call ends with its last DP kernel; the calls before it, the first one's operand build
    among them, are left out)."""
    import csv
    import glob

    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"),
                                                                 recursive=True))
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows.sort()
    dps = [i for i, r in enumerate(rows) if "align_dp" in r[2]]
    if not dps or len(dps) % calls:
        raise SystemExit(f"{path}: {len(dps)} DP kernels do not divide into {calls} calls")
    per_call = len(dps) // calls
    rows = rows[dps[-per_call - 1] + 1:] if calls > 1 else rows
    state, out = {}, {}
    for t0, t1, name in rows:
        c = classify(name, state, n_layers)
        out[c] = out.get(c, 0.0) + (t1 - t0) / 1e6
    out["total"] = sum(out.values())
    out["kernels"] = len(rows)
    return out


def leg_main(args, torch):
    """--leg SHAPE:DTYPE: `--calls` align() calls and nothing else (the program of a kernel trace)."""
    import bench
    import whisperx_amd

    which, dname = args.leg.split(":")
    segs, audio, model, meta = bench.e2e_leg_inputs("cuda:0") if which == "base" else bench.config5_inputs("cuda:0")
    if dname != "float32":
        meta = dict(meta, dtype=getattr(torch, dname))
    audio = audio.to("cuda:0")
    for _ in range(args.calls):
        whisperx_amd.align([dict(s) for s in segs], model, meta, audio, "cuda:0")
    torch.cuda.synchronize()


def merge_traces(args):
    """--traces DIR --out JSON: fold DIR/<shape>_<dtype>/ kernel traces into the record."""
    with open(args.out) as f:
        result = json.load(f)
    for which, r in result["shapes"].items():
        r["kernels_ms"] = {}
        for dname in ("float32", "float16", "bfloat16"):
            d = os.path.join(args.traces, f"{which}_{dname}")
            r["kernels_ms"][dname] = summarize_trace(d, N_LAYERS[which], args.calls) if os.path.isdir(d) else "not measured"
    result["kernels_ms_source"] = (f"rocprofv3 --kernel-trace of `--leg SHAPE:DTYPE --calls {args.calls}`, one process per leg; "
                                   "kernel time per category of the last call")
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({w: r["kernels_ms"] for w, r in result["shapes"].items()}))


def accuracy(ref, got):
    """bench.py's mae_e2e measure between two align() results with char alignments."""
    errs, n_words, n_path = [], 0, 0
    for a, b in zip(got, ref):
        for x, y in zip(a["words"], b["words"]):
            for k in ("start", "end"):
                if k in x and k in y:
                    errs.append(abs(x[k] - y[k]) * 1000.0)
            n_words += 1
        ca = [(c.get("start"), c.get("end")) for c in a.get("chars", [])]
        cb = [(c.get("start"), c.get("end")) for c in b.get("chars", [])]
        n_path += int(ca != cb)
    return {"word_boundary_mae_ms": sum(errs) / len(errs) if errs else None, "max_ms": max(errs) if errs else None,
            "words": n_words, "segments": len(got), "segments_with_differing_token_paths": n_path}


def shape_leg(which, args, torch):
    import bench
    import whisperx_amd
    from whisperx_amd import _lib, alignment, emission

    dev = "cuda:0"
    if which == "base":
        segs, audio, model, meta = bench.e2e_leg_inputs(dev)
        seg_s = 30.0
    else:
        segs, audio, model, meta = bench.config5_inputs(dev)
        seg_s = 60.0
    audio = audio.to(dev)
    dtypes = {"float32": None, "float16": torch.float16, "bfloat16": torch.bfloat16}
    r = {"segments": len(segs), "segment_s": seg_s, "align": {}, "accuracy_vs_float32": {}, "forward": {},
         "stock_cast_model": {}}

    def metadata(dt):
        return meta if dt is None else dict(meta, dtype=dt)

    outs = {}
    for name, dt in dtypes.items():
        def call(chars=False):
            return whisperx_amd.align([dict(s) for s in segs], model, metadata(dt), audio, dev,
                                      return_char_alignments=chars)
        r["align"][name] = timed(call, args.repeat, 2, torch.cuda.synchronize)
        r["align"][name]["audio_s_per_s"] = seg_s * len(segs) / r["align"][name]["median_s"]
        outs[name] = call(chars=True)["segments"]
    for name in ("float16", "bfloat16"):
        r["align"][name]["vs_float32"] = beats(r["align"][name], r["align"]["float32"])
        r["accuracy_vs_float32"][name] = accuracy(outs["float32"], outs[name])
    # the forward of the first pack alone
    wavs = [audio[None, int(s["start"] * 16000): int(s["end"] * 16000)] for s in segs]
    Ts = [emission.n_frames(int(w.shape[-1]), model) for w in wavs]
    a, b = alignment._pack_ranges(Ts)[0]
    pack, psegs = wavs[a:b], _lib.PackedSegments(Ts[a:b])
    streams = [torch.cuda.current_stream()]
    layers = emission._fe_layers(model.wav2vec2.feature_extractor)
    for name, dt in dtypes.items():
        if dt is None:
            fwd = lambda i: emission.packed_logits(model, pack, psegs, streams)  # noqa: E731
            half = None
        else:
            fwd = lambda i, dt=dt: emission.packed_logits(model, pack, psegs, streams, dtype=dt)  # noqa: E731
            half = emission.half_operands(model, dt)

        def feats(i, half=half):
            with torch.inference_mode():
                return emission.packed_features(model.wav2vec2.feature_extractor, layers, pack, psegs,
                                                torch.device(dev), half=half)
        r["forward"][name] = {"pack_segments": b - a, "rows": psegs.rows,
                              "packed_logits": event_timed(fwd, args.repeat, 2, 1, torch),
                              "feature_encoder": event_timed(feats, args.repeat, 2, 1, torch)}
    # the comparator: the stock model cast to the type, one forward per segment
    for name in ("float16", "bfloat16"):
        cast = copy.deepcopy(model).to(dtypes[name])
        xs = [w.to(dtypes[name]) for w in wavs]

        def stock(i):
            with torch.inference_mode():
                for x in xs:
                    cast(x).logits
        r["stock_cast_model"][name] = event_timed(stock, args.repeat, 2, 1, torch)
        del cast, xs
    del model
    torch.cuda.empty_cache()
    return r


def attention_leg(args, torch):
    from whisperx_amd import _lib

    out = {}
    for H, n, T in ((12, 16, 1499), (16, 8, 2999)):
        D = 64 * H
        segs = _lib.PackedSegments([T] * n)
        R = segs.rows
        for dname, dt in (("float16", torch.float16), ("bfloat16", torch.bfloat16)):
            torch.manual_seed(H)
            qkv = torch.randn((R, 3 * D), device="cuda").to(dt)
            q, k, v = (qkv[None, :, j * D:(j + 1) * D].view(1, R, H, 64).transpose(1, 2) for j in range(3))
            qkv32 = qkv.float()
            q32, k32, v32 = (qkv32[None, :, j * D:(j + 1) * D].view(1, R, H, 64).transpose(1, 2) for j in range(3))

            def per_segment(i):
                for a, b in zip(segs.offsets[:-1], segs.offsets[1:]):
                    _lib.attention_h16(q[:, :, a:b], k[:, :, a:b], v[:, :, a:b], 0.125)
            arms = {"wx_attention_h16_packed": lambda i: _lib.attention_h16_packed(q, k, v, 0.125, segs),
                    "wx_attention_f32_packed": lambda i: _lib.attention_f32_packed(q32, k32, v32, 0.125, segs),
                    "wx_attention_h16_per_segment": per_segment}
            r = {"shape": {"H": H, "segments": n, "T": T, "rows": R, "flop": 4 * T * T * 64 * H * n}}
            for arm, fn in arms.items():
                r[arm] = event_timed(fn, args.repeat, 2, args.steps, torch)
                r[arm]["tflop_per_s"] = r["shape"]["flop"] / r[arm]["median_s"] / 1e12
            r["packed_vs_per_segment"] = beats(r["wx_attention_h16_packed"], r["wx_attention_h16_per_segment"])
            r["packed_vs_f32_packed"] = beats(r["wx_attention_h16_packed"], r["wx_attention_f32_packed"])
            out[f"H{H}_{n}x{T}_{dname}"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="base,large")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--attention", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--leg", help="SHAPE:DTYPE: only `--calls` align() calls (for a kernel trace)")
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--traces", help="directory of <shape>_<dtype>/ kernel traces to fold into --out")
    args = ap.parse_args()
    if args.traces:
        return merge_traces(args)
    import torch

    from whisperx_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("align_half_bench: needs a HIP device")
    if args.leg:
        return leg_main(args, torch)
    result = {"tool": "tools/align_half_bench.py", "device": torch.cuda.get_device_name(0),
              "lib": os.path.basename(_lib.LIB_PATH), "repeat": args.repeat,
              "timing": "median of `repeat` warm repetitions with min and max; align: wall time, synchronised; "
                        "forward, stock, attention: device events", "shapes": {}}
    for which in [s for s in args.shapes.split(",") if s]:
        result["shapes"][which] = shape_leg(which, args, torch)
    if args.attention:
        result["attention"] = attention_leg(args, torch)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

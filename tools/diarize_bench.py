#!/usr/bin/env python3
"""Times of assign_word_speakers on seeded synthetic workloads (no threshold: a record).

Workloads, shaped like a diarizer's output and align()'s result (whisperx_amd.synthetic's
style: seeded, never real data):
  file_1h    one 1 h file: ~600 segments, ~9,000 timed words, ~1,500 turns, 4 speakers
  corpus_10h BASELINE config 4's corpus (synthetic.corpus_durations: 40 files, 10 h) as one
             assign_word_speakers_batch call

Legs (--legs, comma separated), each the median of --repeat calls:
  kernel     wx_assign_speakers alone on resident inputs: back-to-back launches between two
             device events, per launch
  e2e        the kernel route end to end: query gathering, packing, uploads, launch, copy
             back, write-back of the 'speaker' keys and the two columns
  host       the host route (device='cpu'), end to end
  reference  the reference's own assign_word_speakers under pandas on the same inputs, file by
             file — needs WHISPERX_ROOT (a reference checkout) and pandas, so it runs on a
             machine that has them, on that machine's CPU; it also checks that the host route
             assigns the same labels

Prints one JSON line; --out writes it to a file (profiles/diarize_bench_*.json).
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import platform
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def synth_file(seed: int, duration_s: float, n_speakers: int = 4):
    """(turn table as a dict of arrays, transcript result) of one file: turns of 0.3-6 s with a
    quarter talked over by a second speaker (~1,500 per hour), segments of 2-10 s (~600 per
    hour) holding ~15 words each, times rounded to 3 decimals as align() leaves them."""
    rng = np.random.default_rng(seed)
    labels = [f"SPEAKER_{i:02d}" for i in range(n_speakers)]
    start, end, spk = [], [], []
    t = 0.3
    while t < duration_s:
        d = float(rng.uniform(0.3, 6.0))
        s = int(rng.integers(n_speakers))
        start.append(t), end.append(t + d), spk.append(labels[s])
        if rng.random() < 0.25:
            o = float(rng.uniform(0.0, d))
            start.append(t + o), end.append(t + o + float(rng.uniform(0.3, 3.0)))
            spk.append(labels[(s + 1 + int(rng.integers(n_speakers - 1))) % n_speakers])
        t += d + float(rng.uniform(0.0, 0.5))
    segments = []
    t = 0.5
    while t < duration_s - 10.0:
        dur = float(rng.uniform(2.0, 10.0))
        words, w = [], t
        while w < t + dur - 0.1:
            wd = float(rng.uniform(0.1, 0.5))
            word = {"word": "w"}
            if rng.random() > 0.03:
                word.update(start=round(w, 3), end=round(min(w + wd, t + dur), 3), score=0.9)
            words.append(word)
            w += wd + float(rng.uniform(0.0, 0.2))
        segments.append({"start": round(t, 3), "end": round(t + dur, 3), "text": "x", "words": words})
        t += dur
    table = {"start": np.asarray(start), "end": np.asarray(end), "speaker": spk}
    return table, {"segments": segments, "language": "en"}


def workloads():
    from whisperx_amd.synthetic import corpus_durations

    return {"file_1h": [synth_file(1, 3600.0)],
            "corpus_10h": [synth_file(100 + i, d) for i, d in enumerate(corpus_durations())]}


def fresh(pairs):
    return [({k: (v.copy() if isinstance(v, np.ndarray) else list(v)) for k, v in t.items()}, copy.deepcopy(r))
            for t, r in pairs]


def shape_of(pairs):
    from whisperx_amd.diarize import _queries

    return {"files": len(pairs), "turns": int(sum(len(t["start"]) for t, _ in pairs)),
            "segments": int(sum(len(r["segments"]) for _, r in pairs)),
            "queries": int(sum(len(_queries(r)[0]) for _, r in pairs)),
            "speakers_per_file": len(set(pairs[0][0]["speaker"]))}


def time_calls(fn, prepare, repeat):
    out = []
    for _ in range(repeat):
        arg = prepare()
        t0 = time.perf_counter()
        fn(arg)
        out.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(out), "min_s": min(out), "repeat": repeat}


def kernel_leg(pairs, fill, steps, warmup):
    import ctypes

    import torch

    from whisperx_amd import _lib
    from whisperx_amd.diarize import _queries

    turns = _lib.SpeakerTurns([(t["start"], t["end"], t["speaker"]) for t, _ in pairs])
    qs, qe, q_off = [], [], [0]
    for _, r in pairs:
        _, a, b = _queries(r)
        qs.append(a), qe.append(b), q_off.append(q_off[-1] + len(a))
    qs, qe = np.concatenate(qs), np.concatenate(qe)
    Q = len(qs)
    dev = torch.device("cuda:0")
    spk = torch.empty(Q, dtype=torch.int32, device=dev)
    best = torch.empty(Q, dtype=torch.float64, device=dev)
    run = lambda: _lib.assign_speakers(turns, qs, qe, q_off, fill, device=dev, speaker_out=spk, best_out=best)  # noqa: E731
    run()
    torch.cuda.synchronize()
    # resident inputs: the same launch without the uploads
    lib = _lib.load()
    d = {k: torch.as_tensor(v).to(dev) for k, v in (("ts", turns.start), ("te", turns.end), ("to", turns.turn_off),
                                                     ("go", turns.grp_off), ("qs", qs), ("qe", qe),
                                                     ("qo", np.asarray(q_off, dtype=np.int64)))}
    p = {k: ctypes.c_void_p(v.data_ptr()) for k, v in d.items()}
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def launch():
        rc = lib.wx_assign_speakers(p["ts"], p["te"], p["to"], p["go"], turns.G, turns.n_turns, p["qs"], p["qe"], p["qo"],
                                    turns.F, Q, int(fill), ctypes.c_void_p(spk.data_ptr()),
                                    ctypes.c_void_p(best.data_ptr()), stream)
        assert rc == 0, rc

    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return {"per_launch_s": e0.elapsed_time(e1) / 1e3 / steps, "steps": steps, "warmup": warmup}


def reference_leg(pairs, fill, repeat):
    import pandas as pd

    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_diarize_golden import load_reference_diarize

    ref = load_reference_diarize()

    def prepare():
        return [(pd.DataFrame(t), r) for t, r in fresh(pairs)]

    def call(ps):
        for df, r in ps:
            ref.assign_word_speakers(df, r, fill_nearest=fill)
        call.last = ps

    res = time_calls(call, prepare, repeat)
    from whisperx_amd import diarize

    ours = fresh(pairs)
    diarize.assign_word_speakers_batch(ours, fill_nearest=fill, device="cpu")
    same = all(a[1] == b[1] for a, b in zip(ours, call.last))
    res.update(pandas=pd.__version__, host_route_labels_equal=bool(same))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="kernel,e2e,host")
    ap.add_argument("--workloads", default="file_1h,corpus_10h")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fill-nearest", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    legs = args.legs.split(",")
    from whisperx_amd import diarize

    fill = bool(args.fill_nearest)
    result = {"tool": "tools/diarize_bench.py", "fill_nearest": fill, "legs": legs,
              "cpu": platform.processor() or platform.machine(), "workloads": {}}
    if "kernel" in legs or "e2e" in legs:
        import torch

        result["device"] = torch.cuda.get_device_name(0)
    all_w = workloads()
    for name in args.workloads.split(","):
        pairs = all_w[name]
        w = {"shape": shape_of(pairs)}
        if "kernel" in legs:
            w["kernel"] = kernel_leg(pairs, fill, args.steps, args.warmup)
        if "e2e" in legs:
            diarize.assign_word_speakers_batch(fresh(pairs), fill_nearest=fill, device="cuda:0")  # warm-up
            w["e2e"] = time_calls(lambda ps: diarize.assign_word_speakers_batch(ps, fill_nearest=fill, device="cuda:0"),
                                  lambda: fresh(pairs), args.repeat)
        if "host" in legs:
            w["host"] = time_calls(lambda ps: diarize.assign_word_speakers_batch(ps, fill_nearest=fill, device="cpu"),
                                   lambda: fresh(pairs), max(1, args.repeat // 2))
        if "reference" in legs:
            w["reference"] = reference_leg(pairs, fill, 1)
        result["workloads"][name] = w
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

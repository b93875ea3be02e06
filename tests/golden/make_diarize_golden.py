"""Golden cases of the reference's assign_word_speakers (whisperx/diarize.py:35-67).

TEST INFRASTRUCTURE ONLY — run by hand where a reference checkout and pandas are present,
never on the GPU machine, never imported by the package or by the tests.  WHISPERX_ROOT names
the directory that holds the reference's `whisperx` package.  Its diarize.py is loaded behind a
stand-in for pyannote.audio (only DiarizationPipeline, which is not run, uses it), fed seeded
synthetic turn tables and transcripts, and only inputs and outputs are written to
diarize_cases.json.gz: the turn table, the transcript before and after, the two columns the
call leaves on the table and, for single-query cases, the per-speaker sums — pandas' own
groupby().sum() over the `intersection` column the reference leaves.

    WHISPERX_ROOT=/path/to/checkout python tests/golden/make_diarize_golden.py
"""
import copy
import gzip
import importlib.util
import json
import os
import sys
import types
from importlib.machinery import ModuleSpec

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference_diarize():
    root = os.environ.get("WHISPERX_ROOT")
    if not root:
        raise SystemExit("set WHISPERX_ROOT to the directory that holds the reference's whisperx package")
    pkg_dir = os.path.join(root, "whisperx")
    for name, attrs in (("pyannote", {}), ("pyannote.audio", {"Pipeline": object})):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__spec__ = ModuleSpec(name, None)
            for k, v in attrs.items():
                setattr(m, k, v)
            sys.modules[name] = m
    # a bare package object, so that diarize.py's `from .audio import ...` resolves without
    # running the reference's __init__.py (which imports everything else)
    pkg = types.ModuleType("ref_whisperx")
    pkg.__path__ = [pkg_dir]
    pkg.__spec__ = ModuleSpec("ref_whisperx", None, is_package=True)
    sys.modules["ref_whisperx"] = pkg
    spec = importlib.util.spec_from_file_location("ref_whisperx.diarize", os.path.join(pkg_dir, "diarize.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_whisperx.diarize"] = mod
    spec.loader.exec_module(mod)
    return mod


def table(start, end, speaker):
    return {"start": [float(x) for x in start], "end": [float(x) for x in end], "speaker": list(speaker)}


def single(qs, qe, **extra):
    """A transcript of one segment without words: one query."""
    return {"segments": [dict({"start": qs, "end": qe, "text": "x"}, **extra)]}


# ------------------------------------------------------------------------------ case 1
def realistic(seed):
    rng = np.random.default_rng(seed)
    n_spk = int(rng.integers(3, 7))
    labels = [f"SPEAKER_{i:02d}" for i in range(n_spk)]
    start, end, spk = [], [], []
    t = 0.5
    while t < 120.0:
        d = float(rng.uniform(0.4, 9.0))
        s = int(rng.integers(n_spk))
        start.append(t), end.append(t + d), spk.append(labels[s])
        if rng.random() < 0.35:  # a second speaker talks over the first
            o = float(rng.uniform(0.1, d))
            start.append(t + o), end.append(t + o + float(rng.uniform(0.3, 4.0)))
            spk.append(labels[(s + 1 + int(rng.integers(n_spk - 1))) % n_spk])
        t += d + (float(rng.uniform(0.0, 1.5)) if rng.random() < 0.6 else -float(rng.uniform(0.0, 0.3)))
    segments = []
    t = 0.8
    k = 0
    while t < 118.0:
        dur = float(rng.uniform(1.5, 8.0))
        seg = {"start": round(t, 3), "end": round(t + dur, 3), "text": f"segment {k}"}
        if k % 5 != 3:  # (every fifth segment has no 'words' key)
            words, w = [], t
            while w < t + dur - 0.05:
                wd = float(rng.uniform(0.08, 0.6))
                word = {"word": f"w{len(words)}"}
                if rng.random() > 0.12:  # (a word the aligner could not time has no 'start')
                    word.update(start=round(w, 3), end=round(min(w + wd, t + dur), 3), score=round(float(rng.random()), 3))
                words.append(word)
                w += wd + float(rng.uniform(0.0, 0.15))
            seg["words"] = words
        segments.append(seg)
        t += dur + float(rng.uniform(0.0, 1.0))
        k += 1
    # a segment (and words) past the last turn: overlaps nothing; its 'speaker' survives a miss
    far = max(end) + 50.0
    segments.append({"start": far, "end": far + 2.0, "text": "nothing here", "speaker": "KEPT",
                     "words": [{"word": "a", "start": far, "end": far + 0.5, "score": 0.5, "speaker": "KEPT_W"},
                               {"word": "b", "start": far + 0.6, "end": far + 1.0, "score": 0.5}]})
    segments.append({"start": round(far + 3.0, 3), "end": round(far + 4.0, 3), "text": "no words, no hit"})
    return table(start, end, spk), {"segments": segments, "language": "en"}


# ------------------------------------------------------------------------------ case 2
def ties(n, seed):
    """n speakers with exactly equal sums (dyadic lengths inside one query), rows shuffled."""
    rng = np.random.default_rng(seed)
    labels = [f"SPEAKER_{i:02d}" for i in range(n)]
    rows = []
    for lab in labels:  # two turns per speaker, 0.5 + 1.25 s, at dyadic positions
        a, b = float(rng.integers(0, 64)) * 0.25, float(rng.integers(0, 64)) * 0.25
        rows += [(2.0 + a, 2.5 + a, lab), (2.0 + b, 3.25 + b, lab)]
    order = rng.permutation(len(rows))
    while rows[order[0]][2] == labels[0]:  # the first row is not the first label
        order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    return table(*zip(*rows)), single(1.0, 40.0)


# ------------------------------------------------------------------------------ case 3
def summation_order(ref):
    """Two speakers with the same multiset of turn lengths in different row order inside one
    long query, such that a plain left-to-right fp64 sum picks another winner than the
    reference (Kahan-compensated groupby sum).  Every turn starts at 0, so x is the length."""
    for seed in range(2000):
        rng = np.random.default_rng(seed)
        n = 24
        small = rng.random(n) < 0.5
        lens = np.where(small, 0.01 * (1 + rng.random(n)), 50.0 * (1 + rng.random(n)))
        pa, pb = rng.permutation(n), rng.permutation(n)
        rows = [(0.0, float(lens[i]), "SPEAKER_00") for i in pa] + [(0.0, float(lens[i]), "SPEAKER_01") for i in pb]
        rows = [rows[i] for i in rng.permutation(2 * n)]
        tab = table(*zip(*rows))
        plain = {}
        for s, e, lab in rows:
            plain[lab] = plain.get(lab, 0.0) + (min(e, 1000.0) - max(s, 0.0))
        if plain["SPEAKER_00"] == plain["SPEAKER_01"]:
            continue
        plain_winner = max(sorted(plain), key=lambda k: plain[k])
        res = ref.assign_word_speakers(pd.DataFrame(tab), single(0.0, 1000.0), fill_nearest=False)
        if res["segments"][0]["speaker"] != plain_winner:
            return seed, tab, single(0.0, 1000.0), plain
    raise AssertionError("no seed separates the plain sum from the reference")


# ------------------------------------------------------------------------------ case 4
def degenerate():
    nan = float("nan")
    t3 = table([5.0, 1.0, 3.0, 2.0], [6.0, 2.5, 4.5, 3.5], ["B", "A", "B", "A"])  # not sorted by time
    out = [
        ("empty_table", table([], [], []), single(1.0, 2.0, speaker="KEPT")),
        ("one_turn_hit", table([1.0], [2.0], ["A"]), single(1.5, 3.0)),
        ("one_turn_miss", table([1.0], [2.0], ["A"]), single(2.5, 3.0, speaker="KEPT")),
        ("zero_length_query", t3, single(2.25, 2.25)),
        ("negative_length_query", t3, single(3.0, 2.0)),
        ("abutting", table([1.0, 4.0], [2.0, 5.0], ["A", "B"]), single(2.0, 4.0, speaker="KEPT")),
        ("nan_turn_start", table([nan, 1.0, 3.0], [2.0, 2.0, 3.5], ["A", "B", "A"]), single(0.5, 4.0)),
        ("nan_only_speaker", table([nan, 10.0], [2.0, 11.0], ["A", "B"]), single(0.5, 4.0)),
        ("unsorted_turns", t3, {"segments": [
            {"start": 0.5, "end": 6.5, "text": "all", "words": [
                {"word": "a", "start": 1.1, "end": 1.4}, {"word": "b", "start": 5.2, "end": 5.9},
                {"word": "c"}, {"word": "d", "start": 2.4, "end": 3.2}]}]}),
        ("no_segments", t3, {"segments": []}),
    ]
    return out


def n_queries(transcript):
    return sum(1 + sum("start" in w for w in s.get("words", [])) for s in transcript["segments"])


def run_case(ref, name, tab, transcript, fill_nearest, note=None):
    df = pd.DataFrame({"start": np.asarray(tab["start"], dtype=np.float64),
                       "end": np.asarray(tab["end"], dtype=np.float64), "speaker": tab["speaker"]})
    after = copy.deepcopy(transcript)
    got = ref.assign_word_speakers(df, after, fill_nearest=fill_nearest)
    assert got is after
    case = {"name": name, "fill_nearest": fill_nearest, "table": tab, "before": transcript, "after": after,
            "columns": None, "sums": None}
    if "intersection" in df.columns:
        case["columns"] = {"intersection": df["intersection"].tolist(), "union": df["union"].tolist()}
    if n_queries(transcript) == 1 and len(df):
        part = df if fill_nearest else df[df["intersection"] > 0]
        case["sums"] = {k: float(v) for k, v in part.groupby("speaker")["intersection"].sum().items()}
    if note:
        case["note"] = note
    return case


def main():
    ref = load_reference_diarize()
    cases = []
    for seed in (11, 12, 13):
        tab, tr = realistic(seed)
        for fill in (False, True):
            cases.append(run_case(ref, f"realistic_{seed}", tab, tr, fill))
    for n in (2, 3, 40):
        tab, tr = ties(n, 100 + n)
        for fill in (False, True):
            c = run_case(ref, f"tie_{n}", tab, tr, fill)
            assert len(set(c["sums"].values())) == 1 and len(c["sums"]) == n, c["sums"]
            assert c["after"]["segments"][0]["speaker"] == "SPEAKER_00"
            cases.append(c)
    seed, tab, tr, plain = summation_order(ref)
    c = run_case(ref, "summation_order", tab, tr, False,
                 note={"seed": seed, "plain_fp64_sums": plain})
    assert c["after"]["segments"][0]["speaker"] != max(sorted(plain), key=lambda k: plain[k])
    cases.append(c)
    for name, tab, tr in degenerate():
        for fill in (False, True):
            cases.append(run_case(ref, name, tab, tr, fill))
    path = os.path.join(HERE, "diarize_cases.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps({"cases": cases, "pandas": pd.__version__}, ensure_ascii=False).encode("utf-8"))
    print(len(cases), "cases,", os.path.getsize(path), "bytes; summation-order seed", seed)


if __name__ == "__main__":
    main()

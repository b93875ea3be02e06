"""Shared by test_diarize.py (host route) and test_gpu_diarize.py (kernel): the golden cases of
tests/golden/make_diarize_golden.py and the checks every case gets on either route."""
import copy
import gzip
import json
import os

import numpy as np

from conftest import GOLDEN

with gzip.open(os.path.join(GOLDEN, "diarize_cases.json.gz"), "rt", encoding="utf-8") as f:
    CASES = json.load(f)["cases"]
CASE_IDS = [f"{c['name']}-{'fill' if c['fill_nearest'] else 'hits'}" for c in CASES]


def table_of(case):
    """The case's turn table as a plain dict of arrays (a fresh one: the call adds columns)."""
    t = case["table"]
    return {"start": np.asarray(t["start"], dtype=np.float64), "end": np.asarray(t["end"], dtype=np.float64),
            "speaker": list(t["speaker"])}


def check_case(case, device):
    """Labels, untouched keys, the two columns and, where the fixture has them, the winning sum
    bit for bit, on the route `device` selects."""
    from whisperx_amd import diarize

    df = table_of(case)
    result = copy.deepcopy(case["before"])
    out = diarize.assign_word_speakers(df, result, fill_nearest=case["fill_nearest"], device=device)
    assert out is result
    assert result == case["after"], case["name"]  # every key: labels set, and nothing else changed
    if case["columns"] is None:
        assert set(df) == {"start", "end", "speaker"}
    else:
        for col in ("intersection", "union"):
            want = np.asarray(case["columns"][col], dtype=np.float64)
            assert np.array_equal(np.asarray(df[col], dtype=np.float64), want, equal_nan=True), (case["name"], col)
    if case["sums"] is not None:
        seg = case["before"]["segments"][0]
        spk, best, labels = diarize.assign_queries([(df["start"], df["end"], df["speaker"])], [seg["start"]],
                                                   [seg["end"]], [0, 1], case["fill_nearest"], device=device)
        if case["sums"]:
            winner = case["after"]["segments"][0]["speaker"]
            assert labels[0][int(spk[0])] == winner
            assert float(best[0]) == case["sums"][winner], (case["name"], float(best[0]), case["sums"][winner])
        else:
            assert int(spk[0]) == -1 and float(best[0]) == 0.0


def random_file(rng, n_queries, n_turns, n_speakers, sorted_queries, span=600.0):
    """One file's (table, q_start, q_end): turns shuffled in time, some times on a 0.25 s grid
    (equal sums and x == 0 happen), queries in sorted or shuffled time order."""
    ts = rng.uniform(0.0, span, n_turns)
    te = ts + rng.uniform(0.05, 12.0, n_turns)
    grid = rng.random(n_turns) < 0.3
    ts = np.where(grid, np.round(ts * 4) / 4, ts)
    te = np.where(grid, np.round(te * 4) / 4 + 0.25, te)
    if n_turns >= 300:
        ts[7] = np.nan  # a NaN turn start adds nothing in either mode
    labels = [f"SPEAKER_{i:02d}" for i in rng.permutation(n_speakers)]
    spk = [labels[i] for i in rng.integers(0, n_speakers, n_turns)]
    qs = rng.uniform(-5.0, span + 5.0, n_queries)
    qe = qs + rng.uniform(0.0, 6.0, n_queries)
    g = rng.random(n_queries) < 0.3
    qs = np.where(g, np.round(qs * 4) / 4, np.round(qs, 3))
    qe = np.where(g, np.round(qe * 4) / 4, np.round(qe, 3))
    if sorted_queries:
        order = np.argsort(qs, kind="stable")
        qs, qe = qs[order], qe[order]
    return (ts, te, spk), qs, qe

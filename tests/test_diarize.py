"""assign_word_speakers on the host route vs the reference's own results
(tests/golden/make_diarize_golden.py ran whisperx/diarize.py:35-67 under pandas): labels,
untouched keys, the two columns left on the turn table and, for single-query cases, the winning
per-speaker sum bit for bit (pandas' Kahan-compensated groupby().sum()).  CPU only; the same
cases run through the HIP kernel in test_gpu_diarize.py."""
import copy
import ctypes
import sys
import types

import numpy as np
import pytest

from diarize_helpers import CASES, CASE_IDS, check_case, random_file, table_of


@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_golden_case_host_route(ci):
    check_case(CASES[ci], "cpu")


def test_fixture_covers_the_issue_cases():
    names = {c["name"] for c in CASES}
    for n in ("realistic_11", "tie_2", "tie_3", "tie_40", "summation_order", "empty_table", "one_turn_hit",
              "zero_length_query", "negative_length_query", "abutting", "nan_turn_start", "unsorted_turns",
              "no_segments"):
        assert n in names
    for c in CASES:
        if c["name"] != "summation_order":
            assert any(d["name"] == c["name"] and d["fill_nearest"] != c["fill_nearest"] for d in CASES)


def test_summation_order_case_separates_kahan_from_a_plain_sum():
    """The fixture's own record: on this table a plain left-to-right fp64 sum ranks the two
    speakers the other way round than the reference did (so the golden test above fails for an
    implementation that sums with `s += x`)."""
    (case,) = [c for c in CASES if c["name"] == "summation_order"]
    plain = case["note"]["plain_fp64_sums"]
    winner = case["after"]["segments"][0]["speaker"]
    assert max(sorted(plain), key=lambda k: plain[k]) != winner
    assert max(sorted(case["sums"]), key=lambda k: case["sums"][k]) == winner


def test_device_none_without_a_device_is_the_host_route():
    import torch

    from whisperx_amd import diarize

    case = CASES[0]
    a, b = copy.deepcopy(case["before"]), copy.deepcopy(case["before"])
    diarize.assign_word_speakers(table_of(case), a, fill_nearest=case["fill_nearest"])
    diarize.assign_word_speakers(table_of(case), b, fill_nearest=case["fill_nearest"], device="cpu")
    assert a == b == case["after"]
    if not torch.cuda.is_available():
        assert not diarize._kernel_available()


def test_dataframe_and_dict_of_arrays_agree():
    pd = pytest.importorskip("pandas")
    from whisperx_amd import diarize

    for case in (CASES[0], CASES[1], [c for c in CASES if c["name"] == "nan_turn_start"][0]):
        d = table_of(case)
        df = pd.DataFrame(table_of(case))
        ra = diarize.assign_word_speakers(d, copy.deepcopy(case["before"]), case["fill_nearest"], device="cpu")
        rb = diarize.assign_word_speakers(df, copy.deepcopy(case["before"]), case["fill_nearest"], device="cpu")
        assert ra == rb == case["after"]
        assert list(df.columns) == ["start", "end", "speaker", "intersection", "union"]
        for col in ("intersection", "union"):
            assert np.array_equal(df[col].to_numpy(), d[col], equal_nan=True)


@pytest.mark.parametrize("fill", [False, True])
def test_batch_equals_per_file_calls(fill):
    from whisperx_amd import diarize

    cases = [c for c in CASES if c["fill_nearest"] == fill]
    pairs = [(table_of(c), copy.deepcopy(c["before"])) for c in cases]
    outs = diarize.assign_word_speakers_batch(pairs, fill_nearest=fill, device="cpu")
    assert len(outs) == len(cases)
    for c, (df, result), out in zip(cases, pairs, outs):
        assert out is result and result == c["after"], c["name"]
        single = table_of(c)
        diarize.assign_word_speakers(single, copy.deepcopy(c["before"]), fill, device="cpu")
        assert set(df) == set(single)
        for col in set(single) - {"speaker"}:
            assert np.array_equal(df[col], single[col], equal_nan=True), (c["name"], col)
    assert diarize.assign_word_speakers_batch([], device="cpu") == []


def test_host_route_on_random_shapes_matches_a_scalar_restatement():
    """The vectorised host route against a per-query scalar loop written from the semantics
    (DESIGN.md): participation, Kahan in group / row order, strict > over sorted labels."""
    from whisperx_amd import diarize

    rng = np.random.default_rng(5)
    for fill in (False, True):
        (ts, te, spk), qs, qe = random_file(rng, 37, 40, 5, sorted_queries=False)
        got, best, labels = diarize.assign_queries([(ts, te, spk)], qs, qe, [0, len(qs)], fill, device="cpu")
        for k in range(len(qs)):
            win, win_sum = -1, 0.0
            for r, lab in enumerate(labels[0]):
                s = c = 0.0
                exists = False
                for i in range(len(ts)):
                    if spk[i] != lab:
                        continue
                    x = float(np.minimum(te[i], qe[k]) - np.maximum(ts[i], qs[k]))
                    if fill:
                        exists = True
                    if (x == x) if fill else (x > 0):
                        y = x - c
                        t = s + y
                        c = (t - s) - y
                        s = t
                        exists = True
                if exists and (win < 0 or s > win_sum):
                    win, win_sum = r, s
            assert (int(got[k]), float(best[k])) == (win, win_sum), k


def test_labels_print_through_the_writers(tmp_path):
    from whisperx_amd import diarize, writers

    case = [c for c in CASES if c["name"] == "realistic_11" and not c["fill_nearest"]][0]
    result = diarize.assign_word_speakers(table_of(case), copy.deepcopy(case["before"]), device="cpu")
    result["language"] = "en"
    result["segments"] = [s for s in result["segments"] if "words" in s]  # (the subtitle writers need words)
    opts = {"max_line_width": None, "max_line_count": None, "highlight_words": False}
    writers.get_writer("srt", str(tmp_path))(result, "audio.wav", opts)
    text = (tmp_path / "audio.srt").read_text(encoding="utf-8")
    spoken = {s["speaker"] for s in result["segments"] if "speaker" in s and s["speaker"].startswith("SPEAKER_")}
    assert len(spoken) >= 2
    for lab in spoken:
        assert f"[{lab}]: " in text


def test_segment_is_re_exported():
    from whisperx_amd import diarize, vad
    import whisperx_amd

    assert diarize.Segment is vad.Segment
    assert whisperx_amd.assign_word_speakers is diarize.assign_word_speakers


def test_install_rebinds_assign_word_speakers():
    import whisperx_amd

    pkg = types.ModuleType("fake_whisperx_diar")
    pkg.align = None
    pkg.assign_word_speakers = None
    sys.modules["fake_whisperx_diar"] = pkg
    try:
        done = whisperx_amd.install(pkg, import_missing=False)
        assert ("fake_whisperx_diar", "assign_word_speakers") in done
        assert pkg.assign_word_speakers is whisperx_amd.assign_word_speakers
        assert whisperx_amd.integration.installed(pkg)
    finally:
        del sys.modules["fake_whisperx_diar"]


def test_speaker_turns_packing():
    from whisperx_amd import _lib

    t = _lib.SpeakerTurns([([5.0, 1.0, 3.0, 2.0], [6.0, 2.5, 4.5, 3.5], ["B", "A", "B", "A"]), ([], [], []),
                           ([1.0], [2.0], ["Z"])])
    assert t.labels == [["A", "B"], [], ["Z"]]
    assert t.start.tolist() == [1.0, 2.0, 5.0, 3.0, 1.0] and t.end.tolist() == [2.5, 3.5, 6.0, 4.5, 2.0]
    assert t.turn_off.tolist() == [0, 2, 4, 5] and t.grp_off.tolist() == [0, 2, 2, 3]
    assert (t.F, t.G, t.n_turns) == (3, 3, 5)


def test_abi_argument_validation_without_launch():
    from whisperx_amd import _lib

    _lib.build()  # as test_abi.py's fixture: a no-op once the library is built, a full build on a fresh tree
    lib = _lib.load(require_device=False)
    d = ctypes.c_void_p(8)
    call = lib.wx_assign_speakers
    #             ts te to go G  nt qs qe qo F  Q  fill spk best stream
    assert call(None, None, None, None, 0, 0, None, None, None, -1, 0, 0, None, None, None) == 1001
    assert call(d, d, d, d, 1, 1, d, d, d, 1, -1, 0, d, d, None) == 1001
    assert call(d, d, d, d, -1, 1, d, d, d, 1, 1, 0, d, d, None) == 1001
    assert call(d, d, d, d, 1, -1, d, d, d, 1, 1, 0, d, d, None) == 1001
    assert call(None, None, None, None, 0, 0, None, None, None, 0, 0, 0, None, None, None) == 0   # F == 0
    assert call(d, d, d, d, 1, 1, None, None, d, 1, 0, 1, None, None, None) == 0                   # Q == 0
    for missing in (2, 3, 6, 7, 8, 12):  # turn_off, grp_off, q_start, q_end, q_off, speaker
        args = [d, d, d, d, 1, 1, d, d, d, 1, 1, 0, d, d, None]
        args[missing] = None
        assert call(*args) == 1001, missing
    assert call(None, d, d, d, 1, 1, d, d, d, 1, 1, 0, d, None, None) == 1001  # turns without turn_start

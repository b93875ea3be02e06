"""wx_assign_speakers on the device: every golden case of the reference through the kernel, and
the kernel against the host route (pinned to the reference by test_diarize.py) bit for bit in
`speaker` and `best_sum`, at the shapes where a one-lane-per-query, 64-queries-per-wave kernel
can go wrong: Q around the wave size, empty / tiny / long turn tables, one to 40 speaker
groups, queries in shuffled time order (a wave's span is wide: the wave-uniform skip rarely
fires) and in sorted order (it fires often), both modes."""
import numpy as np
import pytest

from diarize_helpers import CASES, CASE_IDS, check_case, random_file, table_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_golden_case_kernel(ci):
    check_case(CASES[ci], "cuda:0")


def _both_routes(files, fill):
    """Kernel and host route on a batch of random_file() files; returns the two results."""
    import torch

    from whisperx_amd import _lib, diarize

    turns = _lib.SpeakerTurns([f[0] for f in files])
    q_off = np.cumsum([0] + [len(f[1]) for f in files])
    qs = np.concatenate([f[1] for f in files])
    qe = np.concatenate([f[2] for f in files])
    spk_d, best_d = _lib.assign_speakers(turns, qs, qe, q_off, fill, device="cuda:0")
    torch.cuda.synchronize()
    return (spk_d.cpu().numpy(), best_d.cpu().numpy()), diarize.assign_speakers_host(turns, qs, qe, q_off, fill)


def _assert_bit_equal(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64)), what


@pytest.mark.parametrize("Q", [1, 63, 64, 65, 257])
def test_kernel_equals_host_route_per_shape(Q):
    rng = np.random.default_rng(1000 + Q)
    hits = 0
    for n_turns in (0, 1, 2, 300):
        for n_spk in (1, 2, 5, 40):
            for sorted_q in (False, True):
                f = random_file(rng, Q, n_turns, n_spk, sorted_q)
                for fill in (False, True):
                    got, want = _both_routes([f], fill)
                    _assert_bit_equal(got, want, (Q, n_turns, n_spk, sorted_q, fill))
                    hits += int((want[0] >= 0).sum())
                    if n_turns == 0:
                        assert (got[0] == -1).all() and (got[1] == 0.0).all()
                    elif fill:
                        assert (got[0] >= 0).all()
    assert hits > 0


@pytest.mark.parametrize("fill", [False, True])
def test_batch_of_mixed_files_in_one_launch(fill):
    """Files of every shape above packed back to back: waves that straddle files, files
    without turns, files without queries."""
    rng = np.random.default_rng(77)
    files = [random_file(rng, q, t, s, bool(k % 2))
             for k, (q, t, s) in enumerate([(65, 300, 5), (0, 300, 2), (1, 0, 1), (63, 2, 40), (257, 300, 40), (0, 0, 1),
                                            (64, 1, 1), (3, 300, 1), (130, 40, 3)])]
    got, want = _both_routes(files, fill)
    _assert_bit_equal(got, want, fill)
    assert (want[0] >= 0).any() and (fill or (want[0] == -1).any())


@pytest.mark.parametrize("fill", [False, True])
def test_three_files_one_without_turns_one_without_queries(fill):
    import copy

    from whisperx_amd import diarize

    names = ("realistic_11", "empty_table", "no_segments")
    cases = [c for c in CASES if c["fill_nearest"] == fill and c["name"] in names]
    assert len(cases) == 3
    pairs = [(table_of(c), copy.deepcopy(c["before"])) for c in cases]
    diarize.assign_word_speakers_batch(pairs, fill_nearest=fill, device="cuda:0")
    for c, (df, result) in zip(cases, pairs):
        assert result == c["after"], c["name"]
        assert ("intersection" in df) == (c["columns"] is not None)


def test_outputs_as_views_leave_their_surroundings_untouched():
    import torch

    from whisperx_amd import _lib, diarize

    rng = np.random.default_rng(9)
    Q, pad = 65, 64
    tab, qs, qe = random_file(rng, Q, 300, 5, False)
    turns = _lib.SpeakerTurns([tab])
    spk_buf = torch.full((Q + 2 * pad,), -777, dtype=torch.int32, device="cuda:0")
    best_buf = torch.full((Q + 2 * pad,), -777.0, dtype=torch.float64, device="cuda:0")
    spk, best = _lib.assign_speakers(turns, qs, qe, [0, Q], False, device="cuda:0", speaker_out=spk_buf[pad:pad + Q],
                                     best_out=best_buf[pad:pad + Q])
    torch.cuda.synchronize()
    assert spk.data_ptr() == spk_buf[pad:].data_ptr()
    want = diarize.assign_speakers_host(turns, qs, qe, [0, Q], False)
    _assert_bit_equal((spk_buf[pad:pad + Q].cpu().numpy(), best_buf[pad:pad + Q].cpu().numpy()), want, "views")
    for buf, sentinel in ((spk_buf, -777), (best_buf, -777.0)):
        h = buf.cpu().numpy()
        assert (h[:pad] == sentinel).all() and (h[pad + Q:] == sentinel).all()


def test_install_style_default_device_uses_the_kernel():
    """device=None takes the kernel when a HIP device is present (and gives the fixture's result)."""
    from whisperx_amd import diarize

    assert diarize._kernel_available()
    check_case(CASES[0], None)


@pytest.mark.parametrize("spelling", ["str", "device", "device_index"])
def test_device_spellings_take_the_kernel(spelling, monkeypatch):
    """An index-less HIP device (the usual whisperX spelling, and what align() accepts) is the
    current device: the call runs the kernel, not the host route, and gives the fixture's result."""
    import torch

    from whisperx_amd import diarize

    device = {"str": "cuda", "device": torch.device("cuda"), "device_index": torch.device("cuda", 0)}[spelling]
    monkeypatch.setattr(diarize, "assign_speakers_host",
                        lambda *a, **k: pytest.fail("the host route ran for a HIP device"))
    check_case(CASES[0], device)
    check_case(CASES[1], device)

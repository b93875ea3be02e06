"""The selection probes' own conditions (tests/selection_probes.py), without a GPU: the numpy emulation
of wx_sample_token's and wx_beam_topk's structure passes every probe; each faulty variant of it, the
kind of mistake a kernel could make, is rejected by the probe named for it and accepted by the
probes it cannot act on; and the margins, skipped shares and gaps the probes rely on hold on the fp64
definition alone, so that another seed cannot weaken them unseen.  The emulation runs the square
probes (4101 rows) on edge_rows(): every 16th row and those about every edge of the column map."""
import contextlib
import io
import math

import numpy as np
import pytest

import sample_helpers as sh
import selection_probes as sp

ROWS = sp.edge_rows()
CONSTANT = [(V, m) for V in (1, 5, 1025, sp.N_EDGE) for m in (False, True) if not (m and V <= 3)]


def _sample_probes():
    """family -> [(probe, the rows the emulation runs)]"""
    masked = lambda t: [(sp.masked_units(u, via, t), None) for u in sp.UNITS for via in ("mask", "logits")]  # noqa: E731
    return {
        "every column wins, T 0": [(sp.every_column_wins(0.0), ROWS)],
        "every column wins, T 1": [(sp.every_column_wins(1.0), ROWS)],
        "ties": [(sp.tie_rows(), ROWS)],
        "constant rows": [(sp.constant_row(V, m), None) for V, m in CONSTANT],
        "pair rows": [(sp.pair_rows(t, s), ROWS) for t in (0.2, 1.0) for s in (0, 7)],
        "masked units, T 0": masked(0.0),
        "masked units, T 0.7": masked(0.7),
        "66 slices, T 0": [(sp.many_slices(0.0), None)],
        "66 slices, T 0.7": [(sp.many_slices(0.7), None)],
    }


def _topk_probes():
    return {
        "concentrated winners": [sp.concentrated_winners(G) for G in (1, 5, 8)],
        "constant rows": [sp.topk_constant_rows(G) for G in (1, 5, 8)],
        "equal maxima": [sp.topk_equal_maxima(G, span) for G in (1, 5, 8) for span in sp.TIE_SPANS],
        "identical beams": [sp.topk_identical_beams(G) for G in (2, 5, 8)],
        "edge V": [sp.topk_edge_v(G, V) for G in sp.EDGE_G for V in sp.edge_v(G)],
        "masked units": [sp.topk_masked_units(G) for G in (5, 8)],
        "66 slices": [sp.topk_many_slices(k) for k in ("beam 0", "beam 1")],
        "66 slices, tie": [sp.topk_many_slices("tie")],
    }


SAMPLE_FAMILIES = ("every column wins, T 0", "every column wins, T 1", "ties", "constant rows", "pair rows",
                   "masked units, T 0", "masked units, T 0.7", "66 slices, T 0", "66 slices, T 0.7")
TOPK_FAMILIES = ("concentrated winners", "constant rows", "equal maxima", "identical beams", "edge V", "masked units",
                 "66 slices", "66 slices, tie")


def _accepts(check) -> bool:
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            check()
        return True
    except AssertionError:
        return False


# --------------------------------------------------------------------------------- the emulation
@pytest.mark.parametrize("family", SAMPLE_FAMILIES)
def test_sample_emulation_passes(family):
    for p, rows in _sample_probes()[family]:
        assert p.check(p.emulate(rows), "emulation", rows) <= 1.0
        assert p.R == len(p.token) and not np.isnan(p.logprob).any()


@pytest.mark.parametrize("family", TOPK_FAMILIES)
def test_topk_emulation_passes(family):
    for p in _topk_probes()[family]:
        assert p.check(p.emulate(), "emulation") <= 1.0


def test_the_emulation_draws_the_definitions_uniforms():
    """_philox against Random123's known answers and sample_helpers' words."""
    for counter, key, out in sh.KNOWN_ANSWERS:
        assert tuple(int(w) for w in sp._philox(*counter, *key)) == out
    step = sp.STEPS[2]
    w = sp._philox(np.arange(5, dtype=np.uint64)[None, :], np.arange(3, dtype=np.uint64)[:, None], step & 0xFFFFFFFF,
                   step >> 32, sp.SEED & 0xFFFFFFFF, sp.SEED >> 32)
    assert np.array_equal(w.reshape(3, 20)[:, :18], sh._philox_words(3, 18, sp.SEED, step))


# ------------------------------------------------------------------------------------ the faults
# fault: (the family that must reject it, the other families it acts on: the reason)
SAMPLE_FAULTS = {
    "uniform_word_plus_1": ("pair rows", {"masked units, T 0.7"}),  # every drawn winner (a plant wins under any uniforms)
    "group_counter_per_slice": ("pair rows", {"masked units, T 0.7"}),  # drawn winners past slice 0
    "ties_to_higher_column_across_waves": ("ties", {"constant rows"}),  # a constant row is one tie
    # every winner outside wave 0 of its slice; a constant row's is column 0 or 3
    "logit_from_wave_0": ("every column wins, T 1", {"every column wins, T 0", "ties", "pair rows", "masked units, T 0",
                                                     "masked units, T 0.7", "66 slices, T 0", "66 slices, T 0.7"}),
    # only a drawn winner that is not its wave's largest logit: no planted one, no pair (both logits are 0)
    "logit_is_wave_max": ("masked units, T 0.7", set()),
    "merge_drops_slices_past_64": ("66 slices, T 0", {"66 slices, T 0.7"}),
    # a pair row's other slice is empty too
    "empty_slice_wins": ("masked units, T 0", {"masked units, T 0.7", "pair rows"}),
}
TOPK_FAULTS = {
    # edge V: 2G of no more than 65 columns share lanes
    "one_entry_per_lane": ("concentrated winners", {"edge V"}),
    # every tie, a row of -inf among them
    "previous_winner_by_value": ("equal maxima", {"constant rows", "masked units", "66 slices, tie"}),
    "merge_drops_slices_past_64": ("66 slices", {"66 slices, tie"}),
    "unguarded_empty_sum": ("masked units", set()),
    "equal_scores_by_slice": ("equal maxima", set()),
}


def test_the_fault_tables_are_the_modules():
    assert tuple(SAMPLE_FAULTS) == sp.SAMPLE_FAULTS and tuple(TOPK_FAULTS) == sp.TOPK_FAULTS


@pytest.mark.parametrize("fault", sp.SAMPLE_FAULTS)
def test_sample_fault_is_rejected_by_its_probe_and_by_no_other(fault):
    named, acts = SAMPLE_FAULTS[fault]
    for family, probes in _sample_probes().items():
        got = [_accepts(lambda: p.check(p.emulate(rows, fault=fault), fault, rows)) for p, rows in probes]
        if family == named:
            assert not all(got), (fault, family)
        elif family not in acts:
            assert all(got), (fault, family, [p.label for (p, _), ok in zip(probes, got) if not ok])
    if fault == "logit_from_wave_0":  # every probe of the family, and at plant 60 all but the rows of wave 0
        p = sp.every_column_wins(1.0)
        tok, lp = p.emulate(ROWS, fault=fault)
        wrong = np.abs(lp - p.logprob[ROWS]) > p.bound
        assert np.array_equal(tok, ROWS) and np.array_equal(wrong, (ROWS % sp.SLICE) >= 1024)
    if fault == "empty_slice_wins":  # the three units that empty a slice, by either way
        for u in sp.UNITS[1:]:
            for via in ("mask", "logits"):
                p = sp.masked_units(u, via, 0.0)
                assert not _accepts(lambda: p.check(p.emulate(fault=fault), fault)), p.label


@pytest.mark.parametrize("fault", sp.TOPK_FAULTS)
def test_topk_fault_is_rejected_by_its_probe_and_by_no_other(fault):
    named, acts = TOPK_FAULTS[fault]
    for family, probes in _topk_probes().items():
        got = [_accepts(lambda: p.check(p.emulate(fault=fault), fault)) for p in probes]
        if family == named:
            if fault == "equal_scores_by_slice":  # more than one beam, and a tie over two slices
                assert [ok for p, ok in zip(probes, got) if p.G > 1 and "slice edge" in p.label] == [False, False]
            else:
                assert not any(got), (fault, family, got)
        elif family not in acts:
            assert all(got), (fault, family, [p.label for p, ok in zip(probes, got) if not ok])


def test_checks_reject_nan_and_name_the_place():
    p = sp.masked_units("slice 1", "mask", 0.0)
    tok, lp = p.emulate()
    lp[1] = np.nan
    with pytest.raises(AssertionError, match="row 1, column"):
        p.check((tok, lp), "nan")
    tok[2] += 1
    with pytest.raises(AssertionError, match="row 2 took column"):
        p.check((tok, p.emulate()[1]), "token")
    t = sp.topk_masked_units(5)
    s, i = t.emulate()
    bad = s.copy()
    bad[1, 4] = np.nan  # (-inf by the definition)
    with pytest.raises(AssertionError, match="chunk 1 position 4"):
        t.check((bad, i), "nan")
    bad = s.copy()
    bad[0, 2] = np.float32(bad[0, 2] + 1e-3)
    with pytest.raises(AssertionError, match="chunk 0 position 2"):
        t.check((bad, i), "score")


# -------------------------------------------------------------- what the probes rely on, in fp64
def test_every_column_wins_by_the_definition():
    rows = np.arange(sp.N_EDGE)
    for t in (0.0, 1.0):
        p = sp.every_column_wins(t)
        assert np.array_equal(p.sel.token, rows) and p.keep.all() and p.bound == sh.logprob_bound(p.plant, sp.N_EDGE)
        assert float(p.x.max()) == p.plant and float(p.x.abs().max()) == p.plant
        print(f"{p.label}: smallest margin {p.sel.margin.min():.3e}, eps {p.eps:.3e}")
        assert p.sel.margin.min() > max(p.eps, 0.0)
    at60 = sh.definition(sp.every_column_wins(1.0).x, None, 0.0, sp.SEED, 0, np.zeros(sp.N_EDGE, dtype=bool), sp.N_EDGE - 1)
    assert np.array_equal(at60.token, rows)  # (plant 60: both temperatures)
    assert sp.every_column_wins(1.0).sel.margin.min() > 30


def test_ties_by_the_definition():
    p = sp.tie_rows()
    assert np.array_equal(p.sel.token, np.arange(sp.N_EDGE)) and float(p.x.max()) == 12.0
    n = (p.x == 12.0).sum(1)
    assert int(n[0]) == 7 and int(n.min()) == 1 and np.array_equal(p.sel.margin[n.numpy() > 1], np.zeros(int((n > 1).sum())))
    for d in sp.TIE_OFFSETS:
        assert bool((p.x[0, d] == 12.0))
    for V, m in CONSTANT:
        c = sp.constant_row(V, m)
        assert np.array_equal(c.sel.token, c.token) and np.allclose(c.sel.logprob, c.logprob, rtol=0, atol=1e-12)


def test_pair_rows_skip_nothing_and_give_both_answers():
    for t in (0.2, 1.0):
        for step, n_r in ((0, 2042), (7, 2110)):
            p = sp.pair_rows(t, step)
            assert p.eps == sh.eps_tokens(0.0, t) and p.keep.all()  # (check_margins caps the share at 1 %; it is 0)
            own = p.sel.token == np.arange(sp.N_EDGE)
            assert (own | (p.sel.token == (np.arange(sp.N_EDGE) + 1) % sp.N_EDGE)).all()
            print(f"{p.label}: token = r in {int(own.sum())} rows, smallest margin {p.sel.margin.min():.3e}")
            assert int(own.sum()) == n_r  # (the uniforms depend on neither the temperature nor the logits)
            assert np.allclose(p.sel.logprob, -math.log(2.0), rtol=0, atol=1e-12)
            assert int(p.done.sum()) == int((p.sel.token == sp.N_EDGE - 1).sum())


def test_masked_and_many_slice_probes_keep_every_row():
    for t in (0.0, 0.7):
        for u in sp.UNITS:
            m = sp.unit_mask(u)
            for via in ("mask", "logits"):
                p = sp.masked_units(u, via, t)
                assert p.keep.all() and p.sel.scored.all() and np.isfinite(p.logprob).all()
                assert not m.numpy()[p.token].any()
        p = sp.many_slices(t)
        assert p.keep.all() and -(-p.V // sp.SLICE) == 67
        assert [int(c) // sp.SLICE for c in p.token[:4]] == list(sp.MANY_SLICES)
    p = sp.many_slices(0.0)
    assert p.token.tolist() == p.cols and float(p.x[4, 64 * sp.SLICE + 77]) == float(p.x[4, 77]) == float(p.x[4].max())


def test_topk_probes_meet_the_gap_condition():
    n = 0
    for probes in _topk_probes().values():
        for p in probes:
            p.conditions()
            n += 1
    assert len(_topk_probes()["edge V"]) == 88 and n == 88 + 3 + 3 + 6 + 3 + 2 + 3
    sets = sp.concentrated_sets()
    lane = lambda c: (c // 1024, c % 64)  # noqa: E731  (slice and wave, lane)
    assert len({lane(c) for c in sets["one lane's 16 registers"]}) == 1
    assert len({(c % 1024) // 64 for c in sets["16 adjacent lanes of one register"]}) == 1
    assert len({c // 1024 for c in sets["16 columns of one wave"]}) == 1
    assert sorted(c // 1024 for c in sets["4 per wave of one slice"]) == sorted([4, 5, 6, 7] * 4)
    assert sorted(c // sp.SLICE for c in sets["the three slices and the tail"]) == sorted([0, 1, 2, 3] * 4)
    for G in (1, 5, 8):  # the live row's 2G best are the output, in the planted order
        p = sp.concentrated_winners(G)
        for b in range(p.B):
            g = b % G
            assert (p.index[b] // p.V == g).all()
            assert p.x[b * G + g].numpy()[p.index[b] % p.V].tolist() == [30.0 + j for j in range(2 * G)][::-1]
    for G in (5, 8):
        p = sp.topk_masked_units(G)
        assert bool((p.x[3] == -math.inf).all()) and bool((p.x[G] == -math.inf).all())
        assert math.isfinite(float(p.cum[3])) and math.isfinite(float(p.cum[G]))
        assert np.isfinite(p.want_s[0].numpy()).all() and np.isfinite(p.want_s[1, :3].numpy()).all()


"""WhisperDecoder.prefill without a GPU (the host route): first the tests' own causal reference and
checks (prefill_helpers) against two attentions whose mask is off by one key; then the decoder
oracles of whisper_decoder_helpers / beam_helpers / whisper_decoder_half_helpers through
prefill=True, the routes by which a position can be reached, the beams, the errors, and the default,
which must stay what it was bit for bit."""
import pytest
import torch

import beam_helpers as bh
import prefill_helpers as ph
import whisper_decoder_half_helpers as dh
from whisper_decoder_helpers import (GEOMETRIES, N_FORCED, PROMPT, case, check_forced_logits, check_greedy,
                                     check_stopping, check_suppression)

SMALL = GEOMETRIES[0]
BOTH = pytest.mark.parametrize("dtype", dh.DTYPES, ids=dh.name)


def _host(c, dtype=torch.float32):
    from whisperx_amd import WhisperDecoder

    return WhisperDecoder(c.model, device="cpu", dtype=dtype)


# ------------------------------------------------------------ the reference and the checks
@pytest.mark.parametrize("Tq,Tk,causal", [(33, 38, 5), (65, 98, 33), (2, 2, 0), (33, 78, 5), (31, 95, 0)])
def test_the_checks_reject_a_mask_that_is_off_by_one_key(Tq, Tk, causal):
    N = 3
    q, k, v, want, ref_err = ph.case(N, Tq, Tk, causal)
    assert ref_err > 0
    ph.check_accuracy(ph.reference(q, k, v, causal), want, ref_err, "fp32 torch")
    # the reference's mask, stated a second way: query i sees causal + i + 1 keys, never more than Tk
    seen = ph.keep(Tq, Tk, causal).sum(1)
    assert seen.tolist() == [min(Tk, causal + i + 1) for i in range(Tq)]
    row = Tq // 2
    alone = torch.softmax(ph.SCALE * (q[:, row:row + 1].double() @ k[:, :int(seen[row])].double().transpose(-1, -2)), -1) \
        @ v[:, :int(seen[row])].double()
    assert float((alone - want[:, row:row + 1]).abs().max()) < 1e-12
    for shift in (-1, 1):  # one key too few (j < causal + i), one too many (j <= causal + i + 1)
        with pytest.raises(AssertionError):
            ph.check_accuracy(ph.reference(q, k, v, causal, shift), want, ref_err, f"mask shifted by {shift}")
    u = ph.MaskedUniform(N, Tq, causal, Tk)
    # the form every kernel here uses, normalised at the end (attention_probes.reference_deferred)
    o = (ph.keep(Tq, Tk, causal).float() @ u.v) / u.n[None, :, None]
    assert u.check(o) <= 2.0 ** -22
    for shift in (-1, 1):
        w = ph.keep(Tq, Tk, causal, shift).float()
        with pytest.raises(AssertionError):
            u.check((w @ u.v) / w.sum(-1)[None, :, None])


def test_the_covering_set_holds_what_it_must():
    cover = ph.covering()
    assert {c[2] for c in cover} == {1, 2, 31, 32, 33, 65}
    assert {c[3] for c in cover if c[4] is None} == {1, 31, 32, 33, 129, 1500}
    assert {c[4] for c in cover if c[4] is not None and c[3] == c[4] + c[2]} == {0, 1, 5, 31, 32, 33, 100}
    assert {c[4] for c in cover if c[4] is not None and c[3] > c[4] + c[2]} >= {0, 5, 33, 100}
    assert {(c[0], c[1]) for c in cover} == set(ph.BATCHES)
    for m in ph.MUST:
        assert all((B, H, *m) in cover for B, H in ph.BATCHES)


# ------------------------------------------------------------------ the decoder's oracles
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_teacher_forced_logits(geometry):
    c = case(*geometry)
    check_forced_logits(c, ph.Prefilled(_host(c)), "host prefill")


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_greedy_equals_the_fp64_loop(geometry):
    c = case(*geometry)
    check_greedy(c, ph.Prefilled(_host(c)), "host prefill")


def test_stopping_and_suppression():
    c = case(*SMALL)
    dec = ph.Prefilled(_host(c))
    check_stopping(c, dec)
    check_suppression(c, dec, "host prefill")


@pytest.mark.parametrize("G", [2, 5])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_beam_search_equals_the_fp64_search(geometry, G):
    c = case(*geometry)
    got = bh.check_beam_search(c, ph.Prefilled(_host(c)), "host prefill", bh.EOT[c.D], G=G)
    assert all(len(hs) == G for hs in got)


@BOTH
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_half_teacher_forced_logits(geometry, dtype):
    c = case(*geometry)
    dh.check_forced_logits(c, ph.Prefilled(_host(c, dtype)), "host prefill")


@BOTH
def test_half_beam_search(dtype):
    c = case(*SMALL)
    dh.check_beam_search(c, ph.Prefilled(_host(c, dtype)), "host prefill")


# ------------------------------------------------------- the ways to reach a position
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_every_route_to_a_position_agrees(geometry):
    c = case(*geometry)
    ph.check_routes(_host(c), c, "host")


def test_all_positions_and_the_last_one():
    c = case(*SMALL)
    dec = _host(c)
    ids, y64, ref_err = c.forced()
    st = dec.start(c.enc)
    every = dec.prefill(st, ids, all_positions=True)
    assert tuple(every.shape) == (c.B, N_FORCED, c.V) and every.dtype == torch.float32 and st.pos == N_FORCED
    assert float((every.double() - y64).abs().max()) <= 4 * ref_err
    last = dec.prefill(dec.start(c.enc), ids)
    assert float((last - every[:, -1]).abs().max()) <= 8 * ref_err
    lists = dec.prefill(dec.start(c.enc), ids.tolist())  # (ids as lists, as step takes them)
    assert torch.equal(lists, last)
    ph.check_empty_batch(dec, c)


# ------------------------------------------------------------------------------ beams
def test_a_chunks_beams_are_bit_equal_after_prefill():
    c = case(*SMALL)
    ph.check_beams(_host(c), c)


# ----------------------------------------------------------------------------- errors
def test_errors():
    c = case(*SMALL)
    dec = _host(c)
    B, T = c.B, c.T
    st = dec.start(c.enc)
    good = torch.zeros((B, 4), dtype=torch.int64)
    for bad in (torch.zeros((B,), dtype=torch.int64), torch.zeros((B, 0), dtype=torch.int64),
                torch.zeros((B, 2, 2), dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"prefill: tokens must be \[B, n\]"):
            dec.prefill(st, bad)
    with pytest.raises(ValueError, match="prefill: tokens must be integer ids of shape"):
        dec.prefill(st, torch.zeros((B + 1, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="prefill: tokens must be integer ids"):
        dec.prefill(st, torch.zeros((B, 4)))
    with pytest.raises(ValueError, match="prefill: tokens must be integer ids"):
        dec.prefill(st, torch.zeros((B, 4), dtype=torch.bool))
    for lo, hi in ((-1, 0), (0, c.V)):
        ids = good.clone()
        ids[0, 1], ids[1, 2] = lo, hi
        with pytest.raises(ValueError, match="prefill: token ids must lie in"):
            dec.prefill(st, ids)
    with pytest.raises(ValueError, match="past max_target_positions"):
        dec.prefill(st, torch.zeros((B, T + 1), dtype=torch.int64))
    assert st.pos == 0  # no refusal moved the state
    dec.prefill(st, torch.zeros((B, T - 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="past max_target_positions"):
        dec.prefill(st, torch.zeros((B, 3), dtype=torch.int64))
    dec.prefill(st, torch.zeros((B, 2), dtype=torch.int64))  # up to the last position
    assert st.pos == T
    with pytest.raises(ValueError, match="past max_target_positions"):
        dec.prefill(st, torch.zeros((B, 1), dtype=torch.int64))
    with pytest.raises(ValueError):
        dec.step(st, torch.zeros((B,), dtype=torch.int64))
    beams = dec.start(c.enc, beams=2)
    with pytest.raises(ValueError, match="prefill: tokens must be integer ids of shape"):
        dec.prefill(beams, torch.zeros((2 * B, 3), dtype=torch.int64))  # one row per chunk, not per beam
    dec.step(beams, torch.zeros((2 * B,), dtype=torch.int64))
    with pytest.raises(ValueError, match="position 0 only"):
        dec.prefill(beams, good)
    with pytest.raises(ValueError, match="the prompt is empty"):
        dec.generate(c.enc, [], 2, prefill=True)


# ---------------------------------------------------------------------------- default
@pytest.mark.parametrize("dtype", [torch.float32, *dh.DTYPES], ids=["fp32", *map(dh.name, dh.DTYPES)])
def test_the_default_is_unchanged(dtype):
    c = case(*SMALL)
    dec = _host(c, dtype)
    ids, _, _ = c.forced()
    a, b = dec.logits(c.enc, ids), dec.logits(c.enc, ids, prefill=False)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    kw = dict(max_length=len(PROMPT) + 8)
    assert dec.generate(c.enc, PROMPT, 95, **kw) == dec.generate(c.enc, PROMPT, 95, prefill=False, **kw)
    x, y = dec.beam_search(c.enc, PROMPT, 95, 3, **kw), dec.beam_search(c.enc, PROMPT, 95, 3, prefill=False, **kw)
    assert x == y
    # the stepwise default is n calls to step, as before: the same bits as a hand-written loop
    st = dec.start(c.enc)
    loop = torch.stack([dec.step(st, ids[:, i]) for i in range(ids.shape[1])], 1)
    assert torch.equal(a.view(torch.int32), loop.view(torch.int32))

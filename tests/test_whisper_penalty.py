"""repetition_penalty and no_repeat_ngram_size on the host route (CPU only): the defaults change
nothing, greedy decoding, sampling and beam search against the numpy definition of
wx_penalize_logits (penalty_decoder_helpers), decode_with_fallback forwarding the options, and the
argument checks."""
import math

import pytest
import torch

from penalty_decoder_helpers import (N_STEPS, all_but, check_beam, check_defaults, check_greedy, check_host_case,
                                     check_sampled, host_decoder, repeats)
from whisper_decoder_helpers import GEOMETRIES, PROMPT, case


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_unpenalised_rows_repeat_ids_and_no_bigram(geometry):
    """What the cases below rest on."""
    c, dec = case(*geometry), host_decoder(geometry)
    plain = dec.generate(c.enc, PROMPT, c.V - 1, max_length=len(PROMPT) + N_STEPS)
    assert all(len(row) == N_STEPS and 11 <= len(set(row)) <= 15 and not repeats(row, 2) for row in plain)
    assert dec.generate(c.enc, PROMPT, c.V - 1, max_length=len(PROMPT) + N_STEPS, no_repeat_ngram_size=2) == plain


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_defaults_change_nothing(geometry):
    check_defaults(case(*geometry), host_decoder(geometry))


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_greedy_is_the_definition(geometry):
    c, dec = case(*geometry), host_decoder(geometry)
    three = all_but(geometry, 3)
    check_host_case(geometry, 1, repetition_penalty=8.0)
    check_host_case(geometry, 1, no_repeat_ngram_size=1)
    check_host_case(geometry, 2, three, no_repeat_ngram_size=2)
    check_host_case(geometry, 2, three, repetition_penalty=1.3, no_repeat_ngram_size=2, history_from=0)
    check_greedy(c, dec, "host", 1.3, 0)
    check_greedy(c, dec, "host", 8.0, 0)
    got, _ = check_greedy(c, dec, "host", 1.0, 1)
    assert all(len(row) == N_STEPS for row in got)
    check_greedy(c, dec, "host", 1.0, 2, suppress=three)
    check_greedy(c, dec, "host", 1.3, 2, history_from=0, suppress=three)
    # three ids left and none may come twice: every row ends after three, its logits all at -inf
    got, starved = check_greedy(c, dec, "host", 1.3, 1, suppress=three)
    assert starved == c.B and all(len(row) == 3 for row in got)


def test_history_from_counts_the_prompt():
    """With history_from = 0 and n = 1 no prompt id is generated; with the default they may be."""
    geometry = GEOMETRIES[0]
    c, dec = case(*geometry), host_decoder(geometry)
    plain = dec.generate(c.enc, PROMPT, c.V - 1, max_length=len(PROMPT) + N_STEPS, no_repeat_ngram_size=1)
    assert any(set(row) & set(PROMPT) for row in plain)
    for history_from, banned in ((0, PROMPT), (-1, PROMPT[-1:]), (len(PROMPT), [])):
        got, _ = check_greedy(c, dec, "host", 1.0, 1, history_from=history_from)
        assert not any(set(row) & set(banned) for row in got)
    assert check_greedy(c, dec, "host", 1.0, 1, history_from=len(PROMPT))[0] == plain


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_sampling_is_the_definition(geometry, dtype):
    from whisperx_amd import WhisperDecoder

    c = case(*geometry)
    dec = host_decoder(geometry) if dtype == torch.float32 else WhisperDecoder(c.model, device="cpu", dtype=dtype)
    kw = dict(temperature=0.8, best_of=3, seed=7, max_length=len(PROMPT) + 10)
    plain = host_decoder(geometry).sample(c.enc, PROMPT, c.V - 1, **kw)
    assert any(repeats(h.ids, 1) for hs in plain for h in hs)
    assert host_decoder(geometry).sample(c.enc, PROMPT, c.V - 1, repetition_penalty=1.3, no_repeat_ngram_size=2, **kw) != plain
    check_sampled(c, dec, "host", 0.8, 3, 7, 1.3, 2, host=True)
    check_sampled(c, dec, "host", 0.8, 3, 7, 1.3, 2, history_from=0, host=True)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_beam_histories_follow_the_beams(geometry):
    c, dec = case(*geometry), host_decoder(geometry)
    check_beam(c, dec, 1)
    hyps = check_beam(c, dec, 2, suppress=all_but(geometry, 6))
    # generate(beam_size > 1) forwards the options
    got = dec.generate(c.enc, PROMPT, c.V - 1, max_length=len(PROMPT) + N_STEPS, beam_size=5, no_repeat_ngram_size=2,
                       suppress_tokens=list(all_but(geometry, 6)))
    assert got == [hs[0].ids for hs in hyps]


def test_fallback_forwards_the_options():
    geometry = GEOMETRIES[0]
    c, dec = case(*geometry), host_decoder(geometry)
    kw = dict(max_length=len(PROMPT) + N_STEPS)
    beams = dec.beam_search(c.enc, PROMPT, c.V - 1, no_repeat_ngram_size=1, **kw)
    out = dec.decode_with_fallback(c.enc, PROMPT, c.V - 1, temperatures=(0.0,), no_repeat_ngram_size=1, **kw)
    assert [r.ids for r in out] == [hs[0].ids for hs in beams] and not any(repeats(r.ids, 1) for r in out)
    assert [r.sum_logprob for r in out] == [hs[0].sum_logprob for hs in beams]
    assert [r.ids for r in out] != [r.ids for r in dec.decode_with_fallback(c.enc, PROMPT, c.V - 1, temperatures=(0.0,), **kw)]
    options = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, history_from=0)
    for T, seed in ((0.0, 5), (0.7, 11)):  # the sample passes: beam_size 1 at temperature 0, best_of above it
        want = dec.sample(c.enc, PROMPT, c.V - 1, temperature=T, best_of=3 if T else 1, seed=seed, **options, **kw)
        out = dec.decode_with_fallback(c.enc, PROMPT, c.V - 1, temperatures=(T,), beam_size=1, best_of=3, seed=seed,
                                       **options, **kw)
        assert [(r.ids, r.sum_logprob) for r in out] == [(hs[0].ids, hs[0].sum_logprob) for hs in want]
    # every pass gets them: the second pass of a chunk that fails the first is the penalised sample
    out = dec.decode_with_fallback(c.enc, PROMPT, c.V - 1, temperatures=(0.0, 0.7), log_prob_threshold=0.0, best_of=3,
                                   seed=10, **options, **kw)
    want = dec.sample(c.enc, PROMPT, c.V - 1, temperature=0.7, best_of=3, seed=11, **options, **kw)
    assert all(r.attempts == 2 for r in out)
    for r, hs, first in zip(out, want, dec.beam_search(c.enc, PROMPT, c.V - 1, **options, **kw)):
        best = max((first[0], hs[0]), key=lambda h: h.score)
        assert r.ids == best.ids and not repeats(PROMPT + r.ids, 2)


def test_refusals():
    geometry = GEOMETRIES[0]
    c, dec = case(*geometry), host_decoder(geometry)
    calls = (lambda **kw: dec.generate(c.enc, PROMPT, 5, **kw), lambda **kw: dec.generate(c.enc, PROMPT, 5, beam_size=2, **kw),
             lambda **kw: dec.beam_search(c.enc, PROMPT, 5, **kw), lambda **kw: dec.sample(c.enc, PROMPT, 5, **kw),
             lambda **kw: dec.decode_with_fallback(c.enc, PROMPT, 5, **kw))
    started = []
    start = dec.start
    dec.start = lambda *a, **kw: started.append(1) or start(*a, **kw)
    try:
        for call in calls:
            for rho in (0.0, -1.3, math.inf, math.nan, 1e-60, 1e60):
                with pytest.raises(ValueError, match="repetition_penalty"):
                    call(repetition_penalty=rho)
            for n in (-1, 1.5):
                with pytest.raises(ValueError, match="no_repeat_ngram_size"):
                    call(no_repeat_ngram_size=n)
            for i in (len(PROMPT) + 1, -len(PROMPT) - 1):
                with pytest.raises(ValueError, match="history_from"):
                    call(history_from=i)
                with pytest.raises(ValueError, match="history_from"):
                    call(history_from=i, repetition_penalty=1.3)
        assert not started  # every refusal came before start
    finally:
        dec.start = start


def test_a_history_longer_than_the_kernel_reads_is_refused():
    """max_target_positions above WX_PENALTY_MAX_HISTORY: the check is on what the call can reach."""
    from whisperx_amd import WhisperDecoder
    from whisper_decoder_helpers import make_model, make_states

    model = make_model(64, 1, 4, 16, 1100)
    dec = WhisperDecoder(model, device="cpu")
    enc = make_states(1, 4, 64)
    with pytest.raises(ValueError, match="history"):
        dec.generate(enc, PROMPT, 5, max_length=1100, repetition_penalty=1.3)
    with pytest.raises(ValueError, match="history"):
        dec.generate(enc, PROMPT, 5, max_length=1026, no_repeat_ngram_size=2, history_from=0)
    assert len(dec.generate(enc, PROMPT, 15, max_length=len(PROMPT) + 4, no_repeat_ngram_size=1, history_from=0)[0]) <= 4
    assert dec.generate(enc, PROMPT, 5, max_length=1100) is not None  # the defaults read no history

"""repetition_penalty and no_repeat_ngram_size on the HIP route: every rewrite is one
wx_penalize_logits launch on a history kept on the device.  The conditions are the host route's
(penalty_decoder_helpers: the numpy definition on the decoder's own teacher-forced logits, exactly
at temperature 0), then graph=True against graph=False exactly, beam search's histories following
`reorder`, and decode_with_fallback's decisions against the host route's.  Every case is first
shown to be one on the host route."""
import pytest
import torch

from penalty_decoder_helpers import (N_STEPS, all_but, check_beam, check_defaults, check_greedy, check_host_case,
                                     check_sampled, host_decoder, repeats)
from sample_helpers import path_error
from whisper_decoder_helpers import GEOMETRIES, PROMPT, case

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])


def _device(c, dtype=torch.float32):
    from whisperx_amd import WhisperDecoder

    return WhisperDecoder(c.model, device="cuda", dtype=dtype)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_defaults_change_nothing(geometry):
    c = case(*geometry)
    dec = _device(c)
    check_defaults(c, dec)
    check_defaults(c, dec, graph=True)
    assert dec._plans and all(p.selection is None or p.selection.history is None for p in dec._plans.values())  # nothing new


@DTYPES
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_greedy_is_the_definition(geometry, dtype):
    c = case(*geometry)
    three = all_but(geometry, 3)
    check_host_case(geometry, 1, repetition_penalty=8.0)
    check_host_case(geometry, 1, no_repeat_ngram_size=1)
    check_host_case(geometry, 2, three, no_repeat_ngram_size=2)
    check_host_case(geometry, 2, three, repetition_penalty=1.3, no_repeat_ngram_size=2, history_from=0)
    dec = _device(c, dtype)
    cases = ((1.3, 0, None, ()), (8.0, 0, None, ()), (1.0, 1, None, ()), (1.0, 2, None, three), (1.3, 2, 0, three),
             (1.3, 1, None, three))
    for rho, n, history_from, suppress in cases:
        got, starved = check_greedy(c, dec, "hip", rho, n, history_from=history_from, suppress=suppress)
        if (n, suppress) == (1, three):  # three ids left, none twice: every row ends with its logits all at -inf
            assert starved == c.B and all(len(row) == 3 for row in got)
        args = dict(max_length=len(PROMPT) + N_STEPS, suppress_tokens=list(suppress), repetition_penalty=rho,
                    no_repeat_ngram_size=n, history_from=history_from, graph=True)
        for sync_every in (1, 8):
            assert dec.generate(c.enc, PROMPT, c.V - 1, sync_every=sync_every, **args) == got, (rho, n, sync_every)


@DTYPES
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_sampling_is_the_definition(geometry, dtype):
    c = case(*geometry)
    host = host_decoder(geometry)
    kw = dict(temperature=0.8, best_of=3, seed=7, max_length=len(PROMPT) + 10)
    options = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    plain = host.sample(c.enc, PROMPT, c.V - 1, **kw)
    assert any(repeats(h.ids, 1) for hs in plain for h in hs)
    assert host.sample(c.enc, PROMPT, c.V - 1, **options, **kw) != plain
    dec = _device(c, dtype)
    direct = check_sampled(c, dec, "hip", 0.8, 3, 7, 1.3, 2)
    for sync_every in (1, 8):
        assert dec.sample(c.enc, PROMPT, c.V - 1, graph=True, sync_every=sync_every, **options, **kw) == direct
    # the same plan, the other history length: another selection graph, the same step graph
    before = dec.graph_captures
    direct = check_sampled(c, dec, "hip", 0.8, 3, 7, 1.3, 2, history_from=0)
    assert dec.sample(c.enc, PROMPT, c.V - 1, graph=True, history_from=0, **options, **kw) == direct
    assert dec.sample(c.enc, PROMPT, c.V - 1, graph=True, **kw) == dec.sample(c.enc, PROMPT, c.V - 1, **kw)
    assert dec.graph_captures == before


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_beam_histories_follow_the_beams(geometry):
    c = case(*geometry)
    six = all_but(geometry, 6)
    host = host_decoder(geometry)
    check_beam(c, host, 1)
    check_beam(c, host, 2, suppress=six)
    dec = _device(c)
    for n, suppress in ((1, ()), (2, six)):
        direct = check_beam(c, dec, n, suppress=suppress)
        assert check_beam(c, dec, n, suppress=suppress, graph=True) == direct


def test_fallback_forwards_the_options_and_decides_as_the_host_route_does():
    """As test_gpu_whisper_sample's fallback test, with no_repeat_ngram_size = 1 on every pass (a ban
    moves a logit to -inf on both routes alike, so that test's bounds stand): the threshold lies
    between the host route's first-pass averages with more than 8 ref_err on both sides, asserted
    on the CPU before the GPU is asked."""
    c = case(*GEOMETRIES[0])
    host = host_decoder(GEOMETRIES[0])
    eot, kw = c.V - 1, dict(max_length=len(PROMPT) + 10, no_repeat_ngram_size=1)
    first = host.beam_search(c.enc, PROMPT, eot, **kw)
    assert not any(repeats(hs[0].ids, 1) for hs in first)
    avg = sorted(hs[0].score for hs in first)
    gap = max(range(len(avg) - 1), key=lambda i: avg[i + 1] - avg[i])
    threshold = (avg[gap] + avg[gap + 1]) / 2
    ref_err = max(path_error(c, torch.float32, b, (PROMPT + hs[0].ids + [eot])[:len(PROMPT) + 9])[1] for b, hs in enumerate(first))
    failed = [b for b in range(c.B) if first[b][0].score < threshold]
    second = host.sample(c.enc[failed], PROMPT, eot, temperature=0.7, best_of=3, seed=12, **kw)
    near = min([abs(a - threshold) for a in avg] + [abs(hs[0].score - threshold) for hs in second]
               + [abs(hs[0].score - first[b][0].score) for b, hs in zip(failed, second)])
    print(f"threshold {threshold:.4f}, nearest average {near:.3e} away, 8 ref_err {8 * ref_err:.3e}")
    assert failed and len(failed) < c.B and near > 8 * ref_err
    args = dict(temperatures=(0.0, 0.7), log_prob_threshold=threshold, seed=11, best_of=3, **kw)
    want = host.decode_with_fallback(c.enc, PROMPT, eot, **args)
    dec = _device(c)
    beams = dec.beam_search(c.enc, PROMPT, eot, **kw)
    for extra in ({}, dict(graph=True)):
        got = dec.decode_with_fallback(c.enc, PROMPT, eot, **args, **extra)
        assert [(r.temperature, r.attempts) for r in got] == [(r.temperature, r.attempts) for r in want]
        for b, (g, w) in enumerate(zip(got, want)):
            assert abs(g.avg_logprob - w.avg_logprob) <= 16 * ref_err and not repeats(g.ids, 1)
            if g.temperature == 0:  # the greedy pass: beam_search's repeat-free ids
                assert g.ids == beams[b][0].ids


def test_a_plan_serves_penalised_and_plain_calls_in_turn():
    """One plan, one selection: a penalised generate, a plain one and a penalised one with another
    history length give what the direct route gives, whatever ran before on the plan's buffers."""
    c = case(*GEOMETRIES[0])
    dec = _device(c)
    kw = dict(max_length=len(PROMPT) + N_STEPS)
    calls = (dict(no_repeat_ngram_size=1), {}, dict(repetition_penalty=8.0, history_from=0), dict(no_repeat_ngram_size=1), {})
    want = [dec.generate(c.enc, PROMPT, c.V - 1, **kw, **o) for o in calls]
    assert want[0] != want[1] and want[2] != want[1]
    got = [dec.generate(c.enc, PROMPT, c.V - 1, graph=True, **kw, **o) for o in calls]
    assert got == want and dec.graph_captures == 1

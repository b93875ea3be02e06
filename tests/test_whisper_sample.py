"""Sampling and temperature fallback on the host route (CPU only): Philox4x32-10's known answers, the
distribution of the selection's definition (sample_helpers.definition, fp64), WhisperDecoder.sample
against that definition on the decoder's own teacher-forced logits, the fallback loop of
decode_with_fallback on scripted passes and end to end, and the argument checks."""
import math

import numpy as np
import pytest
import torch

from sample_helpers import (KNOWN_ANSWERS, _philox_words, check_sample, chi_square_quantile, definition, philox)
from whisper_decoder_helpers import GEOMETRIES, PROMPT, case, hf_logits

N_STEPS = 10


@pytest.fixture(scope="module")
def decoders():
    from whisperx_amd import WhisperDecoder

    made = {}

    def get(geometry, dtype=torch.float32):
        key = (tuple(geometry), dtype)
        if key not in made:
            made[key] = WhisperDecoder(case(*geometry).model, device="cpu", dtype=dtype)
        return made[key]
    return get


# ------------------------------------------------------------------------------- the generator
def test_philox_known_answers():
    from whisperx_amd.whisper import gumbel_uniforms, philox4x32_10

    for counter, key, want in KNOWN_ANSWERS:
        assert philox(counter, key) == want
        assert tuple(int(w) for w in philox4x32_10(counter, key)) == want
    # the array forms count as the header says: block t >> 2, word t & 3, row r, both words of step and seed
    R, V, seed, step = 3, 10, (7 << 32) + 5, (1 << 32) + 1
    words = _philox_words(R, V, seed, step)
    for r in range(R):
        for t in range(V):
            assert int(words[r, t]) == philox((t >> 2, r, step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32))[t & 3]
    u = gumbel_uniforms(seed, R, V, step)
    assert np.array_equal(u, ((words >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23)
    assert 0 < u.min() and u.max() < 1
    # the extremes are exact in fp32 and neither 0 nor 1
    for x in (0, 0xFFFFFFFF):
        v = np.float32((np.float32(x >> 9) + np.float32(0.5)) * np.float32(2.0 ** -23))
        assert float(v) == ((x >> 9) + 0.5) * 2.0 ** -23 and 0 < float(v) < 1


@pytest.mark.parametrize("temperature", [0.2, 0.6, 1.0])
def test_the_definition_samples_the_tempered_softmax(temperature):
    """8192 identical rows of V = 96 logits (2 randn): Pearson's chi-square of the token counts
    against softmax(l / T), cells with expectation below 5 pooled, stays below the 1 - 1e-6 quantile
    of its distribution, for seeds 1 to 3."""
    R, V = 8192, 96
    row = 2 * torch.randn(V, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    p = torch.softmax(row / float(np.float32(temperature)), -1).numpy()
    logits = row.numpy()[None, :].repeat(R, 0)
    big = p * R >= 5
    expected = np.append(p[big] * R, p[~big].sum() * R)
    for seed in (1, 2, 3):
        sel = definition(logits, None, temperature, seed, 3, np.zeros(R, dtype=bool), V - 1)
        counts = np.bincount(sel.token, minlength=V)
        observed = np.append(counts[big], counts[~big].sum())
        keep = expected > 0
        chi2 = float((((observed - expected) ** 2)[keep] / expected[keep]).sum())
        df = int(keep.sum()) - 1
        bound = chi_square_quantile(df, 1e-6)
        print(f"T {temperature} seed {seed}: chi-square {chi2:.1f} at {df} degrees of freedom, bound {bound:.1f}")
        assert observed.sum() == R and chi2 < bound
        # the log-probability is the untempered one
        assert np.allclose(sel.logprob, torch.log_softmax(row, -1).numpy()[sel.token], rtol=0, atol=1e-12)


def test_the_definition_on_special_rows():
    V, eot = 12, 5
    x = torch.randn((4, V), generator=torch.Generator().manual_seed(1)).numpy()
    x[0, 3] = x[0, 9] = 7.0  # a tie: the lowest id
    x[1, :] = -np.inf  # fully masked
    x[3, eot] = 50.0
    done = np.array([False, False, True, False])
    sel = definition(x, None, 0.0, 0, 0, done, eot)
    assert sel.token.tolist() == [3, eot, eot, eot] and sel.done.tolist() == [False, True, True, True]
    assert sel.logprob[1] == 0 and sel.logprob[2] == 0 and sel.logprob[0] < 0 and sel.scored.tolist() == [True, False, False, True]
    suppress = np.zeros(V, dtype=bool)
    suppress[[3, 9]] = True
    assert definition(x, suppress, 0.0, 0, 0, done, eot).token[0] not in (3, 9)


# -------------------------------------------------------------------- the decoder's host route
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_sample_is_the_definition_on_the_decoders_logits(geometry, dtype, decoders):
    c, dec = case(*geometry), decoders(geometry, dtype)
    check_sample(c, dec, "host", 0.6, 3, seed=4, n_steps=N_STEPS, host=True)
    hyps = check_sample(c, dec, "host", 1.0, 5, seed=9, n_steps=N_STEPS, host=True, eot=c.V // 3)
    assert min(len(h.ids) for hs in hyps for h in hs) < N_STEPS  # this eot ends rows early
    greedy = check_sample(c, dec, "host", 0.0, 1, seed=0, n_steps=N_STEPS, host=True)
    assert [hs[0].ids for hs in greedy] == dec.generate(c.enc, PROMPT, c.V - 1, max_length=len(PROMPT) + N_STEPS)


def test_masks_seeds_and_prefill(decoders):
    c = case(*GEOMETRIES[0])
    dec = decoders(GEOMETRIES[0])
    kw = dict(temperature=1.0, best_of=4, max_length=len(PROMPT) + N_STEPS)
    plain = dec.sample(c.enc, PROMPT, c.V - 1, seed=2, **kw)
    assert dec.sample(c.enc, PROMPT, c.V - 1, seed=2, **kw) == plain
    assert dec.sample(c.enc, PROMPT, c.V - 1, seed=3, **kw) != plain
    seen = sorted({t for hs in plain for h in hs for t in h.ids})
    banned = seen[::2]
    hyps = check_sample(c, dec, "host masks", 1.0, 4, seed=2, n_steps=N_STEPS, suppress=banned, host=True)
    assert not {t for hs in hyps for h in hs for t in h.ids} & set(banned)
    first = sorted({h.ids[0] for hs in plain for h in hs if h.ids})
    hyps = check_sample(c, dec, "host first", 1.0, 4, seed=2, n_steps=N_STEPS, suppress_at_start=first, host=True)
    assert all(h.ids[0] not in first for hs in hyps for h in hs if h.ids)
    assert {t for hs in hyps for h in hs for t in h.ids[1:]} & set(first)  # position 0 only
    # prefill feeds the same prompt through other GEMM shapes: same structure, sums of the same quality
    pre = dec.sample(c.enc, PROMPT, c.V - 1, seed=2, prefill=True, **kw)
    assert [len(hs) for hs in pre] == [4] * c.B and all(x.score >= y.score for hs in pre for x, y in zip(hs, hs[1:]))


# --------------------------------------------------------------------------- the fallback loop
class Script:
    """Stand-ins for the decoder's two passes (_beam_search, _sample: what beam_search and sample
    return, with the scored positions and the no-speech probabilities): chunk b is recognised by
    encoder_states[b, 0, 0] == b, its attempt at temperature T is table[b][T] = (ids, sum, n)."""

    def __init__(self, dec, table, no_speech):
        self.table, self.no_speech, self.calls = table, no_speech, []
        dec._beam_search, dec._sample = self.beam, self.sample

    def _answer(self, kind, sub, T, probe, **info):
        from whisperx_amd import Hypothesis

        chunks = [int(v) for v in sub[:, 0, 0].tolist()]
        self.calls.append(dict(kind=kind, chunks=chunks, T=T, probe=probe, **info))
        rows = [self.table[b][T] for b in chunks]
        prob = None if probe is None else torch.tensor([self.no_speech[b] for b in chunks])
        return [[Hypothesis(i, s, s / n)] for i, s, n in rows], [[n] for _, _, n in rows], prob

    def beam(self, sub, prompt, eot, beam_size, patience, length_penalty, max_length, suppress_tokens, suppress_at_start,
             kernels, prefill, graph, probe=None):
        return self._answer("beam", sub, 0.0, probe, beam_size=beam_size, patience=patience, length_penalty=length_penalty)

    def sample(self, sub, prompt, eot, temperature, best_of, seed, max_length, suppress_tokens, suppress_at_start, kernels,
               prefill, graph, sync_every, probe=None):
        return self._answer("sample", sub, temperature, probe, best_of=best_of, seed=seed)


TEXT = {(1,): "the quick brown fox", (2,): "ab" * 200, (3,): "jumps over the lazy dog"}
TABLE = {
    0: {0.0: ([1], -1.0, 2)},                                                          # passes at once
    1: {0.0: ([1], -3.0, 2), 0.4: ([3], -1.6, 2)},                                     # too unlikely at 0
    2: {0.0: ([2], -0.2, 2), 0.4: ([3], -0.4, 2)},                                     # repetitive at 0
    3: {0.0: ([1], -3.0, 2), 0.4: ([3], -0.2, 2)},                                     # unlikely, but silence
    4: {0.0: ([1], -6.0, 2), 0.4: ([3], -4.0, 2), 0.8: ([1, 3], -6.0, 3)},            # never good enough
}
NO_SPEECH = {0: 0.1, 1: 0.2, 2: 0.3, 3: 0.9, 4: 0.5}


def _fallback(**kw):
    from whisperx_amd import WhisperDecoder

    c = case(*GEOMETRIES[0])
    dec = WhisperDecoder(c.model, device="cpu")
    script = Script(dec, TABLE, NO_SPEECH)
    enc = torch.zeros((5, 2, c.D))
    enc[:, 0, 0] = torch.arange(5.0)
    args = dict(temperatures=(0.0, 0.4, 0.8), no_speech_token=6, sot_index=1, text_of=lambda ids: TEXT[tuple(ids[:1])],
                seed=100, best_of=3)
    args.update(kw)
    return dec.decode_with_fallback(enc, PROMPT, 9, **args), script.calls


def test_fallback_loop_on_scripted_passes():
    from whisperx_amd import DecodingResult
    from whisperx_amd.utils import compression_ratio

    assert compression_ratio(TEXT[(2,)]) > 2.4 > compression_ratio(TEXT[(1,)]) > 0.5
    assert compression_ratio("ab" * 200) == 400 / len(__import__("zlib").compress(b"ab" * 200))
    out, calls = _fallback()
    assert [(k["kind"], k["chunks"], k["T"]) for k in calls] == [("beam", [0, 1, 2, 3, 4], 0.0), ("sample", [1, 2, 4], 0.4),
                                                                  ("sample", [4], 0.8)]
    assert calls[0]["probe"] == (1, 6) and calls[1]["probe"] is None and calls[2]["probe"] is None
    assert (calls[0]["beam_size"], calls[0]["patience"], calls[0]["length_penalty"]) == (5, 1.0, 1.0)
    assert [(k["seed"], k["best_of"]) for k in calls[1:]] == [(101, 3), (102, 3)]
    assert all(isinstance(r, DecodingResult) for r in out)
    assert [(r.ids, r.temperature, r.attempts, r.is_silence) for r in out] == [
        ([1], 0.0, 1, False), ([3], 0.4, 2, False), ([3], 0.4, 2, False), ([1], 0.0, 1, True), ([3], 0.4, 3, False)]
    assert [r.avg_logprob for r in out] == [-0.5, -0.8, -0.2, -1.5, -2.0]  # chunk 4: -2 at 0.4 and at 0.8, the earlier
    assert [r.sum_logprob for r in out] == [-1.0, -1.6, -0.4, -3.0, -4.0]
    assert [r.no_speech_prob for r in out] == pytest.approx([NO_SPEECH[b] for b in range(5)], abs=1e-7)
    assert out[0].compression_ratio == compression_ratio(TEXT[(1,)]) and out[1].compression_ratio == compression_ratio(TEXT[(3,)])


def test_fallback_thresholds_one_at_a_time():
    # no log-probability check: only the repetitive chunk goes on, and nothing is silence
    out, calls = _fallback(log_prob_threshold=None)
    assert [k["chunks"] for k in calls] == [[0, 1, 2, 3, 4], [2]]
    assert [(r.temperature, r.attempts, r.is_silence) for r in out] == [(0.0, 1, False)] * 2 + [(0.4, 2, False)] + [(0.0, 1, False)] * 2
    # no compression check (by the threshold, or for want of text_of): chunk 2 is final at 0
    for kw in (dict(compression_ratio_threshold=None), dict(text_of=None)):
        out, calls = _fallback(**kw)
        assert [k["chunks"] for k in calls] == [[0, 1, 2, 3, 4], [1, 4], [4]]
        assert out[2].temperature == 0.0 and out[2].attempts == 1
        assert (out[2].compression_ratio is None) == ("text_of" in kw)
    # the log-probability check alone, at another level
    out, calls = _fallback(compression_ratio_threshold=None, log_prob_threshold=-2.5, no_speech_threshold=None)
    assert [k["chunks"] for k in calls] == [[0, 1, 2, 3, 4], [4]] and out[4].temperature == 0.4 and out[4].attempts == 2
    # no silence exception (by the threshold, or for want of a token): chunk 3 goes on
    for kw in (dict(no_speech_threshold=None), dict(no_speech_token=None)):
        out, calls = _fallback(**kw)
        assert [k["chunks"] for k in calls] == [[0, 1, 2, 3, 4], [1, 2, 3, 4], [4]]
        assert (out[3].temperature, out[3].attempts, out[3].is_silence) == (0.4, 2, False)
        assert (out[3].no_speech_prob is None) == ("no_speech_token" in kw)
    # beam_size 1: the first pass is sample at temperature 0 with one candidate and the seed itself
    out, calls = _fallback(beam_size=1)
    assert (calls[0]["kind"], calls[0]["T"], calls[0]["best_of"], calls[0]["seed"], calls[0]["probe"]) == ("sample", 0.0, 1, 100, (1, 6))
    # a single temperature: everything is final after it, by the threshold or as the best attempt
    out, calls = _fallback(temperatures=[0.0])
    assert len(calls) == 1 and [r.attempts for r in out] == [1] * 5 and [r.temperature for r in out] == [0.0] * 5


def test_fallback_end_to_end(decoders):
    """The smallest geometry on the host route: the threshold lies between the first pass's average
    log-probabilities, so some chunks are final at temperature 0 and the others are decoded again."""
    c = case(*GEOMETRIES[0])
    dec = decoders(GEOMETRIES[0])
    eot, kw = c.V // 3, dict(max_length=len(PROMPT) + N_STEPS)
    first = dec.beam_search(c.enc, PROMPT, eot, **kw)
    avg = sorted(hs[0].score for hs in first)
    assert avg[0] < avg[-1]
    gap = max(range(len(avg) - 1), key=lambda i: avg[i + 1] - avg[i])
    threshold = (avg[gap] + avg[gap + 1]) / 2
    out = dec.decode_with_fallback(c.enc, PROMPT, eot, temperatures=(0.0, 0.7, 1.0), log_prob_threshold=threshold,
                                   no_speech_token=4, sot_index=1, seed=11, best_of=3, **kw)
    print(f"first pass {[hs[0].score for hs in first]}, threshold {threshold:.4f}: "
          f"{[(r.temperature, r.attempts, round(r.avg_logprob, 4)) for r in out]}")
    passed = [b for b in range(c.B) if first[b][0].score >= threshold]
    failed = [b for b in range(c.B) if b not in passed]
    assert passed and failed
    for b in passed:
        assert (out[b].ids, out[b].sum_logprob, out[b].temperature, out[b].attempts) == (first[b][0].ids, first[b][0].sum_logprob, 0.0, 1)
        assert out[b].avg_logprob == first[b][0].score
    # the second pass is sample on the pending chunks, in order, with seed + 1
    second = dec.sample(c.enc[failed], PROMPT, eot, temperature=0.7, best_of=3, seed=12, **kw)
    for j, b in enumerate(failed):
        assert out[b].attempts >= 2 and not out[b].is_silence
        if second[j][0].score >= threshold:
            assert (out[b].ids, out[b].temperature, out[b].attempts) == (second[j][0].ids, 0.7, 2)
        else:
            assert out[b].attempts == 3 and out[b].avg_logprob >= max(first[b][0].score, second[j][0].score)
    # the no-speech probability: softmax of the logits after prompt[:2], within 2 x the logits' bound of fp64
    ids = torch.tensor([PROMPT[:2]] * c.B)
    y64 = hf_logits(c.model64, c.enc64, ids)[:, -1]
    ref_err = float((hf_logits(c.model, c.enc, ids)[:, -1].double() - y64).abs().max())
    want = torch.softmax(y64, -1)[:, 4]
    for b in range(c.B):
        assert abs(out[b].no_speech_prob - float(want[b])) <= 8 * ref_err
    # ... and through prefill, fed in two pieces around sot_index
    pre = dec.decode_with_fallback(c.enc, PROMPT, eot, temperatures=(0.0,), no_speech_token=4, sot_index=1, prefill=True, **kw)
    for b in range(c.B):
        assert abs(pre[b].no_speech_prob - float(want[b])) <= 8 * ref_err
    assert [r.ids for r in pre] == [hs[0].ids for hs in dec.beam_search(c.enc, PROMPT, eot, prefill=True, **kw)]


# ----------------------------------------------------------------------------------- refusals
def test_refusals(decoders):
    c = case(*GEOMETRIES[0])
    dec = decoders(GEOMETRIES[0])
    for best_of in (0, 9, -1):
        with pytest.raises(ValueError, match="best_of"):
            dec.sample(c.enc, PROMPT, 5, temperature=0.5, best_of=best_of)
    with pytest.raises(ValueError, match="best_of must be 1"):
        dec.sample(c.enc, PROMPT, 5, temperature=0.0, best_of=2)
    for t in (-0.1, math.inf, math.nan):
        with pytest.raises(ValueError, match="temperature"):
            dec.sample(c.enc, PROMPT, 5, temperature=t)
        with pytest.raises(ValueError, match="temperatures"):
            dec.decode_with_fallback(c.enc, PROMPT, 5, temperatures=(0.0, t))
    with pytest.raises(ValueError, match="temperatures is empty"):
        dec.decode_with_fallback(c.enc, PROMPT, 5, temperatures=())
    for i in (-1, len(PROMPT)):
        with pytest.raises(ValueError, match="sot_index"):
            dec.decode_with_fallback(c.enc, PROMPT, 5, sot_index=i)
    with pytest.raises(ValueError, match="no_speech_token"):
        dec.decode_with_fallback(c.enc, PROMPT, 5, no_speech_token=c.V)
    with pytest.raises(ValueError, match="prompt is empty"):
        dec.sample(c.enc, [], 5)
    with pytest.raises(ValueError, match="eot"):
        dec.sample(c.enc, PROMPT, c.V)
    with pytest.raises(ValueError, match="seed"):
        dec.sample(c.enc, PROMPT, 5, seed=-1)
    with pytest.raises(ValueError, match="graph=True"):
        dec.sample(c.enc, PROMPT, 5, graph=True)

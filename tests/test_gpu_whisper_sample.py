"""WhisperDecoder.sample and decode_with_fallback on the HIP route: every selection is one
wx_sample_token launch.  The conditions are those of the host route (sample_helpers.check_sample:
the definition on the decoder's own teacher-forced logits, the sums against transformers' fp64, the
order, temperature 0 equal to generate), then graph=True against graph=False exactly, and the
fallback's decisions against the host route's."""
import pytest
import torch

from sample_helpers import check_sample, path_error
from whisper_decoder_helpers import GEOMETRIES, PROMPT, case

pytestmark = pytest.mark.gpu

N_STEPS = 10


def _device(c, dtype=torch.float32):
    from whisperx_amd import WhisperDecoder

    return WhisperDecoder(c.model, device="cuda", dtype=dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_sample_is_the_definition_on_the_decoders_logits(geometry, dtype):
    c = case(*geometry)
    dec = _device(c, dtype)
    check_sample(c, dec, "hip", 0.6, 3, seed=4, n_steps=N_STEPS)
    hyps = check_sample(c, dec, "hip", 1.0, 5, seed=9, n_steps=N_STEPS, eot=c.V // 3)
    assert min(len(h.ids) for hs in hyps for h in hs) < N_STEPS
    check_sample(c, dec, "hip masks", 1.0, 4, seed=2, n_steps=N_STEPS, suppress=[3, 17, 40], suppress_at_start=[5, 60])
    greedy = check_sample(c, dec, "hip", 0.0, 1, seed=0, n_steps=N_STEPS)
    assert [hs[0].ids for hs in greedy] == dec.generate(c.enc, PROMPT, c.V - 1, max_length=len(PROMPT) + N_STEPS)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_graph_equals_direct_exactly(geometry, dtype):
    """ids equal and sums bit for bit (the same kernel on the same logits), whatever sync_every is
    and although steps are taken after every row finished; a second sample of the same shape
    captures no step graph, and another temperature or seed only another selection graph."""
    c = case(*geometry)
    dec = _device(c, dtype)
    kw = dict(max_length=len(PROMPT) + N_STEPS, suppress_tokens=[3, 17], suppress_at_start=[5])
    for T, G, seed, eot in ((0.6, 3, 4, c.V - 1), (1.0, 5, 9, c.V // 3), (0.0, 1, 0, c.V // 3)):
        direct = dec.sample(c.enc, PROMPT, eot, temperature=T, best_of=G, seed=seed, **kw)
        for sync_every in (1, 8):
            graphed = dec.sample(c.enc, PROMPT, eot, temperature=T, best_of=G, seed=seed, graph=True, sync_every=sync_every, **kw)
            assert graphed == direct, (T, G, sync_every)
    before = dec.graph_captures
    assert before == 3  # one per (B, best_of, P); the decoder keeps the last two plans
    dec.sample(c.enc, PROMPT, c.V // 3, temperature=1.0, best_of=5, seed=9, graph=True, **kw)
    dec.sample(c.enc, PROMPT, c.V - 1, temperature=0.9, best_of=5, seed=5, graph=True, **kw)
    assert dec.graph_captures == before
    # the plans are generate's and beam_search's too
    assert dec.generate(c.enc, PROMPT, c.V // 3, graph=True, **kw) == dec.generate(c.enc, PROMPT, c.V // 3, **kw)
    assert dec.graph_captures == before


def test_prefill_and_the_step_route_agree_in_structure():
    c = case(*GEOMETRIES[0])
    dec = _device(c)
    kw = dict(temperature=0.8, best_of=4, seed=6, max_length=len(PROMPT) + N_STEPS, prefill=True)
    direct = dec.sample(c.enc, PROMPT, c.V // 3, **kw)
    assert dec.sample(c.enc, PROMPT, c.V // 3, graph=True, **kw) == direct
    assert [len(hs) for hs in direct] == [4] * c.B


def test_fallback_decides_as_the_host_route_does():
    """decode_with_fallback on the HIP route returns the host route's temperature and attempts per
    chunk.  The threshold lies between the host route's first-pass averages with more than
    8 ref_err on both sides (a sum of n log-probabilities moves by at most 8 n ref_err, its average
    by 8 ref_err), and the host's second-pass averages keep that distance from it too: chosen and
    asserted on the CPU before the GPU is asked."""
    from whisperx_amd import WhisperDecoder

    c = case(*GEOMETRIES[0])
    host = WhisperDecoder(c.model, device="cpu")
    eot, kw = c.V // 3, dict(max_length=len(PROMPT) + N_STEPS)
    first = host.beam_search(c.enc, PROMPT, eot, **kw)
    avg = sorted(hs[0].score for hs in first)
    gap = max(range(len(avg) - 1), key=lambda i: avg[i + 1] - avg[i])
    threshold = (avg[gap] + avg[gap + 1]) / 2
    ref_err = max(path_error(c, torch.float32, b, (PROMPT + hs[0].ids + [eot])[:len(PROMPT) + N_STEPS - 1])[1]
                  for b, hs in enumerate(first))
    failed = [b for b in range(c.B) if first[b][0].score < threshold]
    second = host.sample(c.enc[failed], PROMPT, eot, temperature=0.7, best_of=3, seed=12, **kw)
    near = min([abs(a - threshold) for a in avg] + [abs(hs[0].score - threshold) for hs in second]
               + [abs(hs[0].score - first[b][0].score) for b, hs in zip(failed, second)])
    print(f"threshold {threshold:.4f}, nearest average {near:.3e} away, 8 ref_err {8 * ref_err:.3e}")
    assert failed and len(failed) < c.B and near > 8 * ref_err
    args = dict(temperatures=(0.0, 0.7), log_prob_threshold=threshold, no_speech_token=4, sot_index=1, seed=11, best_of=3, **kw)
    want = host.decode_with_fallback(c.enc, PROMPT, eot, **args)
    dec = _device(c)
    for extra in ({}, dict(graph=True)):
        got = dec.decode_with_fallback(c.enc, PROMPT, eot, **args, **extra)
        assert [(r.temperature, r.attempts, r.is_silence) for r in got] == [(r.temperature, r.attempts, r.is_silence) for r in want]
        for g, w in zip(got, want):
            # (each route is within 8 ref_err of fp64, so within 16 ref_err of the other)
            assert abs(g.avg_logprob - w.avg_logprob) <= 16 * ref_err and abs(g.no_speech_prob - w.no_speech_prob) <= 16 * ref_err

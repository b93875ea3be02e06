"""WhisperDecoder.beam_search on the host route against the fp64 beam search of beam_helpers (its
rule: the oracle's decisive margin is at least 8 x sum_err, then equal ids for every hypothesis in
order and sums and scores within 4 x sum_err), the keywords of generate, start(beams=G), reorder
and the argument checks.  CPU only."""
import pytest
import torch

from beam_helpers import EOT, N_STEPS, check_beam_search, oracle
from whisper_decoder_helpers import GEOMETRIES, PROMPT, case


def _host(c):
    from whisperx_amd import WhisperDecoder

    return WhisperDecoder(c.model, device="cpu")


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_beam_search_equals_the_fp64_search(geometry):
    c = case(*geometry)
    got = check_beam_search(c, _host(c), "host", EOT[c.D])
    assert all(len(hs) == 5 for hs in got)
    lengths = {len(h.ids) for hs in got for h in hs}
    assert min(lengths) < N_STEPS  # the eot ends hypotheses early
    for hs in got:
        assert [h.score for h in hs] == sorted((h.score for h in hs), reverse=True)


def test_hypotheses_of_every_length_occur():
    lengths = set()
    for geometry in GEOMETRIES:
        want, _, _ = oracle(geometry, EOT[geometry[0]], 8)
        lengths |= {len(h[0]) for hs in want for h in hs}
    assert {0, 1, 2, 3, 12} <= lengths  # (0: an eot at the first step, D 512 at G = 8)


@pytest.mark.parametrize("G", [2, 8])
def test_other_beam_sizes(G):
    c = case(*GEOMETRIES[2])
    got = check_beam_search(c, _host(c), "host", EOT[c.D], G=G)
    assert all(len(hs) == G for hs in got)
    if G == 8:
        assert any(h.ids == [] for hs in got for h in hs)  # the empty hypothesis: n = 1, score = sum
        assert all(h.score == h.sum_logprob for hs in got for h in hs if not h.ids)


def test_patience_keeps_the_search_going():
    c = case(*GEOMETRIES[0])
    dec = _host(c)
    got = check_beam_search(c, dec, "host", EOT[c.D], patience=2.0)
    plain = oracle(c.geometry, EOT[c.D])[0]
    # up to round(5 x 2) = 10 finished hypotheses per chunk: chunk 0 finds a sixth
    assert len(got[0]) > 5 and [len(hs) for hs in plain] == [5, 5, 5]


def test_length_penalty():
    c = case(*GEOMETRIES[1])
    dec = _host(c)
    flat = check_beam_search(c, dec, "host", EOT[c.D], length_penalty=0.0)
    mean = check_beam_search(c, dec, "host", EOT[c.D], length_penalty=1.0)
    assert all(h.score == h.sum_logprob for hs in flat for h in hs)
    for hs in mean:
        for h in hs:
            n = len(h.ids) + (len(h.ids) < N_STEPS)  # (here every hypothesis shorter than the limit ended on eot)
            assert h.score == h.sum_logprob / n
    # the same hypotheses in another order: by sum chunk 0's 12-id hypothesis is last, by mean second
    assert sorted(h.ids for h in flat[0]) == sorted(h.ids for h in mean[0])
    assert [len(h.ids) for h in flat[0]] == [1, 1, 1, 1, 12] and [len(h.ids) for h in mean[0]] == [1, 12, 1, 1, 1]


def test_suppression():
    c = case(*GEOMETRIES[0])
    dec = _host(c)
    plain = oracle(c.geometry, EOT[c.D])[0]
    tok = plain[2][0][0][1]  # the second id of chunk 2's best hypothesis
    got = check_beam_search(c, dec, "host", EOT[c.D], suppress=[tok])
    assert all(tok not in h.ids for hs in got for h in hs)
    first = sorted({h[0][0] for hs in plain for h in hs if h[0]})
    got = check_beam_search(c, dec, "host", EOT[c.D], suppress_at_start=first)
    assert all(h.ids[0] not in first for hs in got for h in hs if h.ids)


def test_length_limit_fills_the_list_with_live_beams():
    c = case(*GEOMETRIES[1])
    got = check_beam_search(c, _host(c), "host", EOT[c.D], n_steps=4)
    assert all(len(hs) == 5 for hs in got)
    assert all(len(h.ids) == 4 for h in got[1])  # chunk 1 finds no eot in 4 steps: its five live beams
    assert [h.sum_logprob for h in got[1]] == sorted((h.sum_logprob for h in got[1]), reverse=True)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_one_beam_is_greedy_and_generate_takes_the_best(geometry):
    c = case(*geometry)
    dec = _host(c)
    eot = EOT[c.D]
    kw = dict(max_length=len(PROMPT) + N_STEPS)
    greedy = dec.generate(c.enc, PROMPT, eot, **kw)
    assert [hs[0].ids for hs in dec.beam_search(c.enc, PROMPT, eot, beam_size=1, **kw)] == greedy
    assert dec.generate(c.enc, PROMPT, eot, beam_size=1, patience=2.0, length_penalty=0.0, **kw) == greedy
    beams = dec.beam_search(c.enc, PROMPT, eot, **kw)
    assert dec.generate(c.enc, PROMPT, eot, beam_size=5, **kw) == [hs[0].ids for hs in beams]
    assert dec.generate(c.enc, PROMPT, eot, beam_size=5, length_penalty=0.0, **kw) == \
        [hs[0].ids for hs in dec.beam_search(c.enc, PROMPT, eot, length_penalty=0.0, **kw)]


def test_beam_state_shares_the_cross_attention_tensors():
    c = case(*GEOMETRIES[0])
    D, layers, P, V, T, B = c.geometry
    dec = _host(c)
    st = dec.start(c.enc, beams=5)
    assert (st.B, st.G, st.rows) == (B, 5, 5 * B)
    assert len(st.cross) == layers and all(tuple(x.shape) == (B, P, 2 * D) for x in st.cross)
    assert all(tuple(x.shape) == (5 * B, D // 64, T, 64) for x in (*st.self_k, *st.self_v))
    # every beam of a chunk computes what a single sequence does
    one = dec.start(c.enc)
    assert (one.G, one.rows) == (1, B)
    for t in PROMPT:
        lg = dec.step(st, torch.full((5 * B,), t))
        want = dec.step(one, torch.full((B,), t))
    assert tuple(lg.shape) == (5 * B, V)
    assert float((lg.view(B, 5, V) - want[:, None]).abs().max()) <= 1e-4


def test_reorder():
    c = case(*GEOMETRIES[2])
    B, G = c.B, 3
    dec = _host(c)
    st = dec.start(c.enc, beams=G)
    g = torch.Generator().manual_seed(3)
    for _ in range(4):
        dec.step(st, torch.randint(0, c.V, (B * G,), generator=g))
    stages = st.stages
    before = [x.clone() for x in (*st.self_k, *st.self_v)]
    ptrs = [x.data_ptr() for x in (*st.self_k, *st.self_v)]
    dec.reorder(st, torch.arange(B * G))
    assert all(torch.equal(x, y) for x, y in zip((*st.self_k, *st.self_v), before))
    parents = torch.tensor([2, 0, 0, 4, 5, 3])  # a permutation with a repeat, within and across chunks' rows
    dec.reorder(st, parents)
    for x, y in zip((*st.self_k, *st.self_v), before):
        assert torch.equal(x[:, :, :4], y[parents][:, :, :4])
        assert torch.equal(x[:, :, 4:], y[:, :, 4:])  # positions >= pos stay
    assert st.stages is stages and [x.data_ptr() for x in (*st.self_k, *st.self_v)] == ptrs
    # the state goes on from the reordered caches: row 1 and row 2 now continue the same history
    lg = dec.step(st, torch.tensor([7, 9, 9, 1, 2, 3]))
    assert torch.equal(lg[1], lg[2])
    with pytest.raises(ValueError):
        dec.reorder(st, torch.arange(B * G - 1))
    with pytest.raises(ValueError):
        dec.reorder(st, torch.tensor([0, 1, 2, 3, 4, B * G]))


def test_argument_checks():
    c = case(*GEOMETRIES[0])
    dec = _host(c)
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            dec.beam_search(c.enc, PROMPT, 49, beam_size=bad)
        with pytest.raises(ValueError):
            dec.generate(c.enc, PROMPT, 49, beam_size=bad)
        with pytest.raises(ValueError):
            dec.start(c.enc, beams=bad)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            dec.beam_search(c.enc, PROMPT, 49, patience=bad)
    st = dec.start(c.enc, beams=5)
    with pytest.raises(ValueError):
        dec.step(st, torch.zeros(c.B, dtype=torch.int64))
    assert tuple(dec.step(st, torch.zeros(5 * c.B, dtype=torch.int64)).shape) == (5 * c.B, c.V)

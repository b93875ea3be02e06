"""WhisperDecoder's graph-replayed step on the GPU (start / generate / beam_search / logits with
graph=True), under the rules of the tests of the direct route: the helpers of
whisper_decoder_helpers, whisper_decoder_half_helpers and beam_helpers see the decoder through a
thin adaptor that passes graph=True.  The replayed step is expected to give the direct step's bits
(the attention is bit-identical by construction and the GEMM calls are the same); the figure is
printed, the assertions are the oracles' bounds."""
import pytest
import torch

import whisper_decoder_half_helpers as hh
from beam_helpers import EOT, N_STEPS, check_beam_search
from whisper_decoder_helpers import (GEOMETRIES, N_FORCED, N_GREEDY, PROMPT, case, check_forced_logits, check_greedy,
                                     check_stopping, check_suppression, make_states)

pytestmark = pytest.mark.gpu


class Graphed:
    """The decoder as the helpers call it, every decoding call with graph=True (and `kw`)."""

    def __init__(self, dec, **kw):
        self.dec, self.kw = dec, kw
        self.dtype = dec.dtype

    def logits(self, *a, **k):
        return self.dec.logits(*a, graph=True, **k)

    def generate(self, *a, **k):
        return self.dec.generate(*a, graph=True, **self.kw, **k)

    def beam_search(self, *a, **k):
        return self.dec.beam_search(*a, graph=True, **k)


def _device(c, dtype=torch.float32):
    from whisperx_amd import WhisperDecoder

    return WhisperDecoder(c.model, device="cuda", dtype=dtype)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_teacher_forced_logits_against_the_oracle(geometry):
    c = case(*geometry)
    dec = _device(c)
    got = check_forced_logits(c, Graphed(dec), "graph")
    assert dec.graph_captures == 1
    eager = dec.logits(c.enc, c.forced()[0])
    print(f"graph {geometry}: max |graph - eager| {float((got - eager).abs().max()):.3e}")


@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_teacher_forced_logits_half(geometry, dtype):
    c = case(*geometry)
    dec = _device(c, dtype)
    got = hh.check_forced_logits(c, Graphed(dec), "graph")
    eager = dec.logits(c.enc, c.forced()[0])
    print(f"graph {hh.name(dtype)} {geometry}: max |graph - eager| {float((got - eager).abs().max()):.3e}")


@pytest.mark.parametrize("dtype", [torch.float32, *hh.DTYPES], ids=["f32", *map(hh.name, hh.DTYPES)])
@pytest.mark.parametrize("beams", [1, 3])
def test_twin_states_step_by_step(beams, dtype):
    """A replayed and a direct state fed the same ids: the difference per step is printed (0 is
    expected); asserted is the oracle's bound on both (fp32, one beam per chunk's rows), and that
    the replayed state keeps its host and device positions together and returns its one buffer."""
    c = case(*GEOMETRIES[0])
    dec = _device(c, dtype)
    ids, y64, ref_err = c.forced()
    a, b = dec.start(c.enc, beams=beams, graph=True), dec.start(c.enc, beams=beams)
    assert a.graph is not None and b.graph is None and a.kernels
    diffs, first = [], None
    for i in range(N_FORCED):
        tok = ids[:, i].repeat_interleave(beams)
        x, y = dec.step(a, tok), dec.step(b, tok)
        first = x if first is None else first
        assert x.data_ptr() == first.data_ptr() and x.dtype == torch.float32 and tuple(x.shape) == (c.B * beams, c.V)
        assert a.pos == b.pos == i + 1 == int(a.graph.pos_dev)
        diffs.append(float((x - y).abs().max()))
        if dtype == torch.float32:
            for got in (x, y):
                assert float((got[::beams].cpu().double() - y64[:, i]).abs().max()) <= 4 * ref_err, i
    print(f"twin states {hh.name(dtype) if dtype != torch.float32 else 'f32'} beams {beams}: max |graph - eager| per step {diffs}")
    assert dec.graph_captures == 1
    for x, y in zip((*a.self_k, *a.self_v), (*b.self_k, *b.self_v)):  # the fused append wrote what copy_ writes
        assert torch.equal(x[:, :, :N_FORCED].view(torch.int16), y[:, :, :N_FORCED].view(torch.int16))


@pytest.mark.parametrize("sync_every", [1, 8])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_greedy_generate_equals_the_fp64_loop(geometry, sync_every):
    c = case(*geometry)
    check_greedy(c, Graphed(_device(c), sync_every=sync_every), "graph")


@pytest.mark.parametrize("sync_every", [1, 8])
def test_stopping_and_suppression(sync_every):
    """check_stopping: row 0 stops within 4 tokens while the others run on, so with sync_every = 8
    steps are taken after rows finished: no row may grow from them."""
    c = case(*GEOMETRIES[0])
    dec = Graphed(_device(c), sync_every=sync_every)
    check_stopping(c, dec)
    check_suppression(c, dec, "graph")
    # every row done well before a multiple of sync_every: the extra steps are discarded
    want, _, _, _ = c.greedy()
    eot = int(want[0, 1])
    eager = dec.dec.generate(c.enc, PROMPT, eot, max_length=len(PROMPT) + N_GREEDY)
    assert dec.generate(c.enc, PROMPT, eot, max_length=len(PROMPT) + N_GREEDY) == eager
    assert all(eot not in row for row in eager)


@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
def test_half_greedy_on_its_own_path(dtype):
    c = case(*GEOMETRIES[0])
    hh.check_stopping_and_suppression(c, Graphed(_device(c, dtype), sync_every=8), "graph")


@pytest.mark.parametrize("sync_every", [1, 8, 5])
def test_the_position_never_passes_the_table(sync_every):
    """max_length = max_target_positions and an eot that comes late or never: the output equals the
    direct route's, and no replay runs at a position >= the table's length (the host mirror and the
    device position are read after every replay)."""
    c = case(*GEOMETRIES[0])
    dec = _device(c)
    T = dec.max_target_positions
    seen = []
    step = dec._graph_step

    def spy(st, tok):
        before = (st.pos, int(st.graph.pos_dev))
        out = step(st, tok)
        seen.append((before, (st.pos, int(st.graph.pos_dev))))
        return out

    dec._graph_step = spy
    for eot in (95, 13):
        eager = dec.generate(c.enc, PROMPT, eot, max_length=T)
        assert dec.generate(c.enc, PROMPT, eot, max_length=T, graph=True, sync_every=sync_every) == eager
        assert dec.generate(c.enc, PROMPT, eot, max_length=T + 100, graph=True, sync_every=sync_every) == eager
    assert seen and all(b[0] == b[1] < T - 1 and a == (b[0] + 1, b[0] + 1) for b, a in seen)
    assert max(a[0] for _, a in seen) == T - 1  # the limit was reached: eot 95 is never emitted
    # a prompt that fills the limit: nothing is generated, nothing replayed
    n = len(seen)
    assert dec.generate(c.enc, PROMPT, 95, max_length=len(PROMPT), graph=True) == [[] for _ in range(c.B)]
    assert len(seen) == n
    st = dec.start(c.enc, graph=True)
    for _ in range(T):
        dec.step(st, torch.zeros(c.B, dtype=torch.int64))
    with pytest.raises(ValueError, match="max_target_positions"):
        dec.step(st, torch.zeros(c.B, dtype=torch.int64))
    assert st.pos == T == int(st.graph.pos_dev)


@pytest.mark.parametrize("G", [2, 5])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_beam_search_equals_the_fp64_search(geometry, G):
    c = case(*geometry)
    dec = _device(c)
    got = check_beam_search(c, dec, "graph", EOT[c.D], G=G, graph=True)
    eager = dec.beam_search(c.enc, PROMPT, EOT[c.D], beam_size=G, max_length=len(PROMPT) + N_STEPS)
    assert [[h.ids for h in hs] for hs in got] == [[h.ids for h in hs] for hs in eager]
    print(f"graph beams {G}: max |sum - eager sum| "
          f"{max(abs(x.sum_logprob - y.sum_logprob) for hx, hy in zip(got, eager) for x, y in zip(hx, hy)):.3e}")
    assert dec.graph_captures == 1
    kw = dict(beam_size=G, max_length=len(PROMPT) + N_STEPS)
    assert dec.generate(c.enc, PROMPT, EOT[c.D], graph=True, **kw) == [hs[0].ids for hs in got]
    assert dec.graph_captures == 1  # the plan of (B, G, P) again


@pytest.mark.parametrize("dtype", hh.DTYPES, ids=hh.name)
def test_half_beam_search(dtype):
    c = case(*GEOMETRIES[0])
    hh.check_beam_search(c, Graphed(_device(c, dtype)), "graph")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_prefill_then_replays(dtype):
    c = case(*GEOMETRIES[0])
    dec = _device(c, dtype)
    kw = dict(max_length=len(PROMPT) + N_GREEDY, prefill=True)
    for eot in (95, int(c.greedy()[0][0, 4])):
        eager = dec.generate(c.enc, PROMPT, eot, **kw)
        for sync_every in (1, 8):
            assert dec.generate(c.enc, PROMPT, eot, graph=True, sync_every=sync_every, **kw) == eager
        hyps = dec.beam_search(c.enc, PROMPT, eot, beam_size=3, **kw)
        got = dec.beam_search(c.enc, PROMPT, eot, beam_size=3, graph=True, **kw)
        assert [[h.ids for h in hs] for hs in got] == [[h.ids for h in hs] for hs in hyps]
    st = dec.start(c.enc, graph=True)
    dec.prefill(st, torch.tensor([PROMPT] * c.B))
    assert st.pos == len(PROMPT) == int(st.graph.pos_dev)


def test_plans_are_reused_and_leak_nothing():
    D, _, P, _, _, B = GEOMETRIES[0]
    c = case(*GEOMETRIES[0])
    dec = _device(c)
    other = make_states(B, P, D, seed=77)
    kw = dict(max_length=len(PROMPT) + N_GREEDY)
    want = [dec.generate(e, PROMPT, 95, **kw) for e in (c.enc, other)]
    assert want[0] != want[1] and dec.graph_captures == 0
    assert dec.generate(c.enc, PROMPT, 95, graph=True, **kw) == want[0]
    assert dec.graph_captures == 1
    plan = next(iter(dec._plans.values()))
    # the second call starts on the first call's caches and cross tensors, refilled and not cleared
    assert dec.generate(other, PROMPT, 95, graph=True, **kw) == want[1]
    assert dec.generate(c.enc, PROMPT, 95, graph=True, sync_every=1, **kw) == want[0]
    assert dec.graph_captures == 1 and list(dec._plans.values()) == [plan]
    dec.logits(other, [PROMPT] * B, graph=True)
    assert dec.graph_captures == 1
    # another B captures once more; a third shape drops the least recently used plan
    assert dec.generate(other[:2], PROMPT, 95, graph=True, **kw) == dec.generate(other[:2], PROMPT, 95, **kw)
    assert dec.graph_captures == 2 and list(dec._plans) == [(B, 1, P), (2, 1, P)]
    assert dec.generate(c.enc[:1], PROMPT, 95, graph=True, **kw) == dec.generate(c.enc[:1], PROMPT, 95, **kw)
    assert dec.graph_captures == 3 and list(dec._plans) == [(2, 1, P), (1, 1, P)]
    # a plan bound to a live state is not handed out twice: another is built for the second state
    a = dec.start(c.enc[:1], graph=True)
    b = dec.start(other[:1], graph=True)
    assert a.graph is not b.graph and a.graph is not None and dec._plans[(1, 1, P)] is b.graph
    tok = torch.tensor([PROMPT[0]])
    la, lb = dec.step(a, tok).clone(), dec.step(b, tok).clone()
    assert dec.graph_captures == 4  # a's plan was captured before, b's is new
    ea, eb = dec.step(dec.start(c.enc[:1]), tok), dec.step(dec.start(other[:1]), tok)
    dist = lambda x, y: float((x - y).abs().max())  # noqa: E731
    print(f"two live states: |a - eager a| {dist(la, ea):.3e}, |b - eager b| {dist(lb, eb):.3e}, |a - b| {dist(la, lb):.3e}")
    assert dist(la, ea) < dist(la, eb) and dist(lb, eb) < dist(lb, ea)  # each state's logits are its own
    del a, b
    dec.release_graphs()
    assert not dec._plans
    assert dec.generate(other, PROMPT, 95, graph=True, **kw) == want[1]
    assert dec.graph_captures == 5

"""Shared by the tests of WhisperDecoder's half route (float16 / bfloat16), on the host route and on
the kernel route: the oracle of whisper_decoder_helpers (a random transformers model, fp64 as the
reference) with another yardstick.

ref_err_half / ref_rms_half = the max / the RMS of |transformers' model deep-copied and cast to
dtype, on the CPU - its fp64 logits| on the same ids: what simply casting the stock model costs.
The half route rounds a subset of what the cast model rounds (not the residual stream, the norms,
the positional table or the softmax statistics), and must be within 2 x of both (the half encoder's
rule; the factor leaves room for the GEMM library's summation orders and for rounding flips).  A
CPU emulation of the route gave max ratios 0.33 .. 0.98 (fp16) and 0.35 .. 1.35 (bf16) and RMS
ratios 0.50 .. 0.87 and 0.57 .. 1.13 over four id seeds.

Token equality with the fp64 greedy loop cannot be required: the fp64 top-2 margins (2.2e-3 and up)
are below the half-precision error, and the cast model itself agrees on 21-24 of 24 and 23-34 of 36
tokens.  check_greedy states what is required instead."""
import copy
import functools
import math

import torch

from beam_helpers import EOT, N_STEPS
from whisper_decoder_helpers import LANGUAGE_IDS, N_FORCED, N_GREEDY, PROMPT, SOT, case, hf_logits
from whisper_half_helpers import DTYPES, name

__all__ = ["DTYPES", "name"]


@functools.lru_cache(maxsize=None)
def cast_model(geometry, dtype):
    """The geometry's transformers model deep-copied and cast to dtype (CPU); shared, left unchanged."""
    return copy.deepcopy(case(*geometry).model).to(dtype)


@functools.lru_cache(maxsize=None)
def _path(geometry, dtype, rows, ids):
    c = case(*geometry)
    rows, t = list(rows), torch.tensor(ids)
    y64 = hf_logits(c.model64, c.enc64[rows], t)
    y16 = hf_logits(cast_model(geometry, dtype), c.enc[rows], t)
    assert y16.dtype == dtype
    d = y16.double() - y64
    return y64, float(d.abs().max()), float(d.pow(2).mean().sqrt())


def path_errors(c, dtype, ids, rows=None):
    """(fp64 logits [len(rows), n, V], ref_err_half, ref_rms_half) of teacher-forcing `ids` [len(rows), n]
    on the chunks `rows` (default: all); computed once per path and shared."""
    rows = tuple(range(c.B)) if rows is None else tuple(rows)
    ids = tuple(tuple(int(t) for t in row) for row in (ids.tolist() if torch.is_tensor(ids) else ids))
    return _path(c.geometry, dtype, rows, ids)


def within_the_rule(got: torch.Tensor, y64: torch.Tensor, ref_err: float, ref_rms: float, label: str):
    """max |got - fp64| <= 2 ref_err_half and its RMS <= 2 ref_rms_half; prints both ratios."""
    d = got.cpu().double() - y64
    err, rms = float(d.abs().max()), float(d.pow(2).mean().sqrt())
    print(f"{label}: |logits - fp64| max {err:.3e} = {err / ref_err:.2f} x ref_err_half {ref_err:.3e}, "
          f"RMS {rms:.3e} = {rms / ref_rms:.2f} x ref_rms_half {ref_rms:.3e}")
    assert ref_err > 0 and ref_rms > 0
    assert err <= 2 * ref_err and rms <= 2 * ref_rms


def check_forced_logits(c, dec, label: str) -> torch.Tensor:
    ids, _, _ = c.forced()
    y64, ref_err, ref_rms = path_errors(c, dec.dtype, ids)
    got = dec.logits(c.enc, ids)
    assert tuple(got.shape) == (c.B, N_FORCED, c.V) and got.dtype == torch.float32
    within_the_rule(got, y64, ref_err, ref_rms, f"{label} {name(dec.dtype)} {c.geometry} forced")
    return got


def _unused_eot(c, dec, kw) -> int:
    """An id that neither the fp64 loop nor this decoder's run emits, so that no row stops."""
    seen = set(c.greedy()[0].flatten().tolist())
    for eot in range(c.V - 1, -1, -1):
        if eot in seen or eot in kw.get("suppress_tokens", ()) or eot in kw.get("suppress_at_start", ()):
            continue
        got = dec.generate(c.enc, PROMPT, eot, max_length=len(PROMPT) + N_GREEDY, **kw)
        if all(len(row) == N_GREEDY for row in got):
            return eot
    raise AssertionError("every id is emitted")


def check_greedy(c, dec, label: str, eot=None, suppress=(), suppress_at_start=()) -> list:
    """generate on the decoder's own path.  With F what the decoder was fed (the prompt and its own
    tokens), on every generated step of every row, none skipped:
      (a) the token is the argmax of dec.logits teacher-forced on F with the masks applied (the same
          batch: exactly);
      (b) those logits are within the 2 x rule of fp64 on F, ref_err_half taken on F;
      (c) fp64 logit[token] >= the fp64 maximum over the unmasked ids - 4 x ref_err_half(F): the token
          and the fp64 winner are each within 2 x ref_err_half of their fp64 logits.
    With `eot` the rows may stop (finished rows are fed eot and ignored)."""
    kw = {}
    if suppress:
        kw["suppress_tokens"] = list(suppress)
    if suppress_at_start:
        kw["suppress_at_start"] = list(suppress_at_start)
    if eot is None:
        eot = _unused_eot(c, dec, kw)
    got = dec.generate(c.enc, PROMPT, eot, max_length=len(PROMPT) + N_GREEDY, **kw)
    n = max(len(row) for row in got)
    n = min(N_GREEDY, n + 1)  # the steps the loop ran: a row that stopped emitted eot at step len(row)
    full = [row + [eot] * (n - len(row)) for row in got]
    fed = torch.tensor([PROMPT + row[:n - 1] for row in full])
    lg = dec.logits(c.enc, fed)[:, len(PROMPT) - 1:].cpu()  # [B, n, V]: step i's logits
    y64, ref_err, ref_rms = path_errors(c, dec.dtype, fed)
    y64 = y64[:, len(PROMPT) - 1:]
    within_the_rule(lg, y64, ref_err, ref_rms, f"{label} {name(dec.dtype)} {c.geometry} greedy path {kw}")  # (b)
    mask = torch.zeros((n, c.V), dtype=torch.bool)
    mask[:, list(suppress)] = True
    mask[0, list(suppress_at_start)] = True
    want = lg.masked_fill(mask, -math.inf).argmax(-1)
    m64 = y64.masked_fill(mask, -math.inf)
    checked = 0
    for b, row in enumerate(got):
        live = len(row) + (1 if len(row) < n else 0)  # the row's tokens and the eot that stopped it
        for i in range(live):
            tok = full[b][i]
            assert int(want[b, i]) == tok, (b, i)  # (a)
            assert not bool(mask[i, tok])
            assert float(m64[b, i, tok]) >= float(m64[b, i].max()) - 4 * ref_err, (b, i)  # (c)
            checked += 1
    assert checked >= c.B
    loop = c.greedy(N_GREEDY, tuple(suppress), tuple(suppress_at_start))[0].tolist()
    agree = sum(x == y for r, w in zip(got, loop) for x, y in zip(r, w))
    print(f"{label} {name(dec.dtype)} {c.geometry} {kw}: {agree} of {sum(len(r) for r in got)} tokens equal the fp64 "
          f"loop's, eot {eot}, {checked} steps checked")
    return got


def check_stopping_and_suppression(c, dec, label: str):
    """eot = a token the unsuppressed run emits: the second run is the first cut at every row's first
    eot.  A suppressed id never appears (and (a) - (c) hold under the mask); suppress_at_start moves
    position 0 only: (a) applies it to step 0 alone."""
    first = check_greedy(c, dec, label)
    eot = first[0][4]
    cut = [row[:row.index(eot)] if eot in row else row for row in first]
    got = check_greedy(c, dec, label, eot=eot)
    print(f"{label} stopping: eot {eot}, lengths {[len(r) for r in got]}")
    assert got == cut and len(got[0]) <= 4 and all(eot not in r for r in got)
    tok = first[1][2]
    got = check_greedy(c, dec, label, suppress=[tok])
    assert all(tok not in row for row in got) and got != first
    start = sorted({row[0] for row in first})
    got = check_greedy(c, dec, label, suppress_at_start=start)
    assert all(row[0] not in start for row in got)


def check_beam_search(c, dec, label: str, G: int = 5):
    """G beams, N_STEPS steps, beam_helpers.EOT.  Every hypothesis' sum_logprob is within
    4 n ref_err_half(path) of the fp64 teacher-forced sum of the log-probabilities of its own ids (and
    eot's when it ended), n the scored positions: a log-softmax moves by at most twice the largest
    logit error, the logits are within 2 x ref_err_half of fp64, so n of them move the sum by at most
    4 n ref_err_half.  score == sum / n ** length_penalty, the scores do not increase, every chunk
    has G hypotheses (beam_search's docstring at patience 1), and beam_size 1 is greedy decoding."""
    eot = EOT[c.D]
    kw = dict(max_length=len(PROMPT) + N_STEPS)
    hyps = dec.beam_search(c.enc, PROMPT, eot, beam_size=G, **kw)
    assert len(hyps) == c.B
    worst = 0.0
    for b, hs in enumerate(hyps):
        assert len(hs) == G
        assert all(x.score >= y.score for x, y in zip(hs, hs[1:]))
        for h in hs:
            assert len(h.ids) <= N_STEPS and eot not in h.ids
            ended = len(h.ids) < N_STEPS  # (a live beam ran to the limit: only a hypothesis that ended is shorter)
            n = len(h.ids) + 1 if ended else max(1, len(h.ids))
            assert h.score == h.sum_logprob / n ** 1.0
            scored = h.ids + [eot] if ended else h.ids
            seq = (PROMPT + scored)[:-1]
            y64, ref_err, _ = path_errors(c, dec.dtype, [seq], rows=[b])
            logp = torch.log_softmax(y64[0, len(PROMPT) - 1:], -1)
            want = float(sum(logp[i, t] for i, t in enumerate(scored)))
            bound = 4 * len(scored) * ref_err
            worst = max(worst, abs(h.sum_logprob - want) / bound)
            assert abs(h.sum_logprob - want) <= bound, (b, h)
    print(f"{label} {name(dec.dtype)} {c.geometry} beam search: |sum - fp64 sum of its ids| at most {worst:.3f} x "
          f"4 n ref_err_half; lengths {[[len(h.ids) for h in hs] for hs in hyps]}")
    greedy = dec.generate(c.enc, PROMPT, eot, **kw)
    assert [hs[0].ids for hs in dec.beam_search(c.enc, PROMPT, eot, beam_size=1, **kw)] == greedy
    assert dec.generate(c.enc, PROMPT, eot, beam_size=G, **kw) == [hs[0].ids for hs in hyps]


def check_reorder(c, dec):
    """reorder leaves dtype caches holding the parents' rows, bit-equal to index_select."""
    B, G = c.B, 3
    st = dec.start(c.enc, beams=G)
    g = torch.Generator().manual_seed(3)
    for _ in range(4):
        dec.step(st, torch.randint(0, c.V, (B * G,), generator=g))
    caches = (*st.self_k, *st.self_v)
    assert all(x.dtype == dec.dtype for x in caches)
    before = [x.clone() for x in caches]
    parents = torch.tensor([2, 0, 0, 4, 5, 3][:B * G])
    dec.reorder(st, parents)
    for x, y in zip(caches, before):
        assert x.dtype == dec.dtype
        assert torch.equal(x[:, :, :4].view(torch.int16), y.index_select(0, parents.to(y.device))[:, :, :4].view(torch.int16))
        assert torch.equal(x[:, :, 4:], y[:, :, 4:])
    lg = dec.step(st, torch.tensor([7, 9, 9, 1, 2, 3][:B * G]))  # the state goes on from the reordered caches
    assert lg.dtype == torch.float32 and bool(torch.isfinite(lg).all())


def check_detect_language(c, dec, label: str):
    ids = torch.full((c.B, 1), SOT)
    p64 = torch.softmax(hf_logits(c.model64, c.enc64, ids)[:, -1][:, LANGUAGE_IDS], -1)
    p16 = torch.softmax(hf_logits(cast_model(c.geometry, dec.dtype), c.enc, ids)[:, -1][:, LANGUAGE_IDS].double(), -1)
    ref_err = float((p16 - p64).abs().max())
    got = dec.detect_language(c.enc, SOT, LANGUAGE_IDS)
    assert tuple(got.shape) == (c.B, len(LANGUAGE_IDS)) and got.dtype == torch.float32
    err = float((got.cpu().double() - p64).abs().max())
    print(f"{label} {name(dec.dtype)} detect_language: |p - fp64| {err:.3e}, cast model {ref_err:.3e}, bound {2 * ref_err:.3e}")
    assert ref_err > 0 and err <= 2 * ref_err
    assert float((got.sum(-1) - 1).abs().max()) <= 1e-6


def check_state(c, dec):
    """What start() holds in dtype, and what step returns."""
    D, layers, P, V, T, B = c.geometry
    st = dec.start(c.enc, beams=2)
    assert len(st.cross) == layers and all(tuple(x.shape) == (B, P, 2 * D) and x.dtype == dec.dtype for x in st.cross)
    assert all(tuple(x.shape) == (2 * B, D // 64, T, 64) and x.dtype == dec.dtype for x in (*st.self_k, *st.self_v))
    lg = dec.step(st, torch.full((2 * B,), PROMPT[0]))
    assert lg.dtype == torch.float32 and tuple(lg.shape) == (2 * B, V)

"""Shared by the tests of WhisperDecoder's repetition_penalty / no_repeat_ngram_size on either route:
the decoder-level conditions, each against penalty_probes.definition (the numpy evaluation of
wx_penalize_logits' header) applied to the decoder's own teacher-forced logits.

What the unpenalised decoder does on these geometries was looked at once on the host route and is
asserted again by every check before it is used: 16 greedy ids of a row hold a repeated id and no
repeated bigram, so rho = 8 and n = 1 change the ids and n = 2 does not; with all but `k` ids
suppressed (eot too) 12 or more ids must repeat a bigram, and then n = 2 changes them.
"""
import functools

import numpy as np
import torch

from penalty_probes import definition
from sample_helpers import definition as select_definition
from sample_helpers import eps_tokens, path_error
from whisper_decoder_helpers import PROMPT, case

N_STEPS = 16


@functools.lru_cache(maxsize=None)
def host_decoder(geometry):
    from whisperx_amd import WhisperDecoder

    return WhisperDecoder(case(*geometry).model, device="cpu")


def repeats(ids, n: int) -> bool:
    """Whether `ids` holds the same n-gram twice."""
    grams = [tuple(ids[i:i + n]) for i in range(len(ids) - n + 1)]
    return len(set(grams)) < len(grams)


@functools.lru_cache(maxsize=None)
def all_but(geometry, k: int) -> tuple:
    """suppress_tokens that leave only k ids: the k lowest the host's unpenalised greedy rows emit
    (eot = V - 1 is none of them: those rows never end)."""
    c = case(*geometry)
    plain = host_decoder(geometry).generate(c.enc, PROMPT, c.V - 1, max_length=len(PROMPT) + N_STEPS)
    keep = sorted({t for row in plain for t in row})[:k]
    assert len(keep) == k and c.V - 1 not in keep
    return tuple(t for t in range(c.V) if t not in keep)


def _prefix(history_from):
    return [] if history_from is None else PROMPT[history_from:]


def _route(kw):
    return {k: v for k, v in kw.items() if k == "kernels"}


def check_host_case(geometry, n_repeat: int, suppress=(), **options):
    """The case is a case: on the host route the unpenalised greedy rows hold a repeated
    `n_repeat`-gram, and the penalised ids differ from them."""
    c, host = case(*geometry), host_decoder(geometry)
    kw = dict(max_length=len(PROMPT) + N_STEPS, suppress_tokens=list(suppress))
    plain = host.generate(c.enc, PROMPT, c.V - 1, **kw)
    assert all(repeats(row, n_repeat) for row in plain), plain
    assert host.generate(c.enc, PROMPT, c.V - 1, **kw, **options) != plain
    return plain


def check_defaults(c, dec, **kw):
    """rho = 1 and n = 0 given explicitly are the calls without them: ids, sums and scores."""
    off = dict(repetition_penalty=1.0, no_repeat_ngram_size=0)
    eot, args = c.V // 3, dict(max_length=len(PROMPT) + 10, suppress_tokens=[3, 17], suppress_at_start=[5], **kw)
    assert dec.generate(c.enc, PROMPT, eot, **args, **off) == dec.generate(c.enc, PROMPT, eot, **args)
    assert dec.generate(c.enc, PROMPT, eot, **args, history_from=0) == dec.generate(c.enc, PROMPT, eot, **args)
    assert dec.beam_search(c.enc, PROMPT, eot, **args, **off) == dec.beam_search(c.enc, PROMPT, eot, **args)
    for T, G in ((0.0, 1), (0.8, 3)):
        s = dict(temperature=T, best_of=G, seed=3)
        assert dec.sample(c.enc, PROMPT, eot, **s, **args, **off) == dec.sample(c.enc, PROMPT, eot, **s, **args)
    f = dict(temperatures=(0.0, 0.8), best_of=3, seed=3, log_prob_threshold=-1.5)
    assert dec.decode_with_fallback(c.enc, PROMPT, eot, **f, **args, **off) == dec.decode_with_fallback(c.enc, PROMPT, eot, **f, **args)


def greedy_definition(c, dec, rho, n, history_from=None, suppress=(), n_steps=N_STEPS, eot=None, **kw):
    """The greedy loop of the definition on the decoder's own logits: a state of the same shape fed
    the definition's ids (the calls generate makes, so the logits it read, bit for bit).  Per step
    the penalty, then the mask, then the argmax (the lowest id on ties); a row with no finite logit
    left ends.  Returns (the ids per row, how many rows ended for want of a finite logit)."""
    V, R = c.V, c.B
    eot = V - 1 if eot is None else eot
    prefix = _prefix(history_from)
    hist = np.zeros((R, len(prefix) + n_steps), dtype=np.int64)
    hist[:, :len(prefix)] = prefix
    st = dec.start(c.enc, **_route(kw))
    for t in PROMPT:
        lg = dec.step(st, torch.full((R,), t))
    done, rows, starved = np.zeros(R, dtype=bool), [[] for _ in range(R)], 0
    for step in range(n_steps):
        x = definition(lg.cpu().numpy(), V, hist, len(prefix) + step, rho, n)
        x[:, list(suppress)] = -np.inf
        dead = np.isneginf(x.max(1))
        starved += int((dead & ~done).sum())
        tok = np.where(done | dead, eot, x.argmax(1))
        for r in range(R):
            if not done[r] and tok[r] != eot:
                rows[r].append(int(tok[r]))
        hist[:, len(prefix) + step] = tok
        done = done | (tok == eot)
        if done.all() or step == n_steps - 1:
            break
        lg = dec.step(st, torch.from_numpy(tok))
    return rows, starved


def check_greedy(c, dec, label, rho, n, history_from=None, suppress=(), **kw):
    """generate with the options equals greedy_definition exactly: at temperature 0 the kernel is
    exact and the selection has one answer, so no selection is skipped.  Returns (ids, starved)."""
    want, starved = greedy_definition(c, dec, rho, n, history_from, suppress, **kw)
    got = dec.generate(c.enc, PROMPT, c.V - 1, max_length=len(PROMPT) + N_STEPS, suppress_tokens=list(suppress),
                       repetition_penalty=rho, no_repeat_ngram_size=n, history_from=history_from, **kw)
    print(f"{label} {c.geometry} rho {rho} n {n} history_from {history_from}: lengths {[len(r) for r in got]}, "
          f"{starved} rows ended with every logit at -inf")
    assert got == want
    if n:
        assert not any(repeats(_prefix(history_from) + row, n) for row in got)
    return got, starved


def penalised64(x: torch.Tensor, h: list, rho: float, n: int) -> torch.Tensor:
    """The definition on one row of fp64 logits (the penalty as the fp32 value the kernel is handed)."""
    x, rho = x.clone(), float(np.float32(rho))
    for t in set(h):
        x[t] = x[t] * rho if x[t] < 0 else x[t] / rho
    if n >= 1:
        for j in range(len(h) - n + 1):
            if h[j:j + n - 1] == h[len(h) - n + 1:]:
                x[h[j + n - 1]] = float("-inf")
    return x


def check_sampled(c, dec, label, temperature, best_of, seed, rho, n, history_from=None, n_steps=10, host=False, **kw):
    """sample_helpers.check_sample's conditions with the penalty applied to the step's logits (in
    fp32, by the numpy definition) before the selection's definition: the ids of every row whose
    selections all had a top-2 margin above eps_tokens of the penalised logits are the definition's,
    at most 1% of the selections lie below it, and a hypothesis' sum is within 8 n ref_err (4 n
    ref_err_half) of the fp64 sum of the penalised log-probabilities of its own ids."""
    G, V, eot = best_of, c.V, c.V - 1
    prefix = _prefix(history_from)
    options = dict(repetition_penalty=rho, no_repeat_ngram_size=n, history_from=history_from)
    hyps = dec.sample(c.enc, PROMPT, eot, temperature=temperature, best_of=G, seed=seed, max_length=len(PROMPT) + n_steps,
                      **options, **kw)
    assert len(hyps) == c.B and all(len(hs) == G for hs in hyps)
    for hs in hyps:
        assert all(x.score >= y.score for x, y in zip(hs, hs[1:]))
    R = c.B * G
    st = dec.start(c.enc, beams=G, **_route(kw))
    for t in PROMPT:
        lg = dec.step(st, torch.full((R,), t))
    hist = np.zeros((R, len(prefix) + n_steps), dtype=np.int64)
    hist[:, :len(prefix)] = prefix
    done, rows, risky = np.zeros(R, dtype=bool), [[] for _ in range(R)], np.zeros(R, dtype=bool)
    below = total = 0
    for step in range(n_steps):
        x = definition(lg.cpu().numpy(), V, hist, len(prefix) + step, rho, n)
        sel = select_definition(x, None, temperature, seed, step, done, eot)
        eps = 1e-9 if host else eps_tokens(float(np.abs(x[np.isfinite(x)]).max()), temperature)
        near = sel.scored & (sel.margin <= eps)
        risky |= near
        below, total = below + int(near.sum()), total + int(sel.scored.sum())
        for r in range(R):
            if not done[r] and sel.token[r] != eot:
                rows[r].append(int(sel.token[r]))
        hist[:, len(prefix) + step] = sel.token
        done = sel.done
        if done.all() or step == n_steps - 1:
            break
        lg = dec.step(st, torch.from_numpy(sel.token))
    print(f"{label} {c.geometry} T {temperature} best_of {G} rho {rho} n {n}: {below} of {total} selections within eps")
    assert below <= 0.01 * total
    for b, hs in enumerate(hyps):
        left = [h.ids for h in hs]
        for r in range(b * G, (b + 1) * G):
            if not risky[r]:
                assert rows[r] in left, (b, r, rows[r], left)
                left.remove(rows[r])
    factor, worst = (8 if dec.dtype == torch.float32 else 4), 0.0
    for b, hs in enumerate(hyps):
        for h in hs:
            assert eot not in h.ids and (not n or not repeats(prefix + h.ids, n))
            scored = h.ids + [eot] if len(h.ids) < n_steps else h.ids
            y64, ref_err = path_error(c, dec.dtype, b, (PROMPT + scored)[:-1])
            want = 0.0
            for i, t in enumerate(scored):
                row = penalised64(y64[0, len(PROMPT) - 1 + i], prefix + scored[:i], rho, n)
                want += float(torch.log_softmax(row, -1)[t])
            assert h.score == h.sum_logprob / len(scored)
            bound = factor * len(scored) * ref_err
            worst = max(worst, abs(h.sum_logprob - want) / bound)
            assert abs(h.sum_logprob - want) <= bound, (b, h, want)
    print(f"{label}: |sum - fp64 sum of its ids' penalised log-probabilities| at most {worst:.3f} x {factor} n ref_err")
    return hyps


def check_beam(c, dec, n, suppress=(), **kw):
    """beam_search at G = 5: unpenalised, some hypothesis repeats an n-gram; with
    no_repeat_ngram_size = n none does, which needs every beam's history to follow its parents."""
    args = dict(beam_size=5, max_length=len(PROMPT) + N_STEPS, suppress_tokens=list(suppress), **kw)
    plain = dec.beam_search(c.enc, PROMPT, c.V - 1, **args)
    assert all(any(repeats(h.ids, n) for h in hs) for hs in plain)
    hyps = dec.beam_search(c.enc, PROMPT, c.V - 1, no_repeat_ngram_size=n, **args)
    assert all(len(hs) == 5 for hs in hyps)
    for hs in hyps:
        for h in hs:
            assert np.isfinite(h.sum_logprob) and len(h.ids) == N_STEPS and not repeats(h.ids, n), h
    return hyps

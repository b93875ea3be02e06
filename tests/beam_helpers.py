"""Shared by the beam-search tests: a plain-Python beam search over the transformers oracle of
whisper_decoder_helpers (no cache, no top-k trick: every step lists all G V candidates of a chunk
and sorts them), written from WhisperDecoder.beam_search's docstring.

`oracle(geometry, eot, G, ...)` runs it in fp64 and returns the hypotheses per chunk, the search's
**decisive margin** and `sum_err`:

  margin   the smallest of (a) per step and chunk, the gap between the G-th chosen live candidate
           and the next candidate that is not `eot`; (b) the distance of every finite `eot`
           candidate from that G-th score (it decides whether the hypothesis is found at this
           step); (c) where a step fills the chunk's list of finished hypotheses, the gaps between
           its `eot` candidates (which of them get in); (d) the gaps between adjacent final scores
           of a chunk.  Gaps between candidates that are both kept decide nothing and do not count.
  sum_err  the largest |fp32 - fp64| of the hypotheses' sums when the stock fp32 model runs the
           same search (it must find the same ids, or the condition below cannot hold).

The tests' rule: margin >= 8 x sum_err (two sums each within 4 x sum_err cannot swap a decision
wider than that); then the decoder's ids equal the oracle's, its sums and scores are within
4 x sum_err."""
import functools
import math

import torch

from whisper_decoder_helpers import PROMPT, case, hf_logits

N_STEPS = 12  # generated positions the tests allow
# per geometry (D) an eot that ends hypotheses early, chosen so that the oracle alone satisfies
# margin >= 8 x sum_err at G = 5 (recomputed by every test that uses it)
EOT = {384: 49, 1280: 55, 512: 41}


def _search(model, enc, eot, G, patience, length_penalty, n_steps, suppress, suppress_at_start):
    B, V = int(enc.shape[0]), model.config.vocab_size
    max_finished = max(1, round(G * patience))
    ninf = -math.inf
    ids = [[[] for _ in range(G)] for _ in range(B)]
    sums = [[0.0] + [ninf] * (G - 1) for _ in range(B)]
    finished = [[] for _ in range(B)]
    margin = math.inf
    for step in range(n_steps):
        # (a done chunk's rows are padded with eot and their logits ignored)
        rows = torch.tensor([(PROMPT + ids[b][g] + [eot] * step)[:len(PROMPT) + step] for b in range(B) for g in range(G)])
        lg = hf_logits(model, enc.repeat_interleave(G, 0), rows)[:, -1].clone()
        if suppress:
            lg[:, list(suppress)] = ninf
        if suppress_at_start and step == 0:
            lg[:, list(suppress_at_start)] = ninf
        logp = torch.log_softmax(lg, -1).double().view(B, G, V)
        for b in range(B):
            if len(finished[b]) >= max_finished:
                continue
            cands = [(sums[b][g] + float(logp[b, g, t]), g, float(lg[b * G + g, t]), t)
                     for g in range(G) for t in range(V)]
            cands.sort(key=lambda c: (-c[0], c[1], -c[2], c[3]))
            live, found, last = [], [], None
            for pos, (s, g, _, t) in enumerate(cands):
                if t == eot:
                    found.append(s)
                    if len(finished[b]) < max_finished:
                        finished[b].append((list(ids[b][g]), s, len(ids[b][g]) + 1))
                else:
                    live.append((g, t, s))
                    if len(live) == G:
                        last = pos
                        break
            s_g = cands[last][0]
            nxt = next(c[0] for c in cands[last + 1:] if c[3] != eot)
            if s_g > ninf:
                margin = min(margin, s_g - nxt)  # (a)
                for s, _, _, t in cands:
                    if t == eot and s > ninf:
                        margin = min(margin, abs(s - s_g))  # (b)
            if len(finished[b]) >= max_finished:
                margin = min([margin] + [x - y for x, y in zip(found, found[1:])])  # (c)
            ids[b] = [ids[b][g] + [t] for g, t, _ in live]
            sums[b] = [s for _, _, s in live]
        if all(len(f) >= max_finished for f in finished):
            break
    out = []
    for b in range(B):
        hyps = list(finished[b])
        if len(hyps) < max_finished:
            for g in range(G):
                if len(hyps) >= G:
                    break
                hyps.append((ids[b][g], sums[b][g], max(1, len(ids[b][g]))))
        ranked = sorted([(i, s, s / n ** length_penalty) for i, s, n in hyps], key=lambda h: -h[2])
        for x, y in zip(ranked, ranked[1:]):
            margin = min(margin, x[2] - y[2])  # (d)
        out.append(ranked)
    return out, margin


@functools.lru_cache(maxsize=None)
def oracle(geometry, eot, G=5, patience=1.0, length_penalty=1.0, n_steps=N_STEPS, suppress=(), suppress_at_start=()):
    """(hypotheses per chunk [(ids, sum, score)] best first, margin, sum_err); computed once, shared."""
    c = case(*geometry)
    args = (eot, G, patience, length_penalty, n_steps, tuple(suppress), tuple(suppress_at_start))
    want, margin = _search(c.model64, c.enc64, *args)
    got32, _ = _search(c.model, c.enc, *args)
    assert [[h[0] for h in hs] for hs in got32] == [[h[0] for h in hs] for hs in want], \
        "the fp32 model's search finds other hypotheses: no sum_err for this eot"
    sum_err = max(abs(x[1] - y[1]) for hx, hy in zip(got32, want) for x, y in zip(hx, hy))
    return want, margin, sum_err


def check_beam_search(c, dec, label, eot, G=5, patience=1.0, length_penalty=1.0, n_steps=N_STEPS, suppress=(),
                      suppress_at_start=(), **kw):
    """dec.beam_search against the oracle under the rule above; prints the figures, returns the
    decoder's hypotheses."""
    want, margin, sum_err = oracle(c.geometry, eot, G, patience, length_penalty, n_steps, tuple(suppress),
                                   tuple(suppress_at_start))
    print(f"{label} {c.geometry} eot {eot} G {G} patience {patience} lp {length_penalty}: decisive margin "
          f"{margin:.3e}, sum_err {sum_err:.3e}, 8 x sum_err {8 * sum_err:.3e}; lengths "
          f"{[[len(h[0]) for h in hs] for hs in want]}")
    assert sum_err > 0 and margin >= 8 * sum_err
    got = dec.beam_search(c.enc, PROMPT, eot, beam_size=G, patience=patience, length_penalty=length_penalty,
                          max_length=len(PROMPT) + n_steps, suppress_tokens=list(suppress),
                          suppress_at_start=list(suppress_at_start), **kw)
    assert [[h.ids for h in hs] for hs in got] == [[h[0] for h in hs] for hs in want]
    err = max(max(abs(h.sum_logprob - w[1]), abs(h.score - w[2])) for hs, ws in zip(got, want) for h, w in zip(hs, ws))
    print(f"{label}: |sum - fp64| and |score - fp64| at most {err:.3e}, bound {4 * sum_err:.3e}")
    assert err <= 4 * sum_err
    return got

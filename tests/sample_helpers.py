"""Shared by the tests of wx_sample_token and WhisperDecoder.sample: an fp64 evaluation of the
selection's definition (include/wx_align.h), written from the header and independent of the
package's code, the error bounds the kernel is held to, and the decoder-level conditions.

The bounds are derived here, from the number formats and the documented accuracy of the device's
math functions, never from what the kernel gives:

  eps_tokens(max|l|, T)   The kernel's z_t = fl(fl(m_t / T) + g_t), g_t = -logf(-logf(u_t)), against
      the real-number z_t.  (a) the division is correctly rounded: 1/2 ulp32(|m / T|).  (b) logf is
      accurate to 2 ulp (HIP's and OpenCL's tables give 1 ulp for log; 2 leaves room): the inner
      a = logf(u) has a relative error of at most 2 * 2^-23, which moves log(-a) by as much
      (d log(x) = dx / x), and the outer logf adds 2 ulp32(|g|), |g| <= 17 (u lies in
      [2^-24, 1 - 2^-24]: g in [-2.82, 16.64]), so at most 2^-22 + 2 ulp32(17).  (c) the addition:
      1/2 ulp32(|z|).  With |m / T| and |z| at most max|l| / T + 17:
          |z32 - z| <= ulp32(max|l| / T + 17) + 2^-22 + 2 ulp32(17)
      and two entries can swap only if their fp64 margin is at most twice that: eps is twice that.
      The fp64 evaluation's own error (1e-15) is nothing beside it.

  logprob_bound(max|m|, V)   logprob = m_tok - (M + logf(L)), L the sum of expf(m_t - M') in the
      documented order.  With U = ulp32(max(max|m|, 1)) >= 2^-23: a term's exponent m_t - M' is
      rounded (at most 1/2 ulp32(2 max|m|) = U) and expf is accurate to 2 ulp (<= 2U relative): 3U
      per term; partial sums are rescaled twice (the 4 waves of a slice, the slices of a row), each
      time by expf of a rounded difference and one multiplication: 2 x 3.5U; a term passes through at
      most 15 + 6 + 4 + ceil(slices / 64) + 6 additions of 2^-24 <= U / 2 each.  All terms are
      positive, so L's relative error is at most the sum, and log(L) moves by as much.  logf(L): 2
      ulp32(max(ln V, 1)) (1 <= L <= V).  M + log L and m_tok - lse: 1/2 ulp32 each of at most
      2 max|m| + ln V.  The sum of these is the bound: about (log2 V + 4) ulps of max|m| at V =
      51865, as the selection's specification expects.
"""
import functools
import math

import numpy as np
import torch

from whisper_decoder_helpers import PROMPT, case, hf_logits

SLICE = 4096  # WX_SAMPLE_TOKEN_SLICE
KNOWN_ANSWERS = [  # Random123's known-answer vectors of Philox4x32-10: (counter, key, output)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox(counter, key):
    """Philox4x32-10 on Python integers: counter (4 words), key (2 words) -> 4 words."""
    c, k = [int(x) for x in counter], [int(x) for x in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return tuple(c)


def _philox_words(R, V, seed, step):
    """x [R, V] uint64: word t & 3 of the block with counter (t >> 2, r, step lo, step hi), key = seed.
    The rounds above on numpy arrays (object-free: 32 x 32-bit products fit a uint64)."""
    u = np.uint64
    lo = u(0xFFFFFFFF)
    c0 = np.broadcast_to(np.arange((V + 3) // 4, dtype=np.uint64)[None, :], (R, (V + 3) // 4)).copy()
    c1 = np.broadcast_to(np.arange(R, dtype=np.uint64)[:, None], c0.shape).copy()
    c2 = np.full(c0.shape, step & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.full(c0.shape, step >> 32, dtype=np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c0, u(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> u(32)) ^ c1 ^ u(k0), p1 & lo, (p0 >> u(32)) ^ c3 ^ u(k1), p0 & lo
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], -1).reshape(R, -1)[:, :V]


def uniforms(R, V, seed, step):
    """u [R, V] fp64 = ((x >> 9) + 0.5) 2^-23."""
    return ((_philox_words(R, V, int(seed), int(step)) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


class Selection:
    """definition()'s result: token [R] int64, logprob [R] fp64, done [R] bool (after the step),
    scored [R] bool (rows whose sum moves: not done on entry, not fully masked), margin [R] fp64
    (the top-2 gap of z; inf where the row is not scored or has one column)."""

    def __init__(self, token, logprob, done, scored, margin):
        self.token, self.logprob, self.done, self.scored, self.margin = token, logprob, done, scored, margin


def definition(logits, suppress, temperature, seed, step, done, eot) -> Selection:
    """wx_sample_token's definition for rows 0 .. R - 1 in fp64: logits [R, V] (array or tensor, -inf
    allowed), suppress [V] bool or None, done [R] bool on entry.  `temperature` is the fp32 value
    the kernel is handed."""
    x = np.array(logits.cpu().numpy() if torch.is_tensor(logits) else logits, dtype=np.float64)
    R, V = x.shape
    done = np.array(done.cpu().numpy() if torch.is_tensor(done) else done, dtype=bool)
    if suppress is not None:
        x[:, np.array(suppress.cpu().numpy() if torch.is_tensor(suppress) else suppress, dtype=bool)] = -np.inf
    z = x
    if temperature > 0:
        with np.errstate(invalid="ignore"):
            z = x / float(np.float32(temperature)) - np.log(-np.log(uniforms(R, V, seed, step)))
    order = np.lexsort((np.arange(V)[None, :].repeat(R, 0), -z), axis=-1)  # z descending, then t ascending
    token = order[:, 0].astype(np.int64)
    top = np.take_along_axis(z, order[:, :2], 1)
    with np.errstate(invalid="ignore"):
        margin = top[:, 0] - top[:, 1] if V > 1 else np.full(R, np.inf)
    M = x.max(1)
    scored = ~done & (M > -np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        lse = M + np.log(np.exp(x - M[:, None]).sum(1))
        logprob = np.take_along_axis(x, token[:, None], 1)[:, 0] - lse
    token = np.where(scored, token, eot)
    logprob = np.where(scored, logprob, 0.0)
    margin = np.where(scored & ~np.isnan(margin), margin, np.inf)
    return Selection(token, logprob, done | ~scored | (token == eot), scored, margin)


def ulp32(x: float) -> float:
    """The spacing of fp32 numbers at |x| (normal range)."""
    return 2.0 ** (math.floor(math.log2(max(abs(x), 2.0 ** -126))) - 23)


def eps_tokens(max_abs_logit: float, temperature: float) -> float:
    """The fp64 top-2 margin of z above which the kernel's token must equal the definition's (the
    module docstring's derivation); -1 at temperature 0, where z is the logit itself and even an
    exact tie (margin 0) has one answer, the lowest id."""
    if temperature == 0:
        return -1.0
    return 2 * (ulp32(max_abs_logit / temperature + 17) + 2.0 ** -22 + 2 * ulp32(17))


def logprob_bound(max_abs_logit: float, V: int) -> float:
    """The module docstring's bound on |kernel's logprob - fp64|."""
    U = ulp32(max(max_abs_logit, 1.0))
    slices = -(-V // SLICE)
    adds = 15 + 6 + 4 + -(-slices // 64) + 6
    lnv = max(math.log(V), 1.0)
    return (3 + 2 * 3.5 + 0.5 * adds) * U + 2 * ulp32(lnv) + ulp32(2 * max_abs_logit + lnv)


def chi_square_quantile(df: int, p_upper: float) -> float:
    """The 1 - p_upper quantile of chi-square with df degrees of freedom: bisection on the
    regularised upper incomplete gamma function (its series below a + 1, Lentz's continued fraction
    above).  52.747 at (13, 1e-6) and 139.830 at (69, 1e-6), as scipy's chi2.isf gives."""
    def upper(x):  # Q(df / 2, x / 2) by the continued fraction (x > df + 1 here) or the series
        a, y = df / 2.0, x / 2.0
        if y < a + 1:
            term = total = 1.0 / a
            n = a
            while abs(term) > 1e-17 * abs(total):
                n += 1
                term *= y / n
                total += term
            return 1.0 - total * math.exp(-y + a * math.log(y) - math.lgamma(a))
        tiny = 1e-300
        b = y + 1 - a
        c, d = 1 / tiny, 1 / b
        h = d
        for i in range(1, 10000):
            an = -i * (i - a)
            b += 2
            d = an * d + b
            d = tiny if abs(d) < tiny else d
            c = b + an / c
            c = tiny if abs(c) < tiny else c
            d = 1 / d
            delta = d * c
            h *= delta
            if abs(delta - 1) < 1e-15:
                break
        return math.exp(-y + a * math.log(y) - math.lgamma(a)) * h

    lo, hi = float(df), float(df) + 20 * math.sqrt(2 * df) + 100
    for _ in range(200):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if upper(mid) > p_upper else (lo, mid)
    return hi


# ------------------------------------------------------------------ the kernel's test inputs
def kernel_case(R: int, V: int, seed: int = 0):
    """The inputs of one kernel test shape: 2 randn logits (the distribution test's scale) with some
    -inf logits, a suppress mask over about 5% of the ids, eot, some `done` rows and, from 3 rows
    on, one fully masked row (row 1: every unsuppressed logit -inf).  Exact ties between the two
    largest logits of row 0 (the lower id must win at temperature 0).  Returns (logits [R, V] fp32,
    suppress [V] bool, done [R] bool, eot)."""
    g = torch.Generator().manual_seed(1000 * V + R + seed)
    x = 2 * torch.randn((R, V), generator=g)
    suppress = torch.rand(V, generator=g) < 0.05
    eot = V // 2
    suppress[eot] = False
    if V >= 8:
        x[torch.rand((R, V), generator=g) < 0.03] = float("-inf")
        free = (~suppress).nonzero()[:, 0]
        a, b = int(free[len(free) // 3]), int(free[2 * len(free) // 3])
        x[0, a] = x[0, b] = 9.5  # an exact tie above every other logit
    else:
        suppress[:] = False
    done = torch.zeros(R, dtype=torch.bool)
    if R >= 3:
        x[1, ~suppress] = float("-inf")
        done[2::5] = True
    return x, suppress, done, eot


def check_margins(sel: Selection, eps: float, label: str):
    """The rows the token comparison may skip (margin <= eps): at most 1% of the rows, asserted on
    the fp64 definition alone."""
    skip = sel.margin <= eps
    print(f"{label}: {int(skip.sum())} of {len(skip)} rows within eps {eps:.3e} (smallest margin "
          f"{float(sel.margin.min()):.3e})")
    assert skip.sum() <= 0.01 * len(skip)
    return ~skip


# ------------------------------------------------------------------- the decoder's conditions
@functools.lru_cache(maxsize=None)
def _path32(geometry, row, ids):
    c = case(*geometry)
    t = torch.tensor([list(ids)])
    y64 = hf_logits(c.model64, c.enc64[[row]], t)
    return y64, float((hf_logits(c.model, c.enc[[row]], t).double() - y64).abs().max())


def path_error(c, dtype, row, ids):
    """(HF fp64 logits [1, n, V] of teacher-forcing `ids` on chunk `row`, the yardstick of `dtype` on
    that path: ref_err of the fp32 stock model, or ref_err_half of the cast model)."""
    if dtype == torch.float32:
        return _path32(c.geometry, row, tuple(int(t) for t in ids))
    from whisper_decoder_half_helpers import path_errors

    y64, ref_err, _ = path_errors(c, dtype, [list(ids)], rows=[row])
    return y64, ref_err


def check_sample(c, dec, label, temperature, best_of, seed, n_steps=10, suppress=(), suppress_at_start=(),
                 eot=None, host=False, **kw):
    """dec.sample against the definition on the decoder's own teacher-forced logits: a second state
    of the same shape (start(beams=best_of), one step per id: the calls sample makes, so the logits
    it read, bit for bit) is fed the definition's tokens, row r and step n as the kernel counts
    them.  A row's ids must be the definition's as long as every selection on its path had a top-2
    margin above eps_tokens of the step's logits (`host`: the host route evaluates z in fp64 as the
    definition does, and eps is 1e-9); at most 1% of the selections may fall below it, and a row
    that met one is not compared.  The sums are within 8 n ref_err (fp32; 4 n ref_err_half for a
    half type) of the fp64 sum of the log-probabilities of the hypothesis' own ids on transformers'
    fp64 logits: the logits are within 4 ref_err (2 ref_err_half) of fp64 and a log-softmax moves by
    at most twice that.  score = sum / n, and the hypotheses are ordered by it.  Returns them."""
    G, V = best_of, c.V
    eot = V - 1 if eot is None else eot
    hyps = dec.sample(c.enc, PROMPT, eot, temperature=temperature, best_of=G, seed=seed, max_length=len(PROMPT) + n_steps,
                      suppress_tokens=list(suppress), suppress_at_start=list(suppress_at_start), **kw)
    assert len(hyps) == c.B and all(len(hs) == G for hs in hyps)
    for hs in hyps:
        assert all(x.score >= y.score for x, y in zip(hs, hs[1:]))
    mask = torch.zeros(V, dtype=torch.bool)
    mask[list(suppress)] = True
    mask0 = mask.clone()
    mask0[list(suppress_at_start)] = True
    R = c.B * G
    st = dec.start(c.enc, beams=G, **{k: v for k, v in kw.items() if k == "kernels"})
    for t in PROMPT:
        lg = dec.step(st, torch.full((R,), t))
    done = np.zeros(R, dtype=bool)
    rows, risky = [[] for _ in range(R)], np.zeros(R, dtype=bool)
    below = total = 0
    max_eps = 0.0
    for step in range(n_steps):
        lg = lg.cpu()
        sel = definition(lg, mask0 if step == 0 else mask, temperature, seed, step, done, eot)
        eps = 1e-9 if host and temperature > 0 else eps_tokens(float(lg[torch.isfinite(lg)].abs().max()), temperature)
        max_eps = max(max_eps, eps)
        risky |= sel.scored & (sel.margin <= eps)
        below += int((sel.scored & (sel.margin <= eps)).sum())
        total += int(sel.scored.sum())
        for r in range(R):
            if not done[r] and sel.token[r] != eot:
                rows[r].append(int(sel.token[r]))
        done = sel.done
        if done.all() or step == n_steps - 1:
            break
        lg = dec.step(st, torch.from_numpy(sel.token))
    print(f"{label} {c.geometry} T {temperature} best_of {G} seed {seed}: {below} of {total} selections within eps "
          f"{max_eps:.3e}; lengths {[[len(h.ids) for h in hs] for hs in hyps]}")
    assert below <= 0.01 * total
    for b, hs in enumerate(hyps):
        left = [h.ids for h in hs]
        for r in range(b * G, (b + 1) * G):
            if not risky[r]:
                assert rows[r] in left, (b, r, rows[r], left)
                left.remove(rows[r])
    worst = 0.0
    factor = 8 if dec.dtype == torch.float32 else 4
    for b, hs in enumerate(hyps):
        for h in hs:
            assert eot not in h.ids and not set(h.ids) & set(suppress)
            assert not h.ids or h.ids[0] not in suppress_at_start
            want, n, ref_err = _fp64_sum(c, dec, b, h.ids, len(h.ids) < n_steps, eot, mask, mask0)
            assert h.score == h.sum_logprob / n
            bound = factor * n * ref_err
            worst = max(worst, abs(h.sum_logprob - want) / bound)
            assert abs(h.sum_logprob - want) <= bound, (b, h, want)
    print(f"{label}: |sum - fp64 sum of its ids| at most {worst:.3f} x {factor} n ref_err")
    return hyps


def _fp64_sum(c, dec, b, ids, ended, eot, mask, mask0):
    scored = ids + [eot] if ended else ids
    if not scored:
        return 0.0, 1, 1.0
    seq = (PROMPT + scored)[:-1]
    y64, ref_err = path_error(c, dec.dtype, b, seq)
    lg = y64[0, len(PROMPT) - 1:].clone()
    lg[:, mask] = float("-inf")
    lg[0, mask0] = float("-inf")
    logp = torch.log_softmax(lg, -1)
    return float(sum(logp[i, t] for i, t in enumerate(scored))), max(1, len(scored)), ref_err

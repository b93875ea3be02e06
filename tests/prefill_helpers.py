"""Shared by the prompt-prefill tests: the causal attention reference, the checks the kernel tests
apply to wx_prefill_attention_f32 / _h16 (so that tests/test_whisper_prefill.py can show, without a
GPU, that they reject an attention whose mask is off by one key), the covering set of shapes, and
the adapter that runs the decoder oracles of whisper_decoder_helpers through prefill.

The attention here is `attend(q, k, v) -> o` with q [N, Tq, 64], k / v [N, Tk, 64], o [N, Tq, 64]
(N = B H) at softmax scale 0.125, as in attention_probes.  `causal`: None for no mask, or the
position of query 0: query i sees keys j <= causal + i.

Tolerance rule (the project's): ref_err = max|torch fp32 on the CPU - fp64| on the same inputs and
the same mask, and the code under test must be within 4 x ref_err of fp64, every output finite."""
import functools

import pytest
import torch

import attention_probes as ap
from whisper_decoder_helpers import N_FORCED, PROMPT

SCALE = ap.SCALE


def keep(Tq: int, Tk: int, causal, shift: int = 0) -> torch.Tensor:
    """[Tq, Tk] bool: key j is visible to query i (j <= causal + i + shift; everything without a mask)."""
    if causal is None:
        return torch.ones((Tq, Tk), dtype=torch.bool)
    return torch.arange(Tk)[None, :] <= causal + torch.arange(Tq)[:, None] + shift


def reference(q, k, v, causal=None, shift: int = 0):
    """softmax(SCALE q k^T + mask) v in the inputs' precision.  `shift` = -1 / +1: the two wrong
    masks (one key too few, j < causal + i; one too many, j <= causal + i + 1)."""
    s = SCALE * (q @ k.transpose(-1, -2))
    s = s.masked_fill(~keep(q.shape[1], k.shape[1], causal, shift), float("-inf"))
    return torch.softmax(s, -1) @ v


@functools.lru_cache(maxsize=None)
def case(N: int, Tq: int, Tk: int, causal, seed: int = 0):
    """(q, k, v, fp64 result, ref_err) of random inputs at scales 2, 2, 2; computed once, shared and
    left unchanged."""
    q, k, v = ap.random_inputs(N, Tq, Tk, seed=seed + (0 if causal is None else 7919 * (causal + 1)))
    want = reference(q.double(), k.double(), v.double(), causal)
    ref_err = float((reference(q, k, v, causal).double() - want).abs().max())
    return q, k, v, want, ref_err


def check_accuracy(o: torch.Tensor, want: torch.Tensor, ref_err: float, label: str = "") -> float:
    """Every output finite and max |o - fp64| <= 4 x ref_err; prints and returns the error."""
    assert o.shape == want.shape and o.dtype == torch.float32
    if not bool(torch.isfinite(o).all()):
        bad = ~torch.isfinite(o).all(-1)
        raise AssertionError(f"{label}: {int(bad.sum())} output rows are not finite (first {bad.nonzero()[0].tolist()})")
    err = float((o.double() - want).abs().max())
    print(f"{label}: |o - fp64| {err:.3e}, ref_err {ref_err:.3e}, bound {4 * ref_err:.3e}")
    if not err <= 4 * ref_err:
        raise AssertionError(f"{label}: |o - fp64| {err:.3e} > 4 x ref_err {4 * ref_err:.3e}")
    return err


class MaskedUniform:
    """attention_probes.Uniform under the causal mask: q = 0 and integer v, so query i must return
    sum_{j <= causal + i} v[j] / (causal + i + 1): every partial sum is an integer below 2^24 (exact
    in fp32 in any order).  One key too few or too many moves an output by at least 1 / L."""

    def __init__(self, N: int, Tq: int, causal: int, Tk=None, seed: int = 0):
        Tk = causal + Tq if Tk is None else Tk
        u = ap.Uniform(N, Tq, Tk, seed)
        self.q, self.k, self.v = u.q, u.k, u.v
        self.n = (causal + 1 + torch.arange(Tq)).clamp_max(Tk)  # visible keys of query i
        self.sum = u.v.long().cumsum(1)[:, self.n - 1]  # [N, Tq, 64]
        self.want = self.sum.double() / self.n[None, :, None].double()
        self.N, self.Tq, self.Tk, self.causal = N, Tq, Tk, causal

    def check(self, o) -> float:
        """Uniform.check's rule per query: relative error <= 2^-22, exactly 0 where the sum is 0."""
        assert o.shape == self.want.shape and o.dtype == torch.float32
        od = o.double()
        zero = self.want == 0
        err = (od - self.want).abs()
        ok = torch.where(zero, od == 0, err <= 2.0 ** -22 * self.want.abs())
        if not bool(ok.all()):
            n, i, d = (int(x) for x in (~ok).nonzero()[0])
            raise AssertionError(f"uniform under the mask (causal {self.causal}, Tq {self.Tq}, Tk {self.Tk}): "
                                 f"{int((~ok).any(-1).sum())} bad rows; first o[{n}, {i}, {d}] = {float(o[n, i, d])!r}, "
                                 f"want {int(self.sum[n, i, d])} / {int(self.n[i])}")
        rel = err / self.want.abs().clamp_min(1e-300)
        return float(rel[~zero].max()) if bool((~zero).any()) else 0.0


# (Tq, Tk, causal): the covering set of the kernel tests.  Tq in {1, 2, 31, 32, 33, 65}; without a
# mask Tk in {1, 31, 32, 33, 129, 1500}; causal in {0, 1, 5, 31, 32, 33, 100} with Tk = causal + Tq
# and with Tk beyond it.  (5, 33): rows that see nothing in a wave's first tile; (33, 65): a second
# query tile with skipped key tiles; (0, 1): three waves without a tile.
SHAPES = [
    (1, 1, None), (2, 31, None), (31, 32, None), (32, 33, None), (33, 129, None), (65, 1500, None), (1, 1500, None),
    (33, 1, None), (65, 31, None),
    (1, 1, 0), (33, 38, 5), (65, 98, 33), (32, 32, 0), (31, 32, 1), (2, 33, 31), (33, 65, 32), (65, 165, 100),
    (65, 65, 0), (1, 34, 33), (32, 37, 5),
    (33, 78, 5), (65, 101, 33), (2, 133, 100), (31, 95, 0), (32, 64, 31), (1, 1500, 1), (65, 129, 32),
]
MUST = [(33, 38, 5), (65, 98, 33), (1, 1, 0)]
assert all(m in SHAPES for m in MUST)
BATCHES = [(1, 1), (3, 6), (2, 20)]


def covering():
    """(B, H, Tq, Tk, causal): every shape once, the (B, H) in turn, and the three named cases at
    every (B, H)."""
    out = [(*BATCHES[i % 3], *s) for i, s in enumerate(SHAPES)]
    out += [(B, H, *m) for m in MUST for B, H in BATCHES if (B, H, *m) not in out]
    return out


class Prefilled:
    """A WhisperDecoder whose logits / generate / beam_search run with prefill=True: what the
    oracle checks of whisper_decoder_helpers, beam_helpers and whisper_decoder_half_helpers call."""

    def __init__(self, dec):
        self.dec = dec

    def __getattr__(self, name):
        return getattr(self.dec, name)

    def logits(self, *a, **kw):
        return self.dec.logits(*a, prefill=True, **kw)

    def generate(self, *a, **kw):
        return self.dec.generate(*a, prefill=True, **kw)

    def beam_search(self, *a, **kw):
        return self.dec.beam_search(*a, prefill=True, **kw)


def routes(dec, c, ids):
    """name -> (last-position logits [B, V], state) of the ways to feed the 12 forced positions."""
    def run(plan):
        st = dec.start(c.enc)
        at = 0
        for kind, n in plan:
            if kind == "prefill":
                lg = dec.prefill(st, ids[:, at:at + n])
                at += n
            else:
                for _ in range(n):
                    lg = dec.step(st, ids[:, at])
                    at += 1
        assert at == N_FORCED
        return lg, st
    return {"steps": run([("step", 12)]), "prefill(12)": run([("prefill", 12)]),
            "prefill(5) prefill(7)": run([("prefill", 5), ("prefill", 7)]),
            "prefill(11) step": run([("prefill", 11), ("step", 1)]),
            "3 steps prefill(9)": run([("step", 3), ("prefill", 9)])}


def check_routes(dec, c, label):
    ids, y64, ref_err = c.forced()
    got = routes(dec, c, ids)
    steps_lg, steps_st = got["steps"]
    for name, (lg, st) in got.items():
        assert st.pos == N_FORCED, name
        assert tuple(lg.shape) == (c.B, c.V) and lg.dtype == torch.float32
        err = float((lg.cpu().double() - y64[:, -1]).abs().max())
        d = float((lg - steps_lg).abs().max())
        dc = max(float((a[:, :, :N_FORCED].float() - b[:, :, :N_FORCED].float()).abs().max())
                 for a, b in zip((*st.self_k, *st.self_v), (*steps_st.self_k, *steps_st.self_v)))
        print(f"{label} {c.geometry} {name}: |logits - fp64| {err:.3e} (bound {4 * ref_err:.3e}), |logits - stepwise| "
              f"{d:.3e}, |caches - stepwise| {dc:.3e} (bound {8 * ref_err:.3e})")
        assert err <= 4 * ref_err and d <= 8 * ref_err and dc <= 8 * ref_err, name
    for a, (la, _) in got.items():
        for b, (lb, _) in got.items():
            assert float((la - lb).abs().max()) <= 8 * ref_err, (a, b)


# ------------------------------------------------------------------------------ beams
def check_beams(dec, c):
    G, n = 5, len(PROMPT)
    st = dec.start(c.enc, beams=G)
    tok = torch.tensor([PROMPT] * c.B)
    lg = dec.prefill(st, tok)
    assert tuple(lg.shape) == (c.B * G, c.V) and st.pos == n and st.rows == c.B * G
    one = dec.prefill(dec.start(c.enc), tok)
    assert torch.equal(lg.view(c.B, G, c.V), one[:, None].expand(c.B, G, c.V))
    plain = dec.start(c.enc)
    dec.prefill(plain, tok)
    for cache, single in zip((*st.self_k, *st.self_v), (*plain.self_k, *plain.self_v)):
        rows = cache.view(c.B, G, *cache.shape[1:])
        assert bool((rows[:, :, :, :n] != 0).any())
        for g in range(G):  # every beam holds the chunk's rows, bit for bit
            assert torch.equal(rows[:, g], single)
        assert bool((rows[:, :, :, n:] == 0).all())
    with pytest.raises(ValueError, match="position 0 only"):
        dec.prefill(st, tok)
    lg = dec.step(st, torch.full((c.B * G,), 3))  # the state goes on
    assert st.pos == n + 1 and bool(torch.isfinite(lg).all())


def check_empty_batch(dec, c):
    """No chunks: prefill, and logits / generate / beam_search through it, return empty results."""
    enc, ids = c.enc[:0], c.forced()[0][:0]
    st = dec.start(enc)
    assert tuple(dec.prefill(st, ids).shape) == (0, c.V) and st.pos == N_FORCED
    assert tuple(dec.prefill(dec.start(enc), ids, all_positions=True).shape) == (0, N_FORCED, c.V)
    assert tuple(dec.logits(enc, ids, prefill=True).shape) == (0, N_FORCED, c.V)
    assert dec.generate(enc, PROMPT, 2, prefill=True) == [] and dec.beam_search(enc, PROMPT, 2, 3, prefill=True) == []

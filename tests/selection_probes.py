"""Probes for the two selection kernels, wx_sample_token (csrc/wx_sample.hip) and wx_beam_topk
(csrc/wx_beam.hip): inputs whose winners sit where the kernels' structure can go wrong (every column
of a slice and a tail, one lane's 16 registers, ties across lanes, waves and slices, whole waves and
slices of -inf, a 65th slice), their expected outputs, and a plain numpy emulation of both kernels'
structure with switches for the mistakes a kernel could make.  CPU tensors only; every probe is
computed once and shared, the tests leave it unchanged.

Expected outputs come from the header's definition (include/wx_align.h) in fp64,
sample_helpers.definition and `_reference` below, or are stated directly where the construction fixes
them (a planted winner, a tie's order, -ln 2, -ln V); nothing a kernel returns goes into one.  The
bounds are sample_helpers.logprob_bound / eps_tokens and the top-k test's 4 x / 8 x ref_err.

The emulation follows the header's maps, column -> (slice, wave, lane, register):
    wx_sample_token   t = 4096 s + 1024 w + 256 e + 4 lane + j   (one Philox block per 4 columns)
    wx_beam_topk      t = 4096 s + 1024 w + 64 e + lane
a lane's 16 terms in order, the butterfly over the wave, the 4 waves in order, the slices 64 apart in
order and a butterfly; fp32 arithmetic with numpy's exp and log, so it is held to the same bounds as
the kernels, not to their bits.  Selections are made under the kernels' total orders, which makes
them independent of the order of the comparisons.  `fault=` gives the structure with one mistake
(SAMPLE_FAULTS, TOPK_FAULTS; test_selection_probes.py shows which probe rejects which).

"The winner's logit replaced by the wave's maximum logit" has two readings.  Taken for the winner's
own wave ("logit_is_wave_max") no planted probe can see it: a plant that wins is its wave's
maximum.  The masked-unit probes at temperature 0.7 reject it, where a drawn winner is not its wave's
largest logit.  Taken for the wave that merges the slice, wave 0 ("logit_from_wave_0": the entry of another
wave keeps wave 0's maximum logit), it is what the every-column probe rejects.

On an MI355X (test_gpu_selection_probes.py; the largest |logprob - fp64| / logprob_bound or
|score - fp64| / (4 ref_err) over all cases of a probe; every token and index as expected, no row
skipped):
    wx_sample_token   every column wins     0.025 (T 0), 0.000 (T 1: the plant's probability rounds to 1)
                      ties                  0.027; constant rows 0.186 (V 1025, masked)
                      pair rows             0.000 (-ln 2 to the bit)
                      masked units          0.016
                      more than 64 slices   0.013
    wx_beam_topk      concentrated winners  0.052
                      ties                  0.250 (constant rows), 0.125 (equal maxima), 0.073 (identical beams)
                      smallest and edge V   0.193 (G 1)
                      masked units          0.052
                      more than 64 slices   0.114 (the tie)
"""
import functools
import math

import numpy as np
import torch

from sample_helpers import SLICE, check_margins, definition, eps_tokens, logprob_bound
from test_gpu_sample_token import SEED, STEPS

assert SLICE == 4096
KNONE = 2 ** 31 - 1  # the column of "no entry"
F32 = np.float32
NINF = F32(-np.inf)
LANES = np.arange(64)

SAMPLE_FAULTS = ("uniform_word_plus_1", "group_counter_per_slice", "ties_to_higher_column_across_waves",
                 "logit_from_wave_0", "logit_is_wave_max", "merge_drops_slices_past_64", "empty_slice_wins")
TOPK_FAULTS = ("one_entry_per_lane", "previous_winner_by_value", "merge_drops_slices_past_64", "unguarded_empty_sum",
               "equal_scores_by_slice")


def _gen(*seed):
    s = 0
    for x in seed:
        s = (s * 1000003 + int(x) + 1) % (2 ** 62)
    return torch.Generator().manual_seed(s)


# ------------------------------------------------------------------------- the emulation's parts
def _butterfly_sum(a):
    """wave_sum on [..., 64] fp32: six xor steps; every lane ends with the same bits."""
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., LANES ^ o]
    return a[..., 0]


def _lane_sum(x, m, guard=True):
    """x [..., 64, 16] fp32, m [...]: per lane l = 0; l += exp(x_i - m) in order, then the butterfly;
    0 where m is -inf (`guard`; without it exp(-inf + inf) = NaN)."""
    mm = m[..., None]
    l = np.zeros(x.shape[:-1], dtype=F32)
    with np.errstate(invalid="ignore"):
        for i in range(x.shape[-1]):
            l = l + np.exp(x[..., i] - mm)
    if guard:
        l = np.where(mm > NINF, l, F32(0))
    return _butterfly_sum(l.astype(F32))


def _merge_sums(m, l, axis_len, guard=True):
    """(M, L) of `axis_len` partial (m, l) on the last axis, added in order: L += exp(m_u - M) l_u
    where m_u > -inf."""
    M = m.max(-1)
    L = np.zeros(M.shape, dtype=F32)
    with np.errstate(invalid="ignore"):
        for u in range(axis_len):
            term = (np.exp(m[..., u] - M) * l[..., u]).astype(F32)
            L = L + (np.where(m[..., u] > NINF, term, F32(0)) if guard else term)
    return M, L.astype(F32)


def _row_sums(M, L, guard=True):
    """The merge kernels' (M, L) over the slices [n, ns]: lane s % 64 adds its slices 64 apart in
    order, then the butterfly."""
    n, ns = M.shape
    trips = -(-ns // 64)
    Mp = np.full((n, trips * 64), NINF, dtype=F32)
    Lp = np.zeros((n, trips * 64), dtype=F32)
    Mp[:, :ns], Lp[:, :ns] = M, L
    Mp, Lp = Mp.reshape(n, trips, 64).transpose(0, 2, 1), Lp.reshape(n, trips, 64).transpose(0, 2, 1)  # [n, lane, trip]
    top = M.max(-1)
    acc = np.zeros((n, 64), dtype=F32)
    with np.errstate(invalid="ignore"):
        for i in range(trips):
            term = (np.exp(Mp[..., i] - top[:, None]) * Lp[..., i]).astype(F32)
            # (a lane past the last slice adds nothing, guarded or not: its loop does not run)
            live = (Mp[..., i] > NINF) if guard else (np.arange(64)[None, :] + 64 * i < ns)
            acc = acc + np.where(live, term, F32(0))
    return top, _butterfly_sum(acc.astype(F32))


def _first(z, c, highest=False):
    """The index, on the last axis, of the entry first under (z descending, c ascending); `highest`:
    equal z go to the higher column instead (KNONE excepted)."""
    zmax = z.max(-1, keepdims=True)
    if highest:
        return np.where((z == zmax) & (c != KNONE), c, -1).argmax(-1)[..., None]
    return np.where(z == zmax, c.astype(np.int64), KNONE + 1).argmin(-1)[..., None]


def _take(i, *arrays):
    return [np.take_along_axis(a, i, -1)[..., 0] for a in arrays]


def _philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words."""
    u = np.uint64
    lo = u(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3))
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c0, u(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> u(32)) ^ c1 ^ u(k0), p1 & lo, (p0 >> u(32)) ^ c3 ^ u(k1), p0 & lo
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], -1)


# ------------------------------------------------------------------ wx_sample_token's emulation
def emulate_sample(x, suppress, temperature, seed, step, eot, rows=None, fault=None, chunk=128):
    """wx_sample_token's structure on the CPU for rows `rows` (default: all) of x [R, V], none done on
    entry: (token [n] int64, logprob [n] fp32, done [n] bool).  The generator counts the rows of x,
    so a subset of rows gives what the whole launch gives them."""
    assert fault is None or fault in SAMPLE_FAULTS
    x = x.numpy() if torch.is_tensor(x) else np.asarray(x)
    assert x.dtype == np.float32
    R, V = x.shape
    rows = np.arange(R) if rows is None else np.asarray(rows)
    sup = None if suppress is None else np.asarray(suppress.numpy() if torch.is_tensor(suppress) else suppress, dtype=bool)
    ns = -(-V // SLICE)
    # col [ns, 4, 64, 16]: lane `lane` of wave w holds columns 256 e + 4 lane + j, in the order (e, j)
    col = np.arange(ns * SLICE).reshape(ns, 4, 4, 64, 4).transpose(0, 1, 3, 2, 4).reshape(ns, 4, 64, 16)
    c = np.where(col < V, col, KNONE)
    T = F32(temperature)
    tok, lp, done = [], [], []
    for a in range(0, len(rows), chunk):
        rr = rows[a:a + chunk]
        n = len(rr)
        xm = np.full((n, ns * SLICE), NINF, dtype=F32)
        xm[:, :V] = x[rr]
        if sup is not None:
            xm[:, :V][:, sup] = NINF
        z = xm
        if temperature > 0:
            q = np.arange(ns * SLICE // 4, dtype=np.uint64)
            if fault == "group_counter_per_slice":
                q = q % np.uint64(SLICE // 4)
            w = _philox(q[None, :], rr.astype(np.uint64)[:, None], np.uint64(step & 0xFFFFFFFF), np.uint64(step >> 32),
                        seed & 0xFFFFFFFF, seed >> 32)  # [n, groups, 4]
            if fault == "uniform_word_plus_1":
                w = np.roll(w, -1, axis=-1)
            u = ((w >> np.uint64(9)).astype(F32) + F32(0.5)) * F32(2.0 ** -23)
            g = -np.log(-np.log(u.reshape(n, -1)))
            assert g.dtype == np.float32
            z = (xm / T) + g
            z[:, V:] = NINF
        zz, xx = z[:, col], xm[:, col]  # [n, ns, 4, 64, 16]
        cc = np.broadcast_to(c, zz.shape)
        # the lane's scan, then the wave's butterfly
        bz, bc, bx = _take(_first(zz, cc), zz, cc, xx)  # [n, ns, 4, 64]
        m = xx.max((-1, -2))
        l = _lane_sum(xx, m)
        bz, bc, bx = _take(_first(bz, bc), bz, bc, bx)  # [n, ns, 4]
        if fault == "logit_is_wave_max":
            bx = m
        # lane 0 of wave 0 merges the 4 waves
        M, L = _merge_sums(m, l, 4)
        i = _first(bz, bc, highest=fault == "ties_to_higher_column_across_waves")
        if fault == "logit_from_wave_0":
            bx = np.broadcast_to(m[..., :1], bx.shape)
        sz, sc, sx = _take(i, bz, bc, bx)  # [n, ns]
        # the merge kernel
        if fault == "merge_drops_slices_past_64":
            M, L, sz, sc, sx = (t[:, :64] for t in (M, L, sz, sc, sx))
        if fault == "empty_slice_wins":
            sz = np.where(M == NINF, F32(np.inf), sz)
        top, total = _row_sums(M, L)
        rz, rc, rx = _take(_first(sz, sc), sz, sc, sx)  # [n]
        with np.errstate(divide="ignore", invalid="ignore"):
            p = (rx - (top + np.log(total))).astype(F32)
        live = rx > NINF
        tok.append(np.where(live, rc, eot).astype(np.int64))
        lp.append(np.where(live, p, F32(0)).astype(F32))
        done.append(~live | (tok[-1] == eot))
    return np.concatenate(tok), np.concatenate(lp), np.concatenate(done)


# --------------------------------------------------------------------- wx_beam_topk's emulation
def _select(v, c, K, by_value=False):
    """The first K entries of the last axis under (v descending, c ascending) as (v, c); an entry
    with c = KNONE is none and what is missing is (-inf, KNONE).  `by_value`: "after the previous
    winner" compared on the value alone, so every value is taken once."""
    order = np.lexsort((c, -v), axis=-1)
    sv, sc = np.take_along_axis(v, order, -1), np.take_along_axis(c, order, -1)
    if by_value:
        keep = np.ones(sv.shape, dtype=bool)
        keep[..., 1:] = sv[..., 1:] != sv[..., :-1]
        keep &= sc != KNONE
        order = np.argsort(~keep, axis=-1, kind="stable")
        sv, sc, keep = (np.take_along_axis(t, order, -1) for t in (sv, sc, keep))
        sv, sc = np.where(keep, sv, NINF), np.where(keep, sc, KNONE)
    sv, sc = sv[..., :K], sc[..., :K]
    if sv.shape[-1] < K:
        pad = [(0, 0)] * (sv.ndim - 1) + [(0, K - sv.shape[-1])]
        sv, sc = np.pad(sv, pad, constant_values=NINF), np.pad(sc, pad, constant_values=KNONE)
    return np.where(sc == KNONE, NINF, sv), sc


def emulate_topk(x, cum, G, fault=None):
    """wx_beam_topk's structure on the CPU: x [B G, V], cum [B G] -> (scores [B, 2G] fp32,
    index [B, 2G] int64)."""
    assert fault is None or fault in TOPK_FAULTS
    x = x.numpy() if torch.is_tensor(x) else np.asarray(x)
    cum = cum.numpy() if torch.is_tensor(cum) else np.asarray(cum)
    assert x.dtype == np.float32 and cum.dtype == np.float32
    R, V = x.shape
    B, K = R // G, 2 * G
    assert B * G == R and V >= K
    ns = -(-V // SLICE)
    guard = fault != "unguarded_empty_sum"
    by_value = fault == "previous_winner_by_value"
    # col [ns, 4, 64, 16]: lane `lane` of wave w holds columns 64 e + lane
    col = np.arange(ns * SLICE).reshape(ns, 4, 16, 64).transpose(0, 1, 3, 2)
    c = np.where(col < V, col, KNONE)
    xp = np.full((R, ns * SLICE), NINF, dtype=F32)
    xp[:, :V] = x
    xx = xp[:, col]  # [R, ns, 4, 64, 16]
    cc = np.broadcast_to(c, xx.shape)
    m = xx.max((-1, -2))
    l = _lane_sum(xx, m)
    if fault == "one_entry_per_lane":
        v1, c1 = _select(xx, cc, 1)
        wv, wc = _select(v1[..., 0], c1[..., 0], K)
    else:
        wv, wc = _select(xx.reshape(R, ns, 4, 1024), cc.reshape(R, ns, 4, 1024), K, by_value)
    # wave 0 merges the 4 waves' entries and their (m, l)
    sv, sc = _select(wv.reshape(R, ns, 4 * K), wc.reshape(R, ns, 4 * K), K, by_value)
    M, L = _merge_sums(m, l, 4, guard)
    # the merge kernel: wave g, row b G + g
    if fault == "merge_drops_slices_past_64":
        M, L, sv, sc = (t[:, :64] for t in (M, L, sv, sc))
    top, total = _row_sums(M, L, guard)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = (top + np.log(total)).astype(F32)
        rv, rc = _select(sv.reshape(R, -1), sc.reshape(R, -1), K, by_value)
        score = (cum[:, None] + (rv - lse[:, None])).astype(F32)
    score = np.where((rv == NINF) | (cum[:, None] == NINF), NINF, score)
    # wave 0: the chunk's 2G best of its G K scored entries
    s, xs, t = (a.reshape(B, G * K) for a in (score, rv, rc))
    g = np.broadcast_to(np.repeat(np.arange(G), K)[None, :], s.shape)
    keys = (t, -xs, g, t // SLICE, -s) if fault == "equal_scores_by_slice" else (t, -xs, g, -s)
    order = np.lexsort(keys, axis=-1)[:, :K]
    s, g, t = (np.take_along_axis(a, order, -1) for a in (s, g, t))
    return s.astype(F32), g.astype(np.int64) * V + t


# ---------------------------------------------------------------------- wx_sample_token's probes
class SampleProbe:
    """One launch of wx_sample_token, no row done on entry: x [R, V] fp32, suppress [V] bool or None,
    temperature, step, eot; `token` [R] (the definition's or the construction's), `keep` [R] (rows
    whose token is compared: all of them unless the probe's margin rule skips some), `logprob` [R]
    fp64 and its `bound`, `done` [R] after the step."""

    def __init__(self, label, x, suppress, temperature, step, top, token=None, logprob=None, skip=False, eot=None):
        R, V = x.shape
        self.label, self.x, self.suppress, self.temperature, self.step = label, x, suppress, temperature, step
        self.R, self.V = R, V
        self.eot = V - 1 if eot is None else eot
        self.sel = definition(x, suppress, temperature, SEED, step, np.zeros(R, dtype=bool), self.eot)
        self.eps = eps_tokens(top, temperature)
        self.keep = check_margins(self.sel, self.eps, label) if skip else np.ones(R, dtype=bool)
        self.token = self.sel.token if token is None else np.asarray(token, dtype=np.int64)
        self.logprob = self.sel.logprob if logprob is None else np.full(R, float(logprob))
        self.bound = logprob_bound(top, V)
        self.done = self.token == self.eot

    def check(self, got, label, rows=None) -> float:
        """got = (token, logprob) of rows `rows` (default: all): the tokens of the kept rows, every
        logprob finite and within the bound on the rows whose token is the expected one.  Names the
        first failing row; prints and returns the largest |logprob - fp64| / bound."""
        rows = np.arange(self.R) if rows is None else np.asarray(rows)
        tok, lp = (np.asarray(t.cpu().numpy() if torch.is_tensor(t) else t) for t in got)
        assert tok.shape == lp.shape == rows.shape
        who = f"{label} {self.label}"
        want = self.token[rows]
        bad = (tok != want) & self.keep[rows]
        if bad.any():
            i = int(bad.nonzero()[0][0])
            raise AssertionError(f"{who}: {int(bad.sum())} of {len(rows)} rows took another column; first: row {int(rows[i])} "
                                 f"took column {int(tok[i])}, expected {int(want[i])} (margin {self.sel.margin[rows[i]]:.3e}, "
                                 f"eps {self.eps:.3e})")
        if not np.isfinite(lp).all():
            i = int((~np.isfinite(lp)).nonzero()[0][0])
            raise AssertionError(f"{who}: row {int(rows[i])}, column {int(tok[i])}: logprob {lp[i]!r} is not finite")
        agree = tok == want
        err = np.abs(lp.astype(np.float64) - self.logprob[rows]) * agree
        ratio = float(err.max()) / self.bound
        print(f"{who}: {int(agree.sum())} of {len(rows)} tokens as expected; |logprob - fp64| / bound {ratio:.3f} "
              f"(bound {self.bound:.3e})")
        if not ratio <= 1.0:
            i = int(err.argmax())
            raise AssertionError(f"{who}: row {int(rows[i])}, column {int(tok[i])}: logprob {float(lp[i])!r}, fp64 "
                                 f"{float(self.logprob[rows[i]])!r}: err {float(err[i]):.3e} > bound {self.bound:.3e}")
        return ratio

    def emulate(self, rows=None, fault=None):
        tok, lp, _ = emulate_sample(self.x, self.suppress, self.temperature, SEED, self.step, self.eot, rows, fault)
        return tok, lp


N_EDGE = SLICE + 5  # R = V of the square probes: one slice and a tail of 5 columns
TIE_OFFSETS = (1, 63, 64, 256, 1024, 4096)  # the next column, lane 63 / 0 of the next round, ..., wave, slice


def edge_rows(R=N_EDGE, stride=16):
    """The rows a CPU test runs the emulation on: every `stride`th and those about the edges of a
    group, a round of lanes, a wave and the slice."""
    near = [r + d for r in (0, 64, 256, 1024, 2048, 3072, SLICE, R) for d in range(-4, 5)]
    return np.array(sorted({r for r in list(range(0, R, stride)) + near if 0 <= r < R}))


@functools.lru_cache(maxsize=None)
def _square_background():
    return 2.0 * torch.randn((N_EDGE, N_EDGE), generator=_gen(31))


@functools.lru_cache(maxsize=None)
def every_column_wins(temperature: float) -> SampleProbe:
    """Row r: 2 randn with a plant at column r, 12.0 at temperature 0 and 60.0 at temperature 1.0
    (60 + g beats every 2 randn + g': the definition's margin is asserted).  token[r] = r."""
    plant = {0.0: 12.0, 1.0: 60.0}[temperature]
    x = _square_background().clone()
    x[torch.arange(N_EDGE), torch.arange(N_EDGE)] = plant
    p = SampleProbe(f"every column wins, T {temperature} plant {plant}", x, None, temperature, STEPS[1], plant,
                    token=np.arange(N_EDGE))
    p.plant = plant
    return p


@functools.lru_cache(maxsize=None)
def tie_rows() -> SampleProbe:
    """Temperature 0.  Row r: 12.0 at r and at r + 1, r + 63, r + 64, r + 256, r + 1024, r + 4096
    where below V, over 2 randn (cut at 11.5).  token[r] = r, the lowest of the tied columns."""
    x = _square_background().clamp(max=11.5)
    r = torch.arange(N_EDGE)
    for d in (0,) + TIE_OFFSETS:
        ok = r + d < N_EDGE
        x[r[ok], r[ok] + d] = 12.0
    return SampleProbe("ties", x, None, 0.0, 0, 12.0, token=np.arange(N_EDGE))


@functools.lru_cache(maxsize=None)
def constant_row(V: int, masked: bool) -> SampleProbe:
    """Temperature 0, two rows of 1.5: column 0, or the first id after a mask over ids 0 .. 2;
    logprob = -ln of the number of live ids."""
    assert V > 3 or not masked
    sup = None
    if masked:
        sup = torch.zeros(V, dtype=torch.bool)
        sup[:3] = True
    live = V - 3 if masked else V
    return SampleProbe(f"constant row V {V}{' masked' if masked else ''}", torch.full((2, V), 1.5), sup, 0.0, 0, 1.5,
                       token=np.full(2, 3 if masked else 0), logprob=-math.log(live), eot=V - 1)


@functools.lru_cache(maxsize=None)
def _pair_logits():
    x = torch.full((N_EDGE, N_EDGE), -math.inf)
    r = torch.arange(N_EDGE)
    x[r, r] = 0.0
    x[r, (r + 1) % N_EDGE] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def pair_rows(temperature: float, step: int) -> SampleProbe:
    """-inf except 0.0 at columns r and (r + 1) mod V: the token is the column with the larger
    uniform, one bit per pair of neighbouring columns of the generator; logprob = -ln 2."""
    return SampleProbe(f"pair rows, T {temperature} step {step}", _pair_logits(), None, temperature, step, 0.0, logprob=-math.log(2.0),
                       skip=True)


V_UNITS = 3 * SLICE + 5
UNITS = ("wave 2 of slice 1", "slice 1", "tail", "all but one column of the tail")


def unit_mask(unit: str, V: int = V_UNITS):
    m = torch.zeros(V, dtype=torch.bool)
    if unit == "wave 2 of slice 1":
        m[SLICE + 2048:SLICE + 3072] = True
    elif unit == "slice 1":
        m[SLICE:2 * SLICE] = True
    elif unit == "tail":
        m[3 * SLICE:] = True
    else:
        m[:] = True
        m[3 * SLICE + 2] = False
    return m


@functools.lru_cache(maxsize=None)
def masked_units(unit: str, via: str, temperature: float) -> SampleProbe:
    """3 rows of 2 randn with one unit -inf, through the suppress mask or through the logits; the
    unit's neighbours hold the row's largest logits, so a winner leaking out of or into the unit shows."""
    x = 2.0 * torch.randn((3, V_UNITS), generator=_gen(32, UNITS.index(unit)))
    m = unit_mask(unit)
    edges = [i for i in range(1, V_UNITS) if bool(m[i]) != bool(m[i - 1])]
    for j, e in enumerate(edges):
        x[:, e - 1:e + 1] += 6.0 + j
    top = float(x[:, ~m].abs().max()) if via == "mask" else None
    if via == "logits":
        x[:, m] = -math.inf
        top = float(x[torch.isfinite(x)].abs().max())
    return SampleProbe(f"masked {unit} through the {via}, T {temperature}", x, m if via == "mask" else None, temperature,
                       STEPS[1], top, skip=temperature > 0)


V_MANY = 66 * SLICE + 7
MANY_SLICES = (0, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def _many_slices_logits():
    x = 2.0 * torch.randn((5, V_MANY), generator=_gen(33))
    cols = [s * SLICE + o for s, o in zip(MANY_SLICES, (1500, 4095, 0, 4093))]
    for r, col in enumerate(cols):
        x[r, col] = 40.0
    x[4, 77], x[4, 64 * SLICE + 77] = 40.0, 40.0  # the same lane of the merge, one trip apart
    return x, cols


@functools.lru_cache(maxsize=None)
def many_slices(temperature: float) -> SampleProbe:
    """V = 66 slices and 7 columns: the merge's loops take a second trip.  Rows 0 .. 3 hold their
    largest logit (40 over 2 randn) in slice 0, 63, 64 and 65; row 4 holds it twice, in
    slice 0 and slice 64."""
    x, cols = _many_slices_logits()
    p = SampleProbe(f"66 slices, T {temperature}", x, None, temperature, STEPS[1], 40.0, skip=temperature > 0)
    p.cols = cols + [77]
    return p


# ------------------------------------------------------------------------- wx_beam_topk's probes
def _reference(x, cum, G, n):
    """The definition in fp64: the first n candidates of every chunk as (scores [B, n], index [B, n])."""
    x, cum = x.double(), cum.double()
    R, V = x.shape
    lse = torch.logsumexp(x, 1)
    score = cum[:, None] + (x - lse[:, None])
    score = torch.where((x == -math.inf) | (cum[:, None] == -math.inf), -math.inf, score)
    s, xs = score.view(R // G, G * V).numpy(), x.view(R // G, G * V).numpy()
    flat = np.arange(G * V)
    sc, idx = [], []
    for b in range(R // G):
        order = np.lexsort((flat % V, -xs[b], flat // V, -s[b]))[:n]  # score desc, g, logit desc, t
        sc.append(s[b][order])
        idx.append(order)
    return torch.from_numpy(np.stack(sc)), torch.from_numpy(np.stack(idx))


def topk_ref_err(x) -> float:
    """The top-k test's yardstick, the largest |fp32 torch.log_softmax - fp64| on these rows, over
    the finite logits of the rows that have one."""
    live = torch.isfinite(x).any(1)
    a, b = torch.log_softmax(x[live], 1).double(), torch.log_softmax(x[live].double(), 1)
    return float(torch.where(torch.isfinite(b), (a - b).abs(), torch.zeros_like(b)).max())


class TopkProbe:
    """One launch of wx_beam_topk: x [B G, V], cum [B G], G, and the conditions of the top-k test:
    the fp64 definition's gaps among its first 2G + 1 candidates exceed 8 ref_err, then equal indices
    and scores within 4 ref_err.  `runs`: (b, first, last) positions among the 2G + 1 whose scores are
    equal by construction (a tie, or -inf); there the gap is 0 or undefined, the order is `index`
    [B, 2G], stated by the probe, and the scores inside the output must be equal bit for bit."""

    def __init__(self, label, x, cum, G, index=None, runs=()):
        R, V = x.shape
        self.label, self.x, self.cum, self.G, self.V = label, x, cum, G, V
        self.B, self.K = R // G, 2 * G
        n = min(self.K + 1, G * V)
        self.want_s, self.want_i = _reference(x, cum, G, n)
        self.ref_err = topk_ref_err(x)
        with np.errstate(invalid="ignore"):
            gaps = (self.want_s[:, :-1] - self.want_s[:, 1:]).numpy().copy()
        self.runs = tuple(runs)
        for b, first, last in self.runs:
            assert 0 <= first < last <= n - 1
            inside = self.want_s[b, first:last + 1]
            assert bool((inside == inside[0]).all()), (label, b, first, last)  # equal in fp64 too
            gaps[b, first:last] = np.inf
        self.smallest_gap = float(gaps.min()) if gaps.size else math.inf
        self.index = self.want_i[:, :self.K].numpy() if index is None else np.asarray(index, dtype=np.int64)
        assert self.index.shape == (self.B, self.K)

    def conditions(self):
        """What the probe asks of its own input, on the CPU."""
        print(f"beam_topk {self.label} B {self.B} G {self.G} V {self.V}: smallest gap {self.smallest_gap:.3e}, ref_err "
              f"{self.ref_err:.3e}, 8 x ref_err {8 * self.ref_err:.3e}")
        assert self.ref_err > 0 and self.smallest_gap > 8 * self.ref_err, self.label
        assert np.array_equal(self.index, self.want_i[:, :self.K].numpy()), self.label  # the construction and the definition

    def check(self, got, label) -> float:
        """got = (scores [B, 2G], index [B, 2G]).  Names the chunk, position, beam and column of the
        first failure; prints and returns the largest |score - fp64| / (4 ref_err)."""
        self.conditions()
        s, i = (np.asarray(t.cpu().numpy() if torch.is_tensor(t) else t) for t in got)
        who = f"{label} {self.label}"
        assert s.shape == i.shape == (self.B, self.K), (who, s.shape, i.shape)
        if not np.array_equal(i, self.index):
            b, k = (int(v) for v in np.argwhere(i != self.index)[0])
            raise AssertionError(f"{who}: chunk {b} position {k}: beam {int(i[b, k]) // self.V} column {int(i[b, k]) % self.V}"
                                 f", expected beam {int(self.index[b, k]) // self.V} column {int(self.index[b, k]) % self.V}")
        want = self.want_s[:, :self.K].numpy()
        if np.isnan(s).any() or not np.array_equal(np.isfinite(s), np.isfinite(want)) or (s == np.inf).any():
            b, k = (int(v) for v in np.argwhere(np.isnan(s) | (np.isfinite(s) != np.isfinite(want)))[0])
            raise AssertionError(f"{who}: chunk {b} position {k} (beam {int(i[b, k]) // self.V} column {int(i[b, k]) % self.V}"
                                 f"): score {s[b, k]!r}, fp64 {want[b, k]!r}")
        for b, first, last in self.runs:
            inside = s[b, first:min(last + 1, self.K)].view(np.int32)
            assert (inside == inside[0]).all(), f"{who}: chunk {b} positions {first} .. {last}: the tied scores differ: {inside}"
        fin = np.isfinite(want)
        err = np.where(fin, np.abs(np.where(fin, s, 0).astype(np.float64) - np.where(fin, want, 0)), 0.0)
        bound = 4 * self.ref_err
        ratio = float(err.max()) / bound
        print(f"{who}: |score - fp64| / bound {ratio:.3f} (bound {bound:.3e})")
        if not ratio <= 1.0:
            b, k = (int(v) for v in np.argwhere(err == err.max())[0])
            raise AssertionError(f"{who}: chunk {b} position {k} (beam {int(i[b, k]) // self.V} column {int(i[b, k]) % self.V}"
                                 f"): score {float(s[b, k])!r}, fp64 {float(want[b, k])!r}: err {float(err[b, k]):.3e} > bound "
                                 f"{bound:.3e}")
        return ratio

    def emulate(self, fault=None):
        return emulate_topk(self.x, self.cum, self.G, fault)


def concentrated_sets():
    """The five column sets of the concentrated-winners probe, 16 ascending columns each."""
    g = np.random.default_rng(34)
    pick = lambda lo, hi, n: sorted(int(t) for t in g.choice(np.arange(lo, hi), n, replace=False))  # noqa: E731
    sets = {
        "one lane's 16 registers": [SLICE + 2048 + 37 + 64 * e for e in range(16)],
        "16 adjacent lanes of one register": [2 * SLICE + 1024 + 64 * 5 + 20 + i for i in range(16)],
        "16 columns of one wave": pick(3072, SLICE, 16),
        "4 per wave of one slice": sum((pick(SLICE + 1024 * w, SLICE + 1024 * (w + 1), 4) for w in range(4)), []),
        "the three slices and the tail": sum((pick(SLICE * s, SLICE * (s + 1), 4) for s in range(3)), [])
        + pick(3 * SLICE, V_UNITS, 4),
    }
    assert all(len(v) == 16 and v == sorted(v) and len(set(v)) == 16 for v in sets.values())
    return sets


@functools.lru_cache(maxsize=None)
def concentrated_winners(G: int) -> TopkProbe:
    """V = 3 slices and 5 columns, randn; chunk (set, direction) has its 2G best, 30 + j, on the first
    2G columns of the set, rising or falling with the column, in one beam (another for every chunk),
    the other beams at cum = -1000: the output is that row's 2G best."""
    K, V = 2 * G, V_UNITS
    sets = concentrated_sets()
    B = 2 * len(sets)
    x = torch.randn((B * G, V), generator=_gen(35, G))
    cum = torch.full((B * G,), -1000.0)
    index = np.zeros((B, K), dtype=np.int64)
    for b, (cols, rising) in enumerate((c, d) for c in sets.values() for d in (True, False)):
        g = b % G
        cols = cols[:K]
        vals = [30.0 + j for j in range(K)]
        for col, v in zip(cols, vals if rising else vals[::-1]):
            x[b * G + g, col] = v
        cum[b * G + g] = -0.5
        index[b] = [g * V + col for col in (cols[::-1] if rising else cols)]
    p = TopkProbe(f"concentrated winners G {G}", x, cum, G, index=index)
    p.sets = sets
    return p


def _tied_index(G, V, cols):
    """Every beam holds the same row with equal sums: the order is beam 0's tied columns ascending,
    then beam 1's, ..."""
    return [g * V + t for g in range(G) for t in cols][:2 * G]


@functools.lru_cache(maxsize=None)
def topk_constant_rows(G: int) -> TopkProbe:
    V, K = V_UNITS, 2 * G
    return TopkProbe(f"constant rows G {G}", torch.full((G, V), 1.5), torch.full((G,), -0.75), G,
                     index=[list(range(K))], runs=[(0, 0, K)])


TIE_SPANS = {"slice edge": list(range(SLICE - 6, SLICE + 6)), "wave edge": list(range(1020, 1031))}


@functools.lru_cache(maxsize=None)
def topk_equal_maxima(G: int, span: str) -> TopkProbe:
    """Every beam: the same randn row with 12.0 on 12 columns across a slice edge, or 11 across a
    wave edge, and the same sum.  All G x 12 (11) candidates tie: beam 0's by column, then beam 1's."""
    V, K, cols = V_UNITS, 2 * G, TIE_SPANS[span]
    row = torch.randn(V, generator=_gen(36, G))
    row[cols] = 12.0
    return TopkProbe(f"equal maxima at a {span} G {G}", row[None].repeat(G, 1), torch.full((G,), -0.75), G,
                     index=[_tied_index(G, V, cols)], runs=[(0, 0, min(K, G * len(cols) - 1))])


@functools.lru_cache(maxsize=None)
def topk_identical_beams(G: int) -> TopkProbe:
    """Every beam: the same 4 randn row and the same sum: each of the row's best columns ties with
    itself in every beam, and beam 0's entry comes first."""
    V, K = V_UNITS, 2 * G
    row = 4.0 * torch.randn(V, generator=_gen(37, G))
    best = torch.argsort(row, descending=True)[:K].tolist()
    index = [g * V + t for t in best for g in range(G)]
    runs = [(0, j * G, j * G + G - 1) for j in range(K // G + 1) if G > 1 and j * G + G - 1 <= K]
    return TopkProbe(f"identical beams G {G}", row[None].repeat(G, 1), torch.full((G,), -0.75), G, index=[index[:K]],
                     runs=runs)


EDGE_G = tuple(range(1, 9))


def edge_v(G: int):
    return sorted({2 * G, 2 * G + 1, 63, 64, 65, 1023, 1024, 1025, SLICE - 1, SLICE, SLICE + 1})


@functools.lru_cache(maxsize=None)
def topk_edge_v(G: int, V: int) -> TopkProbe:
    """B = 3, 4 randn rows, sums of a few steps: test_topk_against_the_fp64_definition's inputs and seed rule."""
    g = torch.Generator().manual_seed(1 + V + 10 * G)
    x = 4.0 * torch.randn((3 * G, V), generator=g)
    cum = -2.0 * torch.rand(3 * G, generator=g)
    return TopkProbe(f"edge V {V} G {G}", x, cum, G)


@functools.lru_cache(maxsize=None)
def topk_masked_units(G: int) -> TopkProbe:
    """V = 3 slices and 5 columns, G = 5 or 8.  Chunk 0: beams with wave 2 of slice 1, all of slice 1
    and the tail at -inf, a beam of only -inf with a finite sum, the others plain; the units'
    neighbours hold the rows' largest logits.  Chunk 1: beam 0 only -inf with a finite sum, beam 1 with
    three finite logits, the other beams dead (sum -inf): three finite scores, then -inf by g and t,
    which is beam 0's columns 0, 1, ..."""
    assert G >= 5
    V, K = V_UNITS, 2 * G
    x = 4.0 * torch.randn((2 * G, V), generator=_gen(38, G))
    cum = -2.0 * torch.rand(2 * G, generator=_gen(39, G))
    for g, unit in enumerate(UNITS[:3]):
        m = unit_mask(unit)
        for j, e in enumerate(i for i in range(1, V) if bool(m[i]) != bool(m[i - 1])):
            x[g, e - 1:e + 1] += 14.0 + 3.0 * g + j
        x[g, m] = -math.inf
    x[3] = -math.inf
    x[G] = -math.inf
    x[G + 1] = -math.inf
    live = [SLICE + 2500, 3 * SLICE + 4, 1023]
    x[G + 1, live] = torch.tensor([1.0, 3.0, 2.0])
    cum[G + 2:] = -math.inf
    chunk1 = [V + live[1], V + live[2], V + live[0]] + list(range(K - 3))
    p = TopkProbe(f"masked units G {G}", x, cum, G, runs=[(1, 3, K)])
    assert p.index[1].tolist() == chunk1, (p.index[1].tolist(), chunk1)  # (by construction)
    return p


MANY_KINDS = ("beam 0", "beam 1", "tie")


@functools.lru_cache(maxsize=None)
def topk_many_slices(kind: str) -> TopkProbe:
    """V = 66 slices and 7 columns, B = 1, G = 2: the live beam's four best (30 + j over randn) sit in
    slices 0, 63, 64 and 65; "tie": its two best are equal, in slice 0 and slice 64 (one lane of the
    merge, a trip apart), and the lower column comes first."""
    V = V_MANY
    x = torch.randn((2, V), generator=_gen(40))
    live = 1 if kind == "beam 1" else 0
    cols = [64 * SLICE + 77, 1500, 65 * SLICE + 3, 63 * SLICE + 4095]
    vals = [33.0, 32.0, 31.0, 30.0]
    runs = []
    if kind == "tie":
        cols, vals, runs = [77, 64 * SLICE + 77, 65 * SLICE + 3, 63 * SLICE + 4095], [33.0, 33.0, 31.0, 30.0], [(0, 0, 1)]
    x[live, cols] = torch.tensor(vals)
    cum = torch.full((2,), -1000.0)
    cum[live] = -0.5
    return TopkProbe(f"66 slices, {kind}", x, cum, 2, index=[[live * V + c for c in cols]], runs=runs)

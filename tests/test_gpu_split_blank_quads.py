"""The blank operand of the register-resident split forward (align_dp_split_kernel<1, {32, 64}, {3, 4}>),
which a DP lane keeps once per quad of four lanes: in half-chunk h lane l holds em[16 h + 4 (l & 3) .. + 3,
blank] and every step's stay add fetches its blank from the quad lane that holds it.  Everything is compared
with the CPU oracle exactly: t_start, status, spans, scores.

* Row-to-lane mapping: every T in T_MAP with every N in 1..min(T, 40), in modes 12, 13, 14 and -1, each batch
  with a pin segment that forces the <1, ., 3> or the <1, ., 4> bucket.  The blank column holds distinct
  values, a different one per row and far enough apart to decide the path.  That a mix-up of rows would be
  seen is asserted first, on the CPU (the un-marked tests need no GPU): rolling the blank column by 1, 4 and
  16 rows inside each 32-row chunk changes the oracle's own output, else the case is regenerated with the
  next seed (at most MAX_TRIES seeds; no case is dropped).  "Rolled by k" is what a kernel that is k rows
  off reads: row r of a chunk takes the value of row (r + k) % 32 of that chunk, and a row past the
  segment's end is the last row's copy (the stager clamps its loads to row T - 1).
  Two kinds of case cannot meet that condition for any input and are run on the GPU all the same:
  N = T (every frame is a change, no stay exists: the blank column is never decisive) and T = 1 (one row:
  every roll is the identity).  They are listed by `_exempt` and the CPU test asserts that nothing else is.
* Blank column anywhere: blank_id 0, 5 and V - 1 at V = 32 and V = 64, and one gathered-vocabulary batch
  (V = 300, at most 250 distinct columns per segment, blank != 0).
* Values: rows whose blank is -inf, +0, -0 or NaN, and emissions quantised to multiples of 2^-4 so that stay
  and change tie exactly (asserted on the CPU from a float32 trellis)."""
import numpy as np
import pytest
import torch

from oracle import oracle

DEV = "cuda:0"
MODES = [12, 13, 14, -1]  # split over 2 / 3 / 4 CUs; auto (small batches: 4 CUs)
T_MAP = [1, 3, 4, 5, 15, 16, 17, 20, 31, 32, 33, 36, 47, 48, 49, 63, 64, 65, 96, 97]
ROLLS = (1, 4, 16)
MAX_TRIES = 8
PER_BATCH = 62
gpu = pytest.mark.gpu

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _parts(mode):
    return {12: 2, 13: 3, 14: 4, -1: 4}[mode]


def _capacity(W, P):
    """Tokens the split bucket <1, ., W> holds over P parts: 64 + 32 (W P - 1)."""
    return 64 + 32 * (W * P - 1)


def _ref(c):
    c["ref"] = oracle.align_dp(c["em"], c["tokens"], int(c["blank"]))
    return c


def _peaky(rng, T, N, V, blank, distinct=None, quant=None):
    """test_gpu_parity's form: blank-heavy logits, the tokens' frames raised."""
    logits = rng.standard_normal((T, V)).astype(np.float32)
    logits[:, blank] += 6.0
    pool = np.array([v for v in range(V) if v != blank])
    if distinct is not None:
        pool = rng.choice(pool, size=min(distinct, len(pool)), replace=False)
    toks = pool[rng.integers(0, len(pool), N)]
    if N <= T - 2:
        fr = np.sort(rng.choice(np.arange(1, T - 1), N, replace=False))
        logits[fr, toks] += 12.0
    em = torch.log_softmax(torch.from_numpy(logits), -1).numpy()
    if quant:
        em = (np.round(em * quant) / quant).astype(np.float32)
    return {"em": np.ascontiguousarray(em), "tokens": toks.astype(np.int64), "blank": np.int64(blank)}


def _pin(V, W, P, blank=None, distinct=None):
    """The segment that pins bucket <1, ., W> in a launch of P parts: N = its capacity."""
    def make():
        rng = np.random.default_rng(1000 * V + 7 * W + P)
        cap = _capacity(W, P)
        bl = int(rng.integers(0, V)) if blank is None else blank
        return _ref(_peaky(rng, cap + 61, cap, V, bl, distinct))

    return _cached(("pin", V, W, P, blank, distinct), make)


# ------------------------------------------------------------------ row-to-lane mapping
MAP_V, MAP_BLANK = 32, 5


def _rolled(col, k):
    """The blank column as a forward that is k rows off inside every 32-row chunk reads it."""
    T = len(col)
    r = np.arange(T)
    src = (r & ~31) + ((r & 31) + k) % 32
    return col[np.minimum(src, T - 1)]


def _exempt(T, N):
    return N == T or T == 1


def _map_case(seed, T, N):
    """Every column uniform in [-3, 3); the blank column a permutation of T distinct values 6 / T apart over
    the same range, so which rows pay to stay in decides where the path stays and where it ends (with
    log-probabilities a stay never pays, column N peaks early and few blank rows decide anything)."""
    rng = np.random.default_rng(seed)
    em = 6.0 * rng.random((T, MAP_V), dtype=np.float32) - 3.0
    em[:, MAP_BLANK] = (2.95 - 6.0 * rng.permutation(T) / T).astype(np.float32)
    pool = np.array([v for v in range(MAP_V) if v != MAP_BLANK])
    toks = pool[rng.integers(0, len(pool), N)]
    return {"em": np.ascontiguousarray(em), "tokens": toks.astype(np.int64), "blank": np.int64(MAP_BLANK)}


def _same(a, b):
    return (a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
            and np.array_equal(a[4], b[4], equal_nan=True))


def _rolls_seen(c):
    """For each roll: does the oracle's output change when the blank column is rolled?"""
    seen = []
    for k in ROLLS:
        em = c["em"].copy()
        em[:, MAP_BLANK] = _rolled(c["em"][:, MAP_BLANK], k)
        seen.append(not _same(c["ref"], oracle.align_dp(em, c["tokens"], MAP_BLANK)))
    return seen


def _map_cases():
    def make():
        out = []
        for T in T_MAP:
            for N in range(1, min(T, 40) + 1):
                for attempt in range(MAX_TRIES):
                    c = _ref(_map_case(100000 * attempt + 100 * T + N, T, N))
                    c["seen"], c["tries"] = _rolls_seen(c), attempt + 1
                    if all(c["seen"]) or _exempt(T, N):
                        break
                out.append(c)
        return out

    return _cached("map", make)


def test_inputs_blank_rows_are_decisive():
    cs = _map_cases()
    assert len(cs) == sum(min(T, 40) for T in T_MAP)
    for c in cs:
        T, N = c["em"].shape[0], len(c["tokens"])
        col = c["em"][:, MAP_BLANK]
        assert len(np.unique(col)) == T
        assert c["ref"][0], (T, N)
        if not _exempt(T, N):
            assert all(c["seen"]), (T, N, c["seen"], c["tries"])
    assert sum(_exempt(c["em"].shape[0], len(c["tokens"])) for c in cs) == sum(T <= 40 for T in T_MAP)


# ------------------------------------------------------------------ blank column anywhere
ANY_SHAPES = [(33, 7), (97, 40), (160, 65), (161, 129), (353, 150)]


def _any_cases(V):
    def make():
        rng = np.random.default_rng(50 + V)
        return [_ref(_peaky(rng, T, N, V, bl)) for bl in (0, 5, V - 1) for T, N in ANY_SHAPES]

    return _cached(("any", V), make)


GATHER_V = 300


def _gather_cases():
    def make():
        rng = np.random.default_rng(77)
        shapes = [(100, 40, 30), (161, 129, 100), (353, 150, 250), (97, 33, 60), (400, 200, 250)]
        return [_ref(_peaky(rng, T, N, GATHER_V, int(rng.integers(1, GATHER_V)), distinct=d)) for T, N, d in shapes]

    return _cached("gather", make)


def test_inputs_blank_anywhere():
    for V in (32, 64):
        assert sorted({int(c["blank"]) for c in _any_cases(V)}) == [0, 5, V - 1]
    for c in _gather_cases():
        assert int(c["blank"]) != 0 and len(set(c["tokens"].tolist()) | {0, int(c["blank"])}) <= 256


# ------------------------------------------------------------------ values
def _value_cases():
    """Quantised emissions (exact ties); the blank of some rows replaced.  The rows sit in different quads,
    quad lanes and half-chunks: 10 = half 0, quad lane 2; 37 = chunk 1, half 0, lane 1; 50 = chunk 1, half 1."""
    def make():
        V, out = 32, []
        edits = {"ties": {}, "-inf": {10: -np.inf, 37: -np.inf}, "zeros": {9: 0.0, 10: -0.0, 37: -0.0, 50: 0.0},
                 "nan late": {50: np.nan}, "nan early": {3: np.nan},
                 "mixed": {2: 0.0, 7: -np.inf, 21: -0.0, 44: -np.inf, 60: np.nan}}
        for i, (name, rows) in enumerate(edits.items()):
            for j, (T, N) in enumerate(((97, 40), (65, 20), (160, 70))):
                rng = np.random.default_rng(300 + 10 * i + j)
                c = _peaky(rng, T, N, V, int(rng.integers(1, V)), quant=16)
                for r, v in rows.items():
                    c["em"][r, int(c["blank"])] = np.float32(v)
                c["name"] = name
                out.append(_ref(c))
        return out

    return _cached("values", make)


def _exact_ties(c):
    """Cells of the float32 trellis (alignment.py:359-379) at which stay and change are finite and equal."""
    em, tok, bl = c["em"], c["tokens"], int(c["blank"])
    T, N = em.shape[0], len(tok)
    prev = np.full(N + 1, -np.inf, np.float32)
    prev[0] = 0.0
    col0 = np.cumsum(em[:, 0].astype(np.float64)).astype(np.float32)
    ties = 0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            stay = prev[1:] + em[t, bl]
            chg = prev[:-1] + em[t, tok]
            ties += int(np.sum(np.isfinite(stay) & (stay == chg)))
            cur = np.empty_like(prev)
            cur[1:] = np.where(np.isnan(stay) | np.isnan(chg), np.float32(np.nan), np.maximum(stay, chg))
            cur[0] = np.inf if t + 1 >= T + 1 - N else col0[t]
            prev = cur
    return ties


def test_inputs_values():
    cs = _value_cases()
    names = {c["name"] for c in cs}
    assert names == {"ties", "-inf", "zeros", "nan late", "nan early", "mixed"}
    for c in cs:
        assert np.array_equal(c["em"][np.isfinite(c["em"])] * 16.0, np.round(c["em"][np.isfinite(c["em"])] * 16.0))
        col = c["em"][:, int(c["blank"])]
        if c["name"] == "ties":
            assert c["ref"][0] and _exact_ties(c) > 0
        if c["name"] in ("-inf", "mixed"):
            assert np.isneginf(col).sum() == 2
        if c["name"] in ("zeros", "mixed"):
            assert (np.signbit(col) & (col == 0)).any() and (~np.signbit(col) & (col == 0)).any()
        if c["name"].startswith("nan") or c["name"] == "mixed":
            assert np.isnan(col).sum() == 1
    assert any(c["ref"][0] for c in cs if c["name"] == "-inf") and any(c["ref"][0] for c in cs if c["name"] == "zeros")


# ------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from whisperx_amd import _lib

    _lib.load()
    return _lib


def _dev(c):
    if "dev" not in c:
        c["dev"] = torch.from_numpy(c["em"]).to(DEV)
    return c["dev"]


def _compare(lib, out, b, cases, tag):
    """Every segment against its oracle result; all differing segments are reported together."""
    ss, se, sc, ts, st = out
    bad = []
    for s, c in enumerate(cases):
        ok, tso, sso, seo, sco = c["ref"]
        T, N = c["em"].shape[0], len(c["tokens"])
        if ts[s] != tso:
            bad.append(f"seg {s} (T {T}, N {N}): t_start {ts[s]} vs {tso}")
        elif (int(st[s]) & lib.STATUS_MASK) != (0 if ok else 1):
            bad.append(f"seg {s} (T {T}, N {N}): status {st[s]}")
        elif ok:
            a, e = b.tok_off[s], b.tok_off[s + 1]
            if not (np.array_equal(ss[a:e], sso) and np.array_equal(se[a:e], seo)):
                bad.append(f"seg {s} (T {T}, N {N}): spans")
            elif not np.array_equal(sc[a:e], sco, equal_nan=True):
                bad.append(f"seg {s} (T {T}, N {N}): scores")
    assert not bad, f"{tag}: " + "; ".join(bad)


def _check(lib, cases, V, VS, W, mode, tag):
    assert len(cases) <= 64
    b = lib.Batch([_dev(c) for c in cases], [c["tokens"].tolist() for c in cases], [int(c["blank"]) for c in cases],
                  device=DEV)
    names = lib.align_dp_plan(b.S, b.min_N, b.max_N, V, mode)
    assert any(f"align_dp_split_kernel<1, {VS}, {W}>" in k for k in names), names
    out = tuple(x.cpu().numpy() for x in lib.align_dp(b, mode=mode))
    _compare(lib, out, b, cases, f"{tag}, mode {mode}, W {W}")
    assert not ((out[4][: b.S] & lib.STATUS_RECOVERED) != 0).any(), tag


@gpu
@pytest.mark.parametrize("W", [3, 4])
@pytest.mark.parametrize("mode", MODES)
def test_blank_row_to_lane_mapping(lib, mode, W):
    cs = _map_cases()
    pin = _pin(MAP_V, W, _parts(mode))
    for i in range(0, len(cs), PER_BATCH):
        _check(lib, cs[i:i + PER_BATCH] + [pin], MAP_V, 32, W, mode, f"mapping batch {i // PER_BATCH}")


@gpu
@pytest.mark.parametrize("W", [3, 4])
@pytest.mark.parametrize("V", [32, 64])
@pytest.mark.parametrize("mode", MODES)
def test_blank_column_anywhere(lib, mode, V, W):
    for bl in (0, 5, V - 1):  # (the pin's blank too)
        _check(lib, _any_cases(V) + [_pin(V, W, _parts(mode), blank=bl)], V, V, W, mode, f"V {V}, pin blank {bl}")


@gpu
@pytest.mark.parametrize("W", [3, 4])
def test_blank_column_gathered_vocabulary(lib, W):
    pin = _pin(GATHER_V, W, 4, blank=17, distinct=250)
    _check(lib, _gather_cases() + [pin], GATHER_V, 256, W, 14, "gathered vocabulary")


@gpu
@pytest.mark.parametrize("W", [3, 4])
@pytest.mark.parametrize("mode", MODES)
def test_blank_values(lib, mode, W):
    _check(lib, _value_cases() + [_pin(32, W, _parts(mode))], 32, 32, W, mode, "blank values")


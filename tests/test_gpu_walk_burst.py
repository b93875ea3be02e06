"""The backtrack walk of the write-through split kernels (align_dp_split_kernel<1, 32, W>), through
the C ABI against the CPU oracle: t_start, status and spans equal, scores bit-equal.

The inputs are chosen so that a walk which fetches the wrong decision words — a window that does
not reach the far edge of the cells a path can occupy, a prefetch that stops at a cap, a window
issued from a column the walk never stands on, rows left in LDS by an earlier launch — returns
another path.  Each property the GPU tests rely on is asserted first, on the CPU, from the oracle's
spans (the un-marked tests below run without a GPU):

* far edge: N tokens emitted in N consecutive frames (the run at the start, in the middle and at
  the end of the segment), so some 32-frame block of the path holds 32 changes, and (run at the
  start or the end) the path is at least 128 columns from the straight line (0, 0)-(T, N) at a block
  boundary: a window centred on a straight-line guess misses it.  A run in the middle cannot be
  128 columns off the line within the bucket's capacity (N (T - N) / 2T < 128); it is kept for its
  32-change blocks.  N = T and N = T - 1 at T = 1499 and T = 640 exceed the <1, 32, W> capacity
  (544 tokens over four parts), so they run in a batch of their own through whichever split kernel
  the launch picks;
* cap boundary: T = 32 nb - 7 for every nb in 40..80 in one batch (walkers of 8 to 13 blocks each),
  and a batch of nb <= 12 with fewer than eight walkers, a lone walker and T = 1, 31, 32, 33, 100;
* early t_start: t_start below wave 0's segment (lo(0) restated from walk_spec), and inside
  wave 0's segment but below its top block;
* failure and ties: N > T (the reference's None), emissions quantised to multiples of 2^-4 with
  exact ties, a NaN next to column N;
* the arrival arms on the far-edge batch: fenced, spread over XCDs, and the recovery path three
  times on one plan.

The same shapes drive the walkers' guessed start columns into every clamp and both signs of their
offset from the straight line (N below and above T / 2, N = T, N > T).

The longest segment of a batch pins the launch's split bucket; batches have at most 64 segments
plus the pin so that every mode really splits.  N >= 2 throughout."""
import numpy as np
import pytest
import torch

from oracle import oracle

DEV = "cuda:0"
MODES = [12, 13, 14, -1]  # split over 2 / 3 / 4 CUs; auto (small batches: 4 CUs)
V = 32
W = 4
gpu = pytest.mark.gpu


def _parts(mode):
    return {12: 2, 13: 3, 14: 4, -1: 4}[mode]


def _capacity(P):
    """Tokens the split bucket <1, 32, W> holds over P parts: 64 + 32 (W P - 1)."""
    return 64 + 32 * (W * P - 1)


def _lo0(T):
    """Lowest block of wave 0's walk segment: walk_spec's formula (eight waves per split workgroup,
    kSpecMinBlocks = 4, kSpecArgmaxBlocks = 3)."""
    top = (T - 1) >> 5
    nb = top + 1
    K = max(1, min(8, nb // 4))
    L0 = max((nb + 3 + K // 2) // K - 3, 1)
    if K > 1 and nb - L0 < K - 1:
        K = max(nb - L0 + 1, 1)
    return 0 if (K <= 1 or L0 >= nb) else top - L0 + 1


def _walker_blocks(T):
    """Blocks of the longest first walk of a walker wave >= 1 (T >= 1024: eight walkers): its
    segment plus the kSpecOverlap = 2 blocks it starts above it."""
    nb = ((T - 1) >> 5) + 1
    L0 = max((nb + 3 + 4) // 8 - 3, 1)
    return (nb - L0 + 6) // 7 + 2


def _segment(seed, T, N, frames=None, boost_until=None, edit=None):
    """One segment: noise, the blank raised by 6 (up to row boost_until), token k raised by 12 at
    frames[k] (default: N random frames)."""
    rng = np.random.default_rng(seed)
    bl = int(rng.integers(0, V))
    logits = rng.standard_normal((T, V)).astype(np.float32)
    logits[: (T if boost_until is None else boost_until), bl] += 6.0
    nb = np.array([v for v in range(V) if v != bl])
    toks = nb[rng.integers(0, len(nb), N)]
    if frames is None and N <= T - 2:
        frames = np.sort(rng.choice(np.arange(1, T - 1), N, replace=False))
    if frames is not None:
        logits[np.asarray(frames), toks] += 12.0
    em = torch.log_softmax(torch.from_numpy(logits), -1).numpy()
    if edit == "quant":  # multiples of 2^-4: sums are exact, equal path scores tie exactly
        em = (np.round(em * 16.0) / 16.0).astype(np.float32)
    elif edit == "nan":  # column N is NaN from row T - 3 on: the first NaN is the arg-max
        em[T - 4, int(toks[-1])] = np.nan
    c = {"em": np.ascontiguousarray(em), "tokens": toks.astype(np.int64), "blank": np.int64(bl)}
    c["ref"] = oracle.align_dp(c["em"], c["tokens"], int(c["blank"]))
    return c


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _pin(P):
    cap = _capacity(P)
    return _cached(("pin", P), lambda: _segment(9000 + P, cap + 61, cap))


def _run_of(T, N, where):
    r0 = {"start": 0, "middle": (T - N) // 2, "end": T - N}[where]
    return r0 + np.arange(N)


def _far_edge(P):
    """(segment, placement) pairs: N consecutive frames, N = capacity - 8 at T = 1499 and at most
    T / 2 at T = 640 (a run at an end is N (T - N) / T columns off the line: 160 at N = T / 2)."""
    def make():
        return [(_segment(100 * T + i, T, N, _run_of(T, N, w)), w)
                for T, N in ((1499, _capacity(P) - 8), (640, min(_capacity(P) - 8, 320)))
                for i, w in enumerate(("start", "middle", "end"))]

    return _cached(("far", P), make)


def _far_edge_full():
    return _cached("full", lambda: [_segment(7 * T + N, T, N, _run_of(T, N, "start")) for T in (1499, 640) for N in (T, T - 1)])


def _cap_boundary(P):
    cap = _capacity(P)
    return _cached(("cap", P), lambda: [_segment(32 * nb, 32 * nb - 7, min(int((32 * nb - 7) / 3.6), cap))
                                        for nb in range(40, 81)])


def _short(P):
    cap = _capacity(P)

    def make():
        cs = [_segment(500 + nb, 32 * nb - 7, max(2, min(int((32 * nb - 7) / 3.6), cap))) for nb in range(1, 13)]
        cs += [_segment(600 + T, T, max(2, T // 4)) for T in (31, 32, 33, 100)]
        cs += [_segment(601, 1, 2)]  # T = 1 (N >= 2: the reference's None)
        return cs

    return _cached(("short", P), make)


def _early():
    """t_start below wave 0's segment (tokens in the first fifth, flat noise after it), and inside
    wave 0's segment below its top block."""
    def make():
        T, out = 1499, []
        for i, N in enumerate((200, 280)):
            fr = np.sort(np.random.default_rng(40 + i).choice(np.arange(1, T // 5), N, replace=False))
            out.append(_segment(700 + i, T, N, fr, boost_until=T // 5))
        fr = np.sort(np.random.default_rng(50).choice(np.arange(1, 1425), 249, replace=False))
        out.append(_segment(710, T, 250, np.append(fr, 1425), boost_until=1426))
        return out

    return _cached("early", make)


def _failure_and_ties():
    def make():
        cs = [_segment(800, 40, 41), _segment(801, 100, 250), _segment(802, 2, 3)]  # N > T
        cs += [_segment(810 + i, T, N, edit="quant") for i, (T, N) in enumerate(((1499, 280), (640, 200), (333, 150)))]
        cs += [_segment(820 + i, T, N, edit="nan") for i, (T, N) in enumerate(((1499, 280), (205, 120)))]
        return cs

    return _cached("fail", make)


def _changes_per_block(c):
    ss = np.asarray(c["ref"][2])
    return np.bincount(ss >> 5, minlength=((c["em"].shape[0] - 1) >> 5) + 1)


def _max_off_line(c):
    """Largest distance, over block boundaries t = 32 b, between the path's column (tokens started
    before t) and the straight line N t / T."""
    T, N = c["em"].shape[0], len(c["tokens"])
    ss = np.asarray(c["ref"][2])
    t = np.arange(0, T + 1, 32)
    return float(np.abs(np.searchsorted(ss, t, "left") - N * t / T).max())


# ------------------------------------------------------------------ input properties (CPU)
@pytest.mark.parametrize("P", [2, 3, 4])
def test_inputs_far_edge(P):
    for c, where in _far_edge(P):
        assert c["ref"][0]
        assert _changes_per_block(c).max() == 32, where
        if where != "middle":
            assert _max_off_line(c) >= 128, (where, _max_off_line(c))
    for c in _far_edge_full():
        assert c["ref"][0] and _changes_per_block(c).max() == 32 and len(c["tokens"]) >= 2


def test_inputs_cap_boundary():
    for P in (2, 3, 4):
        cs = _cap_boundary(P)
        assert len(cs) == 41 and all(c["ref"][0] for c in cs)
        # blocks per walker (its segment + kSpecOverlap = 2) run from 8 to 13 over the batch:
        # whatever the burst cap is, both sides of it are taken
        per = sorted({_walker_blocks(c["em"].shape[0]) for c in cs})
        assert per[0] <= 8 and per[-1] >= 13, per
        sh = _short(P)
        assert {c["em"].shape[0] for c in sh} >= {1, 31, 32, 33, 100}
        assert all(len(c["tokens"]) >= 2 for c in cs + sh)
        nbs = [((c["em"].shape[0] - 1) >> 5) + 1 for c in sh]
        assert min(nbs) // 4 <= 1 and any(2 <= n // 4 < 8 for n in nbs)  # a lone walker, and 2..7 walkers


def test_inputs_early_t_start():
    a, b, c = _early()
    for x in (a, b):
        T = x["em"].shape[0]
        assert x["ref"][0] and x["ref"][1] < 32 * _lo0(T), (x["ref"][1], _lo0(T))
    T = c["em"].shape[0]
    tb = (c["ref"][1] - 1) >> 5
    assert c["ref"][0] and _lo0(T) <= tb < (T - 1) >> 5, (c["ref"][1], _lo0(T))


def test_inputs_failure_and_ties():
    cs = _failure_and_ties()
    assert [c["ref"][0] for c in cs[:3]] == [False] * 3
    for c in cs[3:6]:
        assert c["ref"][0] and np.array_equal(c["em"] * 16.0, np.round(c["em"] * 16.0))
    for c in cs[6:]:
        T = c["em"].shape[0]
        assert np.isnan(c["em"][T - 4, int(c["tokens"][-1])])


# ------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from whisperx_amd import _lib

    _lib.load()
    return _lib


def _batch(lib, cases):
    ems = [torch.from_numpy(c["em"]).to(DEV) for c in cases]
    return lib.Batch(ems, [c["tokens"].tolist() for c in cases], [int(c["blank"]) for c in cases], device=DEV)


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


def _check(lib, cases, mode, tag, pinned=True):
    if pinned:
        cases = cases + [_pin(_parts(mode))]
    assert len(cases) <= 65
    b = _batch(lib, cases)
    names = lib.align_dp_plan(b.S, b.min_N, b.max_N, V, mode)
    want = f"align_dp_split_kernel<1, 32, {W}>" if pinned else "align_dp_split_kernel<"
    assert any(want in k for k in names), names
    out = tuple(x.cpu().numpy() for x in lib.align_dp(b, mode=mode))
    _compare(lib, out, b, cases, f"{tag}, mode {mode}")
    return b, cases


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_far_edge_of_the_triangle(lib, mode):
    _check(lib, [c for c, _ in _far_edge(_parts(mode))], mode, "far edge")


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_far_edge_every_frame_a_token(lib, mode):
    _check(lib, _far_edge_full(), mode, "N = T, N = T - 1", pinned=False)


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_cap_boundary(lib, mode):
    _check(lib, _cap_boundary(_parts(mode)), mode, "T = 32 nb - 7, nb 40..80")
    _check(lib, _short(_parts(mode)), mode, "nb <= 12")


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_early_t_start(lib, mode):
    _check(lib, _early(), mode, "early t_start")


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_failure_and_ties(lib, mode):
    _check(lib, _failure_and_ties(), mode, "failure and ties")


@gpu
def test_arrival_arms(lib, monkeypatch):
    """The far-edge batch with the fenced arrival, with the parts spread over XCDs, and on the
    recovery path (the walk then follows generic_forward, which used the same LDS) three times on
    one plan: a row left in LDS by the launch before must not be read."""
    cases = [c for c, _ in _far_edge(4)] + [_pin(4)]
    b = _batch(lib, cases)
    assert any(f"align_dp_split_kernel<1, 32, {W}>" in k for k in lib.align_dp_plan(b.S, b.min_N, b.max_N, V, 14))
    for env in ("WX_SPLIT_FENCED", "WX_SPLIT_XCD_SPREAD"):
        monkeypatch.setenv(env, "1")
        out = tuple(x.cpu().numpy() for x in lib.align_dp(b, mode=14))
        monkeypatch.delenv(env)
        _compare(lib, out, b, cases, env)
        assert not ((out[4][: b.S] & lib.STATUS_RECOVERED) != 0).any(), env
    monkeypatch.setenv("WX_SPIN_LIMIT", "0")
    plan = lib.AlignPlan(b, mode=14)
    for i in range(3):
        out = tuple(x.cpu().numpy() for x in plan.run())
        _compare(lib, out, b, cases, f"recovery path, launch {i + 1}")
        assert ((out[4][: b.S] & lib.STATUS_RECOVERED) != 0).all(), "every segment spans more than one part"
    monkeypatch.delenv("WX_SPIN_LIMIT")

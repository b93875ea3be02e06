"""The column-N history stores, the chunk boundary and the arrival of the split forward, through
the C ABI against the CPU oracle: spans and t_start equal, scores bit-equal, status equal.

t_start is the arg-max of the stored column-N history, so comparing it with the oracle checks the
owner lane's stores directly.  What the shapes cover:

* the owner of column N in every wave of every part: N at each wave's first, second and last
  column (64 + 32 k - 1, 64 + 32 k, 64 + 32 k + 1) up to the launched bucket's capacity, with a
  partial last chunk whose rows past T land in the history's padding (T = N + 5), with N = T,
  and with T a whole number of chunks;
* all four alignments of a segment's history base, with a NaN and a -inf next to column N
  (first-NaN / first-maximum arg-max);
* the other forwards that store the history sixteen bytes at a time: the <2, 64, 3> split kernel
  and a single-CU latency bucket;
* the arrival: fenced, spread over XCDs, on the recovery path, and twice on one plan.

The longest segment of a batch pins the launch's split bucket (one pin segment per batch), and
batches have at most 64 segments so that every mode really splits."""
import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = [12, 13, 14, -1]  # split over 2 / 3 / 4 CUs; auto (small batches: 4 CUs)


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from whisperx_amd import _lib

    _lib.load()


def _parts(mode):
    return {12: 2, 13: 3, 14: 4, -1: 4}[mode]


def _capacity(W, P):
    """Tokens the split bucket <1, ., W> holds over P parts: 64 + 32 (W P - 1)."""
    return 64 + 32 * (W * P - 1)


def _make(rng, T, N, V):
    """One segment: blank-heavy logits, the tokens' frames raised."""
    bl = int(rng.integers(0, V))
    logits = rng.standard_normal((T, V)).astype(np.float32)
    logits[:, bl] += 6.0
    nb = np.array([v for v in range(V) if v != bl])
    toks = nb[rng.integers(0, len(nb), N)]
    if N <= T - 2:
        fr = np.sort(rng.choice(np.arange(1, T - 1), N, replace=False))
        logits[fr, toks] += 12.0
    em = torch.log_softmax(torch.from_numpy(logits), -1).numpy()
    return {"em": np.ascontiguousarray(em), "tokens": toks.astype(np.int64), "blank": np.int64(bl)}


def _with_oracle(c):
    if "ref" not in c:
        c["ref"] = oracle.align_dp(c["em"], c["tokens"], int(c["blank"]))
    return c


_CASES = {}


def _case(T, N, V=32, edit=None):
    """The segment of a shape (and edit), made and run through the oracle once per session."""
    key = (T, N, V, edit)
    if key not in _CASES:
        c = _make(np.random.default_rng(100003 * T + 101 * N + V), T, N, V)
        last = int(c["tokens"][-1])
        if edit == "nan":  # column N is NaN from row T - 3 on: the first NaN is the arg-max
            c["em"][T - 4, last] = np.nan
        elif edit == "ninf":  # column N falls to -inf and recovers: the first maximum after it
            c["em"][T - 6, last] = -np.inf
            c["em"][T - 6, int(c["blank"])] = -np.inf
        _CASES[key] = _with_oracle(c)
    return _CASES[key]


def _batch(cases):
    from whisperx_amd import _lib

    ems = [torch.from_numpy(c["em"]).to(DEV) for c in cases]
    return _lib.Batch(ems, [c["tokens"].tolist() for c in cases], [int(c["blank"]) for c in cases], device=DEV)


def _compare(out, b, cases, tag):
    """Every segment against its oracle result; all differing segments are reported together."""
    from whisperx_amd import _lib

    ss, se, sc, ts, st = out
    bad = []
    for s, c in enumerate(cases):
        ok, tso, sso, seo, sco = c["ref"]
        T, N = c["em"].shape[0], len(c["tokens"])
        if ts[s] != tso:
            bad.append(f"seg {s} (T {T}, N {N}): t_start {ts[s]} vs {tso}")
        elif (int(st[s]) & _lib.STATUS_MASK) != (0 if ok else 1):
            bad.append(f"seg {s} (T {T}, N {N}): status {st[s]}")
        elif ok:
            a, e = b.tok_off[s], b.tok_off[s + 1]
            if not (np.array_equal(ss[a:e], sso) and np.array_equal(se[a:e], seo)):
                bad.append(f"seg {s} (T {T}, N {N}): spans")
            elif not np.array_equal(sc[a:e], sco, equal_nan=True):
                bad.append(f"seg {s} (T {T}, N {N}): scores")
    assert not bad, f"{tag}: " + "; ".join(bad)


def _run(b, mode):
    from whisperx_amd import _lib

    return tuple(x.cpu().numpy() for x in _lib.align_dp(b, mode=mode))


def _launches(b, mode, V):
    from whisperx_amd import _lib

    return _lib.align_dp_plan(b.S, b.min_N, b.max_N, V, mode)


def _owner_ns(cap):
    """Column N in every wave of every part: the waves' first, second and last columns."""
    ns = [1, 2, 63, 64, 65] + [64 + 32 * k + d for k in range(1, 16) for d in (-1, 0, 1)]
    return sorted({min(n, cap) for n in ns})


def _pin(W, P):
    cap = _capacity(W, P)
    return _case(cap + 61, cap)


@pytest.mark.parametrize("shape", ["partial", "exact"])
@pytest.mark.parametrize("W", [3, 4])
@pytest.mark.parametrize("mode", MODES)
def test_owner_in_every_wave_of_every_part(mode, W, shape):
    P = _parts(mode)
    ns = _owner_ns(_capacity(W, P))
    if shape == "partial":  # a partial last chunk: rows past T land in the padding
        cases = [_case(n + 5, n) for n in ns]
    else:  # N = T, and whole chunks with N = T - 1
        cases = [_case(n, n) for n in ns] + [_case(t, t - 1) for t in (32, 64, 96)]
    cases = cases + [_pin(W, P)]
    assert len(cases) <= 64
    b = _batch(cases)
    assert any(f"align_dp_split_kernel<1, 32, {W}>" in k for k in _launches(b, mode, 32)), _launches(b, mode, 32)
    _compare(_run(b, mode), b, cases, f"owner sweep, {shape}, mode {mode} W {W}")


@pytest.mark.parametrize("mode", MODES)
def test_history_base_alignments_nan_and_inf(mode):
    """A segment's history starts at (row0 + 40 s) rounded down to 16 bytes: lengths of 1 mod 4 put
    row0 mod 4 at 0, 1, 2, 3 in turn; every alignment gets a plain segment, one whose column N
    turns NaN and one whose column N passes through -inf."""
    P = _parts(mode)
    cases = []
    for i in range(12):
        T = 101 + 4 * (5 * i % 12)  # (1 mod 4; partial last chunks of several lengths)
        cases.append(_case(T, T - 9 - i, 32, [None, "nan", "ninf"][i // 4]))
    cases = cases + [_pin(4, P)]
    b = _batch(cases)
    assert {b.em_off[s] % 4 for s in range(4)} == {0, 1, 2, 3}
    assert all(b.em_off[s] % 4 == s % 4 for s in range(12))
    _compare(_run(b, mode), b, cases, f"history alignments, mode {mode}")


def test_two_cells_per_lane_split_kernel():
    """The <2, 64, 3> split kernel (V = 40, two parts): N around 230, pinned by a longer segment."""
    cases = [_case(n + 5, n, 40) for n in (226, 229, 230, 231)] + [_case(263, 230, 40), _case(345, 300, 40)]
    b = _batch(cases)
    assert any("align_dp_split_kernel<2, 64, 3>" in k for k in _launches(b, 12, 40)), _launches(b, 12, 40)
    _compare(_run(b, 12), b, cases, "<2, 64, 3> over two parts")


def test_single_cu_latency_bucket():
    """A single-CU latency bucket (WX_MODE_LATENCY): N around 100."""
    from whisperx_amd import _lib

    cases = [_case(n + 5, n) for n in (97, 100, 101, 127)] + [_case(128, 100), _case(100, 100)]
    b = _batch(cases)
    assert any("align_dp_kernel<1, 32, 3, 1>" in k for k in _launches(b, _lib.MODE_LATENCY, 32))
    _compare(_run(b, _lib.MODE_LATENCY), b, cases, "latency bucket <1, 32, 3, 1>")


def _arrival_cases():
    # (segments of one part only: N <= 160 in <1, 32, 4>; the others span two to four parts)
    return [_case(n + 5, n) for n in (33, 100, 300, 301, 420, 500)] + [_case(t, t - 1) for t in (64, 96)] + [_pin(4, 4)]


def test_arrival_arms(monkeypatch):
    """The same small batch with the fenced arrival, with the parts spread over XCDs and on the
    recovery path (no consumer waits: the last part to arrive recomputes the segment): results
    equal the oracle, and WX_STATUS_RECOVERED is set in the recovery arm only — there on every
    segment that spans more than one part, on no other."""
    from whisperx_amd import _lib

    cases = _arrival_cases()
    b = _batch(cases)
    spans_parts = np.array([len(c["tokens"]) > 64 + 32 * 3 for c in cases])
    for env, lost in (("WX_SPLIT_FENCED", False), ("WX_SPLIT_XCD_SPREAD", False), ("WX_SPIN_LIMIT", True)):
        monkeypatch.setenv(env, "0" if env == "WX_SPIN_LIMIT" else "1")
        out = _run(b, 14)
        monkeypatch.delenv(env)
        _compare(out, b, cases, env)
        rec = (out[4][: b.S] & _lib.STATUS_RECOVERED) != 0
        assert np.array_equal(rec, spans_parts if lost else np.zeros(b.S, bool)), f"{env}: recovered {rec}"


def test_arrival_counter_reused_after_reset():
    """Two launches back to back on one plan: the second arrives at the counters the first reset."""
    from whisperx_amd import _lib

    cases = _arrival_cases()
    b = _batch(cases)
    plan = _lib.AlignPlan(b, mode=14)
    for i in range(2):
        plan.run()
    out = tuple(x.cpu().numpy() for x in plan.outs)
    _compare(out, b, cases, "second launch of the plan")
    assert not ((out[4][: b.S] & _lib.STATUS_RECOVERED) != 0).any()
    out = tuple(x.cpu().numpy() for x in plan.run())
    _compare(out, b, cases, "third launch of the plan")

"""The register-resident split forward (align_dp_split_kernel<1, {32, 64}, {3, 4}>) at the
smallest shapes at which its chunk protocol can go wrong, against the CPU oracle: spans and
t_start equal, scores bit-equal, status equal.

What the shapes cover: chunk counts around one, two and three chunks and around the quad-buffer
ring (five buffers: T = 159, 160, 161 and 353), partial last chunks, waves and parts with and
without columns (N around every multiple of 32 up to 161 and at the launched bucket's
capacity), both stagers (V = 32 with 16-byte rows: registers; V = 29: the LDS-DMA ring; V = 40:
64-float rows), exact ties, and a column 0 with -inf, NaN and mixed signs (the column-0 helper's
fp64 chain).  The longest segment of a batch pins the launch's split bucket, so every batch
carries one pin segment; batches have at most 64 segments so that every mode really splits.

Every segment but the pins has N <= 161, below the smallest capacity used (224: <1, ., 3> over
two parts): a longer one would move the launch to another split bucket (max N picks it) and
the short segments to other kernels, which is not what this file is about."""
import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = [12, 13, 14, -1]  # split over 2 / 3 / 4 CUs; auto (small batches: 4 CUs)
RING = 5  # quad buffers of the register-resident forward (Forward::kBufs)
T_SWEEP = [1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 32 * RING - 1, 32 * RING, 32 * RING + 1, 64 * RING + 33, 1499, 1500]
N_SWEEP = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161]
KINDS = {"v32": (32, None), "v32q16": (32, 16), "v29": (29, None), "v40": (40, None)}


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


def _case(rng, T, N, V, quant=None):
    """One segment in test_gpu_parity's peaky form: blank-heavy logits, the tokens' frames raised."""
    bl = int(rng.integers(0, V))
    logits = rng.standard_normal((T, V)).astype(np.float32)
    logits[:, bl] += 6.0
    nb = np.array([v for v in range(V) if v != bl])
    toks = nb[rng.integers(0, len(nb), N)]
    if N <= T - 2:
        fr = np.sort(rng.choice(np.arange(1, T - 1), N, replace=False))
        logits[fr, toks] += 12.0
    em = torch.log_softmax(torch.from_numpy(logits), -1).numpy()
    if quant:
        em = (np.round(em * quant) / quant).astype(np.float32)
    return {"em": np.ascontiguousarray(em), "tokens": toks.astype(np.int64), "blank": np.int64(bl)}


def _with_oracle(c):
    if "ref" not in c:
        c["ref"] = oracle.align_dp(c["em"], c["tokens"], int(c["blank"]))
    return c


_SWEEPS = {}


def _sweep(kind):
    """The shape sweep of one (V, quantisation): built once, oracle results kept with the cases."""
    if kind not in _SWEEPS:
        V, quant = KINDS[kind]
        rng = np.random.default_rng(1000 + sorted(KINDS).index(kind))
        shapes = [(T, min(max(1, T // 2), 140)) for T in T_SWEEP]  # (N below every pin)
        shapes += [(N + 37, N) for N in N_SWEEP]
        shapes += [(64, 64), (33, 33)]  # N = T
        shapes += [(20, 40), (5, 9)]    # N > T: no path (status 1), neighbours unaffected
        cases = [_case(rng, T, N, V, quant) for T, N in shapes]
        # column 0 with a -inf row, a NaN row and mixed signs (T = 97: three full chunks and one row)
        c = _case(rng, 97, 40, V, quant)
        c["em"][::3, 0] = np.abs(c["em"][::3, 0])
        c["em"][10, 0] = -np.inf
        c["em"][50, 0] = np.nan
        cases.append(c)
        _SWEEPS[kind] = [_with_oracle(x) for x in cases]
    return _SWEEPS[kind]


_PINS = {}


def _pin(kind, W, P):
    """The segments that pin bucket <1, ., W> in a launch of P parts: capacity - 1 and capacity."""
    key = (kind, W, P)
    if key not in _PINS:
        V, quant = KINDS[kind]
        rng = np.random.default_rng(7 * W + P)
        cap = _capacity(W, P)
        _PINS[key] = [_with_oracle(_case(rng, cap + 40, cap - 1, V, quant)),
                      _with_oracle(_case(rng, cap + 61, cap, V, quant))]
    return _PINS[key]


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


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("W", [3, 4])
@pytest.mark.parametrize("mode", MODES)
def test_split_small_shapes_vs_oracle(mode, W, kind):
    cases = _sweep(kind) + _pin(kind, W, _parts(mode))
    assert len(cases) <= 64
    b = _batch(cases)
    _compare(_run(b, mode), b, cases, f"{kind} mode {mode} W {W}")


def test_split_plan_rerun_then_other_batch_then_first_again():
    """LDS and the hand-off region are not cleared between launches: one plan run four times
    back to back, then a batch of other shapes, then the first plan again — every result equals
    the oracle (nothing a launch left behind is taken for this launch's)."""
    from whisperx_amd import _lib

    first = _sweep("v32") + _pin("v32", 4, 4)
    other = _sweep("v29")[5:30] + _pin("v29", 3, 4)
    ba, bb = _batch(first), _batch(other)
    plan = _lib.AlignPlan(ba, mode=14)
    for i in range(4):
        out = tuple(x.cpu().numpy() for x in plan.run())
        _compare(out, ba, first, f"plan run {i}")
    _compare(_run(bb, 14), bb, other, "other batch")
    out = tuple(x.cpu().numpy() for x in plan.run())
    _compare(out, ba, first, "plan run after the other batch")


def test_split_small_shapes_identical_across_arrival_arms(monkeypatch):
    """WX_SPLIT_FENCED x WX_SPLIT_XCD_SPREAD (fence-free or fenced arrival, the parts of a
    segment on one XCD or spread over several): identical outputs at the small shapes."""
    cases = _sweep("v32") + _pin("v32", 4, 4)
    b = _batch(cases)
    ref = None
    for fenced in ("0", "1"):
        for spread in ("0", "1"):
            monkeypatch.setenv("WX_SPLIT_FENCED", fenced)
            monkeypatch.setenv("WX_SPLIT_XCD_SPREAD", spread)
            out = _run(b, 14)
            _compare(out, b, cases, f"fenced {fenced} spread {spread}")
            # (the per-token entries of a segment that did not align are not defined by the ABI)
            ss, se, sc, ts, st = out
            sig = [ts[: b.S].tobytes(), (st[: b.S] & 15).tobytes()]
            for s, c in enumerate(cases):
                if c["ref"][0]:
                    a, e = b.tok_off[s], b.tok_off[s + 1]
                    sig += [ss[a:e].tobytes(), se[a:e].tobytes(), sc[a:e].tobytes()]
            if ref is None:
                ref = sig
            else:
                assert sig == ref, f"fenced {fenced} spread {spread}: differs from the unfenced same-XCD launch"

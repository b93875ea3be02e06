"""Shared by the tests of wx_penalize_logits: an fp32 numpy evaluation of the definition in
include/wx_align.h, written from the header and independent of the package's code; an emulation of
the kernel's phases (ids narrowed into a table, a ban flag per position, one owner per distinct id
and one store) that can be run with one fault at a time; and the probes, the smallest inputs at
which each fault, and each boundary of the definition, shows.

A probe's logits are a [R, stride] fp32 array with stride = V + PAD: the columns [V, stride) must
come back untouched.  Its history is [R, cap] int64, entry [r, i] = h_i of row r, with cap > L
wherever L < MAX_HISTORY: the entries from L on are in-range ids that no correct evaluation reads.
Everything is exact: the definition names one fp32 multiplication or one correctly rounded fp32
division per column, which numpy's float32 scalars perform, so results are compared bit for bit.
"""
from typing import NamedTuple

import numpy as np

MAX_HISTORY = 1024  # WX_PENALTY_MAX_HISTORY
PAD = 3
GUARD = 8  # floats around the emulation's flat buffer
FAULTS = ("per_occurrence", "no_prefix", "j_short", "j_long", "penalty_after_ban", "no_skip")


class Probe(NamedTuple):
    name: str
    logits: np.ndarray  # [R, V + PAD] fp32
    V: int
    hist: np.ndarray    # [R, cap] int64
    count: int
    offset: int
    max_history: int
    rho: float
    n: int


def length(count: int, offset: int, max_history: int) -> int:
    return min(max(count + offset, 0), max_history)


def _penalised(x: np.float32, rho: np.float32) -> np.float32:
    with np.errstate(all="ignore"):
        return np.float32(x * rho) if x < 0 else np.float32(x / rho)


def definition(logits: np.ndarray, V: int, hist: np.ndarray, L: int, rho: float, n: int) -> np.ndarray:
    """The header's definition on logits [R, >= V] fp32 and hist [R, >= L] int64 -> the new logits."""
    out = np.array(logits, dtype=np.float32)
    rho = np.float32(rho)
    for r in range(out.shape[0]):
        h = [int(t) for t in hist[r, :L]]
        inside = [0 <= t < V for t in h]
        if rho != 1:
            for t in sorted({t for t, ok in zip(h, inside) if ok}):  # every distinct in-range id, once
                out[r, t] = _penalised(logits[r, t], rho)
        if n >= 1:
            for j in range(0, L - n + 1):
                p = j + n - 1
                window, suffix = range(j, p), range(L - n + 1, L)
                if all(inside[a] and inside[b] and h[a] == h[b] for a, b in zip(window, suffix)) and inside[p]:
                    out[r, h[p]] = -np.inf  # after the penalty: the ban wins
    return out


def emulate(logits: np.ndarray, V: int, hist: np.ndarray, L: int, rho: float, n: int, fault=None) -> np.ndarray:
    """The kernel's phases on a flat guarded copy of `logits`, with one of FAULTS or none; returns the
    flat buffer (GUARD floats, the rows, GUARD floats), to be compared with `flat(definition(...))`."""
    R, stride = logits.shape
    buf = flat(logits)
    rho = np.float32(rho)

    def store(r, t, value):
        at = GUARD + r * stride + t
        if 0 <= at < buf.size:
            buf[at] = value

    def load(r, t):
        at = GUARD + r * stride + t
        return buf[at] if 0 <= at < buf.size else np.float32(0)

    cap = hist.shape[1]
    for r in range(R):
        reach = min(L + 1, cap) if fault == "j_long" else L
        if fault == "no_skip":  # narrowed without the range check
            ids = [int(np.int64(t).astype(np.int32)) for t in hist[r, :reach]]
            skip = [False] * reach
        else:
            ids = [int(t) if 0 <= int(t) < V else -1 for t in hist[r, :reach]]
            skip = [t < 0 for t in ids]
        ban = [False] * reach
        if n >= 1:
            last = {"j_short": L - 2, "j_long": reach - 1}.get(fault, L - 1)
            for p in range(n - 1, last + 1):
                same = not skip[p]
                if fault != "no_prefix":
                    for k in range(1, n):
                        same = same and ids[p - k] == ids[L - k] and not skip[p - k]
                ban[p] = same
        original = {t: load(r, t) for t in set(ids)}
        if fault == "per_occurrence":
            for i in range(L):
                if not skip[i] and rho != 1:
                    store(r, ids[i], _penalised(load(r, ids[i]), rho))
            for i in range(reach):
                if ban[i]:
                    store(r, ids[i], -np.inf)
            continue
        for i in range(reach):
            if skip[i] or ids[i] in ids[:i]:
                continue  # not the owner
            t = ids[i]
            banned = any(ban[p] for p in range(reach) if ids[p] == t)
            if banned:
                store(r, t, -np.inf)
            if rho != 1 and i < L and (not banned or fault == "penalty_after_ban"):
                store(r, t, _penalised(original[t], rho))
    return buf


def flat(logits: np.ndarray) -> np.ndarray:
    guard = np.full(GUARD, 77.0, dtype=np.float32)
    return np.concatenate([guard, np.asarray(logits, dtype=np.float32).reshape(-1), guard])


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------ the probes
def _logits(rng, R: int, V: int) -> np.ndarray:
    """4 randn, never denormal after a division by 8; a few +-0 and +-inf where V allows."""
    x = (4 * rng.standard_normal((R, V + PAD))).astype(np.float32)
    x[np.abs(x) < 1e-3] = 1.0
    if V >= 5:
        for r in range(R):
            cols = rng.choice(V, 4, replace=False)
            x[r, cols] = [0.0, -0.0, np.inf, -np.inf]
    return x


def _probe(name, rng, R, V, hist, rho, n, L=None, count=None, offset=0, max_history=None, logits=None) -> Probe:
    hist = np.asarray(hist, dtype=np.int64).reshape(R, -1)
    L = hist.shape[1] if L is None else L
    if L < MAX_HISTORY:  # stale in-range entries behind the history
        hist = np.concatenate([hist[:, :L], rng.integers(0, V, (R, 4))], 1)
    count = L - offset if count is None else count
    max_history = min(hist.shape[1], MAX_HISTORY) if max_history is None else max_history
    assert length(count, offset, max_history) == L <= hist.shape[1] and max_history <= hist.shape[1]
    return Probe(name, _logits(rng, R, V) if logits is None else logits, V, hist, count, offset, max_history, rho, n)


SHAPES = [(1, 1), (3, 5), (5, 4097)]
LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1024]
RHOS = [0.5, 1.0, 1.3, 8.0]


def probes() -> list:
    rng = np.random.default_rng(2024)
    out = []
    k = 0
    for R, V in SHAPES:  # every length at every shape, rho and n in turn; random ids repeat freely
        for L in LENGTHS:
            rho, n = RHOS[k % 4], (k // 4 + k) % 5
            k += 1
            out.append(_probe(f"random R{R} V{V} L{L}", rng, R, V, rng.integers(0, V, (R, L)), rho, n, offset=k % 3))
    R, V = 3, 5
    for n in range(1, 5):  # the window arithmetic around L = n
        for L in (n - 2, n - 1, n, n + 1):
            if L >= 0:
                out.append(_probe(f"all-same L{L} n{n}", rng, R, V, np.full((R, L), 2), 1.3, n))
    # a count above max_history is clamped, one below zero is zero
    out.append(_probe("clamped", rng, 5, 4097, rng.integers(0, 50, (5, 400)), 1.3, 2, L=300, count=1500, offset=7,
                      max_history=300))
    out.append(_probe("negative", rng, 3, 5, rng.integers(0, 5, (3, 6)), 8.0, 1, L=0, count=2, offset=-9))
    out.append(_probe("int64 count", rng, 3, 5, rng.integers(0, 5, (3, 6)), 8.0, 1, L=0, count=-(1 << 40), offset=5))
    for R, V in SHAPES[1:]:
        out.append(_probe(f"all equal V{V}", rng, R, V, np.full((R, 300), V - 1), 8.0, 3))
    out.append(_probe("all distinct", rng, 5, 4097, np.stack([rng.permutation(4097)[:1024] for _ in range(5)]), 0.5, 2))
    h = np.stack([rng.permutation(4097)[:257] for _ in range(5)])
    h[:, -1] = h[:, 0]
    out.append(_probe("duplicate at both ends", rng, 5, 4097, h, 1.3, 0))
    out.append(_probe("duplicate at both ends, banned", rng, 5, 4097, h, 1.3, 1))
    # the only match at j = L - n, and none at all
    out.append(_probe("last j only", rng, 1, 5, [1, 2, 3, 4, 4], 1.0, 2))
    out.append(_probe("last j only n3", rng, 1, 5, [0, 1, 3, 3, 3], 1.3, 3))
    out.append(_probe("no match", rng, 1, 5, [1, 2, 3, 4, 0], 1.3, 2))
    out.append(_probe("aaaa n3", rng, 1, 5, [4, 4, 4, 4], 1.0, 3))
    # out-of-range ids: in the window, in the suffix, as the id to ban; 2^40 narrows to 0
    V = 5
    for bad in (-1, V, 1 << 40, (1 << 32) + 1, -(1 << 32) + 2):
        out.append(_probe(f"{bad} in the window", rng, 1, V, [0, bad, 3, 2, 0, 1], 1.3, 3))
        out.append(_probe(f"{bad} in the suffix", rng, 1, V, [0, bad, 3, 2, 0, bad], 1.3, 3))
        out.append(_probe(f"{bad} to ban", rng, 1, V, [0, 1, bad, 2, 0, 1], 8.0, 3))
        out.append(_probe(f"{bad} against its narrowing", rng, 1, V, [bad & 0xFFFFFFFF if 0 <= bad & 0xFFFFFFFF < V else 0, 1, 3,
                                                                      2, bad, 1], 0.5, 3))
        out.append(_probe(f"{bad} everywhere", rng, 3, V, np.full((3, 70), bad), 8.0, 1))
    big = rng.integers(0, 4097, (5, 257))
    big[0, ::7], big[1, ::7], big[2, ::7] = -1, 4097, 1 << 40
    out.append(_probe("out of range at V 4097", rng, 5, 4097, big, 1.3, 1))
    # +-0 and +-inf under the penalty: -0 is divided and stays -0, the infinities stay
    special = np.array([[-0.0, 0.0, -np.inf, np.inf, 1.5, 9.0, 9.0, 9.0]], dtype=np.float32)
    for rho in (0.5, 1.3):
        out.append(_probe(f"special values rho {rho}", rng, 1, 5, [0, 1, 2, 3, 4, 0], rho, 0, logits=special.copy()))
    # the issue's fixed case
    fixed = np.array([[-1, 2, -3, 4, -5, 6, -7, 8, -9, 0, 0, 0]], dtype=np.float32)
    for rho, n in ((1.5, 0), (1.0, 1), (1.0, 2), (1.0, 3), (1.0, 7), (1.0, 8), (1.5, 2), (1.5, 1)):
        out.append(_probe(f"fixed rho {rho} n {n}", rng, 1, 9, [3, 5, 3, 7, 3, 5], rho, n, logits=fixed.copy()))
    return out

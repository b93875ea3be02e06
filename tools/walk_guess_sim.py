#!/usr/bin/env python
"""How often do walk_spec's walkers enter their segment off the true path?  (CPU only, numpy.)

A walker of the speculative walk (csrc/wx_dp_walk.h) starts kSpecOverlap = 2 blocks above its
segment on a guessed column and is only useful if its path has merged with the true one when it
enters the segment; otherwise wave 0 walks that segment's top again after the barrier, and the
launch ends with its slowest segment.  This tool builds the decision bits of synthetic segments
(the bench's peaky emissions), follows the true backtrack and every walker's, and counts the
segment tops a walker enters on another column, for guesses moved off the straight line
(0, 0)-(T, N) by a constant or by k (T - 2 N) / T columns.

    python tools/walk_guess_sim.py [--segments 256] [--waves 8]
"""
import argparse

import numpy as np

V = 32
OVERLAP = 2  # kSpecOverlap


def segment(rng, T, n_lo, n_hi):
    N = int(rng.integers(n_lo, n_hi + 1))
    x = rng.standard_normal((T, V))
    x[:, 0] += 6.0
    tk = rng.integers(1, V, N)
    x[np.sort(rng.choice(np.arange(1, T - 1), N, replace=False)), tk] += 12.0
    m = x.max(1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(1, keepdims=True)), tk


def decisions(em, tk):
    """D[t, j]: the backtrack moves from column j to j - 1 at step t (alignment.py:400-404)."""
    T, N = em.shape[0], len(tk)
    tr = np.full(N + 1, -np.inf)
    tr[0] = 0.0
    D = np.zeros((T, N + 1), bool)
    col_n = np.full(T + 1, -np.inf)
    et = em[:, tk]
    for t in range(T):
        stay = tr + em[t, 0]
        ch = np.concatenate(([-np.inf], tr[:-1] + et[t]))
        D[t, 1:] = ch[1:] > stay[1:]
        tr = np.maximum(stay, ch)
        col_n[t + 1] = tr[N]
    return D, int(np.argmax(col_n))


def back(D, t, j, t_end):
    while t > t_end and j > 0:
        j -= int(D[t - 1, j])
        t -= 1
    return j


def plan(T, waves=8):
    """walk_spec's segments: (K, lo) with segment k over blocks lo(k) .. lo(k - 1) - 1."""
    top = (T - 1) >> 5
    nb = top + 1
    K = max(1, min(waves, nb // 4))
    L0 = max((nb + 3 + K // 2) // K - 3, 1)
    if K > 1 and nb - L0 < K - 1:
        K = max(nb - L0 + 1, 1)
    if K <= 1 or L0 >= nb:
        return 1, lambda k: 0
    Lb, ex = divmod(nb - L0, K - 1)
    return K, lambda k: top - L0 + 1 if k == 0 else max(top - L0 - (k * Lb + min(k, ex)) + 1, 0)


RULES = {"line": lambda T, N: 0, "+4": lambda T, N: 4 * T, "+8": lambda T, N: 8 * T, "+12": lambda T, N: 12 * T,
         "8 (T-2N)/T": lambda T, N: 8 * (T - 2 * N), "16 (T-2N)/T": lambda T, N: 16 * (T - 2 * N),
         "24 (T-2N)/T": lambda T, N: 24 * (T - 2 * N)}


def sweep(name, shapes, seed, waves):
    rng = np.random.default_rng(seed)
    res = {r: [0, 0, 0, 0] for r in RULES}  # segments with a miss, tops missed, tops, blocks wave 0 walks again
    for T, n_lo, n_hi in shapes:
        em, tk = segment(rng, T, n_lo, n_hi)
        N = len(tk)
        D, ts = decisions(em, tk)
        K, lo = plan(T, waves)
        true_at, j = {}, N
        for t in range(ts, 0, -1):
            if t % 32 == 0:
                true_at[t] = j
            j -= int(j > 0 and D[t - 1, j])
        true_at[0] = j
        for r, num in RULES.items():
            miss = 0
            for k in range(1, K):
                top = lo(k - 1) - 1
                tt = 32 * (top + OVERLAP + 1)
                if tt > ts:
                    continue
                g = (N * tt + T // 2 + num(T, N)) // T
                g = min(max(g, max(1, N - (T - tt))), min(N, tt))
                jw, jt = back(D, tt, g, 32 * (top + 1)), true_at[32 * (top + 1)]
                res[r][2] += 1
                if jw != jt:
                    miss += 1
                    for b in range(top, lo(k) - 1, -1):
                        jw, jt = back(D, 32 * (b + 1), jw, 32 * b), back(D, 32 * (b + 1), jt, 32 * b)
                        res[r][3] += 1
                        if jw == jt:
                            break
            res[r][0] += miss > 0
            res[r][1] += miss
    print(f"{name}: {len(shapes)} segments")
    for r, v in res.items():
        print(f"    {r:12s} segments with a miss {v[0]:3d}   tops missed {v[1]:3d} of {v[2]}   blocks walked again {v[3]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=256)
    ap.add_argument("--waves", type=int, default=8, help="waves of the split workgroup (walk_spec's K <= waves)")
    args = ap.parse_args()
    n, waves = args.segments, args.waves
    sweep("config 2 (T 1499, N 300-500)", [(1499, 300, 500)] * n, 1, waves)
    sweep("sparse (T 1499, N 170-280)", [(1499, 170, 280)] * (n // 2), 2, waves)
    sweep("dense (T 1499, N 500-544)", [(1499, 500, 544)] * (n // 2), 3, waves)
    rr = np.random.default_rng(4321)
    Ts = [int(rr.integers(100, 1500)) for _ in range(3 * n // 4)]
    sweep("ragged (T 100-1499, N T/6-T/3)", [(T, max(2, T // 6), max(3, T // 3)) for T in Ts], 4, waves)
    sweep("T 2999, N 850-951", [(2999, 850, 951)] * (n // 5), 5, waves)


if __name__ == "__main__":
    main()

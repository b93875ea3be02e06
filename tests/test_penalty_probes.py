"""wx_penalize_logits' definition and probes on the CPU: the numpy definition (penalty_probes) on the
issue's fixed case and against transformers' two logits processors, the emulation of the kernel's
phases against the definition on every probe, every fault of the emulation rejected by a probe, and
the package's host route (penalize_logits_host) against the definition."""
import numpy as np
import pytest
import torch

from penalty_probes import FAULTS, MAX_HISTORY, definition, emulate, flat, length, probes, same_bits

IDS = [3, 5, 3, 7, 3, 5]
LOGITS = np.array([[-1, 2, -3, 4, -5, 6, -7, 8, -9]], dtype=np.float32)


def _fixed(rho, n):
    return definition(LOGITS, 9, np.array([IDS]), len(IDS), rho, n)[0]


def test_fixed_case():
    got = _fixed(1.5, 0)
    want = np.array([-1, 2, -3, np.float32(4) / np.float32(1.5), -5, 4, -7, np.float32(8) / np.float32(1.5), -9], dtype=np.float32)
    assert same_bits(got, want)  # id 3 occurs three times and is penalised once
    assert np.allclose(got, [-1, 2, -3, 2.6667, -5, 4, -7, 5.3333, -9], atol=1e-4)

    def banned(n):
        return np.flatnonzero(np.isneginf(_fixed(1.0, n))).tolist()

    assert banned(2) == [3] and banned(3) == [3] and banned(1) == [3, 5, 7]
    assert banned(7) == [] and banned(8) == [] and banned(0) == []
    both = _fixed(1.5, 2)  # column 3 is penalised and banned: the ban wins
    assert np.isneginf(both[3]) and both[5] == 4 and both[7] == np.float32(8) / np.float32(1.5)


def test_length():
    assert length(5, 2, 100) == 7 and length(5, -9, 100) == 0 and length(1500, 7, 300) == 300 and length(0, 0, 0) == 0


@pytest.mark.parametrize("seed", range(6))
def test_definition_is_transformers(seed):
    """Random in-range histories: the definition equals RepetitionPenaltyLogitsProcessor followed by
    NoRepeatNGramLogitsProcessor, bit for bit."""
    from transformers import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    rng = np.random.default_rng(seed)
    R, V = 4, [7, 40, 300][seed % 3]
    for L in (0, 1, 2, 3, 9, 40):
        for rho in (0.5, 1.0, 1.3, 8.0):
            for n in (0, 1, 2, 3, 4):
                hist = rng.integers(0, V, (R, L))
                x = (4 * rng.standard_normal((R, V))).astype(np.float32)
                x[:, 0] = -np.inf
                want = torch.from_numpy(x.copy())
                ids = torch.from_numpy(hist)
                if L:  # (the processors index the last token of an empty history)
                    want = RepetitionPenaltyLogitsProcessor(penalty=rho)(ids, want)
                    if n:
                        want = NoRepeatNGramLogitsProcessor(n)(ids, want)
                assert same_bits(definition(x, V, hist, L, rho, n), want.numpy()), (L, rho, n)


def test_emulation_is_the_definition_on_every_probe():
    ps = probes()
    assert len({p.name for p in ps}) == len(ps)
    for p in ps:
        L = length(p.count, p.offset, p.max_history)
        want = definition(p.logits, p.V, p.hist, L, p.rho, p.n)
        assert same_bits(want[:, p.V:], p.logits[:, p.V:]), p.name
        assert same_bits(emulate(p.logits, p.V, p.hist, L, p.rho, p.n), flat(want)), p.name
    assert max(length(p.count, p.offset, p.max_history) for p in ps) == MAX_HISTORY


@pytest.mark.parametrize("fault", FAULTS)
def test_every_fault_is_rejected(fault):
    caught = []
    for p in probes():
        L = length(p.count, p.offset, p.max_history)
        want = flat(definition(p.logits, p.V, p.hist, L, p.rho, p.n))
        if not same_bits(emulate(p.logits, p.V, p.hist, L, p.rho, p.n, fault), want):
            caught.append(p.name)
    print(f"{fault}: rejected by {len(caught)} probes, e.g. {caught[:4]}")
    assert caught


def test_probes_cover_what_they_claim():
    ps = {p.name: p for p in probes()}
    both = 0
    for p in ps.values():
        L = length(p.count, p.offset, p.max_history)
        if p.rho != 1 and p.n:
            pen = definition(p.logits, p.V, p.hist, L, p.rho, 0)
            ban = definition(p.logits, p.V, p.hist, L, 1.0, p.n)
            both += int(((pen != p.logits) & np.isneginf(ban) & ~np.isneginf(p.logits)).any())
    assert both >= 5  # columns both penalised and banned
    p = ps["last j only"]
    zeros = np.zeros_like(p.logits)
    assert np.flatnonzero(np.isneginf(definition(zeros, p.V, p.hist, 5, 1.0, 2)[0])).tolist() == [4]  # from j = L - n alone
    for name in ("-1 in the window", "5 in the suffix", f"{1 << 40} to ban", f"{1 << 40} against its narrowing"):
        p = ps[name]
        got = definition(p.logits, p.V, p.hist, 6, 1.0, 3)
        assert same_bits(got, p.logits), name  # nothing is banned


def test_host_route_is_the_definition():
    """penalize_logits_host on every probe whose history is in range (the decoder's ids always are)."""
    from whisperx_amd.whisper import penalize_logits_host

    ran = 0
    for p in probes():
        L = length(p.count, p.offset, p.max_history)
        if L and (p.hist[:, :L].min() < 0 or p.hist[:, :L].max() >= p.V):
            continue
        lg = torch.from_numpy(p.logits.copy())
        view = lg[:, :p.V]
        penalize_logits_host(view, torch.from_numpy(p.hist[:, :L].T.copy()), p.rho, p.n)
        assert same_bits(lg.numpy(), definition(p.logits, p.V, p.hist, L, p.rho, p.n)), p.name
        ran += 1
    assert ran >= 50

"""Shared by the Whisper decoder tests: a random transformers WhisperForConditionalGeneration as
the oracle.

No weights are downloaded: the model is built from a tiny WhisperConfig and its decoder's weights
are drawn by whisper_helpers.draw_weights (unit-variance fan-in scaling, q and k projections 3x
that, biases ~0.1, LayerNorm gains 1 +- 0.1, positional table 0.5 randn) with
embed_tokens.weight randn / sqrt(D).  At unit variance the tied output projection makes
the model echo its last input token for ever (logits ~200, top-2 margin ~50) and any attention bug
would pass; with 1 / sqrt(D) the greedy sequences vary and the logits are O(4).

The reference is fp64: `model(encoder_outputs=(enc,), decoder_input_ids=ids).logits` without a
cache, and a hand-written greedy loop over it (transformers' generate needs a generation config).

Tolerance rule (the encoder tests'): ref_err = max|HF fp32 - HF fp64| on the same inputs on the
CPU, and the code under test must be within 4 x ref_err of HF fp64.
"""
import copy
import functools

import torch

from whisper_helpers import draw_weights

# (D, layers, P, V, max_target_positions, B): the geometries of the decoder tests
GEOMETRIES = [(384, 2, 50, 96, 40, 3), (1280, 1, 33, 96, 24, 2), (512, 1, 130, 96, 24, 2)]
PROMPT = [1, 5, 7]
ENC_SEED = 5
N_GREEDY = 12  # generated tokens the greedy tests compare
N_FORCED = 12  # teacher-forced positions


def make_model(D: int, layers: int, P: int, V: int, T: int, seed: int = 0):
    """A transformers WhisperForConditionalGeneration (fp32, eval, CPU) whose decoder has width D,
    D / 64 heads, ffn 4 D, vocabulary V and T target positions.  Only the decoder is used."""
    from transformers import WhisperConfig, WhisperForConditionalGeneration

    cfg = WhisperConfig(d_model=D, encoder_layers=1, encoder_attention_heads=1, encoder_ffn_dim=64,
                        num_mel_bins=80, max_source_positions=P, decoder_layers=layers, decoder_attention_heads=D // 64,
                        decoder_ffn_dim=4 * D, vocab_size=V, max_target_positions=T, pad_token_id=0, bos_token_id=1,
                        eos_token_id=2, decoder_start_token_id=1, dropout=0.0, attention_dropout=0.0,
                        activation_dropout=0.0, decoder_layerdrop=0.0, scale_embedding=False)
    model = WhisperForConditionalGeneration(cfg).eval().requires_grad_(False)
    draw_weights(model.model.decoder, seed, embed_tokens_div=D ** 0.5)
    assert model.proj_out.weight.data_ptr() == model.model.decoder.embed_tokens.weight.data_ptr()  # tied
    return model


def make_states(B: int, P: int, D: int, seed: int = ENC_SEED) -> torch.Tensor:
    """Encoder states [B, P, D]: the encoder ends in a LayerNorm, so O(1) entries."""
    return torch.randn((B, P, D), generator=torch.Generator().manual_seed(seed))


def hf_logits(model, enc: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """The oracle's teacher-forced logits [B, n, V], no cache, in the model's precision."""
    with torch.no_grad():
        return model(encoder_outputs=(enc.to(model.dtype),), decoder_input_ids=ids, use_cache=False).logits


class Case:
    """One geometry's oracle, computed once on the CPU and shared (the tests leave it unchanged)."""

    def __init__(self, D, layers, P, V, T, B):
        self.geometry = (D, layers, P, V, T, B)
        self.D, self.V, self.T, self.B = D, V, T, B
        self.model = make_model(D, layers, P, V, T)
        self.model64 = copy.deepcopy(self.model).double()
        self.enc = make_states(B, P, D)
        self.enc64 = self.enc.double()

    @functools.lru_cache(maxsize=None)
    def forced(self, n: int = N_FORCED, seed: int = 11):
        """(random ids [B, n], HF fp64 logits [B, n, V], ref_err): off the greedy path."""
        ids = torch.randint(0, self.V, (self.B, n), generator=torch.Generator().manual_seed(seed))
        y64 = hf_logits(self.model64, self.enc64, ids)
        ref_err = float((hf_logits(self.model, self.enc, ids).double() - y64).abs().max())
        return ids, y64, ref_err

    @functools.lru_cache(maxsize=None)
    def greedy(self, steps: int = N_GREEDY, suppress=(), suppress_at_start=()):
        """The fp64 greedy loop from PROMPT for `steps` tokens, no stopping: (tokens [B, steps],
        the smallest top-2 margin over every step and row, ref_err of the logits along that path,
        the fp64 logits [B, steps, V] before masking)."""
        ids = torch.tensor([PROMPT] * self.B)
        margin, rows = float("inf"), []
        for i in range(steps):
            lg = hf_logits(self.model64, self.enc64, ids)[:, -1].clone()
            rows.append(lg.clone())
            if suppress:
                lg[:, list(suppress)] = float("-inf")
            if suppress_at_start and i == 0:
                lg[:, list(suppress_at_start)] = float("-inf")
            top = lg.topk(2, -1).values
            margin = min(margin, float((top[:, 0] - top[:, 1]).min()))
            ids = torch.cat([ids, lg.argmax(-1, keepdim=True)], 1)
        fed = ids[:, :-1]  # what the decoder was fed; the logits after each of its positions
        y64 = hf_logits(self.model64, self.enc64, fed)
        ref_err = float((hf_logits(self.model, self.enc, fed).double() - y64).abs().max())
        return ids[:, len(PROMPT):], margin, ref_err, torch.stack(rows, 1)


@functools.lru_cache(maxsize=None)
def case(D, layers, P, V, T, B) -> Case:
    return Case(D, layers, P, V, T, B)


def attention_inputs(B: int, H: int, L: int, seed: int = 0):
    """q [B, H, 64], k / v [B, H, L, 64] on the CPU: k 3x q's scale, so the softmax is peaked."""
    g = torch.Generator().manual_seed(seed + 1000 * L + 10 * H + B)
    q = torch.randn((B, H, 64), generator=g)
    k = 3.0 * torch.randn((B, H, L, 64), generator=g)
    v = torch.randn((B, H, L, 64), generator=g)
    return q, k, v


def attention_ref(q, k, v, scale: float = 0.125):
    """softmax(scale q k^T) v in the inputs' precision: [B, H, 64]."""
    w = torch.softmax(scale * torch.einsum("bhd,bhld->bhl", q, k), -1)
    return torch.einsum("bhl,bhld->bhd", w, v)


# ------------------------------------------------- the oracle conditions, on either device
LANGUAGE_IDS = [3, 17, 42, 60, 88]
SOT = 1


def check_forced_logits(c: Case, dec, label: str) -> torch.Tensor:
    """WhisperDecoder.logits on random ids within 4 x ref_err of HF fp64; returns the logits."""
    ids, y64, ref_err = c.forced()
    got = dec.logits(c.enc, ids)
    assert tuple(got.shape) == (c.B, N_FORCED, c.V) and got.dtype == torch.float32
    err = float((got.cpu().double() - y64).abs().max())
    print(f"{label} {c.geometry}: |logits - fp64| {err:.3e}, ref_err {ref_err:.3e}, bound {4 * ref_err:.3e}, "
          f"|logit| max {float(y64.abs().max()):.2f}")
    assert ref_err > 0 and err <= 4 * ref_err
    return got


def check_greedy(c: Case, dec, label: str, **suppress) -> list:
    """generate equals the fp64 greedy loop token for token.  First the oracle alone: every step's
    fp64 top-2 margin exceeds 8 x ref_err (two logits each within 4 x ref_err cannot swap an
    argmax wider than that)."""
    want, margin, ref_err, _ = c.greedy(N_GREEDY, **{k: tuple(v) for k, v in suppress.items()})
    print(f"{label} {c.geometry} {suppress}: oracle's smallest top-2 margin {margin:.3e}, ref_err {ref_err:.3e}, "
          f"8 x ref_err {8 * ref_err:.3e}")
    assert ref_err > 0 and margin > 8 * ref_err
    eot = next(i for i in range(c.V - 1, -1, -1) if i not in set(want.flatten().tolist()))  # never emitted
    kw = {("suppress_tokens" if k == "suppress" else k): list(v) for k, v in suppress.items()}
    got = dec.generate(c.enc, PROMPT, eot, max_length=len(PROMPT) + N_GREEDY, **kw)
    assert got == want.tolist()
    return got


def check_stopping(c: Case, dec):
    """eot = the id the oracle emits at step 4 of row 0: every row is the oracle's cut at its first
    eot, row 0 stops within 4 tokens and the other rows run on.  (On the 384 geometry row 0 emits
    that id, 13, at steps 3 and 4, so it stops after 3 tokens; rows 1 and 2 emit it at step 5.)"""
    want, margin, ref_err, _ = c.greedy()
    assert margin > 8 * ref_err
    eot = int(want[0, 4])
    cut = [row[:row.index(eot)] if eot in row else row for row in want.tolist()]
    # (the loop ends once every row is done: no row is longer than the step at which the last one stopped)
    assert all(eot in row for row in want.tolist()) or max(len(r) for r in cut) == N_GREEDY
    got = dec.generate(c.enc, PROMPT, eot, max_length=len(PROMPT) + N_GREEDY)
    print(f"stopping: eot {eot}, lengths {[len(r) for r in got]}")
    assert got == cut
    assert len(got[0]) <= 4 and all(len(r) > len(got[0]) for r in got[1:])
    assert all(eot not in r for r in got)


def check_suppression(c: Case, dec, label: str):
    """Suppressing the oracle's step-2 token of row 1 (which no row emits earlier) changes the
    output from step 2 on and matches the fp64 loop run with the same mask; suppress_at_start
    moves position 0 only."""
    plain = c.greedy()[0]
    tok = int(plain[1, 2])
    assert tok not in plain[:, :2].flatten().tolist()
    got = check_greedy(c, dec, label, suppress=[tok])
    assert all(tok not in row for row in got)
    assert [r[:2] for r in got] == plain[:, :2].tolist() and got[1][2] != tok
    first = sorted(set(plain[:, 0].tolist()))
    got = check_greedy(c, dec, label, suppress_at_start=first)
    assert all(row[0] not in first for row in got)
    # position 0 only: the masked loop is free to emit those ids later, and does
    later = c.greedy(N_GREEDY, suppress_at_start=tuple(first))[0][:, 1:].flatten().tolist()
    assert any(t in first for t in later)


def check_detect_language(c: Case, dec, label: str):
    ids = torch.full((c.B, 1), SOT)
    p64 = torch.softmax(hf_logits(c.model64, c.enc64, ids)[:, -1][:, LANGUAGE_IDS], -1)
    p32 = torch.softmax(hf_logits(c.model, c.enc, ids)[:, -1][:, LANGUAGE_IDS], -1)
    ref_err = float((p32.double() - p64).abs().max())
    got = dec.detect_language(c.enc, SOT, LANGUAGE_IDS)
    assert tuple(got.shape) == (c.B, len(LANGUAGE_IDS))
    err = float((got.cpu().double() - p64).abs().max())
    print(f"{label} detect_language: |p - fp64| {err:.3e}, ref_err {ref_err:.3e}, bound {4 * ref_err:.3e}")
    assert ref_err > 0 and err <= 4 * ref_err
    assert float((got.sum(-1) - 1).abs().max()) <= 1e-6

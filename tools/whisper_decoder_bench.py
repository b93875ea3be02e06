#!/usr/bin/env python3
"""Times of Whisper's text decoder, one position per step (no threshold: a record).

Random weights in two geometries (--geometries, comma separated), vocabulary 51865, 448 target
positions, 1500 encoder positions:
  base      D 512, 6 layers, 8 heads
  large-v2  D 1280, 32 layers, 20 heads

(a) attention: wx_decode_attention_f32 (whisperx_amd._lib.decode_attention_f32) against
    F.scaled_dot_product_attention on the same tensors, at L = 1500 (the cross-attention layout: the
    halves of a [B, 1500, 2D] tensor) and L = 224 (the cache layout [B, H, 448, 64]), B in {1, 16}.
    Each arm is the median of --repeat repetitions (with min and max, the spread a difference has to
    exceed) of --steps launches between device events.  The launches of a repetition walk a ring of
    key / value buffers of --ring-bytes in all, so that a launch does not find its rows in the cache
    the launch before left.  Reported with the time: the key / value bytes the shapes say are read
    (2 B H L 64 x 4), and that over the time as bytes/s and as a share of the HBM peak.
(b) decoder: one `step` of 16 rows at position 35 (the state's position is put back before every
    call), and `generate` of 64 tokens for 16 chunks from a 3-token prompt, against transformers'
    fp32 WhisperDecoder with its key / value cache in a greedy loop of the same length on the same
    device (its per-step figure is that loop's time over its 64 steps; it takes the prompt in one
    forward, ours in three steps).  Both loops check for completion, and so synchronise, every step.

(c) --arms beam (its own record, profiles/whisper_beam_<host>.json): beam search at --beams 5.
    The grouped cross-attention launch (wx_decode_attention_f32_grouped: B chunks, G queries each on
    the chunk's one K / V) at G in {1, 5, 8} against the ungrouped launch at B rows and at B G rows on
    K / V replicated G times, L = 1500, B = 16, by (a)'s ring method; wx_beam_topk against torch's
    log_softmax + add + topk on [16 G, 51865] logits; and `beam_search` of 64 tokens for 16 chunks
    against the route without the two kernels: B G rows through the same step machinery with the
    cross-attention tensors replicated by repeat_interleave, the ungrouped kernel and torch's
    selection (the same host walk and cache reorder).  Where the replicated tensors do not fit, the
    baseline's chunk count is halved until they do, and the record says what it was.

(d) --dtype float16 | bfloat16 (its own record, profiles/whisper_decoder_half[_bf16]_<host>.json): the
    half route.  wx_decode_attention_h16 at B = 16, L = 1500 (cross layout) and L = 224 (cache
    layout) against wx_decode_attention_f32 on fp32 tensors of the same shapes in the same run and
    against torch's attention in dtype on the h16 arm's views, by (a)'s ring method, each arm's
    ring sized by its own bytes; the grouped launch at G in {5, 8} against the ungrouped one on a
    replica; one `step`, `generate` and `beam_search` (--beams) of WhisperDecoder(dtype=...) against
    WhisperDecoder in fp32 in the same run and against a greedy loop over transformers' decoder cast
    to dtype; and torch.cuda.max_memory_allocated of decoder + state for 16 chunks x --beams beams
    in both dtypes.  No graphs are captured.

(e) --arms prefill (its own record, profiles/whisper_prefill_<host>.json): the prompt prefill, fp32
    and the half type (--dtype, float16 by default) in the same run.  One wx_prefill_attention_f32 /
    _h16 launch against F.scaled_dot_product_attention with the same boolean mask on the same views,
    B = 16: causal at Tq = Tk in {4, 224} on the cache layout with q the slice of a fused
    [B, Tq, 3D] tensor, and without a mask at Tq in {4, 224} x Tk = 1500 on the cross layout, by
    (a)'s ring method; with the bytes (q, the visible K / V rows, o) and the FLOP (4 x 64 per visible
    (query, key) pair) the shapes give, and those over the time as shares of the HBM and fp32-MFMA
    peaks (the h16 arm computes on the fp32 MFMA too).  Then `generate` (64 tokens x 16 chunks) and
    `beam_search` (--beams) from a 4-id and from a 224-id prompt, and `logits` on [16, 64], each
    with prefill=True against prefill=False in the same run.

(f) --arms graph (its own record, profiles/whisper_graph_<host>.json): the graph-replayed step
    (start / generate / beam_search with graph=True), fp32 and float16 in the same run, every figure
    against the direct arm of the same run.  One `step` of 16 rows at position 35, direct against
    replay (the replay arm puts the device position back with one fill_ per call, the direct arm
    the host position); `generate` of 64 tokens x 16 chunks from a 4-id prompt, and with prefill=True
    from a 224-id prompt; `beam_search` at --beams from the 4-id prompt; the first step of a fresh
    plan (two warm-up passes, the capture and one replay) in ms; torch.cuda.memory_allocated with
    the decoder alone, with a direct state and with a plan; and the self-attention launch alone at
    L = 224 on 16 rows: wx_decode_self_attention_* against the two cache copies and
    wx_decode_attention_* on the same q/k/v GEMM output.

(g) --arms sample (its own record, profiles/whisper_sample_<host>.json): sampling and the selection
    kernel.  The selection launch alone, wx_sample_token on [16, 51865] and [80, 51865] logits at
    temperature 0 and 0.6 with one suppressed id, against the torch chain it replaces (masked_fill,
    log_softmax, argmax or torch.multinomial on softmax(l / T), gather); then, fp32 and float16 in
    the same run, `sample` of 64 tokens x 16 chunks x best_of 5 at temperature 0.6 against
    `beam_search` at --beams and greedy `generate`, each direct and with graph=True.

(h) --arms penalty (its own record, profiles/whisper_penalty_<host>.json): repetition_penalty and
    no_repeat_ngram_size.  The rewrite alone, wx_penalize_logits (rho 1.1, n 3) on [16, 51865] and
    [80, 51865] logits under histories of 32, 224 and 447 ids, against the torch chain it replaces:
    transformers' RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor on the same
    device tensors (the second walks every row's ids on the host).  Then, fp32 with graph=True,
    `generate` and `sample` (best_of 5, temperature 0.6) of 64 tokens x 16 chunks with the options
    off, on, and off again in the same run.

Prints one JSON line; --out writes it to a file (profiles/whisper_decoder_<host>.json).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from benchlib import beats, event_timed, timed  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E, spec
F32_MFMA_PEAK_FLOPS = 157.3e12  # MI355X v_mfma_f32_*_f32, spec
GEOMETRIES = {"base": {"D": 512, "layers": 6}, "large-v2": {"D": 1280, "layers": 32}}
V, T, P = 51865, 448, 1500
PROMPT = [50258, 50259, 50359]
N_TOKENS, CHUNKS, STEP_POS = 64, 16, 35


def attention_rows(D, args, torch, F, _lib, dev):
    H = D // 64
    rows = []
    for L, layout in ((1500, "cross [B, L, 2D] halves"), (224, "cache [B, H, 448, 64]")):
        for B in (1, 16):
            nbytes = 2 * B * H * L * 64 * 4
            ring = max(2, min(32, -(-args.ring_bytes // nbytes)))
            q = torch.randn((B, H, 64), device=dev)
            kv = []
            for _ in range(ring):
                if L == 1500:
                    t = torch.randn((B, L, 2 * D), device=dev)
                    kv.append(tuple(t[:, :, j * D:(j + 1) * D].view(B, L, H, 64).transpose(1, 2) for j in range(2)))
                else:
                    kv.append((torch.randn((B, H, T, 64), device=dev), torch.randn((B, H, T, 64), device=dev)))
            out = torch.empty((B, H, 64), device=dev)

            def ours(i):
                k, v = kv[i % ring]
                return _lib.decode_attention_f32(q, k, v, 0.125, L=L, out=out)

            def sdpa(i):
                k, v = kv[i % ring]
                return F.scaled_dot_product_attention(q.unsqueeze(2), k[:, :, :L], v[:, :, :L], scale=0.125)

            with torch.inference_mode():
                diff = float((ours(0) - sdpa(0).squeeze(2)).abs().max())
                r = {"L": L, "B": B, "H": H, "layout": layout, "kv_bytes": nbytes, "ring_buffers": ring,
                     "max_abs_diff_ours_vs_sdpa": diff,
                     "ours": event_timed(ours, args.repeat, args.warmup, args.steps, torch),
                     "sdpa": event_timed(sdpa, args.repeat, args.warmup, args.steps, torch)}
            for arm in ("ours", "sdpa"):
                r[arm]["kv_bytes_per_s"] = nbytes / r[arm]["median_s"]
                r[arm]["share_of_hbm_peak"] = r[arm]["kv_bytes_per_s"] / HBM_PEAK_BYTES_PER_S
            r["ours_vs_sdpa"] = beats(r["ours"], r["sdpa"])
            rows.append(r)
            del kv
            torch.cuda.empty_cache()
    return rows


def grouped_attention_rows(D, args, torch, _lib, dev, B=CHUNKS, L=P):
    """(c): one cross-attention launch for B chunks of G beams, grouped on [B, L, 2D] against
    ungrouped on B rows (one beam's work) and on B G rows of a [B G, L, 2D] replica."""
    H = D // 64

    def halves(t):
        return tuple(t[:, :, j * D:(j + 1) * D].view(t.shape[0], L, H, 64).transpose(1, 2) for j in range(2))

    rows = []
    for G in (1, 5, 8):
        nbytes = 2 * B * H * L * 64 * 4
        ring = max(2, min(32, -(-args.ring_bytes // (nbytes * G))))
        q = torch.randn((B, G, H, 64), device=dev)
        shared = [torch.randn((B, L, 2 * D), device=dev) for _ in range(ring)]
        out = torch.empty((B, G, H, 64), device=dev)
        out1 = torch.empty((B, H, 64), device=dev)
        q1 = q[:, 0].contiguous()
        qr = q.view(B * G, H, 64)

        def grouped(i):
            k, v = halves(shared[i % ring])
            return _lib.decode_attention_f32_grouped(q, k, v, 0.125, out=out)

        def ungrouped_b(i):
            k, v = halves(shared[i % ring])
            return _lib.decode_attention_f32(q1, k, v, 0.125, out=out1)

        with torch.inference_mode():
            r = {"L": L, "B": B, "G": G, "H": H, "kv_bytes_shared": nbytes, "kv_bytes_replicated": nbytes * G,
                 "ring_buffers": ring,
                 "grouped": event_timed(grouped, args.repeat, args.warmup, args.steps, torch),
                 "ungrouped_B_rows": event_timed(ungrouped_b, args.repeat, args.warmup, args.steps, torch)}
            want = grouped(0).clone()
        del shared
        torch.cuda.empty_cache()
        replicated = [torch.randn((B * G, L, 2 * D), device=dev) for _ in range(ring)]
        outr = torch.empty((B * G, H, 64), device=dev)

        def ungrouped_bg(i):
            k, v = halves(replicated[i % ring])
            return _lib.decode_attention_f32(qr, k, v, 0.125, out=outr)

        with torch.inference_mode():
            r["ungrouped_BG_rows_replicated"] = event_timed(ungrouped_bg, args.repeat, args.warmup, args.steps, torch)
        r["grouped"]["kv_bytes_per_s"] = nbytes / r["grouped"]["median_s"]
        r["grouped"]["share_of_hbm_peak"] = r["grouped"]["kv_bytes_per_s"] / HBM_PEAK_BYTES_PER_S
        r["grouped_vs_ungrouped_BG_rows"] = beats(r["grouped"], r["ungrouped_BG_rows_replicated"])
        r["grouped_vs_ungrouped_B_rows"] = beats(r["grouped"], r["ungrouped_B_rows"])
        r["output_finite"] = bool(torch.isfinite(want).all())
        rows.append(r)
        del replicated
        torch.cuda.empty_cache()
    return rows


def torch_select(lg, cum, G):
    """The selection without wx_beam_topk: log_softmax, add, topk over the chunk's G V candidates."""
    import torch

    R, Vv = lg.shape
    sc = (torch.log_softmax(lg, -1) + cum[:, None]).view(R // G, G * Vv)
    top = sc.topk(2 * G, dim=1)
    return top.values, top.indices.to(torch.int32)


def baseline_beam_search(dec, enc, prompt, eot, G, n_tokens, torch):
    """beam_search's loop on what the decoder had before the grouped kernels: B G rows of a plain
    state over the encoder states replicated G times (so is every cross-attention tensor), the
    ungrouped attention kernel, torch_select, and the same host walk and cache reorder."""
    with torch.inference_mode():
        st = dec.start(enc.repeat_interleave(G, 0))
        R, B = st.B, st.B // G
        for t in prompt:
            lg = dec._step(st, torch.full((R,), t, dtype=torch.int64, device=dec.device))
        sums = [[0.0] + [float("-inf")] * (G - 1) for _ in range(B)]
        ids = [[[] for _ in range(G)] for _ in range(B)]
        identity = list(range(R))
        for step in range(n_tokens):
            lg[:, eot] = float("-inf")
            cum = torch.tensor([x for row in sums for x in row], dtype=torch.float32).to(dec.device)
            sc, idx = torch_select(lg, cum, G)
            both = torch.cat([sc, idx.view(torch.float32)], 1).cpu()
            sc, idx = both[:, :2 * G].tolist(), both[:, 2 * G:].contiguous().view(torch.int32).tolist()
            parents, feed = list(identity), [eot] * R
            for b in range(B):
                live = [(*divmod(i, dec.V), s) for s, i in zip(sc[b], idx[b])][:G]  # (eot is suppressed: all live)
                ids[b] = [ids[b][g] + [t] for g, t, _ in live]
                sums[b] = [s for _, _, s in live]
                for j, (g, t, _) in enumerate(live):
                    parents[b * G + j], feed[b * G + j] = b * G + g, t
            if step + 1 == n_tokens:
                break
            if parents != identity:
                dec.reorder(st, torch.tensor(parents, dtype=torch.int64))
            lg = dec._step(st, torch.tensor(feed, dtype=torch.int64).to(dec.device))
    return [ids[b][0] for b in range(B)]


def beam_arm(name, g, args, torch, _lib, dev):
    from transformers import WhisperConfig, WhisperForConditionalGeneration

    from whisperx_amd import WhisperDecoder

    D, G = g["D"], args.beams
    sync = torch.cuda.synchronize
    eot = V - 1
    r = {"shape": {**g, "heads": D // 64, "vocab": V, "max_target_positions": T, "encoder_positions": P}, "beams": G}
    r["grouped_attention"] = grouped_attention_rows(D, args, torch, _lib, dev)
    print(f"{name}: grouped attention timed", file=sys.stderr, flush=True)
    lg = 4.0 * torch.randn((CHUNKS * G, V), device=dev)
    cum = -torch.rand(CHUNKS * G, device=dev)
    with torch.inference_mode():
        a, b = _lib.beam_topk(lg, cum, G), torch_select(lg, cum, G)
        r["topk"] = {"rows": CHUNKS * G, "G": G, "vocab": V,
                     "index_equal_torch": float((a[1] == b[1]).float().mean()),
                     "max_abs_score_diff_vs_torch": float((a[0] - b[0]).abs().max()),
                     "ours": event_timed(lambda i: _lib.beam_topk(lg, cum, G), args.repeat, args.warmup, args.steps, torch),
                     "torch": event_timed(lambda i: torch_select(lg, cum, G), args.repeat, args.warmup, args.steps, torch)}
    r["topk"]["ours_vs_torch"] = beats(r["topk"]["ours"], r["topk"]["torch"])
    cfg = WhisperConfig(d_model=D, encoder_layers=1, encoder_attention_heads=1, encoder_ffn_dim=64, num_mel_bins=80,
                        max_source_positions=P, decoder_layers=g["layers"], decoder_attention_heads=D // 64,
                        decoder_ffn_dim=4 * D, vocab_size=V, max_target_positions=T, pad_token_id=0, bos_token_id=1,
                        eos_token_id=2, decoder_start_token_id=1)
    hf = WhisperForConditionalGeneration(cfg).eval().model.decoder.to(dev)
    dec = WhisperDecoder(hf, device=dev)
    del hf
    enc = torch.randn((CHUNKS, P, D), device=dev)

    def ours():
        return dec.beam_search(enc, PROMPT, eot, beam_size=G, max_length=len(PROMPT) + N_TOKENS, suppress_tokens=[eot])

    def greedy():
        return dec.generate(enc, PROMPT, eot, max_length=len(PROMPT) + N_TOKENS, suppress_tokens=[eot])

    print(f"{name}: decoder built", file=sys.stderr, flush=True)
    got = ours()
    bs = {"chunks": CHUNKS, "beams": G, "generated_tokens": len(got[0][0].ids),
          "beam_search": timed(ours, args.repeat, args.warmup, sync),
          "greedy_generate": timed(greedy, args.repeat, args.warmup, sync)}
    bs["beam_search_per_step"] = {k: v / N_TOKENS for k, v in bs["beam_search"].items() if k.endswith("_s")}
    torch.cuda.empty_cache()
    print(f"{name}: beam_search timed", file=sys.stderr, flush=True)
    Bb = CHUNKS
    while True:  # the replicated cross tensors: layers x Bb G x P x 2D x 4 bytes
        try:
            want = baseline_beam_search(dec, enc[:Bb], PROMPT, eot, G, N_TOKENS, torch)
            bs["baseline"] = timed(lambda: baseline_beam_search(dec, enc[:Bb], PROMPT, eot, G, N_TOKENS, torch),
                                   args.repeat, args.warmup, sync)
            break
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            if Bb == 1:
                bs["baseline"] = "not measured (the replicated tensors of one chunk do not fit)"
                break
            Bb //= 2
    bs["baseline_chunks"] = Bb
    bs["baseline_replicated_cross_bytes"] = g["layers"] * Bb * G * P * 2 * D * 4
    bs["shared_cross_bytes"] = g["layers"] * CHUNKS * P * 2 * D * 4
    if isinstance(bs["baseline"], dict):
        bs["best_ids_equal_baseline"] = sum(h[0].ids == w for h, w in zip(got, want)) / Bb
        if Bb == CHUNKS:
            bs["beam_search_vs_baseline"] = beats(bs["beam_search"], bs["baseline"])
        else:  # per chunk: the baseline ran fewer
            bs["baseline_s_per_chunk"] = bs["baseline"]["median_s"] / Bb
            bs["beam_search_s_per_chunk"] = bs["beam_search"]["median_s"] / CHUNKS
    r["beam_search"] = bs
    del dec, enc
    torch.cuda.empty_cache()
    return r


def _rates(arm, nbytes):
    arm["kv_bytes"] = nbytes
    arm["kv_bytes_per_s"] = nbytes / arm["median_s"]
    arm["share_of_hbm_peak"] = arm["kv_bytes_per_s"] / HBM_PEAK_BYTES_PER_S


def half_attention_rows(D, dtype, args, torch, F, _lib, dev, B=CHUNKS):
    """(d): wx_decode_attention_h16 against wx_decode_attention_f32 on fp32 tensors of the same shapes
    and against torch's attention in dtype on the h16 arm's views, by (a)'s ring method; every arm's
    ring is sized by its own key / value bytes."""
    H = D // 64
    rows = []
    for L, layout in ((1500, "cross [B, L, 2D] halves"), (224, "cache [B, H, 448, 64]")):
        def buffers(dt, nbytes):
            ring = max(2, min(32, -(-args.ring_bytes // nbytes)))
            kv = []
            for _ in range(ring):
                if L == 1500:
                    t = torch.randn((B, L, 2 * D), device=dev).to(dt)
                    kv.append(tuple(t[:, :, j * D:(j + 1) * D].view(B, L, H, 64).transpose(1, 2) for j in range(2)))
                else:
                    kv.append(tuple(torch.randn((B, H, T, 64), device=dev).to(dt) for _ in range(2)))
            return ring, kv

        n16 = 2 * B * H * L * 64 * 2
        q32 = torch.randn((B, H, 64), device=dev)
        q16 = q32.to(dtype)
        out16, out32 = torch.empty((B, H, 64), dtype=dtype, device=dev), torch.empty((B, H, 64), device=dev)
        ring16, kv16 = buffers(dtype, n16)

        def h16(i):
            k, v = kv16[i % ring16]
            return _lib.decode_attention_h16(q16, k, v, 0.125, L=L, out=out16)

        def sdpa(i):
            k, v = kv16[i % ring16]
            return F.scaled_dot_product_attention(q16.unsqueeze(2), k[:, :, :L], v[:, :, :L], scale=0.125)

        with torch.inference_mode():
            k0, v0 = kv16[0]
            same = bool(torch.equal(h16(0), _lib.decode_attention_f32(q16.float(), k0.float(), v0.float(), 0.125, L=L).to(dtype)))
            r = {"L": L, "B": B, "H": H, "layout": layout, "ring_buffers_h16": ring16,
                 "bit_equal_f32_kernel_rounded": same,
                 "max_abs_diff_h16_vs_sdpa": float((h16(0).float() - sdpa(0).squeeze(2).float()).abs().max()),
                 "h16": event_timed(h16, args.repeat, args.warmup, args.steps, torch),
                 "sdpa_dtype": event_timed(sdpa, args.repeat, args.warmup, args.steps, torch)}
        del kv16, k0, v0
        torch.cuda.empty_cache()
        ring32, kv32 = buffers(torch.float32, 2 * n16)

        def f32(i):
            k, v = kv32[i % ring32]
            return _lib.decode_attention_f32(q32, k, v, 0.125, L=L, out=out32)

        with torch.inference_mode():
            r["f32"] = event_timed(f32, args.repeat, args.warmup, args.steps, torch)
        r["ring_buffers_f32"] = ring32
        _rates(r["h16"], n16)
        _rates(r["sdpa_dtype"], n16)
        _rates(r["f32"], 2 * n16)
        r["h16_vs_f32"] = beats(r["h16"], r["f32"])
        r["h16_vs_sdpa_dtype"] = beats(r["h16"], r["sdpa_dtype"])
        # outside the spreads: the slower arm's fastest repetition is slower than the faster arm's slowest
        r["h16_faster_than_f32_outside_the_spreads"] = bool(r["h16"]["max_s"] < r["f32"]["min_s"])
        rows.append(r)
        del kv32
        torch.cuda.empty_cache()
    return rows


def half_grouped_rows(D, dtype, args, torch, _lib, dev, B=CHUNKS, L=P):
    """(d): wx_decode_attention_h16_grouped at G in {5, 8} against the ungrouped h16 launch at B G rows
    on K / V replicated G times."""
    H = D // 64

    def halves(t):
        return tuple(t[:, :, j * D:(j + 1) * D].view(t.shape[0], L, H, 64).transpose(1, 2) for j in range(2))

    rows = []
    for G in (5, 8):
        nbytes = 2 * B * H * L * 64 * 2
        ring = max(2, min(32, -(-args.ring_bytes // (nbytes * G))))
        q = torch.randn((B, G, H, 64), device=dev).to(dtype)
        shared = [torch.randn((B, L, 2 * D), device=dev).to(dtype) for _ in range(ring)]
        out = torch.empty((B, G, H, 64), dtype=dtype, device=dev)

        def grouped(i):
            k, v = halves(shared[i % ring])
            return _lib.decode_attention_h16_grouped(q, k, v, 0.125, out=out)

        with torch.inference_mode():
            r = {"L": L, "B": B, "G": G, "H": H, "kv_bytes_shared": nbytes, "kv_bytes_replicated": nbytes * G,
                 "ring_buffers": ring, "grouped": event_timed(grouped, args.repeat, args.warmup, args.steps, torch)}
        del shared
        torch.cuda.empty_cache()
        replicated = [torch.randn((B * G, L, 2 * D), device=dev).to(dtype) for _ in range(ring)]
        qr, outr = q.view(B * G, H, 64), torch.empty((B * G, H, 64), dtype=dtype, device=dev)

        def ungrouped_bg(i):
            k, v = halves(replicated[i % ring])
            return _lib.decode_attention_h16(qr, k, v, 0.125, out=outr)

        with torch.inference_mode():
            r["ungrouped_BG_rows_replicated"] = event_timed(ungrouped_bg, args.repeat, args.warmup, args.steps, torch)
        _rates(r["grouped"], nbytes)
        r["grouped_vs_ungrouped_BG_rows"] = beats(r["grouped"], r["ungrouped_BG_rows_replicated"])
        rows.append(r)
        del replicated
        torch.cuda.empty_cache()
    return rows


def half_arm(name, g, dtype, args, torch, F, _lib, dev):
    """(d) for one geometry: the launches, then the decoder in dtype against the fp32 route in the
    same run and against transformers' decoder cast to dtype, and the peak memory of decoder + state."""
    from transformers import WhisperConfig, WhisperForConditionalGeneration

    from whisperx_amd import WhisperDecoder

    D, G = g["D"], args.beams
    sync = torch.cuda.synchronize
    eot = V - 1
    r = {"shape": {**g, "heads": D // 64, "vocab": V, "max_target_positions": T, "encoder_positions": P}}
    r["attention"] = half_attention_rows(D, dtype, args, torch, F, _lib, dev)
    r["grouped_attention"] = half_grouped_rows(D, dtype, args, torch, _lib, dev)
    print(f"{name}: launches timed", file=sys.stderr, flush=True)
    cfg = WhisperConfig(d_model=D, encoder_layers=1, encoder_attention_heads=1, encoder_ffn_dim=64, num_mel_bins=80,
                        max_source_positions=P, decoder_layers=g["layers"], decoder_attention_heads=D // 64,
                        decoder_ffn_dim=4 * D, vocab_size=V, max_target_positions=T, pad_token_id=0, bos_token_id=1,
                        eos_token_id=2, decoder_start_token_id=1)
    hf = WhisperForConditionalGeneration(cfg).eval().model.decoder
    for p in hf.parameters():
        p.requires_grad_(False)
    enc = torch.randn((CHUNKS, P, D), device=dev)
    prompt = torch.tensor([PROMPT] * CHUNKS, device=dev)
    tok = torch.full((CHUNKS,), 7, dtype=torch.int64, device=dev)
    r["memory"], decs = {}, {}
    for dt in (torch.float32, dtype):  # decoder + the state of CHUNKS x G beams, from an empty allocator
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        d = WhisperDecoder(hf, device=dev, dtype=dt)
        st = d.start(enc, beams=G)
        d.step(st, torch.full((CHUNKS * G,), 7, dtype=torch.int64, device=dev))
        sync()
        r["memory"][str(dt).replace("torch.", "")] = {
            "chunks": CHUNKS, "beams": G, "allocated_bytes": torch.cuda.memory_allocated(dev) - base,
            "max_memory_allocated_bytes": torch.cuda.max_memory_allocated(dev) - base}
        del st
        decs[dt] = d
    r["memory"]["half_over_float32_allocated"] = (r["memory"][str(dtype).replace("torch.", "")]["allocated_bytes"]
                                                  / r["memory"]["float32"]["allocated_bytes"])
    hf = hf.to(device=dev, dtype=dtype)
    print(f"{name}: decoders built", file=sys.stderr, flush=True)

    def hf_generate():
        with torch.inference_mode():
            o = hf(input_ids=prompt, encoder_hidden_states=enc.to(dtype), use_cache=True)
            steps = []
            for _ in range(N_TOKENS):
                lg = F.linear(o.last_hidden_state[:, -1], hf.embed_tokens.weight)
                lg[:, eot] = float("-inf")
                nxt = lg.argmax(-1)
                steps.append(nxt)
                if bool((nxt == eot).all()):
                    break
                if len(steps) < N_TOKENS:
                    o = hf(input_ids=nxt[:, None], encoder_hidden_states=enc.to(dtype), past_key_values=o.past_key_values,
                           use_cache=True)
            return torch.stack(steps, 1)

    kw = dict(max_length=len(PROMPT) + N_TOKENS, suppress_tokens=[eot])
    for label, d in (("half", decs[dtype]), ("float32", decs[torch.float32])):
        e = {"generated_tokens": len(d.generate(enc, PROMPT, eot, **kw)[0]),
             "generate": timed(lambda: d.generate(enc, PROMPT, eot, **kw), args.repeat, args.warmup, sync),
             "beam_search": timed(lambda: d.beam_search(enc, PROMPT, eot, beam_size=G, **kw), args.repeat, args.warmup, sync)}
        st = d.start(enc)
        for _ in range(STEP_POS):
            d.step(st, tok)

        def step(i):
            st.pos = STEP_POS
            return d._step(st, tok)

        with torch.inference_mode():
            e["step"] = event_timed(step, args.repeat, args.warmup, args.steps, torch)
        e["step"]["rows"], e["step"]["position"] = CHUNKS, STEP_POS
        r[label] = e
        del st
        torch.cuda.empty_cache()
        print(f"{name}: {label} route timed", file=sys.stderr, flush=True)
    r["beams"] = G
    r["hf_cast_generate"] = timed(hf_generate, args.repeat, args.warmup, sync)
    r["hf_cast_step_from_generate"] = {k: v / N_TOKENS for k, v in r["hf_cast_generate"].items() if k.endswith("_s")}
    for what in ("generate", "beam_search", "step"):
        r[f"{what}_half_vs_float32"] = beats(r["half"][what], r["float32"][what])
    r["generate_half_vs_hf_cast"] = beats(r["half"]["generate"], r["hf_cast_generate"])
    del hf, decs, enc
    torch.cuda.empty_cache()
    return r


def prefill_attention_rows(D, dtype, args, torch, F, _lib, dev, B=CHUNKS):
    """(e): one prefill attention launch against torch's attention with the same mask on the same views."""
    H = D // 64
    es = 4 if dtype == torch.float32 else 2
    ours_fn = _lib.prefill_attention_f32 if dtype == torch.float32 else _lib.prefill_attention_h16
    rows = []
    for kind, Tq, Tk in (("causal", 4, 4), ("causal", 224, 224), ("cross", 4, P), ("cross", 224, P)):
        pairs = sum(min(Tk, i + 1) for i in range(Tq)) if kind == "causal" else Tq * Tk  # visible (query, key) pairs
        nbytes = B * H * 64 * es * (2 * Tq + 2 * Tk)  # q and o, the K and V rows some query sees
        flop = 4 * 64 * B * H * pairs
        ring = max(2, min(32, -(-args.ring_bytes // nbytes)))
        fused = torch.randn((B, Tq, 3, H, 64), device=dev).to(dtype)
        q = fused[:, :, 0].transpose(1, 2)  # the q slice of a fused q/k/v GEMM output, in place
        kv = []
        for _ in range(ring):
            if kind == "cross":
                t = torch.randn((B, Tk, 2 * D), device=dev).to(dtype)
                kv.append(tuple(t[:, :, j * D:(j + 1) * D].view(B, Tk, H, 64).transpose(1, 2) for j in range(2)))
            else:
                kv.append(tuple(torch.randn((B, H, T, 64), device=dev).to(dtype) for _ in range(2)))
        causal = 0 if kind == "causal" else None
        mask = None if causal is None else torch.ones((Tq, Tk), dtype=torch.bool, device=dev).tril()

        def ours(i):
            k, v = kv[i % ring]
            return ours_fn(q, k, v, 0.125, causal=causal, Tk=Tk)

        def sdpa(i):
            k, v = kv[i % ring]
            return F.scaled_dot_product_attention(q, k[:, :, :Tk], v[:, :, :Tk], attn_mask=mask, scale=0.125)

        with torch.inference_mode():
            r = {"mask": kind, "Tq": Tq, "Tk": Tk, "B": B, "H": H, "ring_buffers": ring, "bytes": nbytes, "flop": flop,
                 "layout": "cross [B, Tk, 2D] halves" if kind == "cross" else "cache [B, H, 448, 64]",
                 "max_abs_diff_ours_vs_sdpa": float((ours(0).float() - sdpa(0).transpose(1, 2).float()).abs().max()),
                 "ours": event_timed(ours, args.repeat, args.warmup, args.steps, torch),
                 "sdpa": event_timed(sdpa, args.repeat, args.warmup, args.steps, torch)}
        for arm in ("ours", "sdpa"):
            r[arm]["bytes_per_s"] = nbytes / r[arm]["median_s"]
            r[arm]["share_of_hbm_peak"] = r[arm]["bytes_per_s"] / HBM_PEAK_BYTES_PER_S
            r[arm]["flop_per_s"] = flop / r[arm]["median_s"]
        r["ours"]["share_of_f32_mfma_peak"] = r["ours"]["flop_per_s"] / F32_MFMA_PEAK_FLOPS
        r["ours_vs_sdpa"] = beats(r["ours"], r["sdpa"])
        r["hbm_and_mfma_time_separated"] = "not measured"
        rows.append(r)
        del kv
        torch.cuda.empty_cache()
    return rows


def prefill_arm(name, g, half_dtype, args, torch, F, _lib, dev):
    """(e) for one geometry: the launches, then generate / beam_search / logits with and without
    prefill, in fp32 and in the half type."""
    from transformers import WhisperConfig, WhisperForConditionalGeneration

    from whisperx_amd import WhisperDecoder

    D, G = g["D"], args.beams
    sync = torch.cuda.synchronize
    eot = V - 1
    r = {"shape": {**g, "heads": D // 64, "vocab": V, "max_target_positions": T, "encoder_positions": P}, "beams": G}
    cfg = WhisperConfig(d_model=D, encoder_layers=1, encoder_attention_heads=1, encoder_ffn_dim=64, num_mel_bins=80,
                        max_source_positions=P, decoder_layers=g["layers"], decoder_attention_heads=D // 64,
                        decoder_ffn_dim=4 * D, vocab_size=V, max_target_positions=T, pad_token_id=0, bos_token_id=1,
                        eos_token_id=2, decoder_start_token_id=1)
    hf = WhisperForConditionalGeneration(cfg).eval().model.decoder
    for p in hf.parameters():
        p.requires_grad_(False)
    enc = torch.randn((CHUNKS, P, D), device=dev)
    gen = torch.Generator().manual_seed(args.seed)
    prompts = {4: PROMPT + [50363], 224: PROMPT + torch.randint(0, 50257, (221,), generator=gen).tolist()}
    forced = torch.randint(0, 50257, (CHUNKS, N_TOKENS), generator=gen)
    for dt in (torch.float32, half_dtype):
        label = str(dt).replace("torch.", "")
        e = {"attention": prefill_attention_rows(D, dt, args, torch, F, _lib, dev)}
        print(f"{name} {label}: launches timed", file=sys.stderr, flush=True)
        dec = WhisperDecoder(hf, device=dev, dtype=dt)
        for n, prompt in prompts.items():
            kw = dict(max_length=n + N_TOKENS, suppress_tokens=[eot])
            row = {"prompt_ids": n, "chunks": CHUNKS, "generated_tokens": N_TOKENS}
            for what, call in (("generate", lambda pf: dec.generate(enc, prompt, eot, prefill=pf, **kw)),
                               ("beam_search", lambda pf: dec.beam_search(enc, prompt, eot, beam_size=G, prefill=pf, **kw))):
                a, b = call(True), call(False)
                ids = (lambda x: x) if what == "generate" else (lambda x: [h[0].ids for h in x])
                row[what] = {"prefill": timed(lambda: call(True), args.repeat, args.warmup, sync),
                             "stepwise": timed(lambda: call(False), args.repeat, args.warmup, sync),
                             "rows_with_equal_ids": sum(x == y for x, y in zip(ids(a), ids(b))) / CHUNKS}
                row[what]["prefill_vs_stepwise"] = beats(row[what]["prefill"], row[what]["stepwise"])
                row[what]["saved_s_median"] = row[what]["stepwise"]["median_s"] - row[what]["prefill"]["median_s"]
            e[f"prompt_{n}"] = row
            print(f"{name} {label}: prompt of {n} timed", file=sys.stderr, flush=True)
        a, b = dec.logits(enc, forced, prefill=True), dec.logits(enc, forced, prefill=False)
        e["logits"] = {"shape": [CHUNKS, N_TOKENS], "max_abs_diff_prefill_vs_stepwise": float((a - b).abs().max()),
                       "prefill": timed(lambda: dec.logits(enc, forced, prefill=True), args.repeat, args.warmup, sync),
                       "stepwise": timed(lambda: dec.logits(enc, forced, prefill=False), args.repeat, args.warmup, sync)}
        e["logits"]["prefill_vs_stepwise"] = beats(e["logits"]["prefill"], e["logits"]["stepwise"])
        r[label] = e
        del dec, a, b
        torch.cuda.empty_cache()
    del hf, enc
    return r


def graph_arm(name, g, args, torch, _lib, dev):
    """(f) for one geometry: fp32 and float16, the direct arm and the graph arm of every figure."""
    from transformers import WhisperConfig, WhisperForConditionalGeneration

    from whisperx_amd import WhisperDecoder

    D, G, H = g["D"], args.beams, g["D"] // 64
    sync = torch.cuda.synchronize
    eot = V - 1
    r = {"shape": {**g, "heads": H, "vocab": V, "max_target_positions": T, "encoder_positions": P}, "beams": G}
    cfg = WhisperConfig(d_model=D, encoder_layers=1, encoder_attention_heads=1, encoder_ffn_dim=64, num_mel_bins=80,
                        max_source_positions=P, decoder_layers=g["layers"], decoder_attention_heads=H,
                        decoder_ffn_dim=4 * D, vocab_size=V, max_target_positions=T, pad_token_id=0, bos_token_id=1,
                        eos_token_id=2, decoder_start_token_id=1)
    hf = WhisperForConditionalGeneration(cfg).eval().model.decoder
    for p in hf.parameters():
        p.requires_grad_(False)
    enc = torch.randn((CHUNKS, P, D), device=dev)
    gen = torch.Generator().manual_seed(args.seed)
    prompts = {4: PROMPT + [50363], 224: PROMPT + torch.randint(0, 50257, (221,), generator=gen).tolist()}
    tok = torch.full((CHUNKS,), PROMPT[0], dtype=torch.int64, device=dev)
    for dt in (torch.float32, torch.float16):
        label = str(dt).replace("torch.", "")
        dec = WhisperDecoder(hf, device=dev, dtype=dt)
        sync()
        e = {"memory_allocated_bytes": {"decoder": torch.cuda.memory_allocated(dev)}}

        # the self-attention launch alone, L = 224 on 16 rows
        fused, plain = (_lib.decode_self_attention_f32, _lib.decode_attention_f32) if dt == torch.float32 else \
            (_lib.decode_self_attention_h16, _lib.decode_attention_h16)
        qkv = torch.randn((CHUNKS, 3 * D), device=dev).to(dt)
        q, k, v = (qkv[:, j * D:(j + 1) * D].view(CHUNKS, H, 64) for j in range(3))
        ck, cv = (torch.randn((CHUNKS, H, T, 64), device=dev).to(dt) for _ in range(2))
        out = torch.empty((CHUNKS, H, 64), dtype=dt, device=dev)
        pos = torch.full((1,), 223, dtype=torch.int32, device=dev)
        ws = _lib.decode_attention_workspace(CHUNKS, H, T, dev)

        def launch_fused(i):
            return fused(q, k, v, ck, cv, pos, 0.125, out=out, workspace=ws)

        def launch_copies(i):
            ck[:, :, 223].copy_(k)
            cv[:, :, 223].copy_(v)
            return plain(q, ck, cv, 0.125, L=224, out=out, workspace=ws)

        with torch.inference_mode():
            a, b = launch_fused(0).clone(), launch_copies(0).clone()
            e["self_attention_L224"] = {"rows": CHUNKS, "bit_identical": bool(torch.equal(a, b)),
                                        "fused": event_timed(launch_fused, args.repeat, args.warmup, args.steps, torch),
                                        "copies_and_attention": event_timed(launch_copies, args.repeat, args.warmup,
                                                                            args.steps, torch)}
        e["self_attention_L224"]["fused_vs_copies"] = beats(e["self_attention_L224"]["fused"],
                                                            e["self_attention_L224"]["copies_and_attention"])
        del qkv, q, k, v, ck, cv, out, ws

        # one step of 16 rows at position 35
        st = dec.start(enc)
        sync()
        e["memory_allocated_bytes"]["decoder_and_direct_state"] = torch.cuda.memory_allocated(dev)
        for _ in range(STEP_POS):
            dec.step(st, tok)

        def step(i):
            st.pos = STEP_POS
            return dec._step(st, tok)

        with torch.inference_mode():
            e["step"] = {"rows": CHUNKS, "position": STEP_POS,
                         "direct": event_timed(step, args.repeat, args.warmup, args.steps, torch)}
        del st
        torch.cuda.empty_cache()
        first = []
        for _ in range(max(1, min(3, args.repeat))):  # the first step of a fresh plan: warm-up, capture, one replay
            dec.release_graphs()
            torch.cuda.empty_cache()
            gs = dec.start(enc, graph=True)
            sync()
            t0 = time.perf_counter()
            dec.step(gs, tok)
            sync()
            first.append(time.perf_counter() - t0)
            del gs
        e["first_step_of_a_plan_ms"] = {"median": 1e3 * sorted(first)[len(first) // 2], "min": 1e3 * min(first),
                                        "max": 1e3 * max(first), "repeat": len(first)}
        gs = dec.start(enc, graph=True)
        for _ in range(STEP_POS):
            dec.step(gs, tok)
        sync()
        e["memory_allocated_bytes"]["decoder_and_plan"] = torch.cuda.memory_allocated(dev)

        def replay(i):
            gs.pos = STEP_POS
            gs.graph.pos_dev.fill_(STEP_POS)
            return dec._step(gs, tok)

        with torch.inference_mode():
            e["step"]["max_abs_diff_replay_vs_direct"] = float((replay(0) - step_once(dec, enc, tok, torch)).abs().max())
            e["step"]["replay"] = event_timed(replay, args.repeat, args.warmup, args.steps, torch)
        e["step"]["replay_vs_direct"] = beats(e["step"]["replay"], e["step"]["direct"])
        del gs
        print(f"{name} {label}: launch and step timed", file=sys.stderr, flush=True)

        kw4 = dict(max_length=4 + N_TOKENS, suppress_tokens=[eot])
        kw224 = dict(max_length=224 + N_TOKENS, suppress_tokens=[eot], prefill=True)
        for what, call in (("generate_prompt_4", lambda gr: dec.generate(enc, prompts[4], eot, graph=gr, **kw4)),
                           ("generate_prefill_224", lambda gr: dec.generate(enc, prompts[224], eot, graph=gr, **kw224)),
                           ("beam_search_prompt_4", lambda gr: dec.beam_search(enc, prompts[4], eot, beam_size=G, graph=gr, **kw4))):
            a, b = call(True), call(False)
            ids = (lambda x: x) if what.startswith("generate") else (lambda x: [h[0].ids for h in x])
            row = {"chunks": CHUNKS, "generated_tokens": N_TOKENS,
                   "rows_with_equal_ids": sum(x == y for x, y in zip(ids(a), ids(b))) / CHUNKS,
                   "graph": timed(lambda: call(True), args.repeat, args.warmup, sync),
                   "direct": timed(lambda: call(False), args.repeat, args.warmup, sync)}
            row["graph_vs_direct"] = beats(row["graph"], row["direct"])
            e[what] = row
            print(f"{name} {label}: {what} timed", file=sys.stderr, flush=True)
        e["graph_captures"] = dec.graph_captures
        r[label] = e
        dec.release_graphs()
        del dec
        torch.cuda.empty_cache()
    for what in ("generate_prompt_4", "generate_prefill_224", "beam_search_prompt_4"):
        r[f"{what}_graph_float16_vs_float32"] = beats(r["float16"][what]["graph"], r["float32"][what]["graph"])
    r["step_replay_float16_vs_float32"] = beats(r["float16"]["step"]["replay"], r["float32"]["step"]["replay"])
    del hf, enc
    return r


def sample_arm(name, g, args, torch, _lib, dev):
    """(g) for one geometry: the selection launch against the torch chain, then sample against
    beam_search and generate, direct and graph, fp32 and float16."""
    from transformers import WhisperConfig, WhisperForConditionalGeneration

    from whisperx_amd import WhisperDecoder

    D, G, H = g["D"], args.beams, g["D"] // 64
    sync = torch.cuda.synchronize
    eot = V - 1
    r = {"shape": {**g, "heads": H, "vocab": V, "max_target_positions": T, "encoder_positions": P}, "beams": G,
         "best_of": 5, "temperature": 0.6, "selection": []}
    mask = torch.zeros(V, dtype=torch.bool, device=dev)
    mask[eot] = True
    ninf = float("-inf")
    for R in (CHUNKS, CHUNKS * 5):
        for temp in (0.0, 0.6):
            ring = [3 * torch.randn((R, V), device=dev) for _ in range(8)]
            done = torch.zeros(R, dtype=torch.bool, device=dev)
            sums = torch.zeros(R, device=dev)
            token, logprob = torch.empty(R, dtype=torch.int64, device=dev), torch.empty(R, device=dev)
            step = torch.zeros(1, dtype=torch.int64, device=dev)
            ws = _lib.sample_token_workspace(R, V, dev)

            def kernel(i):
                return _lib.sample_token(ring[i % 8], step, eot, done, temp, 1, mask, sums, token=token, logprob=logprob,
                                         workspace=ws)

            def chain(i):
                m = ring[i % 8].masked_fill(mask, ninf)
                lp = torch.log_softmax(m, -1)
                tok = m.argmax(-1) if temp == 0 else torch.multinomial(torch.softmax(m / temp, -1), 1)[:, 0]
                return tok, lp.gather(1, tok[:, None])[:, 0]

            with torch.inference_mode():
                row = {"rows": R, "vocab": V, "temperature": temp, "logit_bytes": 4 * R * V}
                if temp == 0:  # (before the timed launches write the kernel's output tensors again)
                    a, b = kernel(0), chain(0)
                    row["tokens_equal"] = bool(torch.equal(a[0], b[0]))
                    row["max_abs_diff_logprob"] = float((a[1] - b[1]).abs().max())
                row["wx_sample_token"] = event_timed(kernel, args.repeat, args.warmup, args.steps, torch)
                row["torch_chain"] = event_timed(chain, args.repeat, args.warmup, args.steps, torch)
            row["wx_sample_token"]["logit_bytes_per_s"] = 4 * R * V / row["wx_sample_token"]["median_s"]
            row["wx_sample_token"]["share_of_hbm_peak"] = row["wx_sample_token"]["logit_bytes_per_s"] / HBM_PEAK_BYTES_PER_S
            row["kernel_vs_chain"] = beats(row["wx_sample_token"], row["torch_chain"])
            r["selection"].append(row)
            del ring
            torch.cuda.empty_cache()
    print(f"{name}: selection timed", file=sys.stderr, flush=True)
    cfg = WhisperConfig(d_model=D, encoder_layers=1, encoder_attention_heads=1, encoder_ffn_dim=64, num_mel_bins=80,
                        max_source_positions=P, decoder_layers=g["layers"], decoder_attention_heads=H,
                        decoder_ffn_dim=4 * D, vocab_size=V, max_target_positions=T, pad_token_id=0, bos_token_id=1,
                        eos_token_id=2, decoder_start_token_id=1)
    hf = WhisperForConditionalGeneration(cfg).eval().model.decoder
    for p in hf.parameters():
        p.requires_grad_(False)
    enc = torch.randn((CHUNKS, P, D), device=dev)
    prompt = PROMPT + [50363]
    kw = dict(max_length=len(prompt) + N_TOKENS, suppress_tokens=[eot])
    for dt in (torch.float32, torch.float16):
        label = str(dt).replace("torch.", "")
        dec = WhisperDecoder(hf, device=dev, dtype=dt)
        e = {}
        for what, call in (("sample_best_of_5", lambda gr: dec.sample(enc, prompt, eot, temperature=0.6, best_of=5, seed=3, graph=gr, **kw)),
                           ("beam_search", lambda gr: dec.beam_search(enc, prompt, eot, beam_size=G, graph=gr, **kw)),
                           ("generate", lambda gr: dec.generate(enc, prompt, eot, graph=gr, **kw))):
            a, b = call(True), call(False)
            row = {"chunks": CHUNKS, "generated_tokens": N_TOKENS, "graph_equals_direct": a == b,
                   "graph": timed(lambda: call(True), args.repeat, args.warmup, sync),
                   "direct": timed(lambda: call(False), args.repeat, args.warmup, sync)}
            row["graph_vs_direct"] = beats(row["graph"], row["direct"])
            e[what] = row
            print(f"{name} {label}: {what} timed", file=sys.stderr, flush=True)
        for route in ("graph", "direct"):
            e[f"sample_vs_beam_search_{route}"] = beats(e["sample_best_of_5"][route], e["beam_search"][route])
            e[f"sample_vs_generate_{route}"] = beats(e["sample_best_of_5"][route], e["generate"][route])
        e["graph_captures"] = dec.graph_captures
        r[label] = e
        dec.release_graphs()
        del dec
        torch.cuda.empty_cache()
    del hf, enc
    return r


PENALTY = dict(repetition_penalty=1.1, no_repeat_ngram_size=3)


def penalty_kernel_rows(args, torch, _lib, dev):
    """(h): the rewrite launch against transformers' two processors, per row count and history length."""
    from transformers import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    rho, n = PENALTY["repetition_penalty"], PENALTY["no_repeat_ngram_size"]
    chain_of = (RepetitionPenaltyLogitsProcessor(penalty=rho), NoRepeatNGramLogitsProcessor(n))
    rows = []
    for R in (CHUNKS, CHUNKS * 5):
        base = 3 * torch.randn((R, V), device=dev)
        ring = [base.clone() for _ in range(8)]
        for L in (32, 224, 447):
            ids = torch.randint(0, 300, (R, L), device=dev)  # few ids: trigrams do repeat
            hist = ids.t().contiguous()
            count = torch.tensor([L], dtype=torch.int64, device=dev)

            def kernel(i):
                return _lib.penalize_logits(ring[i % 8], hist, count, 0, L, rho, n)

            def chain(i):
                x = ring[i % 8]
                for processor in chain_of:
                    x = processor(ids, x)
                return x

            with torch.inference_mode():
                want = chain_of[1](ids, chain_of[0](ids, base))
                got = kernel_once(kernel, ring, base)
                # (the chain divides by a host scalar, which the device backend may turn into a reciprocal: one ulp)
                row = {"rows": R, "vocab": V, "history": L, "equal_to_chain": bool(torch.equal(got, want)),
                       "max_abs_diff_to_chain": float(torch.nan_to_num(got - want, nan=0.0).abs().max()),
                       "banned_columns": int(torch.isneginf(want).sum())}
                row["wx_penalize_logits"] = event_timed(kernel, args.repeat, args.warmup, args.steps, torch)
                for t in ring:  # (the kernel rewrote them in place, launch after launch)
                    t.copy_(base)
                row["torch_chain"] = event_timed(chain, args.repeat, args.warmup, min(args.steps, 10), torch)
            row["kernel_vs_chain"] = beats(row["wx_penalize_logits"], row["torch_chain"])
            rows.append(row)
            print(f"penalty kernel: {R} rows, history {L} timed", file=sys.stderr, flush=True)
        del ring, base
        torch.cuda.empty_cache()
    return rows


def kernel_once(kernel, ring, base):
    """One launch on a fresh copy of `base` (slot 0 of the ring) -> the rewritten logits."""
    ring[0].copy_(base)
    out = kernel(0).clone()
    ring[0].copy_(base)
    return out


def penalty_arm(name, g, args, torch, _lib, dev):
    """(h) for one geometry: generate and sample with graph=True, the options off, on and off again."""
    from transformers import WhisperConfig, WhisperForConditionalGeneration

    from whisperx_amd import WhisperDecoder

    D, H = g["D"], g["D"] // 64
    sync = torch.cuda.synchronize
    eot = V - 1
    r = {"shape": {**g, "heads": H, "vocab": V, "max_target_positions": T, "encoder_positions": P}, "best_of": 5,
         "temperature": 0.6, "options": PENALTY}
    cfg = WhisperConfig(d_model=D, encoder_layers=1, encoder_attention_heads=1, encoder_ffn_dim=64, num_mel_bins=80,
                        max_source_positions=P, decoder_layers=g["layers"], decoder_attention_heads=H,
                        decoder_ffn_dim=4 * D, vocab_size=V, max_target_positions=T, pad_token_id=0, bos_token_id=1,
                        eos_token_id=2, decoder_start_token_id=1)
    hf = WhisperForConditionalGeneration(cfg).eval().model.decoder
    for p in hf.parameters():
        p.requires_grad_(False)
    enc = torch.randn((CHUNKS, P, D), device=dev)
    prompt = PROMPT + [50363]
    kw = dict(max_length=len(prompt) + N_TOKENS, suppress_tokens=[eot], graph=True)
    dec = WhisperDecoder(hf, device=dev)
    for what, call in (("generate", lambda **o: dec.generate(enc, prompt, eot, **kw, **o)),
                       ("sample_best_of_5", lambda **o: dec.sample(enc, prompt, eot, temperature=0.6, best_of=5, seed=3, **kw, **o))):
        on, off = call(**PENALTY), call()
        row = {"chunks": CHUNKS, "generated_tokens": N_TOKENS, "options_change_the_result": on != off}
        row["off"] = timed(lambda: call(), args.repeat, args.warmup, sync)
        row["on"] = timed(lambda: call(**PENALTY), args.repeat, args.warmup, sync)
        row["off_again"] = timed(lambda: call(), args.repeat, args.warmup, sync)
        row["on_vs_off"] = beats(row["on"], row["off"])
        row["on_minus_off_per_token_s"] = (row["on"]["median_s"] - row["off"]["median_s"]) / N_TOKENS
        r[what] = row
        print(f"{name}: {what} timed", file=sys.stderr, flush=True)
    r["graph_captures"] = dec.graph_captures
    dec.release_graphs()
    del dec, hf, enc
    torch.cuda.empty_cache()
    return r


def step_once(dec, enc, tok, torch):
    """The logits of a direct state's step at STEP_POS after STEP_POS steps on `tok`."""
    st = dec.start(enc)
    for _ in range(STEP_POS):
        dec.step(st, tok)
    return dec.step(st, tok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="float32", choices=["float32", "float16", "bfloat16"],
                    help="float16 / bfloat16: (d), the half route's record (profiles/whisper_decoder_half*_<host>.json)")
    ap.add_argument("--arms", default="decoder", choices=["decoder", "beam", "prefill", "graph", "sample", "penalty"],
                    help="(a) and (b), (c), (e), (f), (g) or (h)")
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--geometries", default="base,large-v2")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50, help="launches per repetition of the attention and step arms")
    ap.add_argument("--ring-bytes", type=int, default=1 << 30, help="key / value bytes the attention arms cycle through")
    ap.add_argument("--seed", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from transformers import WhisperConfig, WhisperForConditionalGeneration

    from whisperx_amd import WhisperDecoder, _lib

    if not torch.cuda.is_available():
        raise SystemExit("whisper_decoder_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    result = {"tool": "tools/whisper_decoder_bench.py", "device": torch.cuda.get_device_name(0),
              "lib": os.path.basename(_lib.LIB_PATH), "dtype": "float32", "decode_chunk": _lib.DECODE_CHUNK,
              "peaks": {"hbm_bytes_per_s": HBM_PEAK_BYTES_PER_S}, "geometries": {}}
    if args.arms == "prefill":
        result["peaks"]["f32_mfma_flop_per_s"] = F32_MFMA_PEAK_FLOPS
        half = getattr(torch, args.dtype if args.dtype != "float32" else "float16")
        result["dtype"] = ["float32", str(half).replace("torch.", "")]
        for name in args.geometries.split(","):
            torch.manual_seed(args.seed)
            result["geometries"][name] = prefill_arm(name, GEOMETRIES[name], half, args, torch, F, _lib, dev)
        args.geometries = ""
    if args.arms == "graph":
        result["dtype"] = ["float32", "float16"]
        for name in args.geometries.split(","):
            torch.manual_seed(args.seed)
            result["geometries"][name] = graph_arm(name, GEOMETRIES[name], args, torch, _lib, dev)
        args.geometries = ""
    if args.arms == "sample":
        result["dtype"] = ["float32", "float16"]
        for name in args.geometries.split(","):
            torch.manual_seed(args.seed)
            result["geometries"][name] = sample_arm(name, GEOMETRIES[name], args, torch, _lib, dev)
        args.geometries = ""
    if args.arms == "penalty":
        torch.manual_seed(args.seed)
        result["kernel"] = penalty_kernel_rows(args, torch, _lib, dev)
        for name in args.geometries.split(","):
            torch.manual_seed(args.seed)
            result["geometries"][name] = penalty_arm(name, GEOMETRIES[name], args, torch, _lib, dev)
        args.geometries = ""
    eot = V - 1  # suppressed: both greedy loops run their full length
    if args.dtype != "float32":
        result["dtype"] = args.dtype
    for name in filter(None, args.geometries.split(",")):
        g = GEOMETRIES[name]
        if args.dtype != "float32":
            torch.manual_seed(args.seed)
            result["geometries"][name] = half_arm(name, g, getattr(torch, args.dtype), args, torch, F, _lib, dev)
            continue
        if args.arms == "beam":
            torch.manual_seed(args.seed)
            result["geometries"][name] = beam_arm(name, g, args, torch, _lib, dev)
            continue
        D = g["D"]
        torch.manual_seed(args.seed)
        r = {"shape": {**g, "heads": D // 64, "vocab": V, "max_target_positions": T, "encoder_positions": P}}
        r["attention"] = attention_rows(D, args, torch, F, _lib, dev)
        cfg = WhisperConfig(d_model=D, encoder_layers=1, encoder_attention_heads=1, encoder_ffn_dim=64, num_mel_bins=80,
                            max_source_positions=P, decoder_layers=g["layers"], decoder_attention_heads=D // 64,
                            decoder_ffn_dim=4 * D, vocab_size=V, max_target_positions=T, pad_token_id=0, bos_token_id=1,
                            eos_token_id=2, decoder_start_token_id=1)
        hf = WhisperForConditionalGeneration(cfg).eval().model.decoder.to(dev)
        for p in hf.parameters():
            p.requires_grad_(False)
        r["shape"]["attn_implementation"] = cfg._attn_implementation
        ours = WhisperDecoder(hf, device=dev)
        enc = torch.randn((CHUNKS, P, D), device=dev)
        prompt = torch.tensor([PROMPT] * CHUNKS, device=dev)

        def hf_generate():
            with torch.inference_mode():
                o = hf(input_ids=prompt, encoder_hidden_states=enc, use_cache=True)
                steps = []
                for _ in range(N_TOKENS):
                    lg = F.linear(o.last_hidden_state[:, -1], hf.embed_tokens.weight)
                    lg[:, eot] = float("-inf")
                    nxt = lg.argmax(-1)
                    steps.append(nxt)
                    if bool((nxt == eot).all()):
                        break
                    if len(steps) < N_TOKENS:
                        o = hf(input_ids=nxt[:, None], encoder_hidden_states=enc, past_key_values=o.past_key_values,
                               use_cache=True)
                return torch.stack(steps, 1)

        def ours_generate():
            return ours.generate(enc, PROMPT, eot, max_length=len(PROMPT) + N_TOKENS, suppress_tokens=[eot])

        got, want = torch.tensor(ours_generate()), hf_generate().cpu()
        r["generated_tokens"] = int(got.shape[1])
        r["greedy_tokens_equal_hf"] = float((got == want).float().mean())  # (fp32 against fp32 on flat random logits)
        r["generate"] = timed(ours_generate, args.repeat, args.warmup, sync)
        r["hf_generate"] = timed(hf_generate, args.repeat, args.warmup, sync)
        r["generate_vs_hf"] = beats(r["generate"], r["hf_generate"])
        r["hf_step_from_generate"] = {k: v / N_TOKENS for k, v in r["hf_generate"].items() if k.endswith("_s")}
        st = ours.start(enc)
        tok = torch.full((CHUNKS,), 7, dtype=torch.int64, device=dev)
        for _ in range(STEP_POS):
            ours.step(st, tok)

        def step(i):
            st.pos = STEP_POS
            return ours._step(st, tok)

        with torch.inference_mode():
            r["step"] = event_timed(step, args.repeat, args.warmup, args.steps, torch)
        r["step"]["rows"], r["step"]["position"] = CHUNKS, STEP_POS
        result["geometries"][name] = r
        del hf, ours, enc, st
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

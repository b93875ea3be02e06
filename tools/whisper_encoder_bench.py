#!/usr/bin/env python3
"""Times of Whisper's audio encoder on 30 s windows (no threshold: a record).

Random weights in two geometries (--geometries, comma separated):
  base      D 512, 6 layers, 80 mels, one hour of audio = 151 chunks
  large-v2  D 1280, 32 layers, 80 mels, 32 chunks
Features are 0.5 randn - 0.5, [chunks, 80, 3000], resident on the device.

Arms per geometry, each the median of --repeat warm repetitions (with min and max, the spread a
difference has to exceed), a repetition being every chunk in batches of --batch-size, synchronised:
  ours        whisperx_amd.WhisperEncoder.encode (wx_whisper_stem, one q/k/v GEMM, wx_attention_f32,
              wx_add_layernorm)
  hf          transformers' fp32 WhisperEncoder with its default attention, same device, same batches
  stem        wx_whisper_stem alone on one batch, between device events over --steps launches
  torch_stem  the same stem through torch (conv1d, gelu, conv1d, gelu, permute, add), likewise

The stem arm also reports what the algorithm needs from the shapes: FLOP (2 x 3 x (n_mels + D) x D
per input / output row pair) over the fp32 MFMA peak as a share of the measured time.  Prints one
JSON line; --out writes it to a file (profiles/whisper_encoder_<host>.json).

--dtype float16 | bfloat16 measures the half route instead (profiles/whisper_encoder_half_<host>.json):
  attention   B 16, T 1500, H 8 and H 20 on the three views of a fused [B, T, 3 x 64 H] buffer of
              that type, between device events over --steps launches: wx_attention_h16, torch's
              scaled_dot_product_attention on the same views, and wx_attention_f32 on fp32 copies of
              them; each with its TFLOP/s for 4 T^2 64 B H and its share of the 16-bit MFMA peak
  encode      per geometry: WhisperEncoder(dtype).encode, this repository's fp32 encode in the same
              run, and transformers' WhisperEncoder cast to the type (sdpa), same device and batches
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from benchlib import beats, event_timed, timed  # noqa: E402

F32_MFMA_PEAK_FLOPS = 157.3e12  # MI355X v_mfma_f32_*_f32, spec
H16_MFMA_PEAK_FLOPS = 2.5e15    # MI355X dense f16 / bf16 MFMA, spec
GEOMETRIES = {"base": {"D": 512, "layers": 6, "n_mels": 80, "chunks": 151},
              "large-v2": {"D": 1280, "layers": 32, "n_mels": 80, "chunks": 32}}
P = 1500


def half_main(args):
    """The --dtype float16 / bfloat16 record."""
    import torch
    import torch.nn.functional as F
    from transformers import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoder as HFEncoder

    from whisperx_amd import WhisperEncoder, _lib

    if not torch.cuda.is_available():
        raise SystemExit("whisper_encoder_bench: needs a HIP device")
    dtype = getattr(torch, args.dtype)
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    bs = args.batch_size
    result = {"tool": "tools/whisper_encoder_bench.py", "device": torch.cuda.get_device_name(0),
              "lib": os.path.basename(_lib.LIB_PATH), "batch_size": bs, "dtype": args.dtype,
              "peaks": {"f32_mfma_flop_per_s": F32_MFMA_PEAK_FLOPS, "h16_mfma_flop_per_s": H16_MFMA_PEAK_FLOPS},
              "attention": {}, "geometries": {}}
    torch.manual_seed(args.seed)
    for H in (8, 20):
        B, D = 16, 64 * H
        qkv = torch.randn((B, P, 3 * D), device=dev).to(dtype)
        q, k, v = (qkv[..., j * D:(j + 1) * D].view(B, P, H, 64).transpose(1, 2) for j in range(3))
        q32, k32, v32 = (t.float() for t in (q, k, v))
        flop = 4 * P * P * 64 * B * H
        arms = {"wx_attention_h16": lambda i: _lib.attention_h16(q, k, v, 0.125),
                "sdpa": lambda i: F.scaled_dot_product_attention(q, k, v, scale=0.125),
                "wx_attention_f32": lambda i: _lib.attention_f32(q32, k32, v32, 0.125)}
        r = {"shape": {"B": B, "H": H, "T": P, "flop": flop}}
        with torch.inference_mode():
            ref = F.scaled_dot_product_attention(q, k, v, scale=0.125).transpose(1, 2).float()
            r["max_abs_diff_h16_vs_sdpa"] = float((_lib.attention_h16(q, k, v, 0.125).float() - ref).abs().max())
            for arm, fn in arms.items():
                t = event_timed(fn, args.repeat, args.warmup, args.steps, torch)
                t["tflop_per_s"] = flop / t["median_s"] / 1e12
                t["h16_mfma_peak_share"] = flop / t["median_s"] / H16_MFMA_PEAK_FLOPS
                r[arm] = t
        r["h16_vs_sdpa"] = beats(r["wx_attention_h16"], r["sdpa"])
        r["h16_vs_f32"] = beats(r["wx_attention_h16"], r["wx_attention_f32"])
        result["attention"][f"H{H}"] = r
        del qkv, q, k, v, q32, k32, v32, ref
        torch.cuda.empty_cache()
    for name in args.geometries.split(","):
        g = GEOMETRIES[name]
        D, M, B = g["D"], g["n_mels"], g["chunks"]
        torch.manual_seed(args.seed)
        cfg = WhisperConfig(d_model=D, encoder_layers=g["layers"], encoder_attention_heads=D // 64, encoder_ffn_dim=4 * D,
                            num_mel_bins=M, max_source_positions=P, decoder_layers=1, decoder_attention_heads=1,
                            decoder_ffn_dim=64, vocab_size=64, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                            decoder_start_token_id=1, attn_implementation="sdpa")
        hf = HFEncoder(cfg).eval().to(dev)
        for p in hf.parameters():
            p.requires_grad_(False)
        ours32, ours = WhisperEncoder(hf, device=dev), WhisperEncoder(hf, device=dev, dtype=dtype)
        hf = hf.to(dtype)
        x = 0.5 * torch.randn((B, M, 2 * P), device=dev) - 0.5
        xh = x.to(dtype)
        r = {"shape": {**g, "frames_per_chunk": 2 * P, "positions": P, "attn_implementation": cfg._attn_implementation}}

        def hf_arm():
            with torch.inference_mode():
                return torch.cat([hf(xh[a:a + bs]).last_hidden_state for a in range(0, B, bs)])

        got, got32, want = ours.encode(x, batch_size=bs), ours32.encode(x, batch_size=bs), hf_arm()
        sync()
        r["max_abs_diff_half_vs_fp32"] = float((got - got32).abs().max())
        r["max_abs_diff_hf_half_vs_fp32"] = float((want.float() - got32).abs().max())
        del got, got32, want
        r["ours_half"] = timed(lambda: ours.encode(x, batch_size=bs), args.repeat, args.warmup, sync)
        r["ours_fp32"] = timed(lambda: ours32.encode(x, batch_size=bs), args.repeat, args.warmup, sync)
        r["hf_half"] = timed(hf_arm, args.repeat, args.warmup, sync)
        r["half_vs_fp32"] = beats(r["ours_half"], r["ours_fp32"])
        r["half_vs_hf_half"] = beats(r["ours_half"], r["hf_half"])
        result["geometries"][name] = r
        del hf, ours, ours32, x, xh
        torch.cuda.empty_cache()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometries", default="base,large-v2")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10, help="stem launches per stem-arm repetition")
    ap.add_argument("--seed", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", choices=("float32", "float16", "bfloat16"), default="float32")
    args = ap.parse_args()
    if args.dtype != "float32":
        return emit(half_main(args), args.out)
    import torch
    import torch.nn.functional as F
    from transformers import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoder as HFEncoder

    from whisperx_amd import WhisperEncoder, _lib

    if not torch.cuda.is_available():
        raise SystemExit("whisper_encoder_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    bs = args.batch_size
    result = {"tool": "tools/whisper_encoder_bench.py", "device": torch.cuda.get_device_name(0),
              "lib": os.path.basename(_lib.LIB_PATH), "batch_size": bs, "dtype": "float32",
              "peaks": {"f32_mfma_flop_per_s": F32_MFMA_PEAK_FLOPS}, "geometries": {}}
    for name in args.geometries.split(","):
        g = GEOMETRIES[name]
        D, M, B = g["D"], g["n_mels"], g["chunks"]
        torch.manual_seed(args.seed)
        cfg = WhisperConfig(d_model=D, encoder_layers=g["layers"], encoder_attention_heads=D // 64, encoder_ffn_dim=4 * D,
                            num_mel_bins=M, max_source_positions=P, decoder_layers=1, decoder_attention_heads=1,
                            decoder_ffn_dim=64, vocab_size=64, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                            decoder_start_token_id=1)
        hf = HFEncoder(cfg).eval().to(dev)
        for p in hf.parameters():
            p.requires_grad_(False)
        ours = WhisperEncoder(hf, device=dev)
        x = 0.5 * torch.randn((B, M, 2 * P), device=dev) - 0.5
        r = {"shape": {**g, "frames_per_chunk": 2 * P, "positions": P, "attn_implementation": cfg._attn_implementation}}

        def hf_arm():
            with torch.inference_mode():
                return torch.cat([hf(x[a:a + bs]).last_hidden_state for a in range(0, B, bs)])

        def torch_stem(xb):
            h = F.gelu(F.conv1d(xb, hf.conv1.weight, hf.conv1.bias, padding=1))
            h = F.gelu(F.conv1d(h, hf.conv2.weight, hf.conv2.bias, stride=2, padding=1))
            return h.permute(0, 2, 1) + hf.embed_positions.weight

        got, want = ours.encode(x, batch_size=bs), hf_arm()
        sync()
        r["max_abs_diff_ours_vs_hf"] = float((got - want).abs().max())
        del got, want
        r["ours"] = timed(lambda: ours.encode(x, batch_size=bs), args.repeat, args.warmup, sync)
        r["hf"] = timed(hf_arm, args.repeat, args.warmup, sync)
        r["ours_vs_hf"] = beats(r["ours"], r["hf"])
        xb = x[:bs]
        nb = int(xb.shape[0])
        out = torch.empty((nb, P, D), dtype=torch.float32, device=dev)
        with torch.inference_mode():
            r["max_abs_diff_stem_vs_torch"] = float((ours.stem(xb, out) - torch_stem(xb)).abs().max())
            r["stem"] = event_timed(lambda i: ours.stem(xb, out), args.repeat, args.warmup, args.steps, torch)
            r["torch_stem"] = event_timed(lambda i: torch_stem(xb), args.repeat, args.warmup, args.steps, torch)
        r["stem"]["chunks"] = r["torch_stem"]["chunks"] = nb
        r["stem"]["algorithmic_flop"] = nb * (2 * 3 * M * D * 2 * P + 2 * 3 * D * D * P)
        r["stem"]["f32_mfma_time_share"] = r["stem"]["algorithmic_flop"] / F32_MFMA_PEAK_FLOPS / r["stem"]["median_s"]
        r["stem_vs_torch_stem"] = beats(r["stem"], r["torch_stem"])
        result["geometries"][name] = r
        del hf, ours, x, out
        torch.cuda.empty_cache()
    emit(result, args.out)


def emit(result, out):
    print(json.dumps(result))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

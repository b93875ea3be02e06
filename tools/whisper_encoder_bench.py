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
GEOMETRIES = {"base": {"D": 512, "layers": 6, "n_mels": 80, "chunks": 151},
              "large-v2": {"D": 1280, "layers": 32, "n_mels": 80, "chunks": 32}}
P = 1500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometries", default="base,large-v2")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10, help="stem launches per stem-arm repetition")
    ap.add_argument("--seed", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
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
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

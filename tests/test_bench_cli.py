"""bench.py's command line: a plain run measures the headline only and --dump-outputs writes
what the last timed step returned; everything else sits behind --full."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("seg_start", "seg_end", "seg_score", "t_start", "status")


def test_dump_outputs_writes_float64_and_zeroes_unaligned_segments(tmp_path):
    import bench

    # three segments of 2, 3 and 1 tokens; the middle one did not align (outcome 1, a route flag set)
    plan = SimpleNamespace(
        b=SimpleNamespace(S=3, tok_off=[0, 2, 5, 6]),
        seg_start=torch.tensor([1, 4, 77, 78, 79, 9, -5], dtype=torch.int32),  # one slot past the tokens
        seg_end=torch.tensor([3, 8, 77, 78, 79, 12, -5], dtype=torch.int32),
        seg_score=torch.tensor([0.5, 0.25, 7.0, 7.0, 7.0, 0.125, -5.0], dtype=torch.float64),
        t_start=torch.tensor([0, 55, 2], dtype=torch.int32),
        status=torch.tensor([0, 1 | 32, 16], dtype=torch.int32))
    bench.dump_outputs(plan, str(tmp_path / "out"))
    got = {k: np.load(tmp_path / "out" / f"{k}.npy") for k in NAMES}
    assert sorted(os.listdir(tmp_path / "out")) == sorted(k + ".npy" for k in NAMES)
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["seg_start"].tolist() == [1, 4, 0, 0, 0, 9]
    assert got["seg_end"].tolist() == [3, 8, 0, 0, 0, 12]
    assert got["seg_score"].tolist() == [0.5, 0.25, 0, 0, 0, 0.125]
    assert got["t_start"].tolist() == [0, 0, 2]
    assert got["status"].tolist() == [0, 33, 16]


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_steps_outputs(tmp_path):
    """One plain run of the benchmark itself: the line carries the headline fields and none of
    the --full legs, --steps is the number of timed steps, and the dumped arrays are the fused
    DP's results on the seeded batch (recomputed here with _lib.align_dp)."""
    import bench
    from whisperx_amd import _lib

    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "audio-sec/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(64 * 1499 * bench.FRAME_S / (line["ms_per_step"] / 1000.0), rel=1e-9)
    for k in ("cpu_baseline", "mae_ms", "mae_e2e_ms"):
        assert k not in line
    assert line["extra"] == {}

    dev = torch.device("cuda", 0)
    ems, toks = bench.make_batch(np.random.default_rng(1000), 64, 1499, len(bench.W2V_VOCAB), 300, 500, dev)
    b = _lib.Batch(ems, toks, [0] * len(ems), device=dev)
    ref = dict(zip(NAMES, (x.cpu().numpy() for x in _lib.align_dp(b))))
    assert bool(_lib.status_ok(ref["status"]).all())
    n_tok = b.tok_off[-1]
    for k in NAMES:
        got = np.load(out / f"{k}.npy")
        assert got.dtype == np.float64
        assert np.array_equal(got, ref[k][: n_tok if k.startswith("seg_") else b.S].astype(np.float64)), k

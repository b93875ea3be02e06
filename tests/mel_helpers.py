"""tests/golden/mel_cases.npz (made from the reference by tests/golden/make_mel_golden.py), as the
mel tests read it."""
import os

import numpy as np

from conftest import GOLDEN

HOP = 160


class MelCases:
    def __init__(self):
        self.d = np.load(os.path.join(GOLDEN, "mel_cases.npz"))
        self.n = int(self.d["n_cases"])
        self.names = [str(s) for s in self.d["names"]]
        self.ref_err = float(self.d["ref_err"])
        # the tolerance is measured, not chosen: 4 x the reference's own largest distance from
        # the fp64 evaluation (make_mel_golden.py asserts it stays below fp16's spacing 2**-11)
        self.tol = 4.0 * self.ref_err
        assert self.tol == float(self.d["tol"]) and self.tol < 2.0 ** -11

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        d, p = self.d, f"c{i:02d}_"
        src = int(d[p + "x_of"]) if p + "x_of" in d.files else i
        x = d[f"c{src:02d}_x"].astype(np.float32) / np.float32(32768.0)
        ref = d[p + "ref"]
        c = {"name": self.names[i], "x": x, "n_mels": int(d[p + "n_mels"]), "padding": int(d[p + "padding"]),
             "frames": d[p + "frames"].astype(np.int64), "ref": ref,
             "f64": ref.astype(np.float64) + d[p + "d64"].astype(np.float64) / 2.0 ** 24,
             "floor_from": int(d[p + "floor_from"]), "n_frames": (len(x) + int(d[p + "padding"])) // HOP}
        if p + "floor_f64" in d.files:
            c["floor_ref"] = float(d[p + "floor_ref"])
            c["floor_f64"] = float(d[p + "floor_f64"])
        return c


def check_against_f64(got, c, tol):
    """`got` [n_mels, n_frames] (numpy) against case c's fp64 column at the stored frames, and the
    floor value on every frame past the stored prefix.  Returns the largest error."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (c["n_mels"], c["n_frames"]), (c["name"], got.shape)
    err = float(np.abs(got[:, c["frames"]] - c["f64"]).max()) if len(c["frames"]) else 0.0
    if c["floor_from"] < c["n_frames"]:
        err = max(err, float(np.abs(got[:, c["floor_from"]:] - c["floor_f64"]).max()))
    assert err <= tol, (c["name"], err, tol)
    return err

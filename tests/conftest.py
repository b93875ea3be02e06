import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (HIP device) — run with -m gpu")


def ulp_diff(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


class DPCases:
    """tests/golden/dp_cases_*.npz, produced from the reference by make_golden.py: whole cases
    per part (each part under the size limit for a committed file), n_cases in every part."""

    def __init__(self):
        import glob

        self.parts = [np.load(f) for f in sorted(glob.glob(os.path.join(GOLDEN, "dp_cases_*.npz")))]
        self.n = int(self.parts[0]["n_cases"])
        assert {k[:4] for d in self.parts for k in d.files if k != "n_cases"} == {f"c{i:03d}" for i in range(self.n)}

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        p = f"c{i:03d}_"
        return {k[len(p):]: d[k] for d in self.parts for k in d.files if k.startswith(p)}


@pytest.fixture(scope="session")
def dp_cases():
    return DPCases()

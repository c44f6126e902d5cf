"""The exact-tie file once more on the paths a small index does not choose by itself.

tests/test_knn_lattice_gpu.py reaches the int8 batch scan, the one-launch sweep cascade for 2..4 queries and the int8-MFMA
sweep only on its one 100 000-row case; the switches that select them are read once per process, so (as
tests/test_knn_i8_forced_gpu.py does for the parity suite) the file runs again in a fresh child ``pytest`` per setting:

* CSS_KNN_SCAN=i8 with CSS_KNN_QREG=1 CSS_KNN_QREG_MIN=0 (every later stage on k_scan_qreg_i8) and with CSS_KNN_QREG=0
  (every stage on k_scan_coarse8): the batched inner-product searches on the int8 rows -- on family T a band of the floor
  term alone, which holds exactly the ties of the k-th best;
* CSS_KNN_SWEEP_FUSED=2 (every 1..4-query search as ONE persistent launch) and 0 (the launch-per-stage cascade);
* CSS_KNN_SWEEP_MFMA=2 (every 3..32-query inner-product search on the int8-MFMA sweep) and 0 (what it replaces).

Every pass leaves out what no switch reaches: the merge kernels on made-up lists (no index) and ``range_search`` (its own
exact fp32 sweep).  The CSS_KNN_SWEEP_MFMA passes also leave out the 100 000-row case, which asserts the paths that
``auto`` chooses BY ITSELF.

Wall times on the MI355X (one process each, start-up and the CPU truth included): tests/test_knn_lattice_gpu.py alone
10 s of pytest time, 11 s of wall time (156 tests; the slowest, the full grid on 20 000 x 768 in exact_fp32, 2 s; the
100 000-row case 0.4 s); the six passes 10.8 / 11.8 / 11.2 / 11.3 / 11.0 / 11.2 s in the order above, 67 s together --
against 186 s (81 + 57 + 10 + 38) for tests/test_knn_i8_forced_gpu.py with the same library in the same session, so no
pass needed trimming beyond the filters above."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
REACHED = "not merge_kernels and not range_search"
SETTINGS = [
    ({"CSS_KNN_SCAN": "i8", "CSS_KNN_QREG": "1", "CSS_KNN_QREG_MIN": "0"}, REACHED),
    ({"CSS_KNN_SCAN": "i8", "CSS_KNN_QREG": "0"}, REACHED),
    ({"CSS_KNN_SWEEP_FUSED": "2"}, REACHED),
    ({"CSS_KNN_SWEEP_FUSED": "0"}, REACHED),
    ({"CSS_KNN_SWEEP_MFMA": "2"}, REACHED + " and not 100k_rows"),
    ({"CSS_KNN_SWEEP_MFMA": "0"}, REACHED + " and not 100k_rows"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("switches,keep", SETTINGS, ids=[" ".join(f"{a}={b}" for a, b in s.items()) for s, _ in SETTINGS])
def test_lattice_suite_with_a_path_forced(switches, keep):
    env = dict(os.environ, **switches)
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_knn_lattice_gpu.py"), "-q", "-x", "-m", "gpu",
                        "-p", "no:cacheprovider", "-k", keep], cwd=str(ROOT), env=env, capture_output=True, text=True,
                       timeout=600)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, f"test_knn_lattice_gpu.py under {switches} failed:\n{tail}\n{r.stderr[-2000:]}"
    assert " passed" in tail

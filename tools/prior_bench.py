#!/usr/bin/env python3
"""Time IndexFlat.search_prior against its sibling, the exact fp32 top-k search (k_scan_small), in ONE process and run.

    python tools/prior_bench.py --out profiles/search_prior_1M.json

1 M x 768 device-generated unit rows with uniform [0, 1) priors, k = 10, for 1 and for 16 queries.  Both calls wait for
the device before they return, so the host clock around a call is the call time (upload of the queries, sweep, merge,
results back: WHOLE-CALL times, not kernel times).  Both are warmed up; then windows of at least --window seconds of
back-to-back calls alternate: baseline, prior, baseline, prior, ...  Reported per shape: the mean call time of every
window, the medians, the spread of the baseline windows among themselves (what a difference has to exceed), and the
bytes per second the sweep's algorithmic reads amount to over the whole call (4 * dpad per row, + 4 for the prior).
A third kind of window calls css_index_search_prior with S = NULL (the raw scores are formed, not copied back): it
separates the copy of the third result column from the extra launch.
Needs a GPU; there is no fallback."""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from claude_semantic_search_amd import _native as nat  # noqa: E402
from claude_semantic_search_amd.flat_index import IndexFlatIP  # noqa: E402
from oracle import knn_oracle as ko  # noqa: E402


def window(f, seconds):
    """Mean milliseconds per call over at least `seconds` of back-to-back calls."""
    n, t0 = 0, time.perf_counter()
    while True:
        f()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e3, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--weight", type=float, default=0.05)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d, k, n = 768, 10, a.rows
    ix = IndexFlatIP(d)
    ix.reserve(n)
    ix.add_synthetic(n, seed=1, first_row=0, normalize=True)
    ix.set_priors(np.random.default_rng(3).random(n, dtype=np.float32))
    ix.set_search_mode("exact_fp32")
    q = ko.normalize_rows(ko.synth_rows(16, d, 2))
    out = {"rows": n, "dim": d, "k": k, "weight": a.weight, "window_s": a.window}
    for nq in (1, 16):
        base = lambda: ix.search(q[:nq], k)                          # noqa: E731
        prior = lambda: ix.search_prior(q[:nq], k, a.weight)         # noqa: E731
        Dn, In = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
        qn = np.ascontiguousarray(q[:nq])

        def prior_no_s():
            nat.check(nat.lib().css_index_search_prior(ix._handle(), qn.ctypes.data, nq, k, ctypes.c_float(a.weight), 0, None,
                                                       Dn.ctypes.data, In.ctypes.data, None))
        for _ in range(20):
            base()
            prior()
            prior_no_s()
        assert np.array_equal(In, ix.search_prior(q[:nq], k, a.weight)[1])
        D0, I0, S0 = ix.search_prior(q[:nq], k, 0.0)                 # same rows, same bits at weight 0
        Db, Ib = ix.search(q[:nq], k)
        assert np.array_equal(I0, Ib) and np.array_equal(D0.view(np.uint32), Db.view(np.uint32)) and np.array_equal(S0, D0)
        tb, tp, tn = [], [], []
        for _ in range(a.repeats):
            tb.append(window(base, a.window))
            tp.append(window(prior, a.window))
            tn.append(window(prior_no_s, a.window))
        mb, mp = statistics.median(t for t, _ in tb), statistics.median(t for t, _ in tp)
        out[f"nq{nq}"] = {
            "exact_fp32_ms_per_window": [round(t, 5) for t, _ in tb], "search_prior_ms_per_window": [round(t, 5) for t, _ in tp],
            "search_prior_without_S_ms_per_window": [round(t, 5) for t, _ in tn],
            "search_prior_without_S_median_ms": statistics.median(t for t, _ in tn),
            "calls_per_window": [c for _, c in tb] + [c for _, c in tp] + [c for _, c in tn],
            "exact_fp32_median_ms": mb, "search_prior_median_ms": mp, "ratio": mp / mb,
            "baseline_spread": (max(t for t, _ in tb) - min(t for t, _ in tb)) / mb,
            "prior_spread": (max(t for t, _ in tp) - min(t for t, _ in tp)) / mp,
            "exact_fp32_GBps_whole_call": n * d * 4 / mb / 1e6, "search_prior_GBps_whole_call": n * (d * 4 + 4) / mp / 1e6,
        }
    ix.close()
    print(json.dumps(out))
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time IndexFlat.search_examples against the exact fp32 top-k search of as many queries (k_scan_small at the same NQ:
the same dot products per row, m lists instead of one), in ONE process and run.

    python tools/examples_bench.py --out profiles/search_examples_1M.json

1 M x 768 device-generated unit rows, k = 10, m = 1, 3, 8, 16 examples (the first half positive, at least one; the rest
negative; all given as vectors).  Both calls wait for the device before they return, so the host clock around a call is
the call time (examples up, sweep, merge, results back: WHOLE-CALL times, not kernel times).  Both are warmed up; then
windows of at least --window seconds of back-to-back calls alternate: baseline, examples, examples without S, ...
Reported per m: the mean call time of every window, the medians, their ratio, the spread of the baseline windows among
themselves (what a difference has to exceed), and the bytes per second the sweep's algorithmic reads (4 * dpad per row)
amount to over the whole call.  The third kind of window calls css_index_search_examples with S = NULL, which skips
k_example_scores and the copy of the third column: the difference isolates them.
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
    ap.add_argument("--gamma", type=float, default=0.5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d, k, n = 768, 10, a.rows
    ix = IndexFlatIP(d)
    ix.reserve(n)
    ix.add_synthetic(n, seed=1, first_row=0, normalize=True)
    ix.set_search_mode("exact_fp32")
    q = ko.normalize_rows(ko.synth_rows(16, d, 2))
    out = {"rows": n, "dim": d, "k": k, "gamma": a.gamma, "window_s": a.window}
    for m in (1, 3, 8, 16):
        npos = max(1, m // 2)
        qm = np.ascontiguousarray(q[:m])
        base = lambda: ix.search(qm, k)                                                       # noqa: E731
        ex = lambda: ix.search_examples(qm[:npos], qm[npos:], k=k, gamma=a.gamma)             # noqa: E731
        Dn, In = np.empty(k, np.float32), np.empty(k, np.int64)

        def ex_no_s():
            nat.check(nat.lib().css_index_search_examples(ix._handle(), qm.ctypes.data, npos, m - npos, None, 0, 0, k,
                                                          ctypes.c_float(a.gamma), 0, 1, None, Dn.ctypes.data, In.ctypes.data, None))
        for _ in range(20):
            base()
            ex()
            ex_no_s()
        De, Ie, Se = ex()
        assert np.array_equal(In, Ie) and np.array_equal(Dn.view(np.uint32), De.view(np.uint32))
        if m == 1:   # one positive: the exact search, bit for bit
            Db, Ib = base()
            assert np.array_equal(Ie, Ib[0]) and np.array_equal(De.view(np.uint32), Db[0].view(np.uint32)) and np.array_equal(Se, De)
        tb, te, tn = [], [], []
        for _ in range(a.repeats):
            tb.append(window(base, a.window))
            te.append(window(ex, a.window))
            tn.append(window(ex_no_s, a.window))
        mb, me, mn = (statistics.median(t for t, _ in ts) for ts in (tb, te, tn))
        out[f"m{m}"] = {
            "npos": npos, "nneg": m - npos,
            "exact_fp32_ms_per_window": [round(t, 5) for t, _ in tb], "search_examples_ms_per_window": [round(t, 5) for t, _ in te],
            "search_examples_without_S_ms_per_window": [round(t, 5) for t, _ in tn],
            "calls_per_window": [c for _, c in tb] + [c for _, c in te] + [c for _, c in tn],
            "exact_fp32_median_ms": mb, "search_examples_median_ms": me, "search_examples_without_S_median_ms": mn,
            "ratio": me / mb, "ratio_without_S": mn / mb,
            "baseline_spread": (max(t for t, _ in tb) - min(t for t, _ in tb)) / mb,
            "examples_spread": (max(t for t, _ in te) - min(t for t, _ in te)) / me,
            "exact_fp32_GBps_whole_call": n * d * 4 / mb / 1e6, "search_examples_GBps_whole_call": n * d * 4 / me / 1e6,
        }
    ix.close()
    print(json.dumps(out))
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

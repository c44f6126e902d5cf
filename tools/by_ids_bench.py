#!/usr/bin/env python3
"""Time IndexFlat.search_by_ids against what a caller had to do without it, in ONE process and run.

    python tools/by_ids_bench.py --out profiles/search_by_ids_10M.json

1000 anchors against 10 M x 768 device-generated unit rows, k = 10: `search_by_ids(anchors, 10)` next to
`search(rows, 11)` of the same 1000 rows exported beforehand (the export itself is timed once and reported apart; the
search call includes the upload of the rows, which is part of that way).  `search` is untouched by this feature, so its
time here is the parent commit's.  3 warm-ups of each, then 20 timed calls of each, interleaved, median.  Both calls
wait for the device before they return, so the host clock around the call is the call time.  The two results are
compared after the anchor is dropped from the second.  Needs a GPU; there is no fallback."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from claude_semantic_search_amd.flat_index import IndexFlatIP, drop_self  # noqa: E402


def timed(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--anchors", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, d, k = a.rows, 768, a.k
    ix = IndexFlatIP(d)
    ix.reserve(n)
    ix.add_synthetic(n, seed=1, first_row=0, normalize=True)
    anchors = np.random.default_rng(7).choice(n, size=a.anchors, replace=False).astype(np.int64)
    export_ms, rows = timed(lambda: np.stack([ix.reconstruct(int(i)) for i in anchors]))
    for _ in range(3):
        got = ix.search_by_ids(anchors, k)
        ref = ix.search(rows, k + 1)
    ta, tb = [], []
    for _ in range(20):
        ta.append(timed(lambda: ix.search_by_ids(anchors, k))[0])
        tb.append(timed(lambda: ix.search(rows, k + 1))[0])
    Dr, Ir = drop_self(ref[0], ref[1], anchors)
    out = {"rows": n, "dim": d, "anchors": a.anchors, "k": k,
           "search_by_ids_median_ms": statistics.median(ta), "search_by_ids_min_ms": min(ta),
           "search_exported_rows_k_plus_1_median_ms": statistics.median(tb), "search_exported_rows_k_plus_1_min_ms": min(tb),
           "ratio": statistics.median(ta) / statistics.median(tb), "export_of_the_rows_ms": export_ms,
           "ids_equal": bool(np.array_equal(got[1], Ir)), "max_score_diff": float(np.abs(got[0] - Dr).max())}
    ix.close()
    print(json.dumps(out))
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time IndexFlat.range_search against its sibling, the exact fp32 top-10 search, in ONE process and run.

    python tools/range_bench.py --out profiles/range_search_10M.json

One query against 10 M x 768 device-generated unit rows, inner-product radius 0.14 (a few hundred hits): 3 warm-ups of
each, then 20 timed calls of each, interleaved, median.  Both calls wait for the device before they return, so the host
clock around the call is the call time.  Also recorded: a 16- and a 1000-query batch on the same index (one sweep per
16 queries: 63 sweeps), the default-path top-10 search of that batch for scale, and the everything-hits / nothing-hits
case of the test suite (50 k rows, 4 queries; the first call includes the growth of the hit pool and its second sweep).
Needs a GPU; there is no fallback."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from claude_semantic_search_amd.flat_index import IndexFlatIP  # noqa: E402
from oracle import knn_oracle as ko  # noqa: E402


def timed(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--radius", type=float, default=0.14)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out, d = {"rows": a.rows, "dim": 768}, 768

    x = ko.normalize_rows(ko.synth_rows(50000, d, 3))
    q4 = ko.normalize_rows(ko.synth_rows(4, d, 31))
    ix = IndexFlatIP(d)
    ix.add(x)
    first_ms, r = timed(lambda: ix.range_search(q4, -2.0))
    ts = [timed(lambda: ix.range_search(q4, -2.0))[0] for _ in range(10)]
    out["all_hits_50k_nq4"] = {"first_call_ms": first_ms, "median_ms": statistics.median(ts), "hits": int(r[0][-1])}
    ts = [timed(lambda: ix.range_search(q4, 2.0))[0] for _ in range(10)]
    out["no_hits_50k_nq4_median_ms"] = statistics.median(ts)
    ix.close()

    n = a.rows
    ix = IndexFlatIP(d)
    ix.reserve(n)
    ix.add_synthetic(n, seed=1, first_row=0, normalize=True)
    q = ko.normalize_rows(ko.synth_rows(1000, d, 2))
    ix.set_search_mode("exact_fp32")
    for _ in range(3):
        ix.search(q[:1], 10)
        res = ix.range_search(q[:1], a.radius)
    ta, tb = [], []
    for _ in range(20):
        ta.append(timed(lambda: ix.search(q[:1], 10))[0])
        tb.append(timed(lambda: ix.range_search(q[:1], a.radius))[0])
    ma, mb = statistics.median(ta), statistics.median(tb)
    out["one_query"] = {"radius": a.radius, "hits": int(res[0][-1]), "exact_fp32_top10_median_ms": ma,
                        "range_search_median_ms": mb, "ratio": mb / ma, "exact_min_ms": min(ta), "range_min_ms": min(tb),
                        "bytes_read": n * d * 4, "range_GBps": n * d * 4 / mb / 1e6}
    for nq in (16, 1000):
        ix.range_search(q[:nq], a.radius)
        t, r = timed(lambda: ix.range_search(q[:nq], a.radius))
        out[f"batch_{nq}"] = {"ms": t, "hits": int(r[0][-1]), "sweeps": (nq + 15) // 16}
    ix.set_search_mode("auto")
    ix.search(q, 10)
    out["auto_top10_1000q_ms"] = timed(lambda: ix.search(q, 10))[0]
    ix.close()
    print(json.dumps(out))
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

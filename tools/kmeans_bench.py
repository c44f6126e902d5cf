#!/usr/bin/env python3
"""Time one Lloyd step (IndexFlat.kmeans_step: assignment, member lists, fixed-point sums, results back) against what
a user of the library could do without it: the centroids in an IndexFlatL2 under set_search_mode("exact_fp32"), searched
with the same rows as queries, k = 1, through search_dev from a device tensor (no upload is timed).  That yardstick
forms the same fp32 matrix-core products, keeps per-query lists, and does NO centroid update.  ONE process and run.

    python tools/kmeans_bench.py --out profiles/kmeans_1M.json

1 M x 768 unit rows generated on the device, nc = 256 and 1024 centroids (rows of the index).  Both are warmed up; then
windows of at least --window seconds of back-to-back calls alternate: yardstick, step, yardstick, ...  Times are
WHOLE-CALL times on the host clock (the step waits for the device itself; the yardstick is followed by a stream
synchronisation).  Reported per nc: the mean call time of every window, the medians, their ratio, the spread of the
yardstick windows among themselves (what a difference has to exceed); and from a separate pass under the library's
kernel timing: the time of k_kmeans_assign with its achieved fp32 TFLOP/s (2 n nc d flop; the fp32-input matrix core
peaks at 157 TFLOP/s), of the list build and of k_kmeans_sum, and their share of the three.
Needs a GPU; there is no fallback."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from claude_semantic_search_amd import _native as nat  # noqa: E402
from claude_semantic_search_amd.flat_index import IndexFlatIP, IndexFlatL2  # noqa: E402


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
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d, n = 768, a.rows
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32)
    x = torch.nn.functional.normalize(x, dim=1).contiguous()
    st = torch.cuda.current_stream().cuda_stream
    ix = IndexFlatIP(d)
    ix.reserve(n)
    ix.add_dev(x.data_ptr(), n, stream=st)
    torch.cuda.synchronize()
    Dy = torch.empty((n, 1), dtype=torch.float32, device="cuda")
    Iy = torch.empty((n, 1), dtype=torch.int64, device="cuda")
    out = {"rows": n, "dim": d, "window_s": a.window}
    for nc in (256, 1024):
        c = ix.reconstruct_batch(np.random.default_rng(nc).choice(n, nc, replace=False))
        yard = IndexFlatL2(d)
        yard.set_search_mode("exact_fp32")
        yard.add(c)

        def base():
            yard.search_dev(x.data_ptr(), n, 1, Dy.data_ptr(), Iy.data_ptr(), st)
            torch.cuda.synchronize()

        step = lambda: ix.kmeans_step(c)                                                      # noqa: E731
        for _ in range(3):
            base()
            step()
        got = ix.kmeans_step(c, want_assign=True)
        agree = float((torch.from_numpy(got.assign.astype(np.int64)).cuda() == Iy[:, 0]).float().mean())
        tb, ts = [], []
        for _ in range(a.repeats):
            tb.append(window(base, a.window))
            ts.append(window(step, a.window))
        mb, ms = (statistics.median(t for t, _ in tt) for tt in (tb, ts))
        nat.prof_enable(True)
        nat.prof_reset()
        for _ in range(5):
            step()
        kern = {k: nat.prof_read(k) for k in ("kmeans_assign", "kmeans_lists", "kmeans_sum")}
        nat.prof_reset()
        for _ in range(5):
            base()
        yk = {k: nat.prof_read(k) for k in ("knn_scan_mfma", "knn_merge")}
        nat.prof_enable(False)
        per = {k: v[0] / max(v[1], 1) for k, v in kern.items()}
        total = sum(per.values())
        out[f"nc{nc}"] = {
            "yardstick_ms_per_window": [round(t, 4) for t, _ in tb], "kmeans_step_ms_per_window": [round(t, 4) for t, _ in ts],
            "calls_per_window": [c_ for _, c_ in tb] + [c_ for _, c_ in ts],
            "yardstick_median_ms": mb, "kmeans_step_median_ms": ms, "ratio": ms / mb,
            "yardstick_spread": (max(t for t, _ in tb) - min(t for t, _ in tb)) / mb,
            "step_spread": (max(t for t, _ in ts) - min(t for t, _ in ts)) / ms,
            "assignments_equal_to_the_yardstick": agree,
            "k_kmeans_assign_ms": per["kmeans_assign"], "lists_ms": per["kmeans_lists"], "k_kmeans_sum_ms": per["kmeans_sum"],
            "k_kmeans_assign_fp32_tflops": 2.0 * n * nc * d / (per["kmeans_assign"] * 1e-3) / 1e12,
            "share_lists_and_sum": (per["kmeans_lists"] + per["kmeans_sum"]) / total,
            "yardstick_k_scan_mfma_ms": yk["knn_scan_mfma"][0] / max(yk["knn_scan_mfma"][1], 1),
            "yardstick_k_merge_ms": yk["knn_merge"][0] / max(yk["knn_merge"][1], 1),
        }
        yard.close()
    ix.close()
    print(json.dumps(out))
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

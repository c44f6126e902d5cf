#!/usr/bin/env python3
"""Time IndexFlat.gram (the fixed-point Gram matrix and column sums on the fp64 matrix core, results back) and
IndexFlat.transform (m = 2 and m = 64 over all rows) against what a user of the library could do without them:
reconstruct_n of the same rows to the host, and X.astype(float64).T @ X in numpy on the CPUs of the run.  ONE process.

    python tools/pca_bench.py --out profiles/pca_1M.json

1 M x 768 unit rows generated on the device.  Everything is warmed up; then windows of at least --window seconds of
back-to-back calls alternate: yardstick, gram, reconstruct_n, transform(2), transform(64), yardstick, ...  Times are
WHOLE-CALL times on the host clock (every call waits for the device itself).  Reported: the mean call time of every
window, the medians, the ratios gram / yardstick and transform(2) / reconstruct_n, the spread of the windows; and from a
separate pass under the library's kernel timing the time of k_gram_fx with its achieved fp64 rate, counted as
2 n dpad^2 flop -- the FULL square, although only the upper tile triangle (21 of 36 tiles at 768) is computed -- and
the rate of the work actually done, and k_transform_rows.
Between windows: every window starts after one small untimed call (transform of 128 rows), whose times are reported
as settle_ms.  In one run without it the first transform(2) behind each reconstruct_n window took 1.7-1.9 s (a 2 ms
call everywhere else) on a host whose pageable copies also ran four times slower than in the next run; the cause was
not found, and the small call keeps whatever it was out of the windows and on the record.
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
from claude_semantic_search_amd.flat_index import IndexFlatIP  # noqa: E402


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
    ix = IndexFlatIP(d)
    ix.reserve(n)
    ix.add_dev(x.data_ptr(), n, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del x
    rng = np.random.default_rng(2)
    A2, A64 = (rng.standard_normal((m, d)).astype(np.float32) for m in (2, 64))

    def yard():
        X = ix.reconstruct_n(0, n).astype(np.float64)
        return X.T @ X, X.sum(axis=0)

    calls = {"yardstick": yard, "gram": ix.gram, "reconstruct_n": lambda: ix.reconstruct_n(0, n),
             "transform_m2": lambda: ix.transform(A2), "transform_m64": lambda: ix.transform(A64)}
    for f in calls.values():                                     # warm-up: allocations, code objects, page faults
        f()
        f()
    # the integers are those of the yardstick's float64 moments, to the quantisation step
    got = ix.gram()
    G, s = yard()
    scale = 2.0 ** (-2 * got.shift)
    gram_err = float(np.abs(got.gram.astype(np.float64) * scale - G).max())
    times = {k: [] for k in calls}
    settle_ms = []
    for _ in range(a.repeats):
        for k, f in calls.items():
            t0 = time.perf_counter()
            ix.transform(A2, None, 0, 128)                       # untimed: "Between windows" above
            settle_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
            times[k].append(window(f, a.window))
    med = {k: statistics.median(t for t, _ in v) for k, v in times.items()}
    nat.prof_enable(True)
    nat.prof_reset()
    for _ in range(5):
        ix.gram()
        ix.transform(A2)
    kern = {k: nat.prof_read(k) for k in ("gram_fx", "transform_rows")}
    nat.prof_enable(False)
    per = {k: v[0] / max(v[1], 1) for k, v in kern.items()}
    dpad = (d + 63) // 64 * 64
    T = (dpad + 127) // 128
    out = {"rows": n, "dim": d, "window_s": a.window, "fx_shift": got.shift, "count": got.count,
           "max_abs_gram_minus_float64": gram_err, "settle_ms": settle_ms}
    for k, v in times.items():
        out[k] = {"ms_per_window": [round(t, 4) for t, _ in v], "calls_per_window": [c for _, c in v], "median_ms": med[k],
                  "spread": (max(t for t, _ in v) - min(t for t, _ in v)) / med[k]}
    out["ratio_gram_to_yardstick"] = med["gram"] / med["yardstick"]
    out["ratio_transform_m2_to_reconstruct_n"] = med["transform_m2"] / med["reconstruct_n"]
    out["k_gram_fx_ms"] = per["gram_fx"]
    out["k_gram_fx_fp64_tflops_full_square"] = 2.0 * n * dpad * dpad / (per["gram_fx"] * 1e-3) / 1e12
    out["k_gram_fx_fp64_tflops_computed_tiles"] = out["k_gram_fx_fp64_tflops_full_square"] * (T * (T + 1) / 2) / (T * T)
    out["k_transform_rows_m2_ms"] = per["transform_rows"]
    ix.close()
    print(json.dumps(out))
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

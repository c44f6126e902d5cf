#!/usr/bin/env python3
"""Time IndexFlat.remove_ids (in-place compaction on the device) against the rebuild into a second index that
HybridStorage used before (reconstruct_n + add, 65 536 ids per block), in one process, on device-generated rows.

    python tools/remove_bench.py --rows 10000000 --dim 768 --fractions 0.1,0.5 --out profiles/remove_ids_10M.json

remove_ids waits for the device before it returns, so the host clock around the call (after a device synchronise)
is the call time.  Each repetition refills the index (reset + add_synthetic); the first repetition is the warm-up and
is not reported.  Bytes: "algorithmic" is the copy formulation (every per-row array of a moved survivor read and
written once, plus the fp32 read of the unmoved prefix for the maxima); "scheme" is what the kernels here touch (the
fp32 row read, every array written: the bf16 / int8 rows are re-derived in registers, never read; bounced rows cross
the scratch once more).  Needs a GPU; there is no fallback."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from claude_semantic_search_amd import _native as nat  # noqa: E402
from claude_semantic_search_amd.flat_index import IndexFlatIP  # noqa: E402

SPEC_BPS, COPY_BPS = 8.0e12, 6.29e12   # HBM3E spec; measured device copy rate of the MI355X


def free_hbm():
    return nat.device_info(0)["hbm_free_bytes"]


def plan_windows(keep, dpad):
    """Mirror of the window planning in css_index_remove_rows (compact_rows): (rows, survivors, bounced) per window."""
    n = keep.shape[0]
    first = int(np.argmin(keep))
    cum = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
    s0, dnext = first & ~31, first
    W = min(1 << 24, max(32, (64 << 20) // (dpad * 4) // 32 * 32), (n - s0 + 31) // 32 * 32)
    out = []
    while s0 < n:
        src0 = max(s0, first)
        gap = src0 - dnext
        L = min(min(gap // 32 * 32, 1 << 24) if gap >= W else W, n - s0)
        surv = int(cum[s0 + L] - cum[src0])
        if surv:
            out.append((L, surv, dnext + surv > src0))
        dnext += surv
        s0 += L
    return first, out


def sync():
    import torch

    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--fractions", default="0.1,0.5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, d = a.rows, a.dim
    dpad = (d + 63) // 64 * 64
    assert nat.device_count() > 0, "remove_bench needs a HIP device"
    free0 = free_hbm()
    ix = IndexFlatIP(d)
    ix.reserve(n)
    res = {"rows": n, "dim": d, "device": nat.device_info(0)["name"], "cases": []}
    for frac in [float(f) for f in a.fractions.split(",")]:
        keep = np.random.default_rng(int(frac * 1000)).random(n) >= frac
        m = int(keep.sum())
        first, wins = plan_windows(keep, dpad)
        moved = m - first
        per_row = dpad * 4 + dpad * 2 + dpad + 8
        times = []
        for rep in range(a.reps + 1):
            ix.reset()
            ix.add_synthetic(n, seed=7, first_row=0, normalize=True)
            sync()
            shadows = ix.shadow_info()
            t0 = time.perf_counter()
            removed = ix.remove_ids(~keep)
            t1 = time.perf_counter()
            assert removed == n - m and ix.ntotal == m
            if rep:
                times.append(t1 - t0)
        in_place_used = free0 - free_hbm()
        # remove_ids includes the host side: keep mask -> bitmap (numpy) and the popcount pass over it
        t = float(np.median(times))
        bounced = [w for w in wins if w[2]]
        alg = moved * per_row * 2 + first * dpad * 4
        scheme = moved * (dpad * 4 + per_row) + sum(w[1] for w in bounced) * dpad * 8 + first * dpad * 4
        case = {
            "removed_fraction": frac, "removed": n - m, "first_removed_row": first, "moved_rows": moved, "shadows": shadows,
            "remove_ids_s": times, "remove_ids_median_s": t,
            "algorithmic_bytes": alg, "algorithmic_bytes_per_s": alg / t,
            "fraction_of_8TBps_spec": alg / t / SPEC_BPS, "fraction_of_6p29TBps_copy": alg / t / COPY_BPS,
            "scheme_bytes": scheme, "scheme_bytes_per_s": scheme / t,
            "windows": len(wins), "bounced_windows": len(bounced), "bounced_rows": sum(w[1] for w in bounced),
            "window_rows_first_last": [wins[0][0], wins[-1][0]] if wins else [],
            "hbm_in_use_after_in_place_bytes": in_place_used,
        }
        if not a.no_baseline:
            ix.reset()
            ix.add_synthetic(n, seed=7, first_row=0, normalize=True)
            sync()
            ids = np.flatnonzero(keep)
            t0 = time.perf_counter()
            fresh = IndexFlatIP(d)
            fresh.reserve(m)
            peak = 0
            for s in range(0, m, 1 << 16):
                part = ids[s:s + (1 << 16)]
                lo, hi = int(part[0]), int(part[-1]) + 1
                fresh.add(ix.reconstruct_n(lo, hi - lo)[part - lo])
                if s == 0:
                    peak = free0 - free_hbm()
            t1 = time.perf_counter()
            q = np.zeros((1, d), np.float32)
            q[0, 0] = 1.0
            ix.remove_ids(~keep)
            same = all(np.array_equal(x, y) for x, y in zip(ix.search(q, 10), fresh.search(q, 10)))
            fresh.close()
            case.update({"rebuild_s": t1 - t0, "rebuild_over_remove_ids": (t1 - t0) / t, "hbm_in_use_during_rebuild_bytes": peak,
                         "same_top10_as_rebuild": bool(same)})
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    ix.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time IndexFlat.search_grouped against its sibling, the plain search for the same over-fetch, in ONE process and run.

    python tools/grouped_bench.py --out profiles/search_grouped_10M.json

10 M x 768 unit rows, inner product, k = 10, labels of about 200 rows per group at random, once per kind of row copy
the index can hold (fp32 rows only, + bf16 rows, int8 rows only).  Every call waits for the device before it returns,
so the host clock around the call is the call time.

 (a) a grouped search that finishes in one pass against ``search(q, kk)`` of the same queries at the same kk = 32: one
     query and 1000 queries, 3 warm-ups of each, then 20 timed calls of each, interleaved, median, and the ratio;
 (b) one query that needs 2 passes (300 near-copies of the query in one group in front of the rows) and 6 (a staircase
     of 5 groups of 200 near-copies): call time, time per extra pass, and the time of k_mask_drop_groups alone from
     the in-library kernel timing against its 4 B + 1/8 B per row;
 (c) ``set_groups`` of all labels.

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
from oracle import knn_oracle as ko  # noqa: E402


def timed(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


def near_copies(qhat, cos, seed):
    u = np.random.default_rng(seed).standard_normal((cos.shape[0], qhat.shape[0]))
    u -= (u @ qhat)[:, None] * qhat[None, :]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    c = cos[:, None]
    return (c * qhat[None, :] + np.sqrt(1.0 - c * c) * u).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--group-rows", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shadows", default="fp32,bf16,int8")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d, k, n = 768, 10, a.rows
    out = {"rows": n, "dim": d, "k": k, "rows_per_group": a.group_rows, "reps": a.reps, "date": time.strftime("%Y-%m-%d")}
    q = ko.normalize_rows(ko.synth_rows(1000, d, 2))
    qhat = q[0].astype(np.float64)
    head = np.concatenate([near_copies(qhat, (0.99 - 0.04 * g) - 1e-4 * np.arange(200), 10 + g) for g in range(5)])
    labels = np.random.default_rng(5).integers(0, max(1, n // a.group_rows), size=n).astype(np.int32)
    policies = {"fp32": False, "bf16": True, "int8": "int8"}
    for name in a.shadows.split(","):
        ix = IndexFlatIP(d)
        ix.set_shadow(policies[name])
        ix.reserve(n)
        ix.add(head)                                             # rows 0..999: the staircase (masked out where not wanted)
        ix.add_synthetic(n - head.shape[0], seed=1, first_row=0, normalize=True)
        rec = {"shadow_info": ix.shadow_info()}
        rec["set_groups_ms"] = timed(lambda: ix.set_groups(labels))[0]                      # (c), first call allocates
        rec["set_groups_again_ms"] = timed(lambda: ix.set_groups(labels))[0]
        no_head = np.ones(n, bool)
        no_head[:head.shape[0]] = False
        for nq in (1, 1000):                                                                # (a)
            for _ in range(3):
                ix.search(q[:nq], 32, allow=no_head)
                ix.search_grouped(q[:nq], k, allow=no_head)
            assert ix.last_group_passes() == 1
            ta, tb = [], []
            for _ in range(a.reps):
                ta.append(timed(lambda: ix.search(q[:nq], 32, allow=no_head))[0])
                tb.append(timed(lambda: ix.search_grouped(q[:nq], k, allow=no_head))[0])
            ma, mb = statistics.median(ta), statistics.median(tb)
            rec[f"one_pass_nq{nq}"] = {"search_kk32_median_ms": ma, "grouped_median_ms": mb, "ratio": mb / ma,
                                       "search_min_ms": min(ta), "grouped_min_ms": min(tb)}
        # (b) the dominating group: the first 300 head rows in ONE group; the staircase: 5 groups of 200
        lay = {}
        for what, head_labels, allow in (("dominating", np.full(300, 2_000_000_000, np.int32), None),
                                         ("staircase", (2_000_000_000 + np.arange(1000) // 200).astype(np.int32), None)):
            ix.set_groups(labels[:1000])
            ix.set_groups(head_labels)
            if what == "dominating":
                allow = np.ones(n, bool)
                allow[300:1000] = False
            for _ in range(3):
                ix.search_grouped(q[:1], k, allow=allow)
            passes = ix.last_group_passes()
            nat.prof_reset()
            nat.prof_enable(True)
            ix.search_grouped(q[:1], k, allow=allow)
            nat.prof_enable(False)
            drop_ms, drop_n = nat.prof_read("knn_mask_drop_groups")
            ts = [timed(lambda: ix.search_grouped(q[:1], k, allow=allow))[0] for _ in range(a.reps)]
            t1 = [timed(lambda: ix.search(q[:1], 128, allow=allow))[0] for _ in range(a.reps)]
            m = statistics.median(ts)
            lay[what] = {"passes": passes, "grouped_median_ms": m, "search_k128_median_ms": statistics.median(t1),
                         "ms_per_extra_pass": (m - rec["one_pass_nq1"]["grouped_median_ms"]) / max(1, passes - 1),
                         "mask_drop_groups_ms_each": drop_ms / max(1, drop_n), "mask_drop_groups_launches": drop_n,
                         "mask_drop_groups_bytes": n * 4 + n // 8,
                         "mask_drop_groups_GBps": (n * 4 + n // 8) / max(drop_ms / max(1, drop_n), 1e-9) / 1e6}
        rec["extra_passes"] = lay
        out[name] = rec
        ix.close()
        print(json.dumps({name: rec}), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

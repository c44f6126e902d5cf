#!/usr/bin/env python3
"""Time IndexFlat.facets against its sibling -- range_search + bincount + per-bucket best on the host, the only way to
the same answer before this call existed -- in ONE process and run.

    python tools/facets_bench.py --out profiles/facets_10M.json

10 M x 768 device-generated unit rows, inner product.  Host clock around the synchronous calls; 3 warm-ups of each, then
20 timed calls of each, interleaved, median (a sibling call that takes longer than --slow-ms gets 1 warm-up and 5 timed
calls, recorded as `reps`).  Before a leg is timed its two answers are checked for equality.  Every facets leg runs
three times in the interleaving: under the library's rule for the table placement, with the table forced to global
memory, and with it forced into LDS (where 160 KB hold it); `placement` says what the rule chose.

  (a) 1 query, radius 0.14, 64 buckets; also range_search alone (it reads the same bytes)
  (b) 1 query, radius 0.0 (about half the rows hit), 8 / 4096 / 2^20 buckets
  (c) 16 queries, radius 0.0, 64 buckets
  (d) leg (a) with the column uploaded per call against the stored labels (set_groups): the difference is the upload

Then the placement sweep behind the library's LDS limit (skipped with --no-placement): stored labels, 1 / 2 / 8 / 16
queries, table sizes that leave many, 3, 2 and 1 blocks per CU, at three hit rates (radius 0.14, 0.05, 0.0), LDS table
against global table, interleaved, median of 7 after 2 warm-ups.

Needs a GPU; there is no fallback."""
import argparse
import datetime
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from claude_semantic_search_amd.flat_index import IndexFlatIP  # noqa: E402
from oracle import knn_oracle as ko  # noqa: E402


def timed(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


def labels(n, nb, seed):
    """Skewed buckets (cubed uniform), 3 % negative, 2 % beyond nb."""
    rng = np.random.default_rng(seed)
    lab = np.minimum((nb * rng.random(n) ** 3).astype(np.int64), nb - 1)
    kind = rng.random(n)
    lab = np.where(kind < 0.03, -1, lab)
    return np.where(kind > 0.98, nb, lab).astype(np.int32)


def sibling(ix, q, radius, lab, nb):
    """The parent commit's way: every hit to the host, sorted, then counted.  The list of a query is best first with
    equal scores by ascending id, so the first entry of a bucket is its best."""
    lims, D, I = ix.range_search(q, radius)
    nq = q.shape[0]
    counts = np.zeros((nq, nb), np.int64)
    best_s = np.full((nq, nb), -np.finfo(np.float32).max, np.float32)
    best_i = np.full((nq, nb), -1, np.int64)
    total, unb = np.diff(lims), np.zeros(nq, np.int64)
    for j in range(nq):
        d, i = D[lims[j]:lims[j + 1]], I[lims[j]:lims[j + 1]]
        lj = lab[i]
        inb = (lj >= 0) & (lj < nb)
        unb[j] = int((~inb).sum())
        lj, d, i = lj[inb], d[inb], i[inb]
        counts[j] = np.bincount(lj, minlength=nb)
        first = np.full(nb, -1, np.int64)
        first[lj[::-1]] = np.arange(lj.shape[0] - 1, -1, -1)          # the last write wins: the first occurrence
        has = first >= 0
        best_s[j, has], best_i[j, has] = d[first[has]], i[first[has]]
    return counts, best_s, best_i, total, unb


def same(res, sib):
    return all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)) for a, b in zip(res, sib))


def race(variants, slow_ms):
    """variants: name -> callable.  Interleaved medians; a variant slower than slow_ms runs 1 + 5 times."""
    first = {k: timed(f)[0] for k, f in variants.items()}
    reps = {k: (5 if first[k] > slow_ms else 20) for k in variants}
    for k, f in variants.items():
        for _ in range(0 if first[k] > slow_ms else 2):
            f()
    ts = {k: [] for k in variants}
    for r in range(20):
        for k, f in variants.items():
            if r < reps[k]:
                ts[k].append(timed(f)[0])
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "reps": reps[k]} for k, v in ts.items()}


def facet_leg(ix, q, radius, lab, nb, slow_ms, stored=False, extra=None):
    kw = dict(nbuckets=nb) if stored else dict(buckets=lab, nbuckets=nb)
    ix.set_facet_lds_entries(-1)
    res = ix.facets(q, radius, **kw)
    sweeps, lds = ix.last_facet_sweeps()
    sib = sibling(ix, q, radius, lab, nb)
    if not same(res, sib):
        raise SystemExit(f"facets and its sibling disagree: nq={q.shape[0]} radius={radius} nb={nb}")

    def run(entries):
        def f():
            ix.set_facet_lds_entries(entries)
            return ix.facets(q, radius, **kw)
        return f

    ix.set_facet_lds_entries(1 << 20)
    forced = ix.facets(q, radius, **kw)
    lds_possible = ix.last_facet_sweeps()[1] > 0
    if not same(forced, sib):
        raise SystemExit("the forced placement disagrees with the sibling")
    variants = {"facets": run(-1), "facets_global": run(0), "sibling": lambda: sibling(ix, q, radius, lab, nb)}
    if lds_possible:
        variants["facets_lds"] = run(1 << 20)
    variants.update(extra or {})
    out = race(variants, slow_ms)
    ix.set_facet_lds_entries(-1)
    out.update({"nq": int(q.shape[0]), "radius": radius, "nbuckets": nb, "hits": [int(t) for t in res.total],
                "sweeps": sweeps, "placement": "lds" if lds == sweeps else "global" if lds == 0 else "mixed",
                "ratio_to_sibling": out["facets"]["median_ms"] / out["sibling"]["median_ms"]})
    return out


PLACEMENT_SHAPES = ((1, (64, 1024, 3157, 4096, 6000, 9000, 13000)), (2, (64, 1024, 3000, 6000)),
                    (8, (16, 170, 400, 1000)), (16, (8, 28, 64, 170, 400, 590)))


def placement_sweep(ix, q, n, d):
    rows = []
    for nq, nbs in PLACEMENT_SHAPES:
        for nb in nbs:
            ix.set_groups(labels(n, nb, nb))
            lds_bytes = nq * d * 4 + nq * nb * 12
            for radius in (0.14, 0.05, 0.0):
                ts, ref = {"lds": [], "global": []}, None
                for r in range(9):
                    for name, entries in (("lds", 1 << 20), ("global", 0)):
                        ix.set_facet_lds_entries(entries)
                        t, res = timed(lambda: ix.facets(q[:nq], radius, nbuckets=nb))
                        if r == 0:
                            if ix.last_facet_sweeps() != (1, 1 if name == "lds" else 0):
                                raise SystemExit(f"placement {name} did not run: nq={nq} nb={nb}")
                            ref = ref or res
                            if not same(res, ref):
                                raise SystemExit(f"the two placements disagree: nq={nq} nb={nb} radius={radius}")
                        if r >= 2:
                            ts[name].append(t)
                ix.set_facet_lds_entries(-1)
                ix.facets(q[:nq], radius, nbuckets=nb)
                rows.append({"nq": nq, "nbuckets": nb, "lds_bytes": lds_bytes, "blocks_per_cu": 160 * 1024 // lds_bytes,
                             "radius": radius, "hits_query0": int(ref.total[0]),
                             "lds_median_ms": statistics.median(ts["lds"]), "global_median_ms": statistics.median(ts["global"]),
                             "rule": "lds" if ix.last_facet_sweeps()[1] else "global"})
                print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--slow-ms", type=float, default=500.0)
    ap.add_argument("--commit", default="", help="the parent commit, where the tree is not a git checkout")
    ap.add_argument("--no-placement", action="store_true", help="skip the placement sweep")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d, n = 768, a.rows
    commit = a.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=str(ROOT), capture_output=True,
                                        text=True).stdout.strip()
    out = {"rows": n, "dim": d, "date": datetime.date.today().isoformat(), "parent_commit": commit or None,
           "tool": "tools/facets_bench.py"}
    ix = IndexFlatIP(d)
    ix.reserve(n)
    ix.add_synthetic(n, seed=1, first_row=0, normalize=True)
    q = ko.normalize_rows(ko.synth_rows(16, d, 2))
    lab64 = labels(n, 64, 64)

    leg = facet_leg(ix, q[:1], 0.14, lab64, 64, a.slow_ms, extra={"range_search": lambda: ix.range_search(q[:1], 0.14)})
    leg["ratio_to_range_search"] = leg["facets"]["median_ms"] / leg["range_search"]["median_ms"]
    leg["GBps"] = n * d * 4 / leg["facets"]["median_ms"] / 1e6
    out["a_1q_r0.14_64b"] = leg
    print(json.dumps({"a": leg}), flush=True)
    for nb in (8, 4096, 1 << 20):
        out[f"b_1q_r0.0_{nb}b"] = leg = facet_leg(ix, q[:1], 0.0, labels(n, nb, nb), nb, a.slow_ms)
        print(json.dumps({f"b{nb}": leg}), flush=True)
    out["c_16q_r0.0_64b"] = leg = facet_leg(ix, q, 0.0, lab64, 64, a.slow_ms)
    print(json.dumps({"c": leg}), flush=True)
    ix.set_groups(lab64)

    def per_call():
        ix.set_facet_lds_entries(-1)
        return ix.facets(q[:1], 0.14, buckets=lab64, nbuckets=64)

    stored = facet_leg(ix, q[:1], 0.14, lab64, 64, a.slow_ms, stored=True, extra={"per_call_column": per_call})
    out["d_1q_r0.14_64b_stored_labels"] = stored
    stored["upload_ms"] = stored["per_call_column"]["median_ms"] - stored["facets"]["median_ms"]
    stored["column_bytes"] = 4 * n
    if not a.no_placement:
        out["placement_sweep"] = placement_sweep(ix, q, n, d)
    ix.close()
    print(json.dumps(out))
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

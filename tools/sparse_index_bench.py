#!/usr/bin/env python3
"""Time the sparse side of the flat index: k_sparse_scores, the column top-k, and k_lex_scores as the yardstick.

    python tools/sparse_index_bench.py --out profiles/sparse_index.json

1 M rows (768 device-generated unit floats each, so that the fp32 sweep of the same process gives an HBM rate to compare
with) carrying the sparse vectors of synth.sparse_vectors (about 118 entries per row) AND term lists made of the very
same terms, so that both column kernels stream the same number of entries E.  Kernel times come from the library's own
event timing (css_prof_*), per launch over --reps calls:

  k_sparse_scores   at m = 8, 32 (64 rows per wave), 33 and 64 (32 rows per wave): ms, the algorithmic bytes
                    (8 E + 8 N read, 4 N written), GB/s, its share of bench.py's HBM_PEAK_GBS (what the roofline leg of
                    ``bench.py --full`` divides by) and of the rate the fp32 sweep k_scan_prior reaches in this process
                    (--hbm-gbps replaces the latter by a figure taken from a bench.py --full line of the same machine)
  k_sparse_topk     alone, and the part merge behind it, at k = 10 and 128
  k_lex_scores      at m = 8 and 32 over the same E (4 E + 12 N read, 4 N written), and the ratio of the times per entry:
                    about 2 if both are HBM bound, because an entry is 8 bytes against 4
  search_sparse     the whole call on the host clock (upload, three launches, one wait)

Needs a GPU; there is no fallback."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from claude_semantic_search_amd import _native as nat  # noqa: E402
from claude_semantic_search_amd import synth  # noqa: E402
from claude_semantic_search_amd.flat_index import IndexFlatIP  # noqa: E402
from oracle import knn_oracle as ko  # noqa: E402

HBM_PEAK_GBS = 8000.0   # bench.py HBM_PEAK_GBS


def query(m, seed):
    rng = np.random.default_rng(seed)
    t = np.floor(synth.TERM_VOCAB * rng.random(64 * m + 64) ** 3).astype(np.int64)
    t = t[np.sort(np.unique(t, return_index=True)[1])][:m]
    return t, (0.25 + rng.random(m)).astype(np.float32)


def timed(names, f, reps):
    """ms per launch of the named profile scopes over `reps` calls of f, and the mean whole-call ms on the host clock."""
    for _ in range(5):
        f()
    nat.prof_reset()
    nat.prof_enable(True)
    for _ in range(reps):
        f()
    out = {}
    for name in names:
        ms, n = nat.prof_read(name)
        out[name] = ms / n if n else None
    nat.prof_enable(False)
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    out["call_ms"] = (time.perf_counter() - t0) / reps * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--hbm-gbps", type=float, default=0.0, help="the HBM rate of a bench.py --full roofline leg on this machine")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, d = a.rows, a.dim
    ix = IndexFlatIP(d)
    ix.reserve(n)
    ix.add_synthetic(n, seed=1, first_row=0, normalize=True)
    step, entries = 100_000, 0
    for r0 in range(0, n, step):                                     # (the generator draws a [rows, 255] matrix)
        off, t, w = synth.sparse_vectors(min(step, n - r0), 301 + r0 // step)
        ix.set_sparse((off, t, w))
        ix.set_terms((off, t))                                       # the same terms once each: the same E for the yardstick
        entries += int(off[-1])
    q = ko.normalize_rows(ko.synth_rows(1, d, 2))
    sparse_bytes, lex_bytes = 8 * entries + 12 * n, 4 * entries + 16 * n
    out = {"rows": n, "dim": d, "entries": entries, "entries_per_row": entries / n, "reps": a.reps,
           "sparse_scores_algorithmic_bytes": sparse_bytes, "lex_scores_algorithmic_bytes": lex_bytes, "hbm_peak_GBps": HBM_PEAK_GBS}
    # the yardsticks: the fp32 sweep of this process, and k_lex_scores over the same entries
    lex = {}
    for m in (8, 32):
        t, w = query(m, 900 + m)
        r = timed(("lex_scores", "knn_scan_prior"), lambda: ix.search_hybrid(q[0], t, w, 10, 0.5, avgdl=118.0), a.reps)
        lex[m] = r["lex_scores"]
        out[f"lex_m{m}"] = {"k_lex_scores_ms": r["lex_scores"], "GBps": lex_bytes / r["lex_scores"] / 1e6,
                            "ns_per_entry": r["lex_scores"] * 1e6 / entries, "k_scan_prior_ms": r["knn_scan_prior"]}
        sweep_gbps = n * ((d + 63) // 64 * 64) * 4 / r["knn_scan_prior"] / 1e6
    out["fp32_sweep_GBps_in_this_process"] = sweep_gbps
    rate = a.hbm_gbps or sweep_gbps
    out["hbm_rate_GBps_used_for_the_share"] = rate
    out["hbm_rate_source"] = "--hbm-gbps" if a.hbm_gbps else "k_scan_prior of this process"
    for m in (8, 32, 33, 64):
        t, w = query(m, 900 + m)
        rec = {}
        for k in (10, 128):
            r = timed(("sparse_scores", "sparse_topk", "knn_merge_parts"), lambda: ix.search_sparse(t, w, k), a.reps)
            rec[f"k{k}"] = {"k_sparse_topk_ms": r["sparse_topk"], "merge_parts_ms": r["knn_merge_parts"], "search_sparse_call_ms": r["call_ms"]}
            ms = r["sparse_scores"]
        gbps = sparse_bytes / ms / 1e6
        rec.update({"instantiation": "<32, 4, 64, 4>" if m <= 32 else "<64, 4, 32, 4>", "k_sparse_scores_ms": ms, "GBps": gbps,
                    "share_of_hbm_peak": gbps / HBM_PEAK_GBS, "share_of_hbm_rate": gbps / rate, "ns_per_entry": ms * 1e6 / entries})
        if m in lex:
            rec["time_per_entry_against_k_lex_scores"] = ms / lex[m]
        out[f"sparse_m{m}"] = rec
    ix.close()
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

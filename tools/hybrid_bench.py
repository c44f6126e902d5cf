#!/usr/bin/env python3
"""Time IndexFlat.search_hybrid against its sibling, search_prior (the same sweep with a stored column), in ONE process
and run.

    python tools/hybrid_bench.py --out profiles/search_hybrid_1M.json

1 M x 768 device-generated unit rows with term lists from synth.term_lists (about 118 distinct terms per row), k = 10,
one query of 4 terms and one of 32.  Both calls wait for the device before they return, so the host clock around a call
is the call time (WHOLE-CALL times, not kernel times).  Both are warmed up; then windows of at least --window seconds of
back-to-back calls alternate: baseline, hybrid, baseline, hybrid, ...  Reported per query: the mean call time of every
window, the medians, the spread of the baseline windows among themselves (what a difference has to exceed).  Then, with
the library's own event timing (css_prof_*), the time of k_lex_scores alone and the bytes per second its algorithmic
traffic amounts to (4 bytes per entry, 12 per row read, 4 per row written).
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
from claude_semantic_search_amd import synth  # noqa: E402
from claude_semantic_search_amd.flat_index import IndexFlatIP  # noqa: E402
from claude_semantic_search_amd.lexical import bm25_weights  # noqa: E402
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
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d, k, n = 768, 10, a.rows
    ix = IndexFlatIP(d)
    ix.reserve(n)
    ix.add_synthetic(n, seed=1, first_row=0, normalize=True)
    ix.set_priors(np.random.default_rng(3).random(n, dtype=np.float32))
    t0 = time.perf_counter()
    step = 100_000
    for r0 in range(0, n, step):                                     # (the generator draws a [rows, 255] matrix)
        ix.set_terms(synth.term_lists(min(step, n - r0), 101 + r0 // step))
    t_lists = time.perf_counter() - t0
    off = np.zeros(n + 1, dtype=np.int64)                            # (the offsets alone: no entry is copied back)
    nat.check(nat.lib().css_index_get_terms(ix._handle(), 0, n, off.ctypes.data, None, None))
    entries = int(off[-1])
    _, ndocs, total_len = ix.term_stats(())
    avgdl = total_len / ndocs
    q = ko.normalize_rows(ko.synth_rows(1, d, 2))
    long_set = np.floor(synth.TERM_VOCAB * np.random.default_rng(501).random(64) ** 3).astype(np.int64)
    long_set = long_set[np.sort(np.unique(long_set, return_index=True)[1])][:32]
    traffic = 4 * entries + 16 * n
    out = {"rows": n, "dim": d, "k": k, "alpha": a.alpha, "window_s": a.window, "entries": entries, "total_len": total_len,
           "set_terms_s_generator_included": round(t_lists, 2), "lex_scores_algorithmic_bytes": traffic}
    for name, terms in (("m4", synth.query_terms(0)), ("m32", long_set)):
        df = ix.term_stats(terms)[0]
        w = bm25_weights(df, ndocs)
        base = lambda: ix.search_prior(q, k, a.alpha)                                     # noqa: E731
        hybrid = lambda: ix.search_hybrid(q[0], terms, w, k, a.alpha, avgdl=avgdl)       # noqa: E731
        for _ in range(20):
            base()
            hybrid()
        tb, th = [], []
        for _ in range(a.repeats):
            tb.append(window(base, a.window))
            th.append(window(hybrid, a.window))
        mb, mh = statistics.median(t for t, _ in tb), statistics.median(t for t, _ in th)
        nat.prof_enable(True)
        nat.prof_reset()
        for _ in range(50):
            hybrid()
        lex_ms, launches = nat.prof_read("lex_scores")
        sweep_ms, sweeps = nat.prof_read("knn_scan_prior")
        nat.prof_enable(False)
        lex = lex_ms / max(launches, 1)
        out[name] = {
            "terms": [int(t) for t in terms], "df": [int(v) for v in df],
            "search_prior_ms_per_window": [round(t, 5) for t, _ in tb], "search_hybrid_ms_per_window": [round(t, 5) for t, _ in th],
            "calls_per_window": [c for _, c in tb] + [c for _, c in th],
            "search_prior_median_ms": mb, "search_hybrid_median_ms": mh, "difference_ms": mh - mb, "ratio": mh / mb,
            "baseline_spread": (max(t for t, _ in tb) - min(t for t, _ in tb)) / mb,
            "hybrid_spread": (max(t for t, _ in th) - min(t for t, _ in th)) / mh,
            "k_lex_scores_ms": lex, "k_lex_scores_launches": launches, "k_lex_scores_TBps": traffic / lex / 1e9 if lex else None,
            "k_scan_prior_ms_under_profiling": sweep_ms / max(sweeps, 1),
        }
    ix.close()
    print(json.dumps(out))
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

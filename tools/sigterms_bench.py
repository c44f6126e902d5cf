#!/usr/bin/env python3
"""Time IndexFlat.subset_terms / significant_terms and their passes, in ONE process and run.

    python tools/sigterms_bench.py --out profiles/significant_terms_1M.json

1 M rows of d = 16 (the rows' values play no part) with term lists from synth.term_lists: about 118 distinct terms per
row out of a vocabulary of 4096, so EVERY term is frequent -- the hardest shape for a scatter-count.  Three selections:
every row, a random 5 %, ten rows.  Per selection, with the library's own event timing (css_prof_*):
  * k_sig_count (the counting pass) with the LDS table at the library's rule and without it (set_sigterm_slots(0)),
    next to the zeroing of the 64 MB table, and the adds per second the pass amounts to;
  * k_lex_scores over THE SAME lists -- an index that holds the lists of the selected rows only -- as the read-only
    floor for the same bytes (4 per entry, 12 per row);
  * numpy's bincount of the same entries on the host, the alternative a user has today (the entries already in host
    memory; fetching them is not counted);
  * the score-and-select pass alone (k_sig_score, the radix select, the sort), for m = 20 and 256;
  * whole-call times of subset_terms and significant_terms on the host clock (both wait for the device).
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

D_ = 16


def prof(f, names, reps):
    """Mean kernel-scope milliseconds per launch of each name over `reps` calls of f."""
    nat.prof_enable(True)
    nat.prof_reset()
    for _ in range(reps):
        f()
    out = {}
    for name in names:
        ms, launches = nat.prof_read(name)
        out[name] = ms / launches if launches else None
    nat.prof_enable(False)
    return out


def wall(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def rows_of(off, ent, sel):
    """CSR (offsets, stored terms) of the selected rows."""
    rows = np.flatnonzero(sel)
    lens = (off[1:] - off[:-1])[rows]
    noff = np.zeros(rows.shape[0] + 1, np.int64)
    np.cumsum(lens, out=noff[1:])
    src = np.repeat(off[:-1][rows] - noff[:-1], lens) + np.arange(int(noff[-1]))
    return noff, ent[src]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = a.rows
    ix = IndexFlatIP(D_)
    ix.reserve(n)
    ix.add_synthetic(n, seed=1, first_row=0, normalize=True)
    step = 100_000
    for r0 in range(0, n, step):
        ix.set_terms(synth.term_lists(min(step, n - r0), 101 + r0 // step))
    off, terms, _, _ = ix.get_terms()                                  # the stored form: distinct terms per row
    entries = int(off[-1])
    rng = np.random.default_rng(7)
    sels = {"full": None, "5pct": rng.random(n) < 0.05, "10rows": np.zeros(n, bool)}
    sels["10rows"][rng.choice(n, size=10, replace=False)] = True
    out = {"rows": n, "entries": entries, "distinct_terms": int(np.unique(terms).size), "reps": a.reps}
    q = np.ones((1, D_), np.float32)
    for name, sel in sels.items():
        soff, sterms = (off, terms) if sel is None else rows_of(off, terms, sel)
        e, r = int(soff[-1]), soff.shape[0] - 1
        res = {"selected_rows": r, "selected_entries": e, "list_bytes": 4 * e + 12 * r}
        call = lambda: ix.subset_terms(sel)                             # noqa: E731
        for label, slots in (("lds_table", -1), ("global_only", 0)):
            ix.set_sigterm_slots(slots)
            call()
            p = prof(call, ("sig_count", "sig_zero"), a.reps)
            res[f"k_sig_count_ms_{label}"] = p["sig_count"]
            res[f"adds_per_s_{label}"] = e / (p["sig_count"] * 1e-3) if p["sig_count"] else None
            res["zero_table_ms"] = p["sig_zero"]
        ix.set_sigterm_slots(-1)
        t, f = call()
        # the read-only floor: k_lex_scores over an index that holds exactly these lists
        fl = ix
        if sel is not None:
            fl = IndexFlatIP(D_)
            fl.add(np.ones((r, D_), np.float32))
            fl.set_terms((soff, sterms))
        qt = t[np.argsort(-f)[:4]]                                      # four frequent terms of the selection
        w = bm25_weights(fl.term_stats(qt)[0], r)
        hyb = lambda: fl.search_hybrid(q, qt, w, 10, 0.5)               # noqa: E731
        hyb()
        res["k_lex_scores_ms_same_lists"] = prof(hyb, ("lex_scores",), a.reps)["lex_scores"]
        if fl is not ix:
            fl.close()
        # the host alternative
        t0 = time.perf_counter()
        cnt = np.bincount(sterms, minlength=1 << 24)
        nz = np.flatnonzero(cnt)
        res["numpy_bincount_ms"] = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(nz, t) and np.array_equal(cnt[nz], f)
        res["subset_terms_call_ms"] = wall(call, a.reps)
        res["terms_with_fg"] = int(t.size)
        if sel is not None:
            for m in (20, 256):
                sig = lambda: ix.significant_terms(allow=sel, m=m, min_count=2)   # noqa: E731
                sig()
                p = prof(sig, ("sig_select", "sig_count"), a.reps)
                res[f"select_ms_m{m}"] = p["sig_select"]
                res[f"significant_terms_call_ms_m{m}"] = wall(sig, a.reps)
            res["qualifying_returned_m256"] = int(ix.significant_terms(allow=sel, m=256, min_count=2).terms.size)
        out[name] = res
    ix.close()
    print(json.dumps(out))
    if a.out:
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

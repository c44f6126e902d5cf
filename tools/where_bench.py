#!/usr/bin/env python3
"""Time the filter kernel of the flat index: k_where over attribute columns, and the whole ``where`` call.

    python tools/where_bench.py --out profiles/where.json

10 M rows of dimension 1 (``where`` never reads the vectors) with eight int32 value columns and one column of
dictionary codes below 2^20.  Kernel times come from the library's own event timing (css_prof_*, scope ``where``), per
launch over --reps calls; next to each the time its algorithmic bytes -- 4 per clause and row read, 1 bit per row
written -- would take at bench.py's HBM_PEAK_GBS, which is an expectation and not a threshold, and the whole call on
the host clock (tables and clauses up, one launch, [count | bitmap] back: 1.25 MB at 10 M rows).

  int32 x 1, 4, 8   comparisons over that many columns
  in (LDS)          one ``in`` over 40 codes: a table of 2 words, staged in LDS
  in (global)       one ``in`` over 2^19 of 2^20 codes: a table of 32768 words (128 KiB) read from global memory

Needs a GPU; there is no fallback."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from claude_semantic_search_amd import _native as nat  # noqa: E402
from claude_semantic_search_amd.flat_index import IndexFlatIP  # noqa: E402

HBM_PEAK_GBS = 8000.0   # bench.py HBM_PEAK_GBS
CODE_SLOT = 8


def timed(f, reps):
    """ms per launch of k_where over `reps` calls of f, and the mean whole-call ms on the host clock."""
    for _ in range(3):
        f()
    nat.prof_reset()
    nat.prof_enable(True)
    for _ in range(reps):
        f()
    ms, n = nat.prof_read("where")
    nat.prof_enable(False)
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    return (ms / n if n else None), (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = a.rows
    ix = IndexFlatIP(1)
    ix.reserve(n)
    ix.add_synthetic(n, seed=1, first_row=0, normalize=False)
    rng = np.random.default_rng(5)
    for slot in range(8):
        ix.set_attribute(slot, rng.integers(0, 1000, n, dtype=np.int32))
    ix.set_attribute(CODE_SLOT, rng.integers(0, 1 << 20, n, dtype=np.int32))
    cases = {f"int32_x{m}": [(s, "<", 900) for s in range(m)] for m in (1, 4, 8)}
    cases["in_lds"] = [(CODE_SLOT, "in", list(range(0, 80, 2)))]
    cases["in_global"] = [(CODE_SLOT, "in", list(range(1, 1 << 20, 2)))]
    out = {"rows": n, "reps": a.reps, "hbm_peak_GBps": HBM_PEAK_GBS, "tile_rows": nat.WHERE_TILE_ROWS,
           "bitmap_bytes": (n + 31) // 32 * 4}
    for name, clauses in cases.items():
        _, count = ix.where_bits(clauses)
        ms, call_ms = timed(lambda: ix.where_bits(clauses), a.reps)
        nbytes = 4 * n * len(clauses) + n // 8
        out[name] = {"clauses": len(clauses), "rows_that_pass": count, "k_where_ms": ms, "algorithmic_bytes": nbytes,
                     "ms_at_hbm_peak": nbytes / HBM_PEAK_GBS / 1e6, "GBps": nbytes / ms / 1e6 if ms else None,
                     "where_call_ms": call_ms}
    ix.close()
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""numpy statements of the significant-terms aggregation for the tests; they live in tests/ only and the product never
falls back to them.

* ``subset_counts`` -- ``(terms ascending, fg)`` of a selection over the stored form of ``lexical_fakes.pack``: ONE
  ``bincount`` of the entries of the selected rows; no table walk, no atomics, no compaction.
* ``FakeSigIndex`` -- ``lexical_fakes.FakeLexIndex`` plus ``subset_terms`` / ``significant_terms``: the TEST DOUBLE of the
  device index for the CPU tests of ``HybridStorage.keywords`` and of the sharded ``significant_terms``.  It counts with
  ``np.unique`` over the rows' own lists and ranks with ``lexical.significant_from_counts``, the one statement of
  qualify, score and order that the product's sharded path and the GPU tests use too."""
import numpy as np

from claude_semantic_search_amd.lexical import significant_args, significant_from_counts
from lexical_fakes import FakeLexIndex


def subset_counts(poff, terms, sel):
    """``sel``: boolean over the rows of the packed lists (``poff`` has one more entry than rows)."""
    n = poff.shape[0] - 1
    erow = np.repeat(np.arange(n), np.diff(poff))
    cnt = np.bincount(terms[np.asarray(sel, bool)[erow]].astype(np.int64), minlength=1)
    t = np.flatnonzero(cnt)
    return t.astype(np.uint32), cnt[t].astype(np.int64)


class FakeSigIndex(FakeLexIndex):
    def _selected(self, mask):
        T = len(self._lists)
        if mask is None:
            return np.ones(T, bool)
        m = np.asarray(mask)
        if m.dtype != np.bool_ or m.shape != (self.ntotal,):
            raise ValueError(f"allow must be a boolean array of ntotal={self.ntotal} entries")
        return m[:T]

    def _counts(self, sel):
        rows = [self._lists[r][0] for r in np.flatnonzero(sel)]
        t, c = np.unique(np.concatenate(rows) if rows else np.zeros(0, np.int64), return_counts=True)
        return t.astype(np.uint32), c.astype(np.int64)

    def subset_terms(self, allow=None):
        self.calls.append(("subset_terms", allow is not None))
        return self._counts(self._selected(allow))

    def significant_terms(self, allow=None, m=20, min_count=2, background=None):
        m, min_count = significant_args(m, min_count)
        sel, back = self._selected(allow), self._selected(background)
        self.calls.append(("significant_terms", m, min_count, allow is not None, background is not None))
        bad = np.flatnonzero(sel & ~back)
        if bad.size:
            raise ValueError(f"significant_terms: row {int(bad[0])} is selected but not in the background")
        t, f = self._counts(sel)
        bt, bc = self._counts(back)
        b = bc[np.searchsorted(bt, t)]   # (the selection lies within the background: every term is there)
        FG = int(sel.sum())
        return significant_from_counts(t, f, b, FG, int(back.sum()) if FG else 0, m, min_count)

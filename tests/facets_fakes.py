"""numpy statements of the facet counts for the tests; they live in tests/ only and the product never falls back to them.

* ``FakeFacetIndex`` -- ``grouped_fakes.FakeGroupedIndex`` (rows, allow masks, ``id_base``, the label column) plus
  ``facets`` and ``range_search``: the TEST DOUBLE of the device index for the CPU tests of ``HybridStorage.facets`` and
  of the sharded ``facets``.  ``facets`` is stated bucket by bucket -- the hit rows of the bucket, their number, and the
  first of them under (best score, lower id) -- with no table, no keys and no atomics.  Callers build rows from
  multiples of 1/8 (or score against a unit axis) so that every score is exact in float32 whatever the summation order.
* ``corpus`` / ``expected`` -- a few hundred chunks laid out so that every count of ``HybridStorage.facets`` is known by
  construction, and the rule that says what they are, restated without the product's bucket arithmetic (calendar
  fields of ``datetime.date``, not day numbers).  The CPU tests run them over the double, the GPU tests over the HIP
  index."""
from datetime import date, datetime, timedelta

import numpy as np

from claude_semantic_search_amd.chunk import Chunk
from claude_semantic_search_amd.flat_index import FacetCounts, facet_args
from grouped_fakes import FakeGroupedIndex
from related_fakes import FLT_MAX


class FakeFacetIndex(FakeGroupedIndex):
    def _hits(self, q, thresh, allow):
        s = self._scores(q)
        r = np.float32(thresh)
        return s, (s > r if self.metric_type == 0 else s < r) & self._ok(s.shape[0], allow)   # strict, as the library

    def facets(self, q, thresh, buckets=None, nbuckets=None, normalize=False, allow=None):
        thresh, b, nb = facet_args(thresh, buckets, nbuckets, self.ntotal)
        self.calls.append(("facets", buckets is None, nb, allow is not None))
        lab = self._g if b is None else b
        s, hit = self._hits(q, thresh, allow)
        nq = s.shape[0]
        out = FacetCounts(np.zeros((nq, nb), np.int64), np.full((nq, nb), -FLT_MAX if self.metric_type == 0 else FLT_MAX, np.float32),
                          np.full((nq, nb), -1, np.int64), hit.sum(1).astype(np.int64),
                          (hit & ((lab < 0) | (lab >= nb))[None, :]).sum(1).astype(np.int64))
        for j in range(nq):
            for v in np.unique(lab[hit[j] & (lab >= 0) & (lab < nb)]):
                rows = np.flatnonzero(hit[j] & (lab == v))
                first = rows[np.lexsort((rows, -s[j, rows] if self.metric_type == 0 else s[j, rows]))[0]]
                out.counts[j, v], out.best_score[j, v], out.best_id[j, v] = rows.size, s[j, first], first + self.base
        return out

    def range_search(self, q, thresh, normalize=False, allow=None):
        self.calls.append(("range_search", np.float32(thresh), allow is not None))
        s, hit = self._hits(q, thresh, allow)
        lims, D, I = [0], [np.zeros(0, np.float32)], [np.zeros(0, np.int64)]
        for j in range(s.shape[0]):
            ids = np.flatnonzero(hit[j])
            order = np.lexsort((ids, -s[j, ids] if self.metric_type == 0 else s[j, ids]))
            D.append(s[j, ids][order])
            I.append(ids[order].astype(np.int64) + self.base)
            lims.append(lims[-1] + ids.size)
        return np.array(lims, np.int64), np.concatenate(D).astype(np.float32), np.concatenate(I)


# ------------------------------------------------------------------ a corpus whose facet counts are known by construction
D_ = 8
N = 240
LEVELS = (0.9, 0.7, 0.5, 0.3, 0.1, -0.2)          # the similarity of chunk i to Q is LEVELS[i % 6] (to within 1e-6)
PROJECTS = ("alpha", "beta", "gamma", None)
TYPES = ("conversation", "code", "tool")
Q = [1.0] + [0.0] * (D_ - 1)
T0 = datetime(2024, 1, 1, 12, 0, 0)


def fields(i):
    """The metadata of chunk ``i`` (``None``: the key is absent and the column NULL)."""
    ts = None if i % 10 == 9 else T0 + timedelta(days=2 * i, hours=i % 7)        # 16 months; every tenth without
    return {"project_name": PROJECTS[(i // 6) % 4], "session_id": None if i % 5 == 4 else f"s{i % 5}{(i // 60) % 2}",
            "chunk_type": TYPES[i % 3], "has_code": i % 2 == 0, "has_tools": i % 4 == 0,
            "timestamp": None if ts is None else ts.isoformat() + ("Z" if i % 3 == 0 else "")}


def corpus(lo=0, hi=N):
    out = []
    for i in range(lo, hi):
        c = LEVELS[i % 6]
        e = np.zeros(D_, np.float32)
        e[0], e[1] = c, np.sqrt(1.0 - c * c)                                       # a unit vector at cos = level
        out.append(Chunk(f"c{i}", f"text {i}", {k: v for k, v in fields(i).items() if v is not None}, e))
    return out


def bucket_value(i, by):
    """What bucket chunk ``i`` belongs to under ``by`` (``None``: missing), from calendar fields."""
    f = fields(i)
    if by in ("day", "week", "month"):
        if f["timestamp"] is None:
            return None
        d = date.fromisoformat(f["timestamp"][:10])
        if by == "week":
            d = d - timedelta(days=d.weekday())                                   # the Monday of the week
        if by == "month":
            d = d.replace(day=1)
        return d.isoformat()
    return f[by]


def expected(by, threshold, l2=False, dead=(), keep=lambda i: True, top=None, n=N):
    """``(total, missing, [(value, count, best chunk id), ...])`` in the order of ``HybridStorage.facets``."""
    score = (lambda i: 2.0 - 2.0 * LEVELS[i % 6]) if l2 else (lambda i: LEVELS[i % 6])
    hit = [i for i in range(n) if i not in dead and keep(i)
           and (score(i) <= threshold + 1e-5 if l2 else score(i) >= threshold - 1e-5)]
    groups = {}
    for i in hit:
        v = bucket_value(i, by)
        if v is not None:
            groups.setdefault(v, []).append(i)
    rows = []
    for v, members in groups.items():
        best = min(members, key=lambda i: (score(i) if l2 else -score(i), i))
        rows.append((v, len(members), best))
    rows.sort(key=lambda r: (-r[1], score(r[2]) if l2 else -score(r[2]), r[0]))
    return len(hit), len(hit) - sum(r[1] for r in rows), [(v, c, f"c{b}") for v, c, b in (rows if top is None else rows[:top])]


def as_tuples(res):
    """A ``Facets`` in the shape ``expected`` returns."""
    return res.total, res.missing, [(f.value, f.count, f.best.chunk_id) for f in res.buckets]

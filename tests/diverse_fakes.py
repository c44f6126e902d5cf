"""numpy TEST DOUBLE of the diversified search for the CPU tests of ``HybridStorage.search_diverse`` and of the sharded
diversified search: ``related_fakes.FakeIndex`` plus ``search_diverse``, and ``mmr_loop``, the selection rule written as
plain loops over scalars -- INDEPENDENTLY of ``flat_index.mmr_select`` (no arrays of penalties carried from step to step:
every step forms ``max_u sim(c, p_u)`` over all picks so far from scratch).  It lives in tests/ only; the product never
falls back to it.

Callers build rows from multiples of 1/8 and weights from multiples of 1/4, so that every similarity, every product and
every difference is exact in float32 whatever the summation order: the loop, the numpy statement, a sharded and an
unsharded double then give the same bits, and ties are plentiful."""
import numpy as np

from related_fakes import FLT_MAX, FakeIndex


def mmr_loop(S, I, X, k, lam, metric):
    """``S, I``: [nq, m] best-first lists, pads (I = -1) at the tail; ``X``: [nq, m, d] the candidates' rows.  Returns the
    picks ``(D[nq, k], I[nq, k])`` in pick order, padded."""
    nq, m = I.shape
    lam = np.float32(lam)
    oml = np.float32(1.0) - lam
    Do = np.full((nq, k), -FLT_MAX if metric == 0 else FLT_MAX, np.float32)
    Io = np.full((nq, k), -1, np.int64)

    def sim(a, b):   # float64 sum, rounded once: exact on the grid the callers use
        a, b = a.astype(np.float64), b.astype(np.float64)
        return np.float32((a * b).sum()) if metric == 0 else np.float32(-((a - b) ** 2).sum())

    for j in range(nq):
        valid = [c for c in range(m) if I[j, c] >= 0]
        picks = []
        while len(picks) < min(k, len(valid)):
            if not picks:
                picks.append(valid[0])
                continue
            best, best_v = None, None
            for c in valid:                      # ascending c: a later candidate must be strictly better
                if c in picks:
                    continue
                rel = np.float32(S[j, c]) if metric == 0 else np.float32(-S[j, c])
                pen = max(sim(X[j, c], X[j, p]) for p in picks)
                v = np.float32(lam * rel) - np.float32(oml * np.float32(pen))
                if best is None or v > best_v:
                    best, best_v = c, v
            picks.append(best)
        for t, c in enumerate(picks):
            Do[j, t], Io[j, t] = S[j, c], I[j, c]
    return Do, Io


def auto_fetch(k, fetch):
    return fetch if fetch else (32 if 4 * k <= 32 else 128)


class FakeDiverseIndex(FakeIndex):
    def search_diverse(self, q, k, lam=0.5, fetch=0, normalize=False, allow=None):
        k, fetch = int(k), auto_fetch(int(k), int(fetch))
        assert 1 <= k <= fetch <= 128 and 0.0 <= float(lam) <= 1.0
        self.calls.append(("search_diverse", k, allow is not None))
        s = self._scores(q)
        S, I = self._topk(s, self._ok(s.shape[0], allow), fetch)
        X = self._x[np.maximum(I - self.base, 0)] if self.ntotal else np.zeros(I.shape + (self.d,), np.float32)
        return mmr_loop(S, I, X, k, lam, self.metric_type)

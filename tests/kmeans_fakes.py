"""numpy TEST DOUBLE of the device index for the CPU tests of k-means: ``related_fakes.FakeIndex`` plus ``kmeans_step``,
``kmeans``, ``reconstruct_batch`` and ``bounds``.  The step states the rule of ``css_index_kmeans_step`` INDEPENDENTLY of
the kernels: keys in float64 (``<x, c> - ||c||^2 / 2``), argmax with ties to the lower index, distances
``max(0, ||x||^2 - 2 key)`` rounded to float32, and the sums through ``flat_index.fixed_point_sums``.  It lives in tests/
only; the product never falls back to it.

Callers that compare a sharded and an unsharded double, or the double and the device, build rows from multiples of 1/8
so that every key is exact whatever the summation order."""
import numpy as np

from claude_semantic_search_amd import flat_index as fi
from related_fakes import FakeIndex


def keys64(x, c):
    """``[n, nc]`` float64 keys ``<x, c> - ||c||^2 / 2`` of float32 rows and centroids."""
    x64, c64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(c, np.float32).astype(np.float64)
    return x64 @ c64.T - 0.5 * (c64 * c64).sum(axis=1)[None, :]


def assign64(x, c, allow=None):
    """``(assign int32, dist float32, key64 of the winner)``: the float64 statement of the assignment."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    a = np.full(n, -1, np.int32)
    d = np.zeros(n, np.float32)
    kw = np.zeros(n, np.float64)
    if n:
        key = keys64(x, c)
        best = key.argmax(axis=1)                       # (the first maximum: the lower index)
        kw = key[np.arange(n), best]
        n2 = (x.astype(np.float64) ** 2).sum(axis=1)
        ok = np.ones(n, bool) if allow is None else np.asarray(allow, bool)
        a[ok] = best[ok]
        d[ok] = np.maximum(0.0, n2 - 2.0 * kw)[ok].astype(np.float32)
    return a, d, kw


class FakeKmeansIndex(FakeIndex):
    def bounds(self):
        n2 = (self._x.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
        return {"max_norm2": float(n2.max()) if n2.size else 0.0, "max_bf16_err2": 0.0, "max_int8_err2": 0.0}

    def reconstruct_batch(self, ids):
        a = np.asarray(ids, np.int64).reshape(-1) - self.base
        assert a.size == 0 or (a.min() >= 0 and a.max() < self.ntotal)
        return self._x[a].copy()

    def kmeans_step(self, centroids, allow=None, fx_shift=None, want_assign=False, want_dist=False):
        c = np.asarray(centroids, np.float32).reshape(-1, self.d)
        self.calls.append(("kmeans_step", c.shape[0], allow is not None))
        assert 2 <= c.shape[0] <= fi.MAX_CENTROIDS and np.isfinite(c).all()
        if allow is not None:
            assert np.asarray(allow).dtype == np.bool_ and np.asarray(allow).shape == (self.ntotal,)
        s_own, e, _ = fi.kmeans_shift(self.bounds()["max_norm2"], self.ntotal)
        s = s_own if fx_shift is None else int(fx_shift)
        assert s <= s_own
        t = s - e - 2
        a, d, _ = assign64(self._x, c, allow)
        sums, counts = fi.fixed_point_sums(self._x, a, c.shape[0], s)
        return fi.KmeansStep(sums, counts, fi.fixed_point_objective(d, a, t), s, t, a if want_assign else None,
                             d if want_dist else None)

    def kmeans(self, nc, niter=20, seed=0, init=None, spherical=None, allow=None, max_points_per_centroid=0):
        n = self.ntotal
        rows = np.arange(n, dtype=np.int64) if allow is None else np.flatnonzero(np.asarray(allow)).astype(np.int64)
        sph = self.metric_type == 0 if spherical is None else bool(spherical)
        train = fi.kmeans_train_mask(rows, n, nc, int(max_points_per_centroid), seed)
        return fi.run_kmeans(lambda c, a, want: self.kmeans_step(c, allow=a, want_assign=want, want_dist=want),
                             lambda ids: self.reconstruct_batch(np.asarray(ids, np.int64) + self.base), nc, niter=niter,
                             seed=seed, init=init, spherical=sph, init_rows=rows,
                             train_allow=allow if train is None else train, allow=allow)


def planted(n, d, centres, seed, spread=1):
    """``n`` rows around ``centres`` well-separated points, every entry a multiple of 1/8: ``(rows, labels, centres)``.
    Centres are +-2 patterns that differ in at least d / 4 coordinates; the noise is at most ``spread / 8`` per entry."""
    rng = np.random.default_rng(seed)
    C = np.zeros((centres, d), np.float32)
    for c in range(centres):
        C[c] = np.where((np.arange(d) // max(1, d // (2 * centres)) + c) % centres == 0, 2.0, -1.0)
    lab = rng.integers(0, centres, size=n)
    lab[:centres] = np.arange(centres)   # (every cluster has a member)
    x = C[lab] + rng.integers(-spread, spread + 1, size=(n, d)).astype(np.float32) / 8.0
    return x.astype(np.float32), lab.astype(np.int64), C


# the Gaussian cases of the GPU test: (d, scale of the rows, seed); n rows and nc centroids each
GAUSS_N, GAUSS_NC = 1037, 129
GAUSS_CASES = ((768, 1.0, 101), (768, 30.0, 102), (100, 1.0, 103), (100, 30.0, 104))


def gaussian_case(d, scale, seed, n=GAUSS_N, nc=GAUSS_NC):
    """Unit Gaussian rows times ``scale`` and ``nc`` centroids: a third are copies of rows, the rest blends of two rows
    (so many rows have two centroids at comparable distance): ``(rows float32, centroids float32)``."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    x = (scale * x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    pick = rng.choice(n, (nc, 2), replace=False)
    w = rng.uniform(0.3, 0.7, size=(nc, 1))
    w[: nc // 3] = 1.0
    c = (w * x[pick[:, 0]] + (1.0 - w) * x[pick[:, 1]]).astype(np.float32)
    return x, c

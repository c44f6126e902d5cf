"""numpy TEST DOUBLE of the device index for the CPU tests of PCA: ``kmeans_fakes.FakeKmeansIndex`` plus ``gram``, ``pca``
and ``transform``.  It states the contract of ``css_index_gram`` / ``css_index_transform`` INDEPENDENTLY of the kernels:
the Gram matrix through ``flat_index.fixed_point_gram`` with a few entries cross-checked against Python-int sums (which
cannot wrap), the transform in float64 rounded once.  It lives in tests/ only; the product never falls back to it."""
import numpy as np

from claude_semantic_search_amd import flat_index as fi
from kmeans_fakes import FakeKmeansIndex


def python_int_entries(x, allow, p, entries):
    """``{(i, j): gram[i][j], (j,): colsum[j]}`` for the asked entries, summed as Python ints from float64 quantisation."""
    x = np.asarray(x, np.float32)
    keep = np.ones(x.shape[0], bool) if allow is None else np.asarray(allow, bool)
    q = [[int(v) for v in np.rint(np.ldexp(row.astype(np.float64), p))] for row in x[keep]]
    out = {}
    for at in entries:
        out[at] = sum(r[at[0]] * r[at[1]] for r in q) if len(at) == 2 else sum(r[at[0]] for r in q)
    return out


def planted_pca(n, d, seed, variances=(0.4, 0.2, 0.1), floor=0.001, mean=0.0):
    """``n`` rows ``mean + sum_k a_k u_k + noise``: orthonormal ``u_k``, ``a_k`` of the given variances, white noise of
    variance ``floor`` per coordinate: ``(rows float32, U [k, d] float64)``."""
    rng = np.random.default_rng(seed)
    U = np.linalg.qr(rng.standard_normal((d, len(variances))))[0].T
    a = rng.standard_normal((n, len(variances))) * np.sqrt(np.asarray(variances))
    x = a @ U + rng.standard_normal((n, d)) * np.sqrt(floor) + mean
    return x.astype(np.float32), U


def pca64(x, m):
    """The float64 PCA of the raw rows: ``(eigenvalues descending [m], components [m, d], all eigenvalues)``."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    c = x64 - x64.mean(axis=0)
    w, V = np.linalg.eigh(c.T @ c / x64.shape[0])
    return w[::-1][:m], V[:, ::-1][:, :m].T, w[::-1]


def transform64(x, A, b=None):
    """``y = A x + b`` in float64 and the magnitude sum ``sum_j |x_j A_cj| + |b_c|`` the rounding bound scales with."""
    x64, A64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(A, np.float32).astype(np.float64)
    b64 = np.zeros(A64.shape[0]) if b is None else np.asarray(b, np.float32).astype(np.float64)
    return x64 @ A64.T + b64, np.abs(x64) @ np.abs(A64).T + np.abs(b64)


class FakePcaIndex(FakeKmeansIndex):
    def gram(self, allow=None, fx_shift=None):
        self.calls.append(("gram", 0, allow is not None))
        if allow is not None:
            assert np.asarray(allow).dtype == np.bool_ and np.asarray(allow).shape == (self.ntotal,)
        own = fi.pca_shift(self.bounds()["max_norm2"], self.ntotal)[0]
        p = own if fx_shift is None else int(fx_shift)
        assert p <= own
        gram, colsum, count = fi.fixed_point_gram(self._x, allow, p)
        d = self.d
        want = python_int_entries(self._x, allow, p, [(0, 0), (0, d - 1), (d - 1, d // 2), (d // 2,)])
        for at, v in want.items():
            assert int(gram[at] if len(at) == 2 else colsum[at[0]]) == v
        return fi.GramResult(gram, colsum, count, p)

    def pca(self, n_components, allow=None, whiten=False):
        g = self.gram(allow=allow)
        return fi.pca_from_gram(g.gram, g.colsum, g.count, g.shift, n_components, whiten=whiten)

    def transform(self, A, b=None, row0=0, n=None):
        A = np.asarray(A, np.float32).reshape(-1, self.d)
        self.calls.append(("transform", A.shape[0], b is not None))
        assert 1 <= A.shape[0] <= fi.MAX_TRANSFORM_ROWS and np.isfinite(A).all()
        n = self.ntotal - row0 if n is None else n
        assert 0 <= row0 and 0 <= n and row0 + n <= self.ntotal
        return transform64(self._x[row0:row0 + n], A, b)[0].astype(np.float32)

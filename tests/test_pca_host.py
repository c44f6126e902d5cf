"""CPU: the host statements of PCA on the flat index (``pca_shift``, ``fixed_point_gram``, ``pca_from_gram``), the
premise of the Gram kernel stated in numpy, and ``PCAMatrix`` / ``HybridStorage.map`` over the numpy double
``pca_fakes.FakePcaIndex``."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from claude_semantic_search_amd import flat_index as fi  # noqa: E402
from claude_semantic_search_amd.chunk import Chunk  # noqa: E402
from claude_semantic_search_amd.storage import HybridStorage, MapPoint, StorageConfig  # noqa: E402
from kmeans_fakes import FakeKmeansIndex, planted  # noqa: E402
from pca_fakes import FakePcaIndex, pca64, planted_pca, python_int_entries, transform64  # noqa: E402


# unit rows: ||x||^2 = 1 = 0.5 * 2^1, ex = 1, e = 1.  Norm 3.7: 13.69 = 0.856 * 2^4, ex = 4, e = 2.
@pytest.mark.parametrize("max_norm2, n, want", [
    (1.0, 1, (19, 1)),                  # b = 0: min(20, 31) - 1
    (1.0, 1 << 22, (19, 1)),            # b = 22: min(20, 40 >> 1) - 1
    (1.0, (1 << 22) + 1, (18, 1)),      # b = 23: (39 >> 1) - 1
    (1.0, 10 ** 7, (18, 1)),            # b = 24: (38 >> 1) - 1
    (3.7 * 3.7, 8270, (18, 2)),         # b = 14: min(20, 24) - 2
    (0.0, 0, (20, 0)),
    (2.0 ** 40, 1000, (-1, 21)),        # ex = 41, e = 21: a negative shift is a legal answer
])
def test_pca_shift_by_hand(max_norm2, n, want):
    assert fi.pca_shift(max_norm2, n) == want


def test_the_shift_keeps_every_sum_below_2_to_the_62():
    for n in (0, 1, 2, 3, 1000, 8192, 8193, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, 10 ** 7, 1 << 31, (1 << 40) + 7):
        for m in (0.0, 1e-30, 0.24, 0.25, 0.5, 0.99, 1.0, 1.01, 3.99, 4.0, 13.69, 900.0, 2.0 ** 40, 3e38):
            p, e = fi.pca_shift(m, n)
            assert np.sqrt(float(np.float32(m))) <= 2.0 ** e
            assert p + e <= 20                                   # |q| <= 2^20: a product is at most 2^40
            assert max(n, 1) * (1 << (2 * (p + e))) <= 1 << 62, (n, m)
            # and the rule is tight: one more bit would break one of the two
            assert p + e == 20 or max(n, 1) * (1 << (2 * (p + e + 1))) > 1 << 62


def test_8192_extreme_rows_sum_exactly_in_float64_and_8193_need_not():
    """The premise of k_gram_fx.  At the extreme magnitude 2^e (1 - 2^-20) under p + e = 20 a quantised entry is
    2^20 - 1 and its square 2^40 - 2^21 + 1 (odd).  8192 of them sum to less than 2^53, so every partial sum is an
    integer a double holds and float64 addition is exact in ANY order; 8193 of them sum to an odd number above 2^53,
    which no double holds -- which is why the kernel folds into int64 every 8192 rows."""
    p, e = fi.pca_shift(1.0, 8192)
    assert (p, e) == (19, 1)
    v = np.float32(2.0 ** e * (1.0 - 2.0 ** -20))
    q = fi._fixed(np.full(8193, v, np.float32), p)
    assert int(q[0]) == (1 << 20) - 1
    sq = q.astype(np.float64) * q.astype(np.float64)
    exact = [int(t) * int(t) for t in q]
    assert float(np.cumsum(sq[:8192])[-1]) == float(sum(exact[:8192])) and sum(exact[:8192]) < 1 << 53
    assert int(np.cumsum(sq[:8192])[-1]) == sum(exact[:8192]) == int(sq[:8192].sum()) == int(np.cumsum(sq[:8192][::-1])[-1])
    rng = np.random.default_rng(0)                               # mixed signs, a shuffled order: still exact
    sign = rng.choice([-1.0, 1.0], size=8192)
    other = (q[:8192].astype(np.float64) * sign) * q[:8192].astype(np.float64)
    assert int(np.cumsum(rng.permutation(other))[-1]) == int(sign.sum()) * exact[0]
    assert sum(exact) > 1 << 53 and sum(exact) % 2 == 1
    assert int(np.cumsum(sq)[-1]) != sum(exact)


def test_fixed_point_gram_is_the_python_int_sum_and_honours_the_mask():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((300, 12)) * 1.3).astype(np.float32)
    allow = np.arange(300) % 3 == 0
    for mask in (None, allow):
        p = fi.pca_shift(float((x.astype(np.float64) ** 2).sum(1).max()), 300)[0]
        gram, colsum, count = fi.fixed_point_gram(x, mask, p)
        assert gram.dtype == np.int64 and colsum.dtype == np.int64 and count == (300 if mask is None else 100)
        assert np.array_equal(gram, gram.T)
        at = [(i, j) for i in range(12) for j in range(12)] + [(j,) for j in range(12)]
        want = python_int_entries(x, mask, p, at)
        assert all(int(gram[a]) == want[a] for a in at if len(a) == 2)
        assert all(int(colsum[a[0]]) == want[a] for a in at if len(a) == 1)
    gram, colsum, count = fi.fixed_point_gram(x, np.zeros(300, bool), 10)
    assert not gram.any() and not colsum.any() and count == 0
    # the largest magnitudes the shift rule admits, across two 4096-row chunks, and entries past the limb path
    big = (rng.choice([-2.0, 2.0], size=(5000, 6)) * (1.0 - 2.0 ** -20)).astype(np.float32)
    for shift, rows in ((19, big), (26, big[:100])):
        gram, colsum, _ = fi.fixed_point_gram(rows, None, shift)
        q = fi._fixed(rows, shift)
        assert int(np.abs(q).max()) == ((1 << 20) - 1) << (shift - 19)
        assert np.array_equal(gram, q.T @ q) and np.array_equal(colsum, q.sum(axis=0))
        assert int(gram[0, 0]) == rows.shape[0] * int(q[0, 0]) ** 2
    half = fi.fixed_point_gram(np.array([[0.5, 1.5, 2.5, -0.5]], np.float32), None, 0)        # ties go to even
    assert half[1].tolist() == [0, 2, 2, 0]


D64, N64 = 64, 4000


def _planted():
    x, U = planted_pca(N64, D64, seed=3, mean=0.05)
    fake = FakePcaIndex(D64, 1)
    fake.add(x)
    return x, U, fake


def test_pca_from_gram_on_planted_data_is_within_the_perturbation_bounds():
    """The quantised rows are xq = q 2^-p with |xq - x| <= delta = 2^-(p+1) per entry, eps = xq - x.  The covariance of
    xq is C + cov(x, eps) + cov(eps, x) + cov(eps, eps).  |cov(x_i, eps_j)| = |E[(x_i - mu_i) eps_j]| <= E|x_i - mu_i|
    delta <= 2 * 2^e * delta (every |x| < 2^e), twice; |cov(eps_i, eps_j)| <= 2 delta^2.  So every entry of the
    perturbation E is at most 4 * 2^e * delta + 2 delta^2, ||E||_2 <= ||E||_F <= d max|E_ij| = tol, and by Weyl every
    eigenvalue moves by at most tol; by Davis-Kahan the top-3 subspace turns by sin(theta) <= 2 tol / gap, gap being the
    distance from the third to the fourth eigenvalue."""
    x, U, fake = _planted()
    g = fake.gram()
    p, e = fi.pca_shift(fake.bounds()["max_norm2"], N64)
    assert g.shift == p and g.count == N64
    delta = 2.0 ** -(p + 1)
    tol = D64 * (4.0 * 2.0 ** e * delta + 2.0 * delta * delta)
    res = fi.pca_from_gram(g.gram, g.colsum, g.count, g.shift, D64)
    w64, V64, _ = pca64(x, D64)
    print(f"p={p} e={e} tol={tol:.3g}: worst eigenvalue error {np.abs(res.eigenvalues - w64).max():.3g}")
    assert np.abs(res.eigenvalues - w64).max() <= tol
    cos = np.linalg.svd(V64[:3] @ res.components[:3].astype(np.float64).T, compute_uv=False)
    sin = float(np.sqrt(max(0.0, 1.0 - cos.min() ** 2)))
    gap = w64[2] - w64[3]
    print(f"sin(theta) of the top-3 subspace {sin:.3g}, bound {2 * tol / gap:.3g}")
    assert sin <= 2.0 * tol / gap + 3e-7                         # (the components were rounded to float32)
    # the data is what it claims: three planted directions over a floor, recovered
    assert np.allclose(w64[:3], (0.4, 0.2, 0.1), rtol=0.12) and w64[3] < 0.0015
    assert np.linalg.svd(U @ res.components[:3].astype(np.float64).T, compute_uv=False).min() > 0.999
    assert np.abs(res.mean.astype(np.float64) - x.astype(np.float64).mean(axis=0)).max() <= delta + 2.0 ** -24
    assert abs(res.total_variance - w64.sum()) <= D64 * tol
    assert res.mean.dtype == np.float32 and res.components.dtype == np.float32 and res.eigenvalues.dtype == np.float64


def test_pca_from_gram_orders_signs_whitens_and_refuses_nothing():
    x, U, fake = _planted()
    g = fake.gram()
    res = fi.pca_from_gram(g.gram, g.colsum, g.count, g.shift, 5)
    assert res.components.shape == (5, D64) and res.eigenvalues.shape == (5,)
    assert (np.diff(res.eigenvalues) <= 0).all() and (res.eigenvalues >= 0).all()
    lead = np.abs(res.components).argmax(axis=1)
    assert (res.components[np.arange(5), lead] > 0).all()
    # the sign rule does not depend on the sign eigh happened to return: a mirrored data set gives mirrored components
    mirrored = FakePcaIndex(D64, 1)
    mirrored.add(-x)
    gm = mirrored.gram()
    assert np.array_equal(gm.gram, g.gram) and np.array_equal(gm.colsum, -g.colsum)
    rm = fi.pca_from_gram(gm.gram, gm.colsum, gm.count, gm.shift, 5)
    assert rm.components.tobytes() == res.components.tobytes() and np.array_equal(rm.mean, -res.mean)
    # whitening: component i over sqrt(eigenvalue i), the transformed rows have unit variance
    white = fi.pca_from_gram(g.gram, g.colsum, g.count, g.shift, 3, whiten=True)
    assert np.array_equal(white.eigenvalues, res.eigenvalues[:3])
    assert np.allclose(white.components, res.components[:3] / np.sqrt(res.eigenvalues[:3])[:, None].astype(np.float32), rtol=1e-6, atol=0)
    y = (x.astype(np.float64) - white.mean.astype(np.float64)) @ white.components.astype(np.float64).T
    assert np.allclose(y.var(axis=0), 1.0, atol=1e-3)
    # the same integers, the same bytes
    again = fi.pca_from_gram(g.gram.copy(), g.colsum.copy(), g.count, g.shift, 5)
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(again, res))
    with pytest.raises(ValueError, match="no rows"):
        fi.pca_from_gram(np.zeros((4, 4), np.int64), np.zeros(4, np.int64), 0, 19, 2)
    for m in (0, D64 + 1):
        with pytest.raises(ValueError, match="n_components"):
            fi.pca_from_gram(g.gram, g.colsum, g.count, g.shift, m)
    # a constant data set: zero variance, eigenvalues clipped at 0, whitening stays finite
    same = fi.fixed_point_gram(np.full((7, 4), 0.3, np.float32), None, 19)
    flat = fi.pca_from_gram(*same, 19, 2, whiten=True)
    assert (flat.eigenvalues == 0).all() and np.isfinite(flat.components).all()


# ----------------------------------------------------------------------------- PCAMatrix and HybridStorage.map over the double
def _use(monkeypatch, cls):
    monkeypatch.setattr(fi, "IndexFlat", cls)
    monkeypatch.setattr(fi, "IndexFlatIP", lambda d, device=0: cls(d, 0, device))
    monkeypatch.setattr(fi, "IndexFlatL2", lambda d, device=0: cls(d, 1, device))


def test_pcamatrix_over_the_double(monkeypatch):
    _use(monkeypatch, FakePcaIndex)
    x, U, fake = _planted()
    ref = fake.pca(3)
    pm = fi.PCAMatrix(D64, 3)
    assert not pm.is_trained
    with pytest.raises(RuntimeError):
        pm.apply(x[:2])
    pm.train(x)
    assert pm.is_trained and pm.A.shape == (3, D64) and pm.b.shape == (3,)
    assert pm.A.tobytes() == ref.components.tobytes() and pm.mean.tobytes() == ref.mean.tobytes()
    assert np.array_equal(pm.eigenvalues, ref.eigenvalues)
    assert pm.b.tobytes() == (-(pm.A.astype(np.float64) @ pm.mean.astype(np.float64))).astype(np.float32).tobytes()
    y = pm.apply(x)
    assert y.shape == (N64, 3) and y.dtype == np.float32 and pm.apply_py(x[:5]).tobytes() == y[:5].tobytes()
    want = (x.astype(np.float64) - ref.mean.astype(np.float64)) @ ref.components.astype(np.float64).T
    assert np.abs(y - want).max() <= 1e-6
    assert np.allclose(y.astype(np.float64).var(axis=0), ref.eigenvalues, rtol=1e-4)
    back = pm.reverse_transform(y)
    assert back.shape == x.shape and np.sqrt(((back - x).astype(np.float64) ** 2).mean()) <= 1.1 * np.sqrt(0.001)
    white = fi.PCAMatrix(D64, 3, eigen_power=-0.5)
    white.train(x)
    yw = white.apply(x)
    assert np.allclose(yw.astype(np.float64).var(axis=0), 1.0, atol=1e-3)
    assert np.abs(white.reverse_transform(yw) - back).max() <= 1e-4
    with pytest.raises(ValueError, match="eigen_power"):
        fi.PCAMatrix(D64, 3, eigen_power=-1.0)
    for bad in (0, D64 + 1):
        with pytest.raises(ValueError, match="d_out"):
            fi.PCAMatrix(D64, bad)
    with pytest.raises(ValueError):
        pm.train(x[:, :10])


D_ = 16


def _storage(tmp_path, n=90):
    lab = np.repeat([0, 1, 2], [n // 2, n // 3, n - n // 2 - n // 3])
    C = planted(3, D_, 3, seed=0)[2]
    x = (C[lab] + np.random.default_rng(21).integers(-1, 2, size=(n, D_)) / 8.0).astype(np.float32)
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=D_, normalize_embeddings=False,
                                    auto_save=False))
    s.initialize()
    s.add_chunks([Chunk(f"c{i}", f"text {i}", {"project_name": "alpha" if i % 2 else "beta", "session_id": f"s{lab[i]}"}, x[i])
                  for i in range(n)])
    return s, lab, x


def _expect(x, allow):
    """The map of the allowed rows of x stated through the double: {row: (x, y)}."""
    fake = FakePcaIndex(D_, 1)
    fake.add(x)
    res = fake.pca(2, allow=allow)
    y = fake.transform(res.components, fi.pca_offset(res.components, res.mean))
    return {int(r): (float(y[r, 0]), float(y[r, 1])) for r in np.flatnonzero(allow)}


def test_map_coordinates_tombstones_filters_and_topics(tmp_path, monkeypatch):
    _use(monkeypatch, FakePcaIndex)
    s, lab, x = _storage(tmp_path)
    pts = s.map()
    assert all(isinstance(p, MapPoint) for p in pts) and [p.chunk_id for p in pts] == [f"c{i}" for i in range(90)]
    want = _expect(x, np.ones(90, bool))
    assert all((p.x, p.y) == want[i] and p.topic is None for i, p in enumerate(pts))
    # the three planted groups are apart on the map: nearest centre of the map = the planted label
    xy = np.array([(p.x, p.y) for p in pts])
    cen = np.stack([xy[lab == c].mean(axis=0) for c in range(3)])
    assert np.array_equal(((xy[:, None, :] - cen[None]) ** 2).sum(-1).argmin(axis=1), lab)
    assert ("gram", 0, True) in s.faiss_index.calls and ("transform", 2, True) in s.faiss_index.calls
    # tombstones are left out of the PCA and of the result
    assert s.delete_chunk("c0") and s.delete_chunk("c89")
    live = np.ones(90, bool)
    live[[0, 89]] = False
    pts = s.map()
    want = _expect(x, live)
    assert [p.chunk_id for p in pts] == [f"c{i}" for i in range(1, 89)]
    assert all((p.x, p.y) == want[int(p.chunk_id[1:])] for p in pts)
    # a filter: the PCA is that of the selection
    sel = live & (np.arange(90) % 2 == 1)
    pts = s.map(filters={"project_name": "alpha"})
    want = _expect(x, sel)
    assert [int(p.chunk_id[1:]) for p in pts] == np.flatnonzero(sel).tolist()
    assert all((p.x, p.y) == want[int(p.chunk_id[1:])] for p in pts)
    # topics: the k-means assignment under the same mask and seed, i.e. what topics() reports
    pts = s.map(n_topics=3, seed=4)
    topics = s.topics(n_topics=3, seed=4)
    member = {c: k for k, t in enumerate(topics) for c in t.chunk_ids}
    assert len(pts) == 88 and all(p.topic is not None and 0 <= p.topic < 3 for p in pts)
    pairs = {(p.topic, member[p.chunk_id]) for p in pts}
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})    # one-to-one
    assert all(p.topic is None for p in s.map(n_topics=1))
    calls = len(s.faiss_index.calls)
    short = s.map(n_topics=3, seed=4, niter=1)                   # niter is passed on: one Lloyd step and the final one
    assert sum(c[0] == "kmeans_step" for c in s.faiss_index.calls[calls:]) == 2
    member = {c: k for k, t in enumerate(s.topics(n_topics=3, seed=4, niter=1)) for c in t.chunk_ids}
    pairs = {(p.topic, member[p.chunk_id]) for p in short}
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})
    # nothing selected, and one chunk
    assert s.map(filters={"project_name": "nobody"}) == []
    one = s.map(filters={"session_id": "s2", "project_name": "alpha"}, n_topics=2)
    few = [i for i in range(1, 89) if lab[i] == 2 and i % 2 == 1]
    assert len(one) == len(few)
    for i in few[1:]:
        assert s.delete_chunk(f"c{i}")
    one = s.map(filters={"session_id": "s2", "project_name": "alpha"}, n_topics=2)
    assert one == [MapPoint(f"c{few[0]}", 0.0, 0.0, 0)]
    s.close()


def test_map_on_an_empty_index_and_on_an_index_without_pca(tmp_path, monkeypatch):
    _use(monkeypatch, FakePcaIndex)
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "e"), embedding_dim=D_, normalize_embeddings=False, auto_save=False))
    s.initialize()
    assert s.map() == []
    s.close()
    _use(monkeypatch, FakeKmeansIndex)
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "f"), embedding_dim=D_, normalize_embeddings=False, auto_save=False))
    s.initialize()
    s.add_chunks([Chunk("a", "t", {}, np.ones(D_, np.float32)), Chunk("b", "t", {}, -np.ones(D_, np.float32))])
    with pytest.raises(NotImplementedError, match="pca"):
        s.map()
    s.close()

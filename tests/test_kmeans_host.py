"""CPU: the host statements of k-means in ``flat_index`` -- ``kmeans_shift``, ``fixed_point_sums``, ``lloyd_update``,
``kmeans_init_ids``, ``run_kmeans`` -- against values worked out by hand or in float64, ``run_kmeans`` and
``HybridStorage.topics`` over the numpy double ``kmeans_fakes.FakeKmeansIndex``."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from claude_semantic_search_amd import flat_index as fi  # noqa: E402
from claude_semantic_search_amd.chunk import Chunk  # noqa: E402
from claude_semantic_search_amd.storage import HybridStorage, StorageConfig, Topic  # noqa: E402
from kmeans_fakes import GAUSS_CASES, FakeKmeansIndex, assign64, gaussian_case, planted  # noqa: E402
from related_fakes import FakeIndex  # noqa: E402


# ----------------------------------------------------------------------------- kmeans_shift
@pytest.mark.parametrize("max_norm2, n, want", [
    (1.0, 1, (61, 1, 58)),                  # frexp(1.0) = (0.5, 1): ex = 1, e = 1, b = 0
    (1.0, 1 << 24, (37, 1, 34)),            # b = bit_length(2^24 - 1) = 24
    (0.0, 7, (59, 0, 57)),                  # ex = 0 by definition, b = bit_length(6) = 3
    (0.999, 2, (61, 0, 59)),                # frexp(0.999) = (0.999, 0): every |x| < 1
    (2.0 ** -100, 5, (108, -49, 155)),      # a tiny maximum: ex = -99, e = ceil(-99 / 2) = -49, b = 3
    (2.0 ** 127, 1000, (-12, 64, -78)),     # a huge one: ex = 128, e = 64, b = 10
    (900.0 * 900.0, 1037, (41, 10, 29)),    # 810000 < 2^20: ex = 20, e = 10, b = 11
])
def test_kmeans_shift_by_hand(max_norm2, n, want):
    s, e, t = fi.kmeans_shift(max_norm2, n)
    assert (s, e, t) == want
    assert t == s - e - 2
    assert max(n, 1) * 2 ** (s + e) <= 2 ** 62            # no sum of n values below 2^(s + e) reaches 2^63
    assert math.sqrt(float(np.float32(max_norm2))) < 2.0 ** e   # every |x| < 2^e


def test_fixed_point_sums_rounds_to_even_and_skips_unassigned_rows():
    X = np.array([[0.5, -0.25], [1.5, 0.75], [2.5, 1.0], [8.0, 8.0], [-0.5, 0.25]], np.float32)
    sums, counts = fi.fixed_point_sums(X, [1, 1, 1, -1, 0], 3, 0)
    # llrint: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2 (ties to even); -0.25 -> 0, 0.75 -> 1
    assert sums.tolist() == [[0, 0], [4, 2], [0, 0]] and counts.tolist() == [1, 3, 0]
    assert sums.dtype == np.int64 and counts.dtype == np.int64
    sums, counts = fi.fixed_point_sums(X, [1, 1, 1, -1, 0], 3, 3)
    assert sums.tolist() == [[-4, 2], [36, 12], [0, 0]]
    # a large shift stays exact: 0.5 * 2^61 three times
    sums, _ = fi.fixed_point_sums(np.full((3, 1), 0.5, np.float32), [0, 0, 0], 2, 61)
    assert sums.tolist() == [[3 << 60], [0]]
    assert fi.fixed_point_objective([0.5, 1.5, 9.0], [0, 1, -1], 0) == 2
    assert fi.fixed_point_objective([0.375, 0.25], [0, 0], 3) == 5
    empty, none = fi.fixed_point_sums(np.zeros((0, 4), np.float32), [], 2, 10)
    assert empty.shape == (2, 4) and not empty.any() and none.tolist() == [0, 0]


# ----------------------------------------------------------------------------- lloyd_update
def test_lloyd_update_means_in_float64_rounded_once():
    s = 20
    X = np.array([[1.0, 0.125], [0.25, 0.5], [3.0, 1.0]], np.float32)
    sums, counts = fi.fixed_point_sums(X, [0, 0, 1], 2, s)
    new, split = fi.lloyd_update(sums, counts, s, np.zeros((2, 2), np.float32))
    assert split == []
    assert new.dtype == np.float32
    assert new.tolist() == [[0.625, 0.3125], [3.0, 1.0]]
    # a third of something: the float64 quotient rounded to float32 once
    sums, counts = fi.fixed_point_sums(np.array([[1.0], [0.0], [0.0], [5.0]], np.float32), [0, 0, 0, 1], 2, s)
    new, _ = fi.lloyd_update(sums, counts, s, np.array([[9.0], [7.0]], np.float32))
    assert new[0, 0] == np.float32(1.0 / 3.0) and new[1, 0] == 5.0


def test_lloyd_update_refills_one_empty_cluster_from_the_largest():
    prev = np.array([[9.0, 9.0], [5.0, 5.0], [7.0, 7.0]], np.float32)
    sums = np.array([[8, 16], [0, 0], [24, 48]], np.int64) << 10
    new, split = fi.lloyd_update(sums, np.array([2, 0, 3], np.int64), 10, prev)
    assert split == [(1, 2)]
    up, down = np.float32(1.0 + 1.0 / 1024.0), np.float32(1.0 - 1.0 / 1024.0)
    donor = np.array([8.0, 16.0], np.float32)
    assert new[0].tolist() == [4.0, 8.0]
    assert np.array_equal(new[1], donor * up) and np.array_equal(new[2], donor * down)


def test_lloyd_update_two_empties_and_a_tie_for_the_donor():
    # counts 4, 0, 4, 0: empty 1 takes from 0 (tie to the lowest index), which leaves 2 | 2 | 4 | 0, so empty 3 takes from 2
    prev = np.zeros((4, 1), np.float32)
    sums = np.array([[4], [0], [8], [0]], np.int64) << 5
    new, split = fi.lloyd_update(sums, np.array([4, 0, 4, 0], np.int64), 5, prev)
    assert split == [(1, 0), (3, 2)]
    up, down = np.float32(1.0 + 1.0 / 1024.0), np.float32(1.0 - 1.0 / 1024.0)
    assert new[:, 0].tolist() == [np.float32(1.0) * down, np.float32(1.0) * up, np.float32(2.0) * down, np.float32(2.0) * up]
    # counts 5, 0, 0: the first empty halves the donor to 3 | 2, the second takes from cluster 0 again (3 > 2)
    _, split = fi.lloyd_update(np.array([[5], [0], [0]], np.int64), np.array([5, 0, 0], np.int64), 0, np.zeros((3, 1), np.float32))
    assert split == [(1, 0), (2, 0)]
    # nothing anywhere: the previous centroids stay
    keep = np.array([[1.0], [2.0]], np.float32)
    new, split = fi.lloyd_update(np.zeros((2, 1), np.int64), np.zeros(2, np.int64), 7, keep)
    assert split == [] and np.array_equal(new, keep)


def test_lloyd_update_spherical_and_a_zero_vector():
    sums = np.array([[3, 4], [0, 0], [1, 1]], np.int64) << 8
    new, split = fi.lloyd_update(sums, np.array([2, 5, 1], np.int64), 8, np.ones((3, 2), np.float32), spherical=True)
    assert split == []
    assert np.array_equal(new[0], np.array([0.6, 0.8], np.float64).astype(np.float32))   # (1.5, 2) / 2.5 in float64
    assert new[1].tolist() == [0.0, 0.0]                                                # a zero mean stays zero
    assert np.array_equal(new[2], (np.array([1.0, 1.0]) / math.sqrt(2.0)).astype(np.float32))


def test_kmeans_init_ids_is_the_seeded_choice():
    rows = np.arange(10, 60, 2)
    ids = fi.kmeans_init_ids(rows, 7, 3)
    assert np.array_equal(ids, np.random.default_rng(3).choice(rows, 7, replace=False))
    assert len(set(ids.tolist())) == 7 and ids.dtype == np.int64
    with pytest.raises(ValueError, match="3 allowed rows for 4 centroids"):
        fi.kmeans_init_ids([1, 2, 3], 4, 0)


# ----------------------------------------------------------------------------- run_kmeans over the double
def _fake(x, metric=1):
    ix = FakeKmeansIndex(x.shape[1], metric)
    ix.add(x)
    return ix


def test_run_kmeans_recovers_planted_clusters_and_stops_at_the_fixpoint():
    x, lab, C = planted(600, 24, 4, seed=5)
    ix = _fake(x)
    res = ix.kmeans(4, niter=20, seed=1, init=C + np.float32(0.125))
    assert isinstance(res, fi.KmeansResult)
    assert np.array_equal(res.assign, lab)                       # init c sits next to centre c: the labels themselves
    assert res.sizes.tolist() == np.bincount(lab, minlength=4).tolist()
    for c in range(4):   # the centroid is the float64 mean of its members rounded once
        assert np.array_equal(res.centroids[c], x[lab == c].astype(np.float64).mean(axis=0).astype(np.float32))
    # step 1 moves the centroids to the means, step 2 finds them unchanged: two iterations, not twenty
    assert res.iterations == 2 and len(res.obj) == 2 and res.obj[1] <= res.obj[0]
    steps = [c for c in ix.calls if c[0] == "kmeans_step"]
    assert len(steps) == 3                                       # two training steps and the final one
    d64 = ((x.astype(np.float64) - res.centroids.astype(np.float64)[lab]) ** 2).sum(axis=1)
    assert np.allclose(res.dist, d64, rtol=1e-6, atol=1e-6)
    # from seeded random rows the partition is recovered up to the names of the clusters
    seed = next(sd for sd in range(64) if len(set(lab[fi.kmeans_init_ids(np.arange(600), 4, sd)].tolist())) == 4)
    res2 = ix.kmeans(4, niter=20, seed=seed)                     # (a start with one row of every cluster)
    pairs = set(zip(res2.assign.tolist(), lab.tolist()))
    assert len(pairs) == 4 and res2.iterations < 20
    assert np.array_equal(res2.centroids, ix.kmeans(4, niter=20, seed=seed).centroids)      # the same call, the same bytes


def test_run_kmeans_honours_init_niter_and_masks():
    x, lab, C = planted(300, 16, 3, seed=9)
    ix = _fake(x)
    res = ix.kmeans(3, niter=0, init=C)
    assert np.array_equal(res.centroids, C) and res.iterations == 0 and res.obj == []
    assert np.array_equal(res.assign, lab)
    allow = (np.arange(300) % 3) != 0
    res = ix.kmeans(3, niter=5, init=C, allow=allow)
    assert (res.assign[~allow] == -1).all() and (res.dist[~allow] == 0).all()
    assert np.array_equal(res.assign[allow], lab[allow]) and int(res.sizes.sum()) == int(allow.sum())
    # a training subset: the final step still assigns every allowed row
    res = ix.kmeans(3, niter=5, seed=4, init=C, max_points_per_centroid=10)
    train_calls = [c for c in ix.calls if c[0] == "kmeans_step"][-res.iterations - 1:]
    assert all(c[2] for c in train_calls[:-1]) and not train_calls[-1][2]
    assert int(res.sizes.sum()) == 300 and np.array_equal(res.assign, lab)
    with pytest.raises(ValueError, match="init must be"):
        ix.kmeans(3, init=C[:2])


def test_run_kmeans_refuses_too_few_rows_and_bad_nc():
    x, _, _ = planted(5, 8, 2, seed=1)
    ix = _fake(x)
    with pytest.raises(ValueError, match="5 allowed rows for 6 centroids"):
        ix.kmeans(6)
    with pytest.raises(ValueError, match="2 allowed rows for 3 centroids"):
        ix.kmeans(3, allow=np.array([True, False, True, False, False]))
    for nc in (1, fi.MAX_CENTROIDS + 1):
        with pytest.raises(ValueError, match="outside"):
            ix.kmeans(nc)


def test_an_empty_cluster_is_split_and_reported():
    x, lab, C = planted(200, 16, 2, seed=3)
    far = np.full((1, 16), 64.0, np.float32)                     # a third centroid nobody is near
    res = _fake(x).kmeans(3, niter=6, init=np.concatenate([C, far]))
    assert res.splits[0] == ((2, int(np.argmax(np.bincount(lab, minlength=2)))),)
    assert (res.sizes > 0).all() and int(res.sizes.sum()) == 200


@pytest.mark.parametrize("d, scale, seed", GAUSS_CASES)
def test_gaussian_cases_of_the_gpu_test_stay_far_inside_the_mismatch_cap(d, scale, seed):
    """The GPU test allows the device's assignment to differ from the float64 argmax on at most 1 % of the rows (inside
    the rounding tolerance).  A float32 restatement in numpy -- another summation order than the device's, the same
    precision -- differs on far fewer for the chosen seeds, so the cap cannot be what makes that test pass."""
    x, c = gaussian_case(d, scale, seed)
    a64, _, _ = assign64(x, c)
    key32 = x @ c.T - np.float32(0.5) * (c * c).sum(axis=1, dtype=np.float32)[None, :]
    differ = int((key32.argmax(axis=1) != a64).sum())
    assert differ <= x.shape[0] // 1000, differ          # <= 0.1 %, a tenth of the cap
    assert len(set(a64.tolist())) > c.shape[0] // 2       # and the case is no trivial one: most centroids have members


# ----------------------------------------------------------------------------- HybridStorage.topics over the double
D_ = 16


def _use(monkeypatch, cls):
    monkeypatch.setattr(fi, "IndexFlat", cls)
    monkeypatch.setattr(fi, "IndexFlatIP", lambda d, device=0: cls(d, 0, device))
    monkeypatch.setattr(fi, "IndexFlatL2", lambda d, device=0: cls(d, 1, device))


def _storage(tmp_path, n=90):
    lab = np.repeat([0, 1, 2], [n // 2, n // 3, n - n // 2 - n // 3])        # sizes 45, 30, 15
    C = planted(3, D_, 3, seed=0)[2]
    x = (C[lab] + np.random.default_rng(21).integers(-1, 2, size=(n, D_)) / 8.0).astype(np.float32)
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=D_, normalize_embeddings=False,
                                    auto_save=False))
    s.initialize()
    s.add_chunks([Chunk(f"c{i}", f"text {i}", {"project_name": "alpha" if i % 2 else "beta", "session_id": f"s{lab[i]}"}, x[i])
                  for i in range(n)])
    return s, lab


def _good_seed(rows, lab, nc):
    """The first seed whose initial rows (``kmeans_init_ids``) come from ``nc`` different planted clusters: Lloyd's
    steps recover a planted partition from such a start, and from no other with certainty."""
    return next(sd for sd in range(64) if len(set(lab[fi.kmeans_init_ids(rows, nc, sd)].tolist())) == nc)


def test_topics_sizes_order_tombstones_and_filters(tmp_path, monkeypatch):
    _use(monkeypatch, FakeKmeansIndex)
    s, lab = _storage(tmp_path)
    topics = s.topics(n_topics=3, seed=_good_seed(np.arange(90), lab, 3), examples=2)
    assert all(isinstance(t, Topic) for t in topics)
    assert [t.size for t in topics] == [45, 30, 15]              # largest first
    for t, subject in zip(topics, (0, 1, 2)):
        assert sorted(t.chunk_ids, key=lambda c: int(c[1:])) == [f"c{i}" for i in np.flatnonzero(lab == subject)]
        assert t.representative is t.examples[0] and len(t.examples) == 2
        assert all(e.chunk_id in t.chunk_ids for e in t.examples)
        assert t.examples[0].similarity <= t.examples[1].similarity          # an L2 storage: nearest first
    # a deleted chunk is in no topic, and the sizes sum to the live chunks
    assert s.delete_chunk("c0") and s.delete_chunk("c89")
    topics = s.topics(n_topics=3, seed=_good_seed(np.arange(1, 89), lab, 3))
    assert [t.size for t in topics] == [44, 30, 14] and sum(t.size for t in topics) == 88
    assert not any("c0" in t.chunk_ids or "c89" in t.chunk_ids for t in topics)
    # a project filter: only those chunks are clustered
    topics = s.topics(n_topics=3, filters={"project_name": "alpha"}, seed=_good_seed(np.arange(1, 89, 2), lab, 3))
    assert sorted(t.size for t in topics) == sorted(np.bincount(lab[1:89:2]).tolist())
    members = sorted((c for t in topics for c in t.chunk_ids), key=lambda c: int(c[1:]))
    assert members == [f"c{i}" for i in range(1, 89, 2)]
    assert [t.size for t in topics] == sorted((t.size for t in topics), reverse=True)
    # more topics than chunks: cut to the chunks that are there
    topics = s.topics(n_topics=50, filters={"session_id": "s2", "project_name": "beta"})
    assert sum(t.size for t in topics) == len([i for i in range(1, 89) if lab[i] == 2 and i % 2 == 0])
    with pytest.raises(ValueError):
        s.topics(n_topics=0)
    s.close()


def test_topics_on_an_empty_index_and_on_an_index_without_kmeans(tmp_path, monkeypatch):
    _use(monkeypatch, FakeKmeansIndex)
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "e"), embedding_dim=D_, normalize_embeddings=False, auto_save=False))
    s.initialize()
    assert s.topics() == []
    s.close()
    _use(monkeypatch, FakeIndex)
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "f"), embedding_dim=D_, normalize_embeddings=False, auto_save=False))
    s.initialize()
    s.add_chunks([Chunk("a", "t", {}, np.ones(D_, np.float32)), Chunk("b", "t", {}, -np.ones(D_, np.float32))])
    with pytest.raises(NotImplementedError, match="kmeans"):
        s.topics(2)
    s.close()

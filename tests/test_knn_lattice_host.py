"""CPU side of the lattice tests: the truth of tests/lattice_cases.py is checked against the CPU oracle (so it is not
its own reference), and the lattice cases are shown to HAVE the ties that test_knn_lattice_gpu.py relies on (a lattice
test without ties would pass vacuously).  Runs anywhere."""
import numpy as np
import pytest

import lattice_cases as lc
from oracle import knn_oracle as ko


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("family,n,d", [("T", 3000, 200), ("T", 1200, 64), ("E", 2000, 96)])
def test_truth_equals_the_oracle_on_lattice_rows(family, n, d, metric):
    x, q = lc.case(family, n, d)
    q = q[:6]
    ref = ko.FlatIndexOracle(d, metric)
    ref.add(x)
    for k in (1, 10, 129, 300):
        Dt, It = lc.truth_topk(x, q, k, metric)
        Dr, Ir = ref.search(q, k)
        lc.assert_exact(Dt, It, Dr, Ir, f"{family} n={n} d={d} metric={metric} k={k}")
    # masks by sub-indexing; the sparse one allows fewer rows than k, the third only part of the block of copies
    zero, src, blk = lc.planted(n)
    rng = np.random.default_rng(5)
    dense = rng.random(n) < 0.3
    sparse = np.zeros(n, dtype=bool)
    sparse[rng.choice(n, 7, replace=False)] = True
    part = np.ones(n, dtype=bool)
    part[blk + 3:blk + lc.COPIES:2] = False
    for name, allow in (("dense", dense), ("sparse", sparse), ("part", part)):
        sub = ko.FlatIndexOracle(d, metric)
        sub.add(x[allow])
        back = np.flatnonzero(allow)
        for k in (10, 300):
            kk = min(k, back.size)
            Dr, Ir = sub.search(q, kk)
            Dt, It = lc.truth_topk(x, q, k, metric, allow=allow)
            lc.assert_exact(Dt[:, :kk], It[:, :kk], Dr, back[Ir], f"{name} mask, metric={metric} k={k}")
            assert (It[:, kk:] == -1).all() and (Dt[:, kk:] == (-lc.FLT_MAX if metric == 0 else lc.FLT_MAX)).all()
    # exclude: the anchor's own row is left out, its copies stay
    anchors = np.array([blk + 5, zero, 17, src, -1, 0])
    Dt, It = lc.truth_topk(x, x[np.maximum(anchors, 0)], 50, metric, exclude=anchors)
    for j, a in enumerate(anchors):
        keep = np.ones(n, dtype=bool)
        if a >= 0:
            keep[a] = False
        sub = ko.FlatIndexOracle(d, metric)
        sub.add(x[keep])
        Dr, Ir = sub.search(x[max(a, 0)][None, :], 50)
        lc.assert_exact(Dt[j:j + 1], It[j:j + 1], Dr, np.flatnonzero(keep)[Ir], f"exclude anchor {a} metric={metric}")
        assert a not in It[j]


@pytest.mark.parametrize("metric", [0, 1])
def test_truth_of_shards_merges_to_the_truth_of_the_whole(metric):
    x, q = lc.case("T", 3000, 200)
    q = q[:5]
    bounds = [0, 90, 1500, 3000]
    for k in (10, 128, 129, 700):
        parts = [lc.truth_topk(x[lo:hi], q, k, metric) for lo, hi in zip(bounds[:-1], bounds[1:])]
        Dp = np.stack([p[0] for p in parts])
        Ip = np.stack([np.where(p[1] >= 0, p[1] + lo, -1) for p, lo in zip(parts, bounds[:-1])])
        Dm, Im = ko.merge_topk(Dp, Ip, metric)
        Dt, It = lc.truth_topk(x, q, k, metric)
        lc.assert_exact(Dm, Im, Dt, It, f"merge of shard truths, metric={metric} k={k}")


def test_truth_range_is_strict_and_ordered():
    x, q = lc.case("T", 1200, 64)
    q = q[:3]
    for metric in (0, 1):
        S = lc.scores64(x, q, metric)
        D10, _ = lc.truth_topk(x, q, 10, metric)
        r = float(D10[0, 9])                                # an attained score: rows exactly there are no hits
        lims, D, I = lc.truth_range(x, q, r, metric)
        for j in range(3):
            seg = slice(lims[j], lims[j + 1])
            want = np.flatnonzero(S[j] > r if metric == 0 else S[j] < r)
            assert sorted(I[seg].tolist()) == want.tolist() and not (D[seg] == np.float32(r)).any()
            Dk, Ik = lc.truth_topk(x, q[j:j + 1], max(want.size, 1), metric)
            assert np.array_equal(I[seg], Ik[0, :want.size]) and np.array_equal(D[seg], Dk[0, :want.size])
        assert (S[0] == r).sum() >= 1 and lims[1] < 10


def test_assert_exact_reports_and_catches():
    D = np.array([[3.0, 2.0, 2.0]], np.float32)
    I = np.array([[4, 1, 7]], np.int64)
    lc.assert_exact(D, I, D.copy(), I.copy())
    with pytest.raises(AssertionError, match=r"first at \(0, 1\).*id 7.*id 1"):
        lc.assert_exact(D, np.array([[4, 7, 1]], np.int64), D, I, "swap")
    with pytest.raises(AssertionError, match="repeats an id"):
        lc.assert_exact(D, np.array([[4, 1, 1]], np.int64), D, np.array([[4, 1, 1]], np.int64), "dup")
    with pytest.raises(AssertionError, match="shapes"):
        lc.assert_exact(D[:, :2], I[:, :2], D, I)
    with pytest.raises(AssertionError):
        lc.assert_exact(np.nextafter(D, np.float32(9)), I, D, I)


def test_topk_checker_refuses_repeated_ids():
    from knn_checks import assert_topk_matches

    Dr = np.array([[0.9, 0.5, 0.5 - 1e-8, 0.1]], np.float32)
    Ir = np.array([[3, 8, 5, 2]], np.int64)
    D64 = Dr.astype(np.float64)
    assert_topk_matches(Dr, np.array([[3, 5, 8, 2]], np.int64), Dr, Ir, D64)       # a swap inside a near tie is fine
    with pytest.raises(AssertionError, match="repeats an id"):
        assert_topk_matches(Dr, np.array([[3, 8, 8, 2]], np.int64), Dr, Ir, D64)   # a repeated id is not


# ---- construction conditions: the ties are there --------------------------------------------------------------------
# Measured with the seeds of lattice_cases.case on the first 32 queries (share of the queries whose true scores at
# ranks k and k + 1 are equal); every assert asks for at least HALF of what was measured.
#   T 20000 x 768, IP:  k=10 0.62 | k=32 0.78 | k=100 0.88 | k=128 0.94 | k=300: 0.94 at rank 128, 0.94 at 256, 1.0 at 300
#                       groups of equal scores inside the list: 2.1 (k=10) .. 22.4 (k=300); k=1: 0.0 (not asserted)
#   T 20000 x 768, L2:  k=10 0.31 | k=32 0.59 | k=100 0.88 | k=128 0.88 | k=300: 0.88 / 0.91 / 0.97; groups 1.2 .. 36.9
#   T 6000 x 200, IP:   k=10 0.72 | k=128 0.97 | k=2048: 0.97 at rank 128, 1.0 at 256, 1.0 at 2048
#   T 6000 x 200, L2:   k=10 0.56 | k=128 0.94 | k=2048: 0.94 / 0.91 / 1.0
#   T 4000 x 64:        IP k=10 0.94, k=128 0.97; L2 k=10 0.59, k=128 1.0
#   E 20000 x 768:      IP k=10 0.06, k=128 0.19 (groups 14.2); L2 k=128 0.12 -- E is for the band, not for ties
MEASURED = [
    ("T", 20000, 768, 0, {10: 0.62, 32: 0.78, 100: 0.88, 128: 0.94, 300: (1.0, 0.94, 0.94)}),
    ("T", 20000, 768, 1, {10: 0.31, 32: 0.59, 100: 0.88, 128: 0.88, 300: (0.97, 0.88, 0.91)}),
    ("T", 6000, 200, 0, {10: 0.72, 128: 0.97, 2048: (1.0, 0.97, 1.0)}),
    ("T", 6000, 200, 1, {10: 0.56, 128: 0.94, 2048: (1.0, 0.94, 0.91)}),
    ("T", 4000, 64, 0, {10: 0.94, 128: 0.97}),
    ("T", 4000, 64, 1, {10: 0.59, 128: 1.0}),
    ("E", 20000, 768, 0, {128: 0.19}),
]


@pytest.mark.parametrize("family,n,d,metric,shares", MEASURED, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_lattice_cases_have_ties_across_rank_k_and_across_the_pass_boundaries(family, n, d, metric, shares):
    x, q = lc.case(family, n, d)
    prof = lc.tie_profile(x, q[:32], sorted(shares), metric)
    print(f"{family} {n}x{d} metric={metric}: {prof}")
    for k, want in shares.items():
        p = prof[k]
        if isinstance(want, tuple):
            assert p["at_k"] >= want[0] / 2 and p["at_128"] >= want[1] / 2 and p["at_256"] >= want[2] / 2, (k, p)
        else:
            assert p["at_k"] >= want / 2, (k, p)
        if family == "T" and k >= 10:
            assert p["groups"] >= 1.0, (k, p)


def test_planted_rows_are_where_the_gpu_tests_expect_them():
    x, _ = lc.case("T", 4000, 64)
    zero, src, blk = lc.planted(4000)
    assert not x[zero].any() and (x[blk:blk + lc.COPIES] == x[src]).all() and blk - src > 2000
    assert set(np.unique(x).tolist()) == {-1.0, 0.0, 1.0}
    e, _ = lc.case("E", 2000, 96)
    assert np.array_equal(e * 8, np.rint(e * 8)) and np.abs(e).max() == 1.0

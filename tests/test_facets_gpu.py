"""GPU: ``IndexFlat.facets`` (``css_index_facets``, kernel ``k_facet_small``).

Truth is computed here in fp64 with numpy from the very fp32 rows and queries handed to the index
(``oracle.knn_oracle.synth_rows`` + ``normalize_rows``); the code under test is never its own reference.

Band rule (that of ``test_range_search_gpu.py``, restated).  The kernel forms every score as a recursive fp32 sum of
``dpad`` fused multiply-adds.  For a recursive sum of n terms ``|fl(sum) - sum| <= n u sum|t_i|`` with ``u = 2^-24``
(Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5 to first order; an fma rounds each step once), and
``sum |x_i q_i| <= ||x|| ||q||`` (Cauchy-Schwarz), so

    band_IP = dpad * 2^-24 * ||x|| * ||q||                       (4.6e-5 for unit rows of 768)

For L2 every difference ``x_i - q_i`` carries one rounding (relative u, 2u after squaring), the sum adds n u:
``(n + 2) u sum (x_i - q_i)^2 <= (n + 2) u (||x|| + ||q||)^2 <= 4 (n + 2) u max(||x||^2, ||q||^2)``.  The kernel's chains
are dpad / 16 + 4 additions deep, not dpad, which covers the ``+ 2`` many times over:

    band_L2 = 4 * dpad * 2^-24 * max(||x||^2, ||q||^2)           (1.8e-4 for unit rows of 768)

A row whose fp64 score lies strictly outside ``radius +- band`` is surely inside or surely outside; a row inside the
band may go either way.  For every query ``j`` and bucket ``b``: ``#{rows surely inside} <= count <= #{rows possibly
inside}`` (likewise ``total`` and ``unbucketed``, and ``total == counts.sum() + unbucketed`` exactly); ``best_id`` is an
allowed row of bucket ``b`` that is possibly inside; ``best_score`` is within the band of that row's fp64 score,
satisfies the strict predicate against the float32 radius, and is not worse than ``max (score - band)`` over the
bucket's surely-inside rows (the kernel's fp32 value of each of them is at least that, and the best is their
maximum; L2 mirrored); an empty bucket has count 0, id -1 and the pad score of ``search``.  So that the band cannot
hide a failure, every case asserts on the fp64 side that the rows inside the band are at most 5 % of the fp64 hits of
the query (at most 5 where it has fewer than 100 hits).

The exactly representable case needs no band: components in ``{-1, 0, 1} / 8`` at d = 64 make every fp32 score the exact
value, and everything must EQUAL the fp64 truth, ties to the smallest id, rows at the radius not hits.

The grid metric x dim x nq x radius x nbuckets is not pruned; one index, one fp64 score matrix and one set of expected
bounds per (metric, dim) serve every nq (the queries of a smaller batch are a prefix of the 40).
"""
import numpy as np
import pytest

from oracle import knn_oracle as ko

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FMAX = float(np.finfo(np.float32).max)
POLICIES = {"off": False, "bf16": True, "int8": "int8", "auto": None}
LDS_BYTES, ENTRY_BYTES = 160 * 1024, 12


def lds_limit(d, nq_slots):
    """the largest table (entries of 12 bytes) that goes to LDS beside ``nq_slots`` query rows -- one
    block per CU must fit for 1 or 2 query slots, two blocks for 8 or 16."""
    qbytes = nq_slots * ((d + 63) // 64 * 64) * 4
    return (LDS_BYTES // (1 if nq_slots <= 2 else 2) - qbytes) // ENTRY_BYTES


def _rows(n, d, seed):
    return ko.normalize_rows(ko.synth_rows(n, d, seed))


def _queries(x, nq, seed):
    """Half random unit vectors, half noisy copies of rows (unit again): the second kind has a near neighbour."""
    n, d = x.shape
    q = _rows(nq, d, seed)
    rng = np.random.default_rng(seed)
    for j in range(1, nq, 2):
        v = x[rng.integers(0, n)] + (0.5 / np.sqrt(d)) * rng.standard_normal(d).astype(np.float32)
        q[j] = ko.normalize_rows(v)[0]
    return np.ascontiguousarray(q, np.float32)


def _truth(x, q, metric):
    """fp64 scores [nq, n] and the band [nq, n] of the module docstring."""
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    dpad = (x.shape[1] + 63) // 64 * 64
    xn2, qn2 = (x64 * x64).sum(1), (q64 * q64).sum(1)
    dot = q64 @ x64.T
    if metric == 0:
        return dot, dpad * U * np.sqrt(qn2)[:, None] * np.sqrt(xn2)[None, :]
    return np.maximum(qn2[:, None] + xn2[None, :] - 2.0 * dot, 0.0), 4 * dpad * U * np.maximum(qn2[:, None], xn2[None, :])


def _labels(n, nb, seed):
    """Skewed bucket labels (cubed uniform: the low buckets are the big ones), 3 % negative, 2 % >= nb."""
    rng = np.random.default_rng(seed)
    lab = np.minimum((nb * rng.random(n) ** 3).astype(np.int64), nb - 1)
    kind = rng.random(n)
    lab = np.where(kind < 0.03, -1 - rng.integers(0, 1000, n), lab)
    lab = np.where(kind > 0.98, nb + rng.integers(0, 1000, n), lab)
    lab[rng.integers(0, n)] = np.iinfo(np.int32).max
    lab[rng.integers(0, n)] = np.iinfo(np.int32).min
    return lab.astype(np.int32)


def _index(d, metric, x=None, policy="auto"):
    from claude_semantic_search_amd.flat_index import IndexFlat

    ix = IndexFlat(d, metric)
    ix.set_shadow(POLICIES[policy])
    if x is not None and x.shape[0]:
        ix.add(x)
    return ix


def _radius(metric, d, kind):
    ip = 0.12 * np.sqrt(768.0 / d) if kind == "narrow" else 0.0
    return ip if metric == 0 else 2.0 - 2.0 * ip


def _sides(S, band, radius, metric, ok=None):
    """(sure, maybe, fp64 hit) [nq, n] of a radius as the float32 the index is given."""
    r = float(np.float32(radius))
    if metric == 0:
        sure, maybe, hit = S > r + band, S >= r - band, S > r
    else:
        sure, maybe, hit = S < r - band, S <= r + band, S < r
    if ok is not None:
        sure, maybe, hit = sure & ok, maybe & ok, hit & ok
    return sure, maybe, hit


def _assert_cap(sure, maybe, hit, what):
    hits, in_band = hit.sum(1), (maybe & ~sure).sum(1)
    print(f"{what}: fp64 hits per query {hits.min()}-{hits.max()}, worst in-band rows per query {in_band.max()}")
    cap = np.where(hits < 100, 5, 0.05 * hits)
    assert (in_band <= cap).all(), f"{what}: rows inside the band {in_band.tolist()} against hits {hits.tolist()}"


def _expect(S, band, sure, maybe, metric, lab, nb):
    """The bounds of the module docstring for every query: dict of [nq, nb] / [nq] arrays."""
    nq = S.shape[0]
    inb = (lab >= 0) & (lab < nb)
    lb = np.where(inb, lab, 0)
    e = {k: np.zeros((nq, nb), np.int64) for k in ("lo", "hi")}
    e["edge"] = np.full((nq, nb), -np.inf if metric == 0 else np.inf)
    for j in range(nq):
        s, m = sure[j] & inb, maybe[j] & inb
        e["lo"][j] = np.bincount(lb[s], minlength=nb)
        e["hi"][j] = np.bincount(lb[m], minlength=nb)
        if metric == 0:
            np.maximum.at(e["edge"][j], lb[s], (S[j] - band[j])[s])
        else:
            np.minimum.at(e["edge"][j], lb[s], (S[j] + band[j])[s])
    e["tot"] = (sure.sum(1), maybe.sum(1))
    e["unb"] = ((sure & ~inb).sum(1), (maybe & ~inb).sum(1))
    return e


def _check(res, e, S, band, maybe, radius, metric, lab, nb, what, id_base=0):
    nq = res.counts.shape[0]
    n = S.shape[1]
    assert res.counts.dtype == np.int64 and res.best_id.dtype == np.int64 and res.best_score.dtype == np.float32, what
    assert res.total.dtype == np.int64 and res.unbucketed.dtype == np.int64, what
    assert res.counts.shape == res.best_score.shape == res.best_id.shape == (nq, nb), what
    assert res.total.shape == res.unbucketed.shape == (nq,), what
    c = res.counts
    assert (c >= e["lo"][:nq]).all(), f"{what}: a count is below the rows surely inside"
    assert (c <= e["hi"][:nq]).all(), f"{what}: a count exceeds the rows possibly inside"
    assert (res.total >= e["tot"][0][:nq]).all() and (res.total <= e["tot"][1][:nq]).all(), f"{what}: total"
    assert (res.unbucketed >= e["unb"][0][:nq]).all() and (res.unbucketed <= e["unb"][1][:nq]).all(), f"{what}: unbucketed"
    assert np.array_equal(res.total, c.sum(1) + res.unbucketed), f"{what}: total != sum of counts + unbucketed"
    empty = c == 0
    assert (res.best_id[empty] == -1).all(), f"{what}: an empty bucket has a best id"
    assert (res.best_score[empty] == np.float32(-FMAX if metric == 0 else FMAX)).all(), f"{what}: pad score"
    jj, bb = np.nonzero(~empty)
    ids = res.best_id[jj, bb] - id_base
    sc = res.best_score[jj, bb]
    assert ((ids >= 0) & (ids < n)).all(), f"{what}: best ids outside [0, n)"
    assert (lab[ids] == bb).all(), f"{what}: a best row is not of its bucket"
    assert maybe[jj, ids].all(), f"{what}: a best row is clearly outside the radius (or masked)"
    err = np.abs(sc.astype(np.float64) - S[jj, ids])
    assert (err <= band[jj, ids]).all(), f"{what}: best score error {err.max():.3e} beyond the band"
    if metric == 0:
        assert (sc > np.float32(radius)).all(), f"{what}: a best score does not exceed the radius"
        assert (sc.astype(np.float64) >= e["edge"][jj, bb]).all(), f"{what}: a best score is worse than a sure row's"
    else:
        assert ((sc < np.float32(radius)) & (sc >= 0)).all(), f"{what}: a best distance is not inside the radius"
        assert (sc.astype(np.float64) <= e["edge"][jj, bb]).all(), f"{what}: a best distance is worse than a sure row's"


def _same(a, b, what):
    for u, v, name in zip(a, b, a._fields):
        assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u.view(np.uint8), v.view(np.uint8)), \
            f"{what}: {name} differs"


N, NQ_ALL = 100000, 40


_CASES = {}


def _case(metric, d):
    """One index, its rows, 40 queries and the fp64 truth per (metric, dim), shared by the tests below (read only)."""
    if (metric, d) not in _CASES:
        x = _rows(N, d, 11)
        q = _queries(x, NQ_ALL, 12)
        S, band = _truth(x, q, metric)
        for a in (x, q, S, band):
            a.setflags(write=False)
        _CASES[metric, d] = (x, q, S, band, _index(d, metric, x))
    return _CASES[metric, d]


@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_cases():
    yield
    for case in _CASES.values():
        case[4].close()
    _CASES.clear()


# ------------------------------------------------------------------ the grid
@pytest.mark.parametrize("d", [64, 100, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_every_metric_dim_query_count_radius_and_bucket_count(metric, d):
    x, q, S, band, ix = _case(metric, d)
    for kind in ("narrow", "broad"):
        radius = _radius(metric, d, kind)
        sure, maybe, hit = _sides(S, band, radius, metric)
        _assert_cap(sure, maybe, hit, f"metric={metric} d={d} {kind}")
        assert hit.any(1).all()
        for nb in (1, 7, 4096):
            lab = _labels(N, nb, 100 + nb)
            e = _expect(S, band, sure, maybe, metric, lab, nb)
            for nq in (1, 2, 3, 16, 17, 40):
                what = f"metric={metric} d={d} {kind} nb={nb} nq={nq}"
                res = ix.facets(q[:nq], radius, buckets=lab, nbuckets=nb)
                _check(res, e, S, band, maybe, radius, metric, lab, nb, what)
                sweeps, lds = ix.last_facet_sweeps()
                assert sweeps == (nq + 15) // 16 and 0 <= lds <= sweeps, what


# ------------------------------------------------------------------ exactly representable scores: no band at all
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
@pytest.mark.parametrize("metric", [0, 1])
def test_exactly_representable_scores_equal_the_fp64_truth(metric, n):
    d, nq, nb = 64, 3, 5
    rng = np.random.default_rng(1000 + n)
    x = (rng.integers(-1, 2, (n, d)) / 8.0).astype(np.float32)
    q = (rng.integers(-1, 2, (nq, d)) / 8.0).astype(np.float32)
    lab = rng.integers(-1, nb + 1, n).astype(np.int32)           # -1 and nb: unbucketed
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    S = q64 @ x64.T if metric == 0 else ((q64[:, None, :] - x64[None, :, :]) ** 2).sum(2)   # multiples of 1/64: exact
    assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
    ix = _index(d, metric, x)
    inb = (lab >= 0) & (lab < nb)
    at_radius = 0
    levels = sorted(set(np.round(S.ravel() * 64).astype(int).tolist()))
    for radius in levels[:: max(1, len(levels) // 6)]:
        r = radius / 64.0                                        # a score some rows have EXACTLY
        hit = S > r if metric == 0 else S < r
        at_radius += int((S == r).sum())
        res = ix.facets(q, r, buckets=lab, nbuckets=nb)
        for j in range(nq):
            assert res.total[j] == hit[j].sum() and res.unbucketed[j] == (hit[j] & ~inb).sum()
            for b in range(nb):
                rows = np.flatnonzero(hit[j] & (lab == b))
                assert res.counts[j, b] == rows.size, f"metric={metric} n={n} r={r} ({j}, {b})"
                if rows.size:
                    best = S[j, rows].max() if metric == 0 else S[j, rows].min()
                    assert float(res.best_score[j, b]) == best
                    assert res.best_id[j, b] == rows[S[j, rows] == best][0]   # the smallest id of the tie
                else:
                    assert res.best_id[j, b] == -1 and abs(float(res.best_score[j, b])) == FMAX
    assert at_radius > 0
    ix.close()


# ------------------------------------------------------------------ equality with range_search
@pytest.mark.parametrize("d", [768, 100])
@pytest.mark.parametrize("metric", [0, 1])
def test_equals_range_search_on_the_same_index_and_radius(metric, d):
    x, q, S, band, ix = _case(metric, d)
    for kind, nq, nb in (("narrow", 17, 7), ("narrow", 17, 4096), ("broad", 3, 7), ("broad", 3, 4096)):
        radius = _radius(metric, d, kind)
        lab = _labels(N, nb, 100 + nb)
        res = ix.facets(q[:nq], radius, buckets=lab, nbuckets=nb)
        lims, D, I = ix.range_search(q[:nq], radius)
        for j in range(nq):
            dj, ij = D[lims[j]:lims[j + 1]], I[lims[j]:lims[j + 1]]           # best first, ties by ascending id
            lj = lab[ij]
            inb = (lj >= 0) & (lj < nb)
            what = f"metric={metric} d={d} {kind} nb={nb} query {j}"
            assert res.total[j] == ij.size and res.unbucketed[j] == (~inb).sum(), what
            assert np.array_equal(res.counts[j], np.bincount(lj[inb], minlength=nb)), what
            b, first = np.unique(lj[inb], return_index=True)                   # first occurrence = the bucket's best
            assert np.array_equal(res.best_id[j, b], ij[inb][first]), what
            assert np.array_equal(res.best_score[j, b].view(np.uint32), dj[inb][first].view(np.uint32)), what
            assert (res.best_id[j][res.counts[j] == 0] == -1).all(), what


# ------------------------------------------------------------------ both table placements
@pytest.mark.parametrize("nq", [1, 16])
@pytest.mark.parametrize("metric", [0, 1])
def test_bucket_counts_at_and_past_the_lds_limit(metric, nq):
    n, d = 20000, 768
    x = _rows(n, d, 21)
    q = _queries(x, 16, 22)[:nq]
    S, band = _truth(x, q, metric)
    radius = _radius(metric, d, "broad")
    sure, maybe, hit = _sides(S, band, radius, metric)
    ix = _index(d, metric, x)
    at = lds_limit(d, nq) // nq
    assert at >= 1
    for nb, lds in ((at, 1), (at + 1, 0)):
        lab = _labels(n, nb, 300 + nb)
        e = _expect(S, band, sure, maybe, metric, lab, nb)
        res = ix.facets(q, radius, buckets=lab, nbuckets=nb)
        assert ix.last_facet_sweeps() == (1, lds), f"nq={nq} nb={nb}"
        _check(res, e, S, band, maybe, radius, metric, lab, nb, f"metric={metric} nq={nq} nb={nb} lds={lds}")
        ix.set_facet_lds_entries(0 if lds else 1 << 20)          # the other placement: the same bytes
        other = ix.facets(q, radius, buckets=lab, nbuckets=nb)
        if nq * ((d + 63) // 64 * 64) * 4 + nq * nb * ENTRY_BYTES <= LDS_BYTES:
            assert ix.last_facet_sweeps() == (1, 1 - lds)
        ix.set_facet_lds_entries(-1)
        _same(other, res, f"metric={metric} nq={nq} nb={nb}: LDS table against global table")
    ix.close()


@pytest.mark.parametrize("nb", [1, 2])
def test_everything_hits_counts_are_the_bucket_sizes_on_each_placement(nb):
    n, d, nq = 30001, 100, 16
    x = _rows(n, d, 23)
    q = _queries(x, nq, 24)
    lab = (np.arange(n) % 3 != 0).astype(np.int32) if nb == 2 else np.zeros(n, np.int32)
    ix = _index(d, 0, x)
    S, _ = _truth(x, q, 0)
    first = None
    for entries, lds in ((-1, 1), (0, 0)):
        ix.set_facet_lds_entries(entries)
        res = ix.facets(q, float("-inf"), buckets=lab, nbuckets=nb)
        assert ix.last_facet_sweeps() == (1, lds)
        assert (res.counts == np.bincount(lab, minlength=nb)[None, :]).all()
        assert (res.total == n).all() and (res.unbucketed == 0).all()
        for b in range(nb):                                       # the best row of a bucket is fp64's, up to the band
            best64 = np.where(lab == b, S, -np.inf).max(1)
            assert (np.abs(res.best_score[:, b] - best64) <= 128 * U * 1.01).all()
        first = first or res
        _same(res, first, f"nb={nb} entries={entries}")
    ix.close()


def test_a_million_buckets_take_one_query_per_sweep():
    from claude_semantic_search_amd.flat_index import MAX_FACET_BUCKETS

    n, d, nq, nb = 5000, 64, 2, 1 << 20
    assert nb == MAX_FACET_BUCKETS
    x = _rows(n, d, 25)
    q = _queries(x, nq, 26)
    rng = np.random.default_rng(27)
    lab = rng.integers(0, nb, n).astype(np.int32)
    lab[:50] = nb - 1
    lab[50:60] = -1
    S, band = _truth(x, q, 0)
    radius = _radius(0, d, "broad")
    sure, maybe, hit = _sides(S, band, radius, 0)
    ix = _index(d, 0, x)
    res = ix.facets(q, radius, buckets=lab, nbuckets=nb)
    assert ix.last_facet_sweeps() == (2, 0)
    _check(res, _expect(S, band, sure, maybe, 0, lab, nb), S, band, maybe, radius, 0, lab, nb, "2^20 buckets")
    ix.close()


@pytest.mark.parametrize("nb,sweeps", [(4096, 3), (1 << 17, 5)])
def test_sweep_count_follows_the_formula(nb, sweeps):
    n, d, nq = 3000, 64, 40
    assert sweeps == -(-nq // min(16, max(1, (1 << 20) // nb)))
    x = _rows(n, d, 28)
    q = _queries(x, nq, 29)
    lab = (np.arange(n) * 7919 % nb).astype(np.int32)
    ix = _index(d, 0, x)
    res = ix.facets(q, float("-inf"), buckets=lab, nbuckets=nb)
    assert ix.last_facet_sweeps()[0] == sweeps
    assert (res.total == n).all() and (res.counts.sum(1) == n).all()
    assert np.array_equal(res.counts[0], np.bincount(lab, minlength=nb)) and np.array_equal(res.counts[39], res.counts[0])
    ix.close()


# ------------------------------------------------------------------ one shape each
@pytest.mark.parametrize("metric", [0, 1])
def test_allow_masks_and_id_base(metric):
    n, d, nq, nb = 60001, 100, 9, 13
    x = _rows(n, d, 5)
    q = _queries(x, nq, 51)
    S, band = _truth(x, q, metric)
    radius = 0.08 * np.sqrt(768.0 / d)                           # (a few hundred hits: wider than "narrow")
    radius = radius if metric == 0 else 2.0 - 2.0 * radius
    lab = _labels(n, nb, 52)
    ix = _index(d, metric, x)
    half = np.random.default_rng(6).random(n) < 0.5
    sure, maybe, hit = _sides(S, band, radius, metric, ok=half)
    _assert_cap(sure, maybe, hit, f"random 50 % mask metric={metric}")
    res = ix.facets(q, radius, buckets=lab, nbuckets=nb, allow=half)
    _check(res, _expect(S, band, sure, maybe, metric, lab, nb), S, band, maybe, radius, metric, lab, nb, "50 % mask")
    assert res.total.sum() > 100
    none = ix.facets(q, radius, buckets=lab, nbuckets=nb, allow=np.zeros(n, bool))
    assert not none.counts.any() and not none.total.any() and not none.unbucketed.any() and (none.best_id == -1).all()
    ix.set_id_base(10 ** 9)
    based = ix.facets(q, radius, buckets=lab, nbuckets=nb, allow=half)
    assert np.array_equal(based.counts, res.counts) and np.array_equal(based.best_score, res.best_score)
    assert np.array_equal(based.best_id, np.where(res.best_id >= 0, res.best_id + 10 ** 9, -1))
    with pytest.raises(ValueError):
        ix.facets(q, radius, buckets=lab, nbuckets=nb, allow=np.ones(n - 1, bool))
    ix.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_stored_labels_before_set_groups_after_growth_and_after_remove_ids(metric):
    n, d, nq, nb = 40000, 768, 16, 7
    x = _rows(n, d, 8)
    q = _queries(x, nq, 81)
    radius = _radius(metric, d, "narrow")
    lab = np.maximum(_labels(n, nb, 82), -1)                     # (set_groups stores every negative label as -1)
    ix = _index(d, metric)
    ix.add(x[:7000])
    res = ix.facets(q, radius, nbuckets=nb)                      # no label was ever set: every hit is unbucketed
    assert not res.counts.any() and np.array_equal(res.total, res.unbucketed) and res.total.sum() > 0
    ix.set_groups(lab[:7000])
    for r0 in range(7000, n, 7000):                              # incremental adds: the capacity grows several times
        ix.add(x[r0:r0 + 7000])
        ix.set_groups(lab[r0:r0 + 7000], row0=r0)
    S, band = _truth(x, q, metric)
    sure, maybe, hit = _sides(S, band, radius, metric)
    res = ix.facets(q, radius, nbuckets=nb)
    _check(res, _expect(S, band, sure, maybe, metric, lab, nb), S, band, maybe, radius, metric, lab, nb, "after growth")
    _same(res, ix.facets(q, radius, buckets=lab, nbuckets=nb), "stored labels against the same column per call")
    gone = np.flatnonzero(np.random.default_rng(9).random(n) < 0.10)
    assert ix.remove_ids(gone) == gone.shape[0]
    fresh = _index(d, metric, np.delete(x, gone, 0))
    fresh.set_groups(np.delete(lab, gone))
    _same(ix.facets(q, radius, nbuckets=nb), fresh.facets(q, radius, nbuckets=nb), "after remove_ids")
    ix.close()
    fresh.close()


def test_normalize_queries_on_the_device():
    n, d, nq, nb = 30000, 768, 5, 7
    x = _rows(n, d, 14)
    raw = (ko.synth_rows(nq, d, 15) * np.float32(3.7)).astype(np.float32)
    qn = ko.normalize_rows(raw)                                  # q / (||q|| + 1e-8) in fp32, as the reference forms it
    S, band = _truth(x, qn, 0)
    lab = _labels(n, nb, 16)
    sure, maybe, hit = _sides(S, band, 0.08, 0)
    _assert_cap(sure, maybe, hit, "normalize=True")
    ix = _index(d, 0, x)
    res = ix.facets(raw, 0.08, buckets=lab, nbuckets=nb, normalize=True)
    _check(res, _expect(S, band, sure, maybe, 0, lab, nb), S, band, maybe, 0.08, 0, lab, nb, "normalize=True")
    assert res.total.sum() > 100
    ix.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_same_bytes_under_every_shadow_policy_and_on_every_call(metric):
    n, d, nq, nb = 50000, 768, 17, 64
    x = _rows(n, d, 7)
    q = _queries(x, nq, 71)
    lab = _labels(n, nb, 72)
    radius = _radius(metric, d, "narrow")
    first = None
    for policy in POLICIES:
        ix = _index(d, metric, x, policy)
        for _ in range(2):
            res = ix.facets(q, radius, buckets=lab, nbuckets=nb)
            first = first or res
            _same(res, first, f"metric={metric} shadow={policy}")
        ix.close()
    assert first.total.sum() > 0


def test_buckets_default_nbuckets_empty_index_and_no_queries():
    d, nb = 64, 9
    x = _rows(1000, d, 17)
    lab = (np.arange(1000) % nb).astype(np.int64)
    ix = _index(d, 0, x)
    res = ix.facets(x[:2], -2.0, buckets=lab)                    # nbuckets = max + 1
    assert res.counts.shape == (2, nb) and (res.counts.sum(1) == 1000).all()
    res = ix.facets(np.zeros((0, d), np.float32), 0.5, buckets=lab, nbuckets=nb)
    assert res.counts.shape == (0, nb) and res.best_id.shape == (0, nb) and res.total.shape == (0,)
    ix.close()
    for metric in (0, 1):
        empty = _index(d, metric)
        res = empty.facets(x[:3], 0.5, buckets=np.zeros(0, np.int32), nbuckets=nb)
        assert res.counts.shape == (3, nb) and not res.counts.any() and not res.total.any() and not res.unbucketed.any()
        assert (res.best_id == -1).all() and (res.best_score == np.float32(-FMAX if metric == 0 else FMAX)).all()
        assert empty.last_facet_sweeps() == (0, 0)
        empty.close()


def test_errors():
    from claude_semantic_search_amd import _native as nat
    from claude_semantic_search_amd.flat_index import MAX_FACET_BUCKETS

    d, n = 64, 1000
    x = _rows(n, d, 16)
    lab = np.zeros(n, np.int32)
    ix = _index(d, 0, x)
    for bad in (dict(thresh=float("nan")), dict(nbuckets=0), dict(nbuckets=MAX_FACET_BUCKETS + 1), dict(buckets=lab[:-1]),
                dict(buckets=lab.astype(np.float32)), dict(buckets=lab.reshape(2, -1)), dict(buckets=None, nbuckets=None),
                dict(buckets=lab.astype(np.int64) + 2 ** 31), dict(nbuckets=2.5)):
        args = dict(thresh=0.5, buckets=lab, nbuckets=3)
        args.update(bad)
        with pytest.raises(ValueError):
            ix.facets(x[:2], args.pop("thresh"), **args)
    with pytest.raises(ValueError):
        ix.facets(np.zeros((2, d + 1), np.float32), 0.5, buckets=lab, nbuckets=3)
    lib, h = nat.lib(), ix._handle()
    out = np.zeros(8, np.int64)
    for radius, nb in ((float("nan"), 1), (0.5, 0), (0.5, MAX_FACET_BUCKETS + 1)):   # the library's own checks
        rc = lib.css_index_facets(h, x.ctypes.data, 1, radius, 0, None, lab.ctypes.data, nb, out.ctypes.data, None, None,
                                  out.ctypes.data, out.ctypes.data)
        assert rc == nat.CSS_ERR_INVALID and "css_index_facets" in nat.last_error()
    assert lib.css_index_facets(h, x.ctypes.data, 1, 0.5, 0, None, lab.ctypes.data, 1, None, None, None, out.ctypes.data,
                                out.ctypes.data) == nat.CSS_ERR_INVALID and "NULL buffer" in nat.last_error()
    assert lib.css_index_facets(None, x.ctypes.data, 1, 0.5, 0, None, None, 1, out.ctypes.data, None, None, out.ctypes.data,
                                out.ctypes.data) == nat.CSS_ERR_INVALID
    assert lib.css_index_facets(h, x.ctypes.data, 1 << 24, 0.5, 0, None, None, 1, out.ctypes.data, None, None, out.ctypes.data,
                                out.ctypes.data) == nat.CSS_ERR_INVALID
    res = ix.facets(x[:1], 0.999, buckets=lab, nbuckets=1)       # still usable after the errors
    assert res.counts.tolist() == [[1]] and res.best_id.tolist() == [[0]]
    assert ix.facets(x[:1], float("inf"), buckets=lab, nbuckets=1).total.tolist() == [0]   # infinite radii are ordinary
    assert ix.facets(x[:1], float("-inf"), buckets=lab, nbuckets=1).total.tolist() == [n]
    ix.close()
    with pytest.raises(RuntimeError, match="freed"):
        ix.facets(x[:1], 0.5, buckets=lab, nbuckets=1)

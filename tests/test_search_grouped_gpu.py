"""GPU: ``IndexFlat.search_grouped`` (``css_index_search_grouped``) -- the best row of each of the k best groups -- and
the label column behind it (``set_groups`` / ``get_groups``).

Two oracles.

(i)  Rows and queries built from multiples of 1/8 (``tests/related_fakes.py`` says why): every score is exact in
     float32 whatever the summation order, so every mode and every path must return ``I``, ``G`` and ``D``
     BIT-IDENTICAL to a loop-written collapse of the full ranking ``index.search(q, nrows)`` of the same index.  The
     full ranking is limited to ``MAX_K = 2048`` rows: the cases search a 2048-row slice of the 2999 rows through an
     allow mask, or a 2000-row index without a mask.  A third of the rows are exact copies of other rows and the
     score grid is coarse, so ties are plentiful and the tie rule (lower id first) is tested hard.
(ii) Gaussian rows (``ko.synth_rows``) against the collapsed float64 ranking of ``oracle.knn_oracle``, compared by
     ``knn_checks.assert_topk_matches`` (ids exact outside near ties, scores within 1e-3); labels must agree
     wherever ids agree.  A near tie is a float64 gap of 1e-6, or of 8 float32 ulps of the scores where that is more
     (squared L2 distances of raw rows are ~200 at d = 100 and ~1500 at d = 768: ``_tie_eps``).

2999 rows: no multiple of any tile.  d 64 / 100 / 768 (100 is no multiple of 4).  nq 1 / 3 / 5 / 17 / 33 are the
query-count paths named in ``css_hip.h``.  k 16 / 17 sit on either side of the change of over-fetch class (32 -> 128
rows in pass 1), k 128 is the limit."""
import numpy as np
import pytest

from oracle import knn_oracle as ko
from knn_checks import assert_topk_matches

pytestmark = pytest.mark.gpu

N = 2999
NQS = (1, 3, 5, 17, 33)
KS = (1, 10, 16, 17, 64, 128)
FLT_MAX = np.finfo(np.float32).max


def _pad(metric):
    return -FLT_MAX if metric == 0 else FLT_MAX


def _index(d, metric, x, shadow=None, id_base=0, mode=None, reserve=0):
    from claude_semantic_search_amd.flat_index import IndexFlat

    ix = IndexFlat(d, metric)
    ix.set_shadow(shadow)
    if id_base:
        ix.set_id_base(id_base)
    if reserve:
        ix.reserve(reserve)
    if x.shape[0]:
        ix.add(x)
    if mode:
        ix.set_search_mode(mode)
    return ix


def _eighths(n, d, seed, copies=True):
    """Rows of multiples of 1/8 in [-1, 1]; the last third are exact copies of the first rows (ties across ids)."""
    x = (np.random.default_rng(seed).integers(-8, 9, size=(n, d)) / 8.0).astype(np.float32)
    if copies and n >= 3:
        x[n - n // 3:] = x[:n // 3]
    return x


def _labels(n, ngroups, seed, negative=0.1):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, ngroups, size=n).astype(np.int32)
    g[rng.random(n) < negative] = -1
    return g


def _collapse_loop(Df, If, labels, k, metric, id_base=0):
    """The rule, written as a loop over a best-first list of ALL candidate rows: a row is kept iff it is ungrouped or
    its label has not been seen; the first k kept rows, padded."""
    nq = If.shape[0]
    D = np.full((nq, k), _pad(metric), np.float32)
    I = np.full((nq, k), -1, np.int64)
    G = np.full((nq, k), -1, np.int32)
    for j in range(nq):
        seen, m = set(), 0
        for s, i in zip(Df[j].tolist(), If[j].tolist()):
            if i < 0 or m == k:
                break
            l = int(labels[i - id_base])
            if l >= 0:
                if l in seen:
                    continue
                seen.add(l)
            D[j, m], I[j, m], G[j, m] = np.float32(s), i, max(l, -1)
            m += 1
    return D, I, G


def _assert_identical(got, want, what):
    D, I, G = got
    De, Ie, Ge = want
    assert np.array_equal(I, Ie), f"{what}: ids differ at {np.argwhere(I != Ie)[:5].tolist()}"
    assert np.array_equal(G, Ge), f"{what}: labels differ at {np.argwhere(G != Ge)[:5].tolist()}"
    assert np.array_equal(D.view(np.uint32), De.view(np.uint32)), f"{what}: scores differ"


def _check_against_full_ranking(ix, q, labels, metric, allow, what, nqs=NQS, ks=KS, id_base=0):
    """Oracle (i): grouped results of every (nq, k) against the collapsed full ranking of the same index."""
    nrows = int(allow.sum()) if allow is not None else ix.ntotal
    assert nrows <= 2048
    for nq in nqs:
        Df, If = ix.search(q[:nq], nrows, allow=allow)
        want = _collapse_loop(Df, If, labels, max(ks), metric, id_base)
        for k in ks:
            got = ix.search_grouped(q[:nq], k, allow=allow)
            _assert_identical(got, tuple(a[:, :k] for a in want), f"{what} nq={nq} k={k}")


# ---------------------------------------------------------------------------------------------- oracle (i): exact data
@pytest.mark.parametrize("shadow", [None, False, "int8"], ids=["auto", "noshadow", "int8"])
@pytest.mark.parametrize("mode", ["exact_fp32", "coarse", "auto"])
@pytest.mark.parametrize("d", [64, 100, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_every_mode_and_path_is_bit_identical_to_the_collapsed_full_ranking(metric, d, mode, shadow):
    x = _eighths(N, d, 3 + d)
    q = _eighths(max(NQS), d, 1000 + d, copies=False)
    labels = _labels(N, 40, 5)                      # 40 random groups, 10 % ungrouped
    ix = _index(d, metric, x, shadow=shadow, mode=mode)
    ix.set_groups(labels)
    allow = np.zeros(N, bool)
    allow[np.random.default_rng(9).choice(N, size=2048, replace=False)] = True
    _check_against_full_ranking(ix, q, labels, metric, allow, f"metric={metric} d={d} {mode} shadow={shadow}")
    ix.close()


@pytest.mark.parametrize("mode", ["exact_fp32", "coarse", "auto"])
@pytest.mark.parametrize("metric", [0, 1])
def test_without_a_mask_and_with_many_small_groups(metric, mode):
    n, d = 2000, 100
    x = _eighths(n, d, 21)
    q = _eighths(max(NQS), d, 22, copies=False)
    labels = _labels(n, 400, 23)                    # ~4.5 rows per group: k = 128 groups exist, far down the ranking
    ix = _index(d, metric, x, mode=mode)
    ix.set_groups(labels)
    _check_against_full_ranking(ix, q, labels, metric, None, f"metric={metric} {mode} no mask")
    ix.close()


def test_forty_groups_one_pass_for_ten_and_a_padded_tail_for_128():
    d = 64
    x = _eighths(N, d, 31)
    q = _eighths(5, d, 32, copies=False)
    labels = _labels(2048, 40, 33)
    ix = _index(d, 0, x[:2048], mode="exact_fp32")
    ix.set_groups(labels)
    Df, If = ix.search(q, 2048)
    # k = 10: the 32 best rows of a query hold ten of the 40 groups here (checked, not assumed)
    want = _collapse_loop(Df[:, :32], If[:, :32], labels, 10, 0)
    assert (want[1] >= 0).all()
    _assert_identical(ix.search_grouped(q, 10), want, "k=10")
    assert ix.last_group_passes() == 1
    # k = 128: more groups asked for than exist.  Every ungrouped row is a group of its own, so they are masked out
    # here: 40 groups are all there is, and the tail is padded
    grouped_only = labels >= 0
    got = ix.search_grouped(q, 128, allow=grouped_only)
    Dm, Im = ix.search(q, int(grouped_only.sum()), allow=grouped_only)
    want = _collapse_loop(Dm, Im, labels, 128, 0)
    _assert_identical(got, want, "k=128")
    ngroups = np.unique(labels[grouped_only]).size
    assert (got[1][:, :ngroups] >= 0).all() and (got[1][:, ngroups:] == -1).all()
    assert (got[0][:, ngroups:] == -FLT_MAX).all() and (got[2][:, ngroups:] == -1).all()
    ix.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_every_row_in_one_group_gives_one_entry_then_pads(metric):
    d = 100
    x = _eighths(N, d, 41)
    q = _eighths(17, d, 42, copies=False)
    ix = _index(d, metric, x, mode="auto")
    ix.set_groups(np.full(N, 7, np.int32))
    for nq, k in ((1, 1), (1, 10), (17, 17), (3, 128)):
        D, I, G = ix.search_grouped(q[:nq], k)
        D1, I1 = ix.search(q[:nq], 1)
        assert np.array_equal(I[:, :1], I1) and np.array_equal(D[:, :1].view(np.uint32), D1.view(np.uint32))
        assert (G[:, 0] == 7).all()
        assert (I[:, 1:] == -1).all() and (D[:, 1:] == _pad(metric)).all() and (G[:, 1:] == -1).all()
    ix.close()


@pytest.mark.parametrize("labelled", ["never", "all_negative"])
@pytest.mark.parametrize("metric", [0, 1])
def test_without_groups_it_is_the_plain_search_bit_for_bit(metric, labelled):
    """Never labelled: the call IS the masked search, for every (nq, k).  All labels negative: pass 1 searches for
    kk = 32 or 128 rows and keeps the first k.  An ``exact_fp32`` score is a function of the row and of the KERNEL that
    formed it (a blocked fmaf sweep, or the sequential chain of the fp32-input MFMA scan: ~1e-6 apart), and the kernel
    is chosen by (nq, k): up to 16 queries always sweep, more than 16 scan on the MFMA while k <= 64.  So the bits
    equal those of ``search(q, k)`` wherever k and kk fall into the same family -- nq <= 16, or k <= 16 (kk = 32), or
    k > 64; for 17 <= k <= 64 with more than 16 queries the search for k scans and the search for kk = 128 sweeps, and
    the results are held to the suite's comparison against the float64 ranking instead (ids exact outside near ties)."""
    d = 768
    x = ko.synth_rows(N, d, 51)
    x = ko.normalize_rows(x) if metric == 0 else x
    q = ko.synth_rows(33, d, 52)
    ix = _index(d, metric, x, mode="exact_fp32")
    if labelled == "all_negative":
        ix.set_groups(-1 - np.arange(N, dtype=np.int64) % 5)     # any negative label means "ungrouped"
        assert (ix.get_groups() == -1).all()
    else:
        assert (ix.get_groups() == -1).all()
    allow = np.random.default_rng(53).random(N) < 0.5
    for nq in NQS:
        for k in KS:
            for a in (None, allow):
                D, I, G = ix.search_grouped(q[:nq], k, allow=a)
                De, Ie = ix.search(q[:nq], k, allow=a)
                what = f"{labelled} metric={metric} nq={nq} k={k} mask={a is not None}"
                assert (G == -1).all(), what
                if labelled == "all_negative" and nq > 16 and 16 < k <= 64:
                    _assert_matches64((D, I, G), x, q[:nq], metric, np.full(N, -1, np.int32), k, what, allow=a)
                    continue
                assert np.array_equal(I, Ie), what
                assert np.array_equal(D.view(np.uint32), De.view(np.uint32)), what
    ix.close()


@pytest.mark.parametrize("mode", ["exact_fp32", "auto"])
def test_a_mask_that_hides_best_rows_and_one_that_hides_whole_groups(mode):
    d = 64
    x = _eighths(2048, d, 61)
    q = _eighths(5, d, 62, copies=False)
    labels = _labels(2048, 40, 63)
    ix = _index(d, 0, x, mode=mode)
    ix.set_groups(labels)
    _, I0, G0 = ix.search_grouped(q[:1], 10)
    # (a) the best row of the first five groups of query 0 is hidden: the next best allowed row represents each group
    allow = np.ones(2048, bool)
    allow[I0[0, :5]] = False
    Df, If = ix.search(q, 2048 - 5, allow=allow)
    want = _collapse_loop(Df, If, labels, 10, 0)
    got = ix.search_grouped(q, 10, allow=allow)
    _assert_identical(got, want, "best rows hidden")
    assert not np.isin(got[1][0], I0[0, :5]).any()
    # (b) whole groups hidden: they are absent
    gone = [g for g in G0[0].tolist() if g >= 0][:3]
    allow = ~np.isin(labels, gone)
    Df, If = ix.search(q, int(allow.sum()), allow=allow)
    got = ix.search_grouped(q, 10, allow=allow)
    _assert_identical(got, _collapse_loop(Df, If, labels, 10, 0), "groups hidden")
    assert not np.isin(got[2], gone).any()
    ix.close()


def test_id_base_moves_the_ids_and_not_the_labels():
    d, base = 100, 5_000_000_000
    x = _eighths(2000, d, 71)
    q = _eighths(17, d, 72, copies=False)
    labels = _labels(2000, 30, 73)
    ix0 = _index(d, 0, x, mode="auto")
    ix0.set_groups(labels)
    ix = _index(d, 0, x, mode="auto", id_base=base)
    ix.set_groups(labels)
    for nq, k in ((1, 10), (17, 17), (5, 128)):
        D0, I0, G0 = ix0.search_grouped(q[:nq], k)
        D, I, G = ix.search_grouped(q[:nq], k)
        assert np.array_equal(I, np.where(I0 >= 0, I0 + base, -1))
        assert np.array_equal(G, G0) and np.array_equal(D.view(np.uint32), D0.view(np.uint32))
    _check_against_full_ranking(ix, q, labels, 0, None, "id_base", nqs=(3,), ks=(10, 64), id_base=base)
    ix0.close()
    ix.close()


def test_labels_follow_the_rows_through_a_capacity_growth():
    d = 64
    x = _eighths(N, d, 81)
    q = _eighths(5, d, 82, copies=False)
    labels = _labels(N, 40, 83)
    ix = _index(d, 0, x[:1000], mode="exact_fp32", reserve=1000)
    ix.set_groups(labels[:1000])                    # before the growth
    ix.add(x[1000:])                                # 2999 rows > the 1000 reserved: the rows are reallocated
    assert np.array_equal(ix.get_groups(0, 1000), labels[:1000])
    assert (ix.get_groups(1000) == -1).all()        # appended rows start ungrouped
    ix.set_groups(labels[1000:], row0=1000)         # after the growth
    assert np.array_equal(ix.get_groups(), labels)
    fresh = _index(d, 0, x, mode="exact_fp32")
    fresh.set_groups(labels)
    for nq, k in ((1, 10), (5, 64)):
        _assert_identical(ix.search_grouped(q[:nq], k), fresh.search_grouped(q[:nq], k), f"growth nq={nq} k={k}")
    ix.close()
    fresh.close()


def test_remove_ids_compacts_the_labels_with_the_rows():
    d = 100
    x = _eighths(N, d, 91)
    q = _eighths(17, d, 92, copies=False)
    labels = _labels(N, 60, 93)
    ix = _index(d, 0, x, mode="exact_fp32")
    ix.set_groups(labels)
    keep = np.random.default_rng(94).random(N) < 0.7
    keep[:40] = True                                # the first removed row lies inside a keep word
    keep[40] = False
    assert ix.remove_ids(np.flatnonzero(~keep)) == int((~keep).sum())
    assert np.array_equal(ix.get_groups(), labels[keep])
    fresh = _index(d, 0, x[keep], mode="exact_fp32")
    fresh.set_groups(labels[keep])
    for nq, k in ((1, 10), (17, 17), (3, 128)):
        _assert_identical(ix.search_grouped(q[:nq], k), fresh.search_grouped(q[:nq], k), f"removed nq={nq} k={k}")
    # rows added after a removal start ungrouped although their slots held labels before
    ix.add(x[:50])
    assert (ix.get_groups(int(keep.sum())) == -1).all()
    # reset forgets the labels
    ix.reset()
    ix.add(x[:100])
    assert (ix.get_groups() == -1).all()
    ix.close()
    fresh.close()


# ------------------------------------------------------------------------------------------- oracle (ii): float64 ranking
def _ranking64(x, q, metric, labels, k, allow=None):
    """Collapsed float64 ranking: ``(D32, I, G, D64, D64 of the next group)`` for k groups."""
    ref = ko.FlatIndexOracle(x.shape[1], metric)
    ref.add(x)
    nq, n = q.shape[0], x.shape[0]
    s = ref.rescore64(q, np.tile(np.arange(n, dtype=np.int64), (nq, 1)))
    D = np.full((nq, k), _pad(metric), np.float32)
    D64 = np.full((nq, k), float(_pad(metric)))
    I = np.full((nq, k), -1, np.int64)
    G = np.full((nq, k), -1, np.int32)
    nxt = np.full(nq, float(_pad(metric)))
    for j in range(nq):
        ids = np.arange(n) if allow is None else np.flatnonzero(allow)
        order = ids[np.lexsort((ids, -s[j, ids] if metric == 0 else s[j, ids]))]
        seen, m = set(), 0
        for i in order.tolist():
            l = int(labels[i])
            if l >= 0:
                if l in seen:
                    continue
                seen.add(l)
            if m == k:
                nxt[j] = s[j, i]
                break
            D64[j, m], D[j, m], I[j, m], G[j, m] = s[j, i], np.float32(s[j, i]), i, max(l, -1)
            m += 1
    return D, I, G, D64, nxt


def _tie_eps(D64, I):
    """float64 gap below which two neighbouring ranks may swap in a float32 ranking: the suite's 1e-6 for scores of
    unit rows, and 8 float32 ulps of the largest score in the lists where that is more -- the rule of
    ``test_knn_gpu.py`` for squared L2 distances of raw N(0, 1) rows (1e-3 at distances ~1500, where one ulp is
    1.2e-4): each of the two scores carries its final rounding and those of its partial sums."""
    top = float(np.abs(D64[I >= 0]).max()) if (I >= 0).any() else 1.0
    return max(1e-6, 8.0 * float(np.spacing(np.float32(top))))


def _assert_matches64(got, x, q, metric, labels, k, what, allow=None):
    D, I, G = got
    De, Ie, Ge, D64, nxt = _ranking64(x, q, metric, labels, k, allow)
    assert_topk_matches(D, I, De, Ie, D64, what, D64_next=nxt, tie_eps=_tie_eps(D64, Ie))
    assert np.array_equal(G, np.where(I >= 0, np.maximum(labels[np.where(I >= 0, I, 0)], -1), -1)), f"{what}: G is not the label of I"
    same = I == Ie
    assert np.array_equal(G[same], Ge[same]), f"{what}: labels differ where ids agree"


def _gauss(n, d, seed, metric):
    x = ko.synth_rows(n, d, seed)
    return ko.normalize_rows(x) if metric == 0 else x


@pytest.mark.parametrize("mode", ["exact_fp32", "coarse", "auto"])
@pytest.mark.parametrize("d", [64, 100, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_gaussian_rows_against_the_collapsed_float64_ranking(metric, d, mode):
    x = _gauss(N, d, 101 + d, metric)
    q = _gauss(max(NQS), d, 102 + d, metric)
    labels = _labels(N, 40, 103)
    ix = _index(d, metric, x, mode=mode)
    ix.set_groups(labels)
    allow = np.random.default_rng(104).random(N) < 0.6
    for nq, k, a in ((1, 10, None), (3, 16, allow), (5, 17, None), (17, 64, allow), (33, 128, None), (1, 128, allow)):
        _assert_matches64(ix.search_grouped(q[:nq], k, allow=a), x, q[:nq], metric, labels, k,
                          f"metric={metric} d={d} {mode} nq={nq} k={k} mask={a is not None}", allow=a)
    ix.close()


def _near_copies(qhat, cos, seed):
    """Unit rows with inner product ``cos[i]`` to the unit vector ``qhat``."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((cos.shape[0], qhat.shape[0]))
    u -= (u @ qhat)[:, None] * qhat[None, :]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    c = cos[:, None]
    return (c * qhat[None, :] + np.sqrt(1.0 - c * c) * u).astype(np.float32)


@pytest.mark.parametrize("mode", ["exact_fp32", "auto"])
@pytest.mark.parametrize("metric", [0, 1])
def test_one_dominating_group_costs_one_extra_pass(metric, mode):
    d = 64
    x = _gauss(N, d, 111, 0)                         # unit rows for both metrics: L2 then ranks like the inner product
    qhat = ko.normalize_rows(ko.synth_rows(1, d, 112))[0].astype(np.float64)
    x[:300] = _near_copies(qhat, 0.99 - 1e-4 * np.arange(300), 113)     # 300 near-copies of the query ...
    labels = _labels(N, 200, 114)
    labels[:300] = 1000                              # ... in ONE group; row 0 is its best row
    ix = _index(d, metric, x, mode=mode)
    ix.set_groups(labels)
    q = qhat.astype(np.float32)[None, :]
    D, I, G = ix.search_grouped(q, 10)
    assert ix.last_group_passes() >= 2               # pass 1 (32 rows) returns a single group
    assert I[0, 0] == 0 and G[0, 0] == 1000
    _assert_matches64((D, I, G), x, q, metric, labels, 10, f"dominating metric={metric} {mode}")
    # a batch in which only this query needs the extra pass (the others: ten groups within their 32 best rows, with
    # room to spare -- checked on the float64 ranking, not assumed)
    qb = np.concatenate([_gauss(4, d, 115, 0), q])
    for j in range(4):
        _, I32, _, _, _ = _ranking64(x, qb[j:j + 1], metric, np.full(N, -1, np.int32), 32)
        assert np.unique(labels[I32[0, :24]][labels[I32[0, :24]] >= 0]).size + int((labels[I32[0, :24]] < 0).sum()) >= 10
    got = ix.search_grouped(qb, 10)
    assert ix.last_group_passes() == 2
    _assert_matches64(got, x, qb, metric, labels, 10, f"dominating batch metric={metric} {mode}")
    ix.close()


@pytest.mark.parametrize("mode", ["exact_fp32", "coarse"])
@pytest.mark.parametrize("metric", [0, 1])
def test_a_staircase_of_groups_brings_one_new_group_per_pass(metric, mode):
    d = 64
    x = _gauss(N, d, 121, 0)
    qhat = ko.normalize_rows(ko.synth_rows(1, d, 122))[0].astype(np.float64)
    labels = np.full(N, -1, np.int32)
    labels[1000:] = _labels(N - 1000, 100, 123, negative=0.2)
    for g in range(5):                               # 5 groups of 200 near-copies at falling similarity
        x[200 * g:200 * (g + 1)] = _near_copies(qhat, (0.99 - 0.04 * g) - 1e-4 * np.arange(200), 124 + g)
        labels[200 * g:200 * (g + 1)] = 500 + g
    ix = _index(d, metric, x, mode=mode)
    ix.set_groups(labels)
    q = qhat.astype(np.float32)[None, :]
    D, I, G = ix.search_grouped(q, 8)
    assert ix.last_group_passes() >= 5
    assert G[0, :5].tolist() == [500, 501, 502, 503, 504] and I[0, :5].tolist() == [0, 200, 400, 600, 800]
    assert (I[0] >= 0).all()                         # complete: the random rows supply the other three groups
    _assert_matches64((D, I, G), x, q, metric, labels, 8, f"staircase metric={metric} {mode}")
    # ... and a run that ends exhausted: only the staircase rows are allowed, so five groups are all there is
    allow = np.zeros(N, bool)
    allow[:1000] = True
    D, I, G = ix.search_grouped(q, 8, allow=allow)
    assert G[0].tolist() == [500, 501, 502, 503, 504, -1, -1, -1] and (I[0, 5:] == -1).all()
    _assert_matches64((D, I, G), x, q, metric, labels, 8, f"staircase exhausted metric={metric} {mode}", allow=allow)
    ix.close()


# -------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors():
    d = 64
    x = _eighths(500, d, 131)
    ix = _index(d, 0, x)
    q = x[:2]
    for k in (0, 129):
        with pytest.raises((ValueError, RuntimeError)):
            ix.search_grouped(q, k)
    with pytest.raises((ValueError, RuntimeError)):
        ix.set_groups(np.zeros(500, np.float32))                  # wrong dtype
    with pytest.raises((ValueError, RuntimeError)):
        ix.set_groups(np.zeros(500, np.bool_))
    with pytest.raises((ValueError, RuntimeError)):
        ix.set_groups(np.zeros(501, np.int32))                    # wrong length
    with pytest.raises((ValueError, RuntimeError)):
        ix.set_groups(np.zeros(10, np.int32), row0=495)           # range outside [0, ntotal)
    with pytest.raises((ValueError, RuntimeError)):
        ix.set_groups(np.zeros(10, np.int32), row0=-1)
    with pytest.raises((ValueError, RuntimeError)):
        ix.get_groups(490, 20)
    with pytest.raises((ValueError, RuntimeError)):
        ix.set_groups(np.array([2 ** 31], np.int64))              # beyond int32
    # the C entry points refuse the same things (the Python checks sit in front of them)
    import ctypes

    from claude_semantic_search_amd import _native as nat

    buf = np.zeros(10, np.int32)
    D, I = np.empty((2, 129), np.float32), np.empty((2, 129), np.int64)
    assert nat.lib().css_index_set_groups(ix._handle(), 495, 10, buf.ctypes.data) == nat.CSS_ERR_INVALID
    assert nat.lib().css_index_get_groups(ix._handle(), -1, 10, buf.ctypes.data) == nat.CSS_ERR_INVALID
    for k in (0, 129):
        assert nat.lib().css_index_search_grouped(ix._handle(), q.ctypes.data, 2, k, 0, None, D.ctypes.data, I.ctypes.data,
                                                  None) == nat.CSS_ERR_INVALID
    # nq == 0 is a no-op, an empty index gives fully padded rows, G may be left out
    D0, I0, G0 = ix.search_grouped(np.zeros((0, d), np.float32), 5)
    assert D0.shape == (0, 5) and I0.shape == (0, 5) and G0.shape == (0, 5)
    D2, I2 = np.empty((2, 5), np.float32), np.empty((2, 5), np.int64)
    nat.check(nat.lib().css_index_search_grouped(ix._handle(), q.ctypes.data, 2, 5, 0, None, D2.ctypes.data, I2.ctypes.data, None))
    assert np.array_equal(I2, ix.search(q, 5)[1])
    ix.set_groups(np.arange(500, dtype=np.int64) % 7)              # int64 labels that fit are fine
    assert ix.get_groups().dtype == np.int32
    nat.check(nat.lib().css_index_search_grouped(ix._handle(), q.ctypes.data, 2, 5, 0, None, D2.ctypes.data, I2.ctypes.data, None))
    assert np.array_equal(I2, ix.search_grouped(q, 5)[1])
    ix.close()
    from claude_semantic_search_amd.flat_index import IndexFlat

    empty = IndexFlat(d, 1)
    D, I, G = empty.search_grouped(q, 4)
    assert (I == -1).all() and (D == FLT_MAX).all() and (G == -1).all()
    assert empty.get_groups().shape == (0,)
    empty.close()

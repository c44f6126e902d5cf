"""GPU: ``IndexFlat.search_examples`` (``css_index_search_examples``, kernels ``k_scan_examples`` and
``k_example_scores``): the k best rows under best positive score - gamma * best negative score.

Truth is built as in ``tests/test_search_prior_gpu.py`` (its helpers are imported): fp64 numpy from the very fp32 rows
and examples handed to the index; the code under test is never its own reference.

    inner product   P = max_pos S64, N = max_neg S64, F = P - g * N      larger is better
    squared L2      P = min_pos S64, N = min_neg S64, F = P - g * N      smaller is better

with ``g`` the float32 gamma the call receives, widened exactly, and ``F = P`` without negatives.

Comparison rule.  Ids and order by ``knn_checks.assert_topk_matches(..., tie_eps=1e-6)``.  Values by the bands of that
module (``band_IP = dpad * 2^-24 * ||x|| * ||e||``, ``band_L2 = 4 * dpad * 2^-24 * max(||x||^2, ||e||^2)``), the band of a
(request, row) being the largest over the request's examples: ``|S - P| <= band`` (an extremum of values inside their
bands is inside the largest band) and ``|D - F| <= band * (1 + gamma) + 2^-24 |F|`` (both extrema, and the one rounding
of the fused multiply-add).  ``D`` is sorted best first with ties by ascending id, ids are unique, and
``D == fma(-gamma, N, S)`` is pinned bit for bit in case 2 through ``D == S`` without negatives.

Tie cap: the slots that the tie rule exempts from the id comparison are at most 5 % of all slots of a (metric, d)
combination, summed over its requests; asserted on the fp64 side and printed.  Reorder share: over a combination's
k = 10 requests with negatives at least 20 % of the returned ids are absent from the positive-only fp64 top-10.

Shapes.  n = 100 003 rows (not a multiple of 4: the last row group is partial), one index and one fp64 score matrix per
(metric, d): 40 example vectors (half random unit vectors, half noisy copies of rows) and 16 stored rows as id
examples; a request draws its examples from those 56 without repetition, so it is given partly as vectors and partly
as ids.  The grid of case 1 is not pruned.
"""
import functools

import numpy as np
import pytest

import knn_checks
from oracle import knn_oracle as ko
from test_search_prior_gpu import FMAX, N, POLICIES, U, _exempt, _queries, _rows, _same, _topk64, _truth

pytestmark = pytest.mark.gpu

NVEC, NIDS = 40, 16
SHAPES = [(1, 0), (2, 0), (1, 1), (3, 0), (2, 1), (5, 3), (8, 0), (1, 7), (9, 0), (4, 5), (16, 0), (8, 8), (1, 15)]


class Pool:
    """The rows, the 56 examples of a (metric, d) combination and their fp64 scores and bands against every row."""

    def __init__(self, metric, d, n=N, seed=11):
        self.metric, self.d, self.n = metric, d, n
        self.x = _rows(n, d, seed)
        self.vec = _queries(self.x, NVEC, seed + 1)
        self.ids = np.random.default_rng(seed + 2).choice(n, NIDS, replace=False).astype(np.int64)
        self.S64, self.band = _truth(self.x, np.concatenate([self.vec, self.x[self.ids]]), metric)

    def split(self, sel):
        """Pool numbers -> (vectors, ids) in the order given."""
        sel = np.asarray(sel, np.int64)
        return self.vec[sel[sel < NVEC]], self.ids[sel[sel >= NVEC] - NVEC]

    def fused(self, pos, neg, gamma):
        """fp64 (F, P, band) [n] of a request over pool numbers."""
        return _fuse64(self.S64[pos], self.S64[neg], self.band[np.concatenate([pos, neg]).astype(np.int64)], gamma, self.metric)

    def search(self, ix, pos, neg, k, gamma, **kw):
        vp, ip = self.split(pos)
        vn, ineg = self.split(neg)
        return ix.search_examples(vp, vn, ip, ineg, k=k, gamma=gamma, **kw)


def _fuse64(Sp, Sn, band, gamma, metric):
    ext = np.max if metric == 0 else np.min
    P = ext(Sp, axis=0)
    F = P if Sn.shape[0] == 0 else P - np.float64(np.float32(gamma)) * ext(Sn, axis=0)
    return F, P, band.max(axis=0)


@functools.lru_cache(maxsize=8)
def _pool(metric, d):
    return Pool(metric, d)


def _index(d, metric, x=None, policy="auto"):
    from claude_semantic_search_amd.flat_index import IndexFlat

    ix = IndexFlat(d, metric)
    ix.set_shadow(POLICIES[policy])
    if x is not None and x.shape[0]:
        ix.add(x)
    return ix


def _check(res, F, P, band, k, gamma, metric, what, allowed=None, id_base=0):
    """(D, I, S) of search_examples against fp64 F, P [n] by the rule of the module docstring.  Returns the number of
    slots exempt from the id comparison."""
    D, I, S = res
    n = F.shape[0]
    assert D.dtype == np.float32 and I.dtype == np.int64 and S.dtype == np.float32, what
    assert D.shape == I.shape == S.shape == (k,), what
    I_ref, V, nxt = _topk64(F[None, :], k, metric, allowed)
    loc = np.where(I >= 0, I - id_base, -1)
    knn_checks.assert_topk_matches(D[None, :], loc[None, :], V.astype(np.float32), I_ref, V, what,
                                   D64_next=np.where(np.isnan(nxt), np.inf, nxt), tie_eps=1e-6)
    pad = np.float32(-FMAX if metric == 0 else FMAX)
    v = loc >= 0
    i = loc[v]
    assert v[:i.size].all(), f"{what}: a pad in front of a result"
    assert (D[~v] == pad).all() and (S[~v] == pad).all(), f"{what}: padded slots must carry the pad score in D and S"
    assert ((i >= 0) & (i < n)).all() and np.unique(i).size == i.size, f"{what}: ids repeated or outside [0, n)"
    if allowed is not None:
        assert np.asarray(allowed, bool)[i].all(), f"{what}: a masked or excluded row was returned"
    d = D[v].astype(np.float64)
    step = np.diff(d)
    assert (step <= 0).all() if metric == 0 else (step >= 0).all(), f"{what}: D not best first"
    assert (np.diff(i)[step == 0] > 0).all(), f"{what}: equal values not by ascending id"
    errD = np.abs(d - F[i])
    assert (errD <= band[i] * (1.0 + gamma) + U * np.abs(F[i])).all(), f"{what}: fused value error {errD.max():.3e} beyond the band"
    errS = np.abs(S[v].astype(np.float64) - P[i])
    assert (errS <= band[i]).all(), f"{what}: best positive score error {errS.max():.3e} beyond the band"
    return _exempt(I_ref, V, nxt)


def _allowed_without(n, ids, mask=None):
    a = np.ones(n, bool) if mask is None else np.array(mask, bool)
    a[np.asarray(ids, np.int64)] = False
    return a


# ------------------------------------------------------------------ case 1: the grid
@pytest.mark.parametrize("d", [64, 100, 384, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_every_metric_dim_example_count_k_and_gamma(metric, d):
    pl = _pool(metric, d)
    ix = _index(d, metric, pl.x)
    rng = np.random.default_rng(100 * metric + d)
    exempt = slots = absent = neg_slots = 0
    for npos, nneg in SHAPES:
        for k in (1, 10, 128):
            for gamma in (0.5, 1.0):
                for r in range(2):
                    sel = rng.permutation(NVEC + NIDS)[:npos + nneg]
                    pos, neg = sel[:npos], sel[npos:]
                    excl = r == 0
                    what = f"metric={metric} d={d} npos={npos} nneg={nneg} k={k} gamma={gamma} request {r}"
                    F, P, band = pl.fused(pos, neg, gamma)
                    allowed = _allowed_without(N, pl.split(sel)[1]) if excl else None
                    res = pl.search(ix, pos, neg, k, gamma, exclude_ids=excl)
                    exempt += _check(res, F, P, band, k, gamma, metric, what, allowed)
                    slots += k
                    if k == 10 and nneg:
                        plain10, _, _ = _topk64(P[None, :], 10, metric, allowed)
                        absent += int((~np.isin(res[1], plain10[0])).sum())
                        neg_slots += k
    print(f"metric={metric} d={d}: {exempt} of {slots} slots exempt from the id comparison ({100.0 * exempt / slots:.2f} %)")
    print(f"metric={metric} d={d}: {absent} of {neg_slots} ids returned with negatives are absent from the positive-only "
          f"fp64 top-10 ({100.0 * absent / neg_slots:.1f} %)")
    assert exempt <= 0.05 * slots, f"metric={metric} d={d}: the tie rule exempts {exempt} of {slots} slots"
    assert absent >= 0.20 * neg_slots, f"metric={metric} d={d}: only {absent} of {neg_slots} ids differ from the positive-only top-10"
    ix.close()


# ------------------------------------------------------------------ case 2: bit identities
@pytest.mark.parametrize("d", [100, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_bit_identities_with_the_exact_fp32_search(metric, d):
    pl = _pool(metric, d)
    ix = _index(d, metric, pl.x)
    ix.set_search_mode("exact_fp32")
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)   # noqa: E731
    for k in (10, 128):
        # one positive vector, no negatives: search(q, k)
        for j in (0, 1, 7):
            D0, I0 = ix.search(pl.vec[j:j + 1], k)
            D, I, S = ix.search_examples(pos=pl.vec[j], k=k)
            what = f"metric={metric} d={d} k={k} vector {j}"
            assert np.array_equal(I, I0[0]), f"{what}: ids differ from search() in exact_fp32 mode"
            assert np.array_equal(bits(D), bits(D0[0])), f"{what}: D differs in bits"
            assert np.array_equal(bits(S), bits(D)), f"{what}: S != D"
        # one positive id with exclusion: search_by_ids([id], k)
        for a in pl.ids[:3]:
            D0, I0 = ix.search_by_ids([int(a)], k)
            D, I, S = ix.search_examples(pos_ids=[int(a)], k=k)
            what = f"metric={metric} d={d} k={k} id {a}"
            assert np.array_equal(I, I0[0]) and np.array_equal(bits(D), bits(D0[0])), f"{what}: differs from search_by_ids"
            assert np.array_equal(bits(S), bits(D)), f"{what}: S != D"
        # gamma = 0 with negatives: the same call without the negatives
        for npos, nneg in ((1, 1), (2, 3), (3, 9)):
            vp, vn = pl.vec[:npos], pl.vec[20:20 + nneg]
            with_neg = ix.search_examples(vp, vn, pl.ids[:1], pl.ids[1:2], k=k, gamma=0.0, exclude_ids=False)
            without = ix.search_examples(vp, None, pl.ids[:1], k=k, gamma=0.0, exclude_ids=False)
            _same(with_neg, without, f"metric={metric} d={d} k={k} gamma=0 npos={npos} nneg={nneg}")
        # npos positives, no negatives: the de-duplicated merge by (score, id) of the single-example searches
        for npos in (2, 5, 9, 16):
            singles = [ix.search(pl.vec[j:j + 1], k) for j in range(npos)]
            Dm = np.concatenate([s[0][0] for s in singles])
            Im = np.concatenate([s[1][0] for s in singles])
            order = np.lexsort((Im, -Dm if metric == 0 else Dm))
            Dm, Im = Dm[order], Im[order]
            seen = set()
            keep = []
            for t, i in enumerate(Im.tolist()):   # best occurrence of every id
                if i not in seen:
                    seen.add(i)
                    keep.append(t)
            keep = np.array(keep[:k])
            D, I, S = ix.search_examples(pos=pl.vec[:npos], k=k)
            what = f"metric={metric} d={d} k={k} npos={npos}"
            assert np.array_equal(I, Im[keep]), f"{what}: ids differ from the merge of the single searches"
            assert np.array_equal(bits(D), bits(Dm[keep])), f"{what}: D differs in bits from the merge"
            assert np.array_equal(bits(S), bits(D)), f"{what}: S != D"
    ix.close()


# ------------------------------------------------------------------ case 3: padded slots
@pytest.mark.parametrize("m", [3, 9])
def test_padded_example_slots_take_no_part_inner_product(m):
    metric, d, k = 0, 64, 10
    pl = _pool(metric, d)
    ix = _index(d, metric, pl.x)
    pos = np.arange(0, 2 * m, 2)     # the random unit vectors of the pool
    allow = (pl.S64[pos] < 0).all(axis=0)
    assert allow.sum() >= k
    F, P, band = pl.fused(pos, pos[:0], 0.5)
    res = pl.search(ix, pos, pos[:0], k, 0.5, allow=allow)
    assert (res[0] < 0).all(), f"m={m}: a padded zero example won a maximum: D = {res[0].tolist()}"
    _check(res, F, P, band, k, 0.5, metric, f"padded slots IP m={m}", allowed=allow)
    ix.close()


@pytest.mark.parametrize("m", [3, 9])
def test_padded_example_slots_take_no_part_l2(m):
    metric, d, k, n = 1, 64, 10, 20011
    x = np.ascontiguousarray(3.0 * _rows(n, d, 41), np.float32)   # rows of norm 3: ||x||^2 = 9
    e = _rows(m, d, 42)                                           # unit examples, close to the origin
    S64, band = _truth(x, e, metric)
    allow = (S64 > 9.5).all(axis=0)                               # every real distance beyond a zero example's 9
    assert allow.sum() >= k
    ix = _index(d, metric, x)
    F, P, bd = _fuse64(S64, S64[:0], band, 0.5, metric)
    res = ix.search_examples(pos=e, k=k, allow=allow)
    assert (res[0] > 9.5).all(), f"m={m}: a padded zero example won a minimum: D = {res[0].tolist()}"
    _check(res, F, P, bd, k, 0.5, metric, f"padded slots L2 m={m}", allowed=allow)
    ix.close()


# ------------------------------------------------------------------ case 4: beyond any over-fetch
@pytest.mark.parametrize("metric", [0, 1])
def test_a_row_at_positive_only_rank_50000_comes_first_and_a_disliked_top_row_leaves(metric):
    d, k = 768, 10
    pl = _pool(metric, d)
    ix = _index(d, metric, pl.x)
    q = pl.vec[0:1]
    order0 = np.lexsort((np.arange(N), -pl.S64[0] if metric == 0 else pl.S64[0]))
    r = int(order0[50000])
    neg = np.ascontiguousarray(-10.0 * pl.x[r:r + 1], np.float32)
    Sn, bn = _truth(pl.x, neg, metric)
    F, P, band = _fuse64(pl.S64[0:1], Sn, np.concatenate([pl.band[0:1], bn]), 1.0, metric)
    assert int(np.argmax(F) if metric == 0 else np.argmin(F)) == r, "fp64: the row is not first under the negative"
    D, I, S = ix.search_examples(pos=q, neg=neg, k=k, gamma=1.0)
    assert I[0] == r, f"metric={metric}: the row at positive-only rank 50000 is not first: {I.tolist()}"
    assert abs(float(S[0]) - P[r]) <= band[r] and abs(float(D[0]) - F[r]) <= 2.0 * band[r] + U * abs(F[r])
    # a near-copy of the plain top-1 row as the negative: that row leaves the answer
    top = int(order0[0])
    rng = np.random.default_rng(44)
    near = ko.normalize_rows(pl.x[top] + (0.1 / np.sqrt(d)) * rng.standard_normal(d).astype(np.float32))
    near = np.ascontiguousarray(near.reshape(1, d), np.float32)
    Sn, bn = _truth(pl.x, near, metric)
    F, P, band = _fuse64(pl.S64[0:1], Sn, np.concatenate([pl.band[0:1], bn]), 1.0, metric)
    assert top not in _topk64(F[None, :], k, metric)[0][0], "fp64: the disliked top row stays"
    res = ix.search_examples(pos=q, neg=near, k=k, gamma=1.0)
    assert top not in res[1].tolist(), f"metric={metric}: the disliked top row was returned"
    _check(res, F, P, band, k, 1.0, metric, f"disliked top row metric={metric}")
    ix.close()


# ------------------------------------------------------------------ case 5: exclusion
@pytest.mark.parametrize("metric", [0, 1])
def test_id_examples_are_excluded_and_only_they(metric):
    d, k = 100, 10
    pl = _pool(metric, d)
    n0 = 30001
    a, b, c = 123, 4567, 29999
    x = np.concatenate([pl.x[:n0], pl.x[a:a + 1]])          # row n0 is a copy of row a under another id
    S64, band = _truth(x, x[[a, b, c]], metric)
    ix = _index(d, metric, x)
    F, P, bd = _fuse64(S64[:2], S64[2:], band, 0.5, metric)
    res = ix.search_examples(pos_ids=[a, b, a], neg_ids=[c, c], k=k, gamma=0.5)     # repeated ids
    assert not np.isin(res[1], [a, b, c]).any(), f"an id example was returned: {res[1].tolist()}"
    _check(res, F, P, bd, k, 0.5, metric, "ids excluded", allowed=_allowed_without(n0 + 1, [a, b, c]))
    assert res[1][0] == n0, "the copy of an anchor under another id must be returned (first: it scores like the anchor)"
    Fa, Pa, ba = _fuse64(S64[:1], S64[:0], band[:1], 0.5, metric)
    D, I, S = ix.search_examples(pos_ids=[a], k=k, exclude_ids=False)
    assert I[0] == a and I[1] == n0, f"exclude_ids=False: anchor and copy must lead (ties by id): {I.tolist()}"
    _check((D, I, S), Fa, Pa, ba, k, 0.5, metric, "ids kept")
    masked = _allowed_without(n0 + 1, [a, b])                 # masked-out anchors are examples all the same
    for excl in (True, False):
        res = ix.search_examples(pos_ids=[a, b], neg_ids=[c], k=k, gamma=0.5, exclude_ids=excl, allow=masked)
        allowed = _allowed_without(n0 + 1, [c], masked) if excl else masked
        _check(res, F, P, bd, k, 0.5, metric, f"masked anchors exclude_ids={excl}", allowed=allowed)
    ix.close()


# ------------------------------------------------------------------ case 6: masks and id base
@pytest.mark.parametrize("metric", [0, 1])
def test_allow_masks_and_id_base(metric):
    d, k, gamma = 384, 10, 0.5
    pl = _pool(metric, d)
    ix = _index(d, metric, pl.x)
    pos, neg = np.array([0, 1, NVEC + 2]), np.array([5, NVEC + 7])
    ids = pl.split(np.concatenate([pos, neg]))[1]
    F, P, band = pl.fused(pos, neg, gamma)
    half = np.random.default_rng(6).random(N) < 0.5
    res = pl.search(ix, pos, neg, k, gamma, allow=half)
    _check(res, F, P, band, k, gamma, metric, "random 50 % mask", allowed=_allowed_without(N, ids, half))
    pad = np.float32(-FMAX if metric == 0 else FMAX)
    D, I, S = pl.search(ix, pos, neg, k, gamma, allow=np.zeros(N, bool))
    assert (I == -1).all() and (D == pad).all() and (S == pad).all()
    one = np.zeros(N, bool)
    one[N - 1] = True
    D, I, S = pl.search(ix, pos, neg, k, gamma, allow=one)
    assert I[0] == N - 1 and (I[1:] == -1).all() and (D[1:] == pad).all() and (S[1:] == pad).all()
    _check((D, I, S), F, P, band, k, gamma, metric, "one-row mask", allowed=one)
    ix.set_id_base(10 ** 9)
    vp, ip = pl.split(pos)
    vn, ineg = pl.split(neg)
    based = ix.search_examples(vp, vn, ip + 10 ** 9, ineg + 10 ** 9, k=k, gamma=gamma, allow=half)
    assert np.array_equal(based[0], res[0]) and np.array_equal(based[2], res[2]) and np.array_equal(based[1], res[1] + 10 ** 9)
    _check(ix.search_examples(vp, vn, ip + 10 ** 9, ineg + 10 ** 9, k=k, gamma=gamma), F, P, band, k, gamma, metric, "id base",
           allowed=_allowed_without(N, ids), id_base=10 ** 9)
    with pytest.raises(ValueError):
        ix.search_examples(vp, vn, k=k, allow=np.ones(N - 1, bool))
    ix.close()


# ------------------------------------------------------------------ case 7: independence
@pytest.mark.parametrize("metric", [0, 1])
def test_result_does_not_depend_on_shadow_policy_search_mode_or_row_history(metric):
    n, d, k, gamma = 50000, 768, 10, 0.5
    pl = _pool(metric, d)
    x = pl.x[:n]
    vp, vn = pl.vec[:3], pl.vec[10:12]
    ip, ineg = np.array([17, 40000]), np.array([25001])
    first = None
    for policy in POLICIES:
        ix = _index(d, metric, x, policy)
        for mode in ("auto", "exact_fp32", "coarse"):
            ix.set_search_mode(mode)
            res = ix.search_examples(vp, vn, ip, ineg, k=k, gamma=gamma)
            if first is None:
                first = res
                S64, band = _truth(x, np.concatenate([vp, x[ip], vn, x[ineg]]), metric)
                F, P, bd = _fuse64(S64[:5], S64[5:], band, gamma, metric)
                _check(res, F, P, bd, k, gamma, metric, f"shadow={policy}", allowed=_allowed_without(n, [17, 40000, 25001]))
            _same(res, first, f"metric={metric} shadow={policy} mode={mode}")
        ix.close()
    # after remove_ids: the results of a fresh index of the kept rows (ids follow the compaction)
    ix = _index(d, metric, x)
    keep = np.random.default_rng(9).random(n) >= 0.10
    keep[[17, 40000, 25001]] = True
    assert ix.remove_ids(np.flatnonzero(~keep)) == int((~keep).sum())
    new_id = np.cumsum(keep) - 1
    fresh = _index(d, metric, x[keep])
    for kk in (k, 128):
        _same(ix.search_examples(vp, vn, new_id[ip], new_id[ineg], k=kk, gamma=gamma),
              fresh.search_examples(vp, vn, new_id[ip], new_id[ineg], k=kk, gamma=gamma), f"after remove_ids k={kk}")
    fresh.close()
    ix.reset()
    ix.add(x[:5000])
    D, I, S = ix.search_examples(pos=vp, k=k)
    assert (I >= 0).all() and (I < 5000).all() and np.array_equal(D.view(np.uint32), S.view(np.uint32))
    ix.close()


# ------------------------------------------------------------------ case 8: errors
def test_errors():
    from claude_semantic_search_amd import _native as nat

    d, n = 64, 1000
    x = _rows(n, d, 16)
    ix = _index(d, 0, x)
    fn = nat.lib().css_index_search_examples
    usable = lambda: ix.search_examples(pos=x[0], k=1)[1].tolist() == [0]   # noqa: E731
    out = lambda k: (np.empty(max(k, 1), np.float32), np.empty(max(k, 1), np.int64), np.empty(max(k, 1), np.float32))  # noqa: E731

    def raw(vec, nvp, nvn, ids, nip, nin, k, gamma):
        D, I, S = out(k)
        ids = np.ascontiguousarray(ids, np.int64)
        return fn(ix._handle(), vec.ctypes.data if vec is not None else None, nvp, nvn, ids.ctypes.data if ids.size else None,
                  nip, nin, k, gamma, 0, 1, None, D.ctypes.data, I.ctypes.data, S.ctypes.data)

    assert usable()
    for k in (0, 129):
        with pytest.raises(ValueError):
            ix.search_examples(pos=x[:2], k=k)
        assert raw(x[:2], 2, 0, [], 0, 0, k, 0.5) == nat.CSS_ERR_INVALID and f"k={k}" in nat.last_error()
        assert usable()
    for bad, name in ((float("nan"), "NaN"), (float("inf"), "infinite"), (-0.25, "negative")):
        with pytest.raises(ValueError):
            ix.search_examples(pos=x[:2], neg=x[2:3], k=5, gamma=bad)
        assert raw(x[:3], 2, 1, [], 0, 0, 5, bad) == nat.CSS_ERR_INVALID
        assert "gamma" in nat.last_error() and name in nat.last_error()
        assert usable()
    for bad in (-1, n, 10 ** 12):                                     # an id outside the index: the message names it
        with pytest.raises(nat.CssError) as e:
            ix.search_examples(pos=x[:1], neg_ids=[5, bad], k=5)
        assert e.value.code == nat.CSS_ERR_INVALID and str(bad) in str(e.value)
        assert raw(None, 0, 0, [3, bad], 2, 0, 5, 0.5) == nat.CSS_ERR_INVALID and str(bad) in nat.last_error()
        assert usable()
    with pytest.raises(ValueError):                                   # no positive
        ix.search_examples(neg=x[:2], neg_ids=[3], k=5)
    with pytest.raises(ValueError):
        ix.search_examples(k=5)
    assert raw(x[:2], 0, 2, [3], 0, 1, 5, 0.5) == nat.CSS_ERR_INVALID and "positive" in nat.last_error()
    assert raw(None, 0, 0, [], 0, 0, 5, 0.5) == nat.CSS_ERR_INVALID and "positive" in nat.last_error()
    assert usable()
    with pytest.raises(ValueError):                                   # m > 16
        ix.search_examples(pos=x[:9], neg=x[9:14], pos_ids=[1, 2], neg_ids=[3], k=5)
    assert raw(x[:17], 9, 8, [], 0, 0, 5, 0.5) == nat.CSS_ERR_INVALID and "16" in nat.last_error()
    assert raw(x[:14], 9, 5, [1, 2, 3], 2, 1, 5, 0.5) == nat.CSS_ERR_INVALID and "16" in nat.last_error()
    assert raw(x[:2], -1, 2, [], 0, 0, 5, 0.5) == nat.CSS_ERR_INVALID
    assert usable()
    with pytest.raises(ValueError):
        ix.search_examples(pos=np.zeros((2, d + 1), np.float32), k=5)   # wrong width
    with pytest.raises(ValueError):
        ix.search_examples(pos=x[:1], pos_ids=[1.5], k=5)               # ids that are no integers
    D, I, S = ix.search_examples(pos=np.zeros((0, d), np.float32), pos_ids=[4], neg=[], neg_ids=np.zeros(0, np.int64), k=3)
    assert I.shape == (3,) and 4 not in I.tolist()                      # empty inputs beside a real one
    D2, I2 = np.empty(3, np.float32), np.empty(3, np.int64)             # S_host may be NULL
    ids = np.array([4], np.int64)
    assert fn(ix._handle(), None, 0, 0, ids.ctypes.data, 1, 0, 3, 0.5, 0, 1, None, D2.ctypes.data, I2.ctypes.data, None) == nat.CSS_OK
    assert np.array_equal(I2, I) and np.array_equal(D2.view(np.uint32), D.view(np.uint32))
    assert usable()
    ix.close()
    with pytest.raises(RuntimeError, match="freed"):
        ix.search_examples(pos=x[:1], k=5)
    assert fn(None, x.ctypes.data, 1, 0, None, 0, 0, 5, 0.5, 0, 1, None, D2.ctypes.data, I2.ctypes.data, None) == nat.CSS_ERR_INVALID
    for metric, pad in ((0, -FMAX), (1, FMAX)):                         # an empty index: padded output, and no id is known
        empty = _index(d, metric)
        D, I, S = empty.search_examples(pos=x[:3], neg=x[3:4], k=4)
        assert (I == -1).all() and (D == np.float32(pad)).all() and (S == np.float32(pad)).all()
        with pytest.raises(nat.CssError):
            empty.search_examples(pos_ids=[0], k=4)
        empty.add(x[:10])
        assert empty.search_examples(pos_ids=[0], k=4, exclude_ids=False)[1][0] == 0
        empty.close()

"""GPU: ``IndexFlat.search_prior`` / ``set_priors`` / ``get_priors`` (``css_index_search_prior``, kernels
``k_scan_prior`` and ``k_prior_scores``).

Truth is computed here in fp64 with numpy from the very fp32 rows, queries and priors handed to the index
(``oracle.knn_oracle.synth_rows`` + ``normalize_rows``); the code under test is never its own reference.

    inner product   F = S64 + w * p     larger is better
    squared L2      F = S64 - w * p     smaller is better (S64 from squared differences)

with ``w`` the float32 weight the call receives and ``p`` the float32 priors, both widened exactly.

Comparison rule.  Ids and order by ``knn_checks.assert_topk_matches(..., tie_eps=1e-6)``, the project's rule for the
exact fp32 sweep (neighbouring fp64 ranks closer than 1e-6 may swap).  Values by the bands of
``tests/test_range_search_gpu.py`` (recursive fp32 sum of ``dpad`` fused multiply-adds):

    band_IP = dpad * 2^-24 * ||x|| * ||q||                 band_L2 = 4 * dpad * 2^-24 * max(||x||^2, ||q||^2)

``|S - S64[I]| <= band`` and ``|D - F[I]| <= band + 2^-24 |F|`` (the one extra rounding of the fused multiply-add).  ``D``
is sorted best first with ties by ascending id, ids are unique.  So that the tie rule cannot hide a failure, every case
asserts on the fp64 side that the slots exempt from the id comparison are at most 5 % of ``nq * k`` and prints the share.

The fused order must differ from the plain one: at k = 10 at least 20 % of the returned ids are absent from the plain
fp64 top-10.  This is asserted for every (metric, d, weight) over the whole query set (nq = 40, 400 slots) and printed
for every nq: with one query the share is a multiple of 10 %, and the fp64 ranking ITSELF gives 10 % for L2, d = 768,
weight 0.05, nq = 1 (squared distances of unit rows are 2 - 2 s, so they spread twice as wide as inner products and the
same weight reorders half as much); over 40 queries fp64 gives at least 28 % in every combination.

Shapes.  The grid of case 1 is NOT pruned: {IP, L2} x d {64, 100, 384, 768} x nq {1, 2, 3, 8, 9, 16, 17, 40} x k {1, 10,
128} x weight {0.05, 0.5} * sqrt(768 / d), at n = 100 003 rows (not a multiple of 4: the last row group is partial), one
index and one fp64 matrix per (metric, d).  The other cases run at one shape each (both metrics where the metric
matters): they do not interact with the arithmetic of the sweep, which the grid covers.
"""
import functools

import numpy as np
import pytest

import knn_checks
from oracle import knn_oracle as ko

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N = 100003
FMAX = np.finfo(np.float32).max
POLICIES = {"off": False, "bf16": True, "int8": "int8", "auto": None}


@functools.lru_cache(maxsize=4)
def _rows(n, d, seed):
    x = ko.normalize_rows(ko.synth_rows(n, d, seed))
    x.setflags(write=False)
    return x


def _queries(x, nq, seed):
    """Half random unit vectors, half noisy copies of rows (unit again), as tests/test_range_search_gpu.py::_queries."""
    n, d = x.shape
    q = np.array(_rows(nq, d, seed))
    rng = np.random.default_rng(seed)
    for j in range(1, nq, 2):
        v = x[rng.integers(0, n)] + (0.5 / np.sqrt(d)) * rng.standard_normal(d).astype(np.float32)
        q[j] = ko.normalize_rows(v)[0]
    return np.ascontiguousarray(q, np.float32)


def _priors(n, seed):
    return np.random.default_rng(seed).random(n, dtype=np.float32)


def _truth(x, q, metric):
    """fp64 raw scores [nq, n] and the band [nq, n] of the module docstring."""
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    dpad = (x.shape[1] + 63) // 64 * 64
    xn2, qn2 = (x64 * x64).sum(1), (q64 * q64).sum(1)
    dot = q64 @ x64.T
    if metric == 0:
        return dot, dpad * U * np.sqrt(qn2)[:, None] * np.sqrt(xn2)[None, :]
    return np.maximum(qn2[:, None] + xn2[None, :] - 2.0 * dot, 0.0), 4 * dpad * U * np.maximum(qn2[:, None], xn2[None, :])


def _fused(S64, p, w, metric):
    wp = np.float64(np.float32(w)) * np.asarray(p, np.float32).astype(np.float64)
    return S64 + wp[None, :] if metric == 0 else S64 - wp[None, :]


def _topk64(F, k, metric, allowed=None):
    """fp64 ranking: ids [nq, k] (padded -1), values [nq, k], and the value of rank k + 1 (nan where there is none)."""
    nq, n = F.shape
    key = -F if metric == 0 else F.copy()
    if allowed is not None:
        key = np.where(np.asarray(allowed, bool)[None, :], key, np.inf)
    m = min(n, k + 1)
    I = np.full((nq, k), -1, np.int64)
    V = np.full((nq, k), -FMAX if metric == 0 else FMAX, np.float64)
    nxt = np.full(nq, np.nan)
    for j in range(nq):
        cand = np.argpartition(key[j], m - 1)[:m] if m < n else np.arange(n)
        # every row tied with the m-th value must be a candidate for the id tie-break
        cand = np.flatnonzero(key[j] <= key[j, cand].max())
        order = cand[np.lexsort((cand, key[j, cand]))]
        order = order[np.isfinite(key[j, order])]
        top = order[:k]
        I[j, :top.size], V[j, :top.size] = top, F[j, top]
        if order.size > k:
            nxt[j] = F[j, order[k]]
    return I, V, nxt


def _exempt(I_ref, V, nxt, tie_eps=1e-6):
    """The slots assert_topk_matches does not compare by id, counted as it forms them."""
    valid = I_ref >= 0
    gaps = np.abs(np.diff(V, axis=1))
    safe = valid.copy()
    safe[:, 1:] &= gaps > tie_eps
    safe[:, :-1] &= gaps > tie_eps
    with np.errstate(invalid="ignore"):
        safe[:, -1] &= ~(np.abs(V[:, -1] - nxt) <= tie_eps)
    return int((valid & ~safe).sum())


def _check(res, F, S64, band, k, metric, what, allowed=None, id_base=0):
    """(D, I, S) of search_prior against the fp64 fused values F and raw scores S64 by the rule of the module
    docstring.  Returns the number of slots exempt from the id comparison."""
    D, I, S = res
    nq, n = F.shape
    assert D.dtype == np.float32 and I.dtype == np.int64 and S.dtype == np.float32, what
    assert D.shape == I.shape == S.shape == (nq, k), what
    I_ref, V, nxt = _topk64(F, k, metric, allowed)
    loc = np.where(I >= 0, I - id_base, -1)
    knn_checks.assert_topk_matches(D, loc, V.astype(np.float32), I_ref, V, what,
                                   D64_next=np.where(np.isnan(nxt), np.inf, nxt), tie_eps=1e-6)
    pad = np.float32(-FMAX if metric == 0 else FMAX)
    for j in range(nq):
        v = loc[j] >= 0
        i = loc[j][v]
        w = f"{what} query {j}"
        assert v[:i.size].all(), f"{w}: a pad in front of a result"
        assert (D[j][~v] == pad).all() and (S[j][~v] == pad).all(), f"{w}: padded slots must carry the pad score in D and S"
        assert ((i >= 0) & (i < n)).all() and np.unique(i).size == i.size, f"{w}: ids repeated or outside [0, n)"
        if allowed is not None:
            assert np.asarray(allowed, bool)[i].all(), f"{w}: a masked row was returned"
        d = D[j][v].astype(np.float64)
        step = np.diff(d)
        assert (step <= 0).all() if metric == 0 else (step >= 0).all(), f"{w}: D not best first"
        assert (np.diff(i)[step == 0] > 0).all(), f"{w}: equal values not by ascending id"
        errD = np.abs(d - F[j, i])
        assert (errD <= band[j, i] + U * np.abs(F[j, i])).all(), f"{w}: fused value error {errD.max():.3e} beyond the band"
        errS = np.abs(S[j][v].astype(np.float64) - S64[j, i])
        assert (errS <= band[j, i]).all(), f"{w}: raw score error {errS.max():.3e} beyond the band"
    return _exempt(I_ref, V, nxt)


def _index(d, metric, x=None, policy="auto", priors=None):
    from claude_semantic_search_amd.flat_index import IndexFlat

    ix = IndexFlat(d, metric)
    ix.set_shadow(POLICIES[policy])
    if x is not None and x.shape[0]:
        ix.add(x)
    if priors is not None:
        ix.set_priors(priors)
    return ix


def _same(a, b, what):
    for u, v, name in zip(a, b, ("D", "I", "S")):
        assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u.view(np.uint8), v.view(np.uint8)), \
            f"{what}: {name} differs"


# ------------------------------------------------------------------ case 1: the grid
@pytest.mark.parametrize("d", [64, 100, 384, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_every_metric_dim_query_count_k_and_weight(metric, d):
    x = _rows(N, d, 11)
    q = _queries(x, 40, 12)
    p = _priors(N, 13)
    S64, band = _truth(x, q, metric)
    plain10, _, _ = _topk64(S64, 10, metric)
    ix = _index(d, metric, x, priors=p)
    for w0 in (0.05, 0.5):
        w = float(np.float32(w0 * np.sqrt(768.0 / d)))
        F = _fused(S64, p, w, metric)
        for nq in (1, 2, 3, 8, 9, 16, 17, 40):
            for k in (1, 10, 128):
                what = f"metric={metric} d={d} nq={nq} k={k} weight={w:.4f}"
                res = ix.search_prior(q[:nq], k, w)
                exempt = _check(res, F[:nq], S64[:nq], band[:nq], k, metric, what)
                print(f"{what}: {exempt} of {nq * k} slots exempt from the id comparison ({100.0 * exempt / (nq * k):.2f} %)")
                assert exempt <= 0.05 * nq * k, f"{what}: the tie rule exempts {exempt} of {nq * k} slots"
                if k == 10:   # the fused order is not the plain one (asserted over the whole query set: docstring)
                    absent = sum(int((~np.isin(res[1][j], plain10[j])).sum()) for j in range(nq))
                    print(f"{what}: {absent} of {nq * k} returned ids are absent from the plain fp64 top-10")
                    if nq == 40:
                        assert absent >= 0.20 * nq * k, f"{what}: only {absent} of {nq * k} ids differ from the plain top-10"
    ix.close()


# ------------------------------------------------------------------ case 2: identity with the exact fp32 search
@pytest.mark.parametrize("d", [100, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_without_priors_or_weight_it_is_the_exact_fp32_search_bit_for_bit(metric, d):
    x = _rows(N, d, 11)
    q = _queries(x, 40, 21)
    ix = _index(d, metric, x)
    ix.set_search_mode("exact_fp32")
    for k in (10, 128):
        plain = {nq: ix.search(q[:nq], k) for nq in (1, 2, 5, 16)}
        parts = [ix.search(q[s:s + 16], k) for s in range(0, 40, 16)]   # (a batch of 40 would take the MFMA scan)
        plain[40] = (np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts]))
        for setup in ("never set", "set, weight 0"):
            if setup == "set, weight 0":
                ix.set_priors(_priors(N, 22))
            for nq in (1, 2, 5, 16, 40):
                for w in ((0.0, 0.7, -3.0) if setup == "never set" else (0.0,)):
                    what = f"metric={metric} d={d} k={k} nq={nq} priors {setup} weight={w}"
                    D, I, S = ix.search_prior(q[:nq], k, w)
                    assert np.array_equal(I, plain[nq][1]), f"{what}: ids differ from search() in exact_fp32 mode"
                    assert np.array_equal(D.view(np.uint32), plain[nq][0].view(np.uint32)), f"{what}: D differs in bits"
                    assert np.array_equal(S.view(np.uint32), D.view(np.uint32)), f"{what}: S != D"
        ix.reset()
        ix.add(x)
    ix.close()


# ------------------------------------------------------------------ case 3: a boosted row far below any over-fetch
@pytest.mark.parametrize("metric", [0, 1])
def test_a_boosted_row_at_plain_rank_50000_comes_first(metric):
    d, k = 768, 10
    x = _rows(N, d, 11)
    q = _queries(x, 3, 31)
    S64, band = _truth(x, q, metric)
    order0 = np.lexsort((np.arange(N), -S64[0] if metric == 0 else S64[0]))
    r = int(order0[50000])
    p = np.zeros(N, np.float32)
    p[r] = 1.0
    ix = _index(d, metric, x, priors=p)
    D, I, S = ix.search_prior(q, k, 1.0)
    assert I[0, 0] == r, f"metric={metric}: the boosted row (plain rank 50000) is not first: {I[0].tolist()}"
    assert abs(float(S[0, 0]) - S64[0, r]) <= band[0, r]
    F = _fused(S64, p, 1.0, metric)
    assert abs(float(D[0, 0]) - F[0, r]) <= band[0, r] + U * abs(F[0, r])
    # slots 1.. of query 0 are the plain top-(k - 1); the other queries' lists hold it only if it ranks there anyway
    _check((D, I, S), F, S64, band, k, metric, f"boosted row metric={metric}")
    I9, V9, nxt9 = _topk64(S64[:1], k - 1, metric)
    knn_checks.assert_topk_matches(D[:1, 1:], I[:1, 1:], V9.astype(np.float32), I9, V9, "plain tail", D64_next=nxt9)
    assert np.array_equal(S[0, 1:].view(np.uint32), D[0, 1:].view(np.uint32))   # prior 0: fused == raw, bit for bit
    ix.close()


# ------------------------------------------------------------------ case 4: the column follows the rows
@pytest.mark.parametrize("metric", [0, 1])
def test_the_prior_column_follows_the_rows(metric):
    n, d, nq, k, w = 40001, 64, 9, 10, 0.3
    x = _rows(n, d, 8)
    q = _queries(x, nq, 81)
    p = _priors(n, 82)
    ix = _index(d, metric)
    assert ix.get_priors().shape == (0,)
    ix.add(x[:7000])
    assert np.array_equal(ix.get_priors(), np.zeros(7000, np.float32))          # never set: zeros
    ix.set_priors(p[1000:3000], row0=1000)                                      # partial set
    want = np.zeros(7000, np.float32)
    want[1000:3000] = p[1000:3000]
    assert np.array_equal(ix.get_priors().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(ix.get_priors(2990, 20), want[2990:3010])
    for r0 in range(7000, n, 7000):                                             # the capacity grows several times
        ix.add(x[r0:r0 + 7000])
        got = ix.get_priors()
        assert np.array_equal(got[:7000].view(np.uint32), want.view(np.uint32)), "priors lost in a capacity growth"
        assert np.array_equal(got[7000:], np.zeros(got.shape[0] - 7000, np.float32)), "appended rows must read back as 0.0"
    ix.set_priors(p)
    S64, band = _truth(x, q, metric)
    _check(ix.search_prior(q, k, w), _fused(S64, p, w, metric), S64, band, k, metric, "after growth")
    gone = np.flatnonzero(np.random.default_rng(9).random(n) < 0.10)
    keep = np.ones(n, bool)
    keep[gone] = False
    assert ix.remove_ids(gone) == gone.shape[0]
    assert np.array_equal(ix.get_priors().view(np.uint32), p[keep].view(np.uint32)), "get_priors != priors[keep] after remove_ids"
    fresh = _index(d, metric, x[keep], priors=p[keep])
    for kk in (k, 128):
        _same(ix.search_prior(q, kk, w), fresh.search_prior(q, kk, w), f"after remove_ids k={kk}")
    S64, band = _truth(x[keep], q, metric)
    _check(ix.search_prior(q, k, w), _fused(S64, p[keep], w, metric), S64, band, k, metric, "after remove_ids")
    fresh.close()
    ix.add(x[:100])                                                             # slots of removed rows are reused
    assert np.array_equal(ix.get_priors(int(keep.sum())), np.zeros(100, np.float32))
    ix.reset()
    ix.add(x[:5000])
    assert np.array_equal(ix.get_priors(), np.zeros(5000, np.float32)), "reset must forget the priors"
    D, I, S = ix.search_prior(q, k, w)
    assert np.array_equal(D.view(np.uint32), S.view(np.uint32))
    ix.close()


# ------------------------------------------------------------------ case 5: masks and id base
@pytest.mark.parametrize("metric", [0, 1])
def test_allow_masks_and_id_base(metric):
    n, d, nq, k, w = 60001, 384, 9, 10, 0.2
    x = _rows(n, d, 5)
    q = _queries(x, nq, 51)
    p = _priors(n, 52)
    S64, band = _truth(x, q, metric)
    F = _fused(S64, p, w, metric)
    ix = _index(d, metric, x, priors=p)
    half = np.random.default_rng(6).random(n) < 0.5
    res = ix.search_prior(q, k, w, allow=half)
    _check(res, F, S64, band, k, metric, "random 50 % mask", allowed=half)
    pad = np.float32(-FMAX if metric == 0 else FMAX)
    D, I, S = ix.search_prior(q, k, w, allow=np.zeros(n, bool))
    assert (I == -1).all() and (D == pad).all() and (S == pad).all()
    one = np.zeros(n, bool)
    one[n - 1] = True
    D, I, S = ix.search_prior(q, k, w, allow=one)
    assert (I[:, 0] == n - 1).all() and (I[:, 1:] == -1).all() and (D[:, 1:] == pad).all() and (S[:, 1:] == pad).all()
    _check((D, I, S), F, S64, band, k, metric, "one-row mask", allowed=one)
    ix.set_id_base(10 ** 9)
    based = ix.search_prior(q, k, w, allow=half)
    assert np.array_equal(based[0], res[0]) and np.array_equal(based[2], res[2]) and np.array_equal(based[1], res[1] + 10 ** 9)
    _check(ix.search_prior(q, k, w), F, S64, band, k, metric, "id base", id_base=10 ** 9)
    with pytest.raises(ValueError):
        ix.search_prior(q, k, w, allow=np.ones(n - 1, bool))
    ix.close()


# ------------------------------------------------------------------ case 6: independence of shadow rows and search mode
@pytest.mark.parametrize("metric", [0, 1])
def test_result_does_not_depend_on_shadow_policy_or_search_mode(metric):
    n, d, nq, k, w = 50000, 768, 17, 10, 0.1
    x = _rows(n, d, 7)
    q = _queries(x, nq, 71)
    p = _priors(n, 72)
    first = None
    for policy in POLICIES:
        ix = _index(d, metric, x, policy, priors=p)
        for mode in ("auto", "exact_fp32", "coarse"):
            ix.set_search_mode(mode)
            res = ix.search_prior(q, k, w)
            if first is None:
                first = res
                S64, band = _truth(x, q, metric)
                _check(res, _fused(S64, p, w, metric), S64, band, k, metric, f"shadow={policy}")
            _same(res, first, f"metric={metric} shadow={policy} mode={mode}")
        ix.close()


# ------------------------------------------------------------------ case 7: errors
def test_errors():
    from claude_semantic_search_amd import _native as nat

    d, n = 64, 1000
    x = _rows(n, d, 16)
    p = _priors(n, 17)
    ix = _index(d, 0, x, priors=p)
    usable = lambda: ix.search_prior(x[:1], 1, 0.0)[1].tolist() == [[0]]   # noqa: E731
    for k in (0, 129):
        with pytest.raises(ValueError):
            ix.search_prior(x[:2], k, 0.1)
        D, I, S = np.empty((2, 129), np.float32), np.empty((2, 129), np.int64), np.empty((2, 129), np.float32)
        rc = nat.lib().css_index_search_prior(ix._handle(), x[:2].ctypes.data, 2, k, 0.1, 0, None, D.ctypes.data, I.ctypes.data,
                                              S.ctypes.data)
        assert rc == nat.CSS_ERR_INVALID and f"k={k}" in nat.last_error()
        assert usable()
    for bad, name in ((float("nan"), "NaN"), (float("inf"), "infinite"), (float("-inf"), "infinite")):
        with pytest.raises(ValueError):
            ix.search_prior(x[:2], 5, bad)
        D, I, S = np.empty((2, 5), np.float32), np.empty((2, 5), np.int64), np.empty((2, 5), np.float32)
        rc = nat.lib().css_index_search_prior(ix._handle(), x[:2].ctypes.data, 2, 5, bad, 0, None, D.ctypes.data, I.ctypes.data,
                                              S.ctypes.data)
        assert rc == nat.CSS_ERR_INVALID and "weight" in nat.last_error() and name in nat.last_error()
        assert usable()
    for bad, name in ((np.nan, "NaN"), (np.inf, "infinite")):      # a bad prior: the message names the row, nothing is written
        vals = np.full(10, 0.5, np.float32)
        vals[7] = bad
        with pytest.raises(nat.CssError) as e:
            ix.set_priors(vals, row0=100)
        assert e.value.code == nat.CSS_ERR_INVALID and "row 107" in str(e.value) and name in str(e.value)
        assert np.array_equal(ix.get_priors().view(np.uint32), p.view(np.uint32)), "a refused set_priors changed the column"
        assert usable()
    with pytest.raises(ValueError):
        ix.set_priors(p[:10], row0=n - 5)
    with pytest.raises(ValueError):
        ix.get_priors(n - 5, 10)
    for fn, args in ((nat.lib().css_index_set_priors, (n - 5, 10, p.ctypes.data)), (nat.lib().css_index_set_priors, (-1, 2, p.ctypes.data)),
                     (nat.lib().css_index_get_priors, (n - 5, 10, np.empty(10, np.float32).ctypes.data))):
        assert fn(ix._handle(), *args) == nat.CSS_ERR_INVALID and "outside" in nat.last_error()
    assert np.array_equal(ix.get_priors().view(np.uint32), p.view(np.uint32))
    with pytest.raises(ValueError):
        ix.set_priors(np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError):
        ix.search_prior(np.zeros((2, d + 1), np.float32), 5, 0.1)          # wrong query width
    assert usable()
    D, I, S = ix.search_prior(np.zeros((0, d), np.float32), 5, 0.1)         # nq = 0
    assert D.shape == I.shape == S.shape == (0, 5)
    ix.close()
    with pytest.raises(RuntimeError, match="freed"):
        ix.search_prior(x[:1], 5, 0.1)
    with pytest.raises(RuntimeError, match="freed"):
        ix.search_prior(np.zeros((0, d), np.float32), 5, 0.1)
    with pytest.raises(RuntimeError, match="freed"):
        ix.get_priors()
    for metric, pad in ((0, -FMAX), (1, FMAX)):                             # an empty index: padded rows
        empty = _index(d, metric)
        D, I, S = empty.search_prior(x[:3], 4, 0.5)
        assert (I == -1).all() and (D == np.float32(pad)).all() and (S == np.float32(pad)).all()
        empty.close()

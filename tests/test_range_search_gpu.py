"""GPU: ``IndexFlat.range_search`` (``css_index_range_search``, kernel ``k_range_small``).

Truth is computed here in fp64 with numpy from the very fp32 rows and queries handed to the index
(``oracle.knn_oracle.synth_rows`` + ``normalize_rows``); the code under test is never its own reference.

Comparison rule.  The kernel forms every score as a recursive fp32 sum of ``dpad`` fused multiply-adds.  For a
recursive sum of n terms ``|fl(sum) - sum| <= n u sum|t_i|`` with ``u = 2^-24`` (Higham, Accuracy and Stability of
Numerical Algorithms, eq. 3.5 to first order; an fma rounds each step once), and ``sum |x_i q_i| <= ||x|| ||q||``
(Cauchy-Schwarz), so

    band_IP = dpad * 2^-24 * ||x|| * ||q||                       (4.6e-5 for unit rows of 768)

For L2 every difference ``x_i - q_i`` carries one rounding (relative u, 2u after squaring), the sum adds n u:
``(n + 2) u sum (x_i - q_i)^2 <= (n + 2) u (||x|| + ||q||)^2 <= 4 (n + 2) u max(||x||^2, ||q||^2)``.  The kernel's chains
are dpad / 16 + 4 additions deep, not dpad, which covers the ``+ 2`` many times over:

    band_L2 = 4 * dpad * 2^-24 * max(||x||^2, ||q||^2)           (1.8e-4 for unit rows of 768)

Rows whose fp64 score lies strictly outside ``radius +- band`` must be in / out exactly as fp64 says; rows inside the
band may go either way.  For every returned pair ``|D - fp64 score| <= band`` and ``D`` itself satisfies the strict
predicate against the float32 radius.  Per query: ids unique, never -1, order = (score best first, id ascending) on the
returned floats, ``lims`` consistent.  So that the band cannot hide a failure, every case asserts on the fp64 side that
the rows inside the band are at most 5 % of the fp64 hit count (at most 5 rows where a case has fewer than 100 hits).

Cases and pruning.  metric x dim x nq x radius is NOT pruned: all of {IP, L2} x {64, 100, 384, 768} x {1, 3, 16, 17,
100} x three radii run at n = 100 000 (one index and one fp64 score matrix per metric and dim).  The radii are those of
the issue at 768 (IP 0.08 / 0.10 / 0.12, L2 1.84 / 1.80 / 1.76 = 2 - 2 IP) and scale with sqrt(768 / d) for the other
dims, which keeps the hit fraction (a few sigma of the score distribution of unit vectors).  Masks, id base, shadow
policies, removal / growth, normalisation and errors run at one shape each (IP and L2 where the metric matters):
they do not interact with the arithmetic of the sweep, which the full grid covers.
"""
import json
from pathlib import Path

import numpy as np
import pytest

from oracle import knn_oracle as ko

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GOLD = Path(__file__).resolve().parent / "golden"
POLICIES = {"off": False, "bf16": True, "int8": "int8", "auto": None}


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


def _check(res, S, band, radius, metric, what, allowed=None, id_base=0):
    """``res`` = (lims, D, I) against fp64 scores S [nq, n] by the rule of the module docstring.  Returns
    (fp64 hits, rows inside the band) for the caller's cap."""
    lims, D, I = res
    nq, n = S.shape
    r = float(np.float32(radius))
    assert lims.dtype == np.int64 and D.dtype == np.float32 and I.dtype == np.int64, what
    assert lims.shape == (nq + 1,) and lims[0] == 0 and (np.diff(lims) >= 0).all(), what
    assert lims[nq] == D.shape[0] == I.shape[0], what
    ok = np.ones(n, bool) if allowed is None else np.asarray(allowed, bool)
    hits = in_band = 0
    for j in range(nq):
        d, i = D[lims[j]:lims[j + 1]], I[lims[j]:lims[j + 1]] - id_base
        w = f"{what} query {j}"
        assert ((i >= 0) & (i < n)).all(), f"{w}: ids outside [0, n)"
        got = np.zeros(n, bool)
        got[i] = True
        assert got.sum() == i.shape[0], f"{w}: repeated ids"
        if metric == 0:
            sure, maybe = S[j] > r + band[j], S[j] >= r - band[j]
            assert (d > np.float32(radius)).all(), f"{w}: a returned score does not exceed the radius"
            step = np.diff(d.astype(np.float64))
            assert (step <= 0).all(), f"{w}: scores not descending"
            truth = S[j] > r
        else:
            sure, maybe = S[j] < r - band[j], S[j] <= r + band[j]
            assert (d < np.float32(radius)).all() and (d >= 0).all(), f"{w}: a returned distance is not inside the radius"
            step = np.diff(d.astype(np.float64))
            assert (step >= 0).all(), f"{w}: distances not ascending"
            truth = S[j] < r
        assert (np.diff(i)[step == 0] > 0).all(), f"{w}: equal scores not by ascending id"
        assert not (sure & ok & ~got).any(), f"{w}: {int((sure & ok & ~got).sum())} rows clearly inside the radius are missing"
        assert not (got & ~(maybe & ok)).any(), f"{w}: {int((got & ~(maybe & ok)).sum())} rows clearly outside (or masked) returned"
        err = np.abs(d.astype(np.float64) - S[j, i])
        assert (err <= band[j, i]).all(), f"{w}: score error {err.max():.3e} beyond the band {band[j, i].min():.3e}"
        hits += int((truth & ok).sum())
        in_band += int((maybe & ~sure & ok).sum())
    return hits, in_band


def _assert_cap(hits, in_band, what):
    print(f"{what}: {hits} fp64 hits, {in_band} rows inside the band")
    if hits < 100:
        assert in_band <= 5, f"{what}: {in_band} rows inside the band with {hits} hits"
    else:
        assert in_band <= 0.05 * hits, f"{what}: {in_band} rows inside the band are more than 5 % of {hits} hits"


def _index(d, metric, x=None, policy="auto"):
    from claude_semantic_search_amd.flat_index import IndexFlat

    ix = IndexFlat(d, metric)
    ix.set_shadow(POLICIES[policy])
    if x is not None and x.shape[0]:
        ix.add(x)
    return ix


def _radii(metric, d):
    ip = [r * np.sqrt(768.0 / d) for r in (0.08, 0.10, 0.12)]
    return ip if metric == 0 else [2.0 - 2.0 * r for r in ip]


def _same(a, b, what):
    for u, v, name in zip(a, b, ("lims", "D", "I")):
        assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u.view(np.uint8), v.view(np.uint8)), \
            f"{what}: {name} differs"


# ------------------------------------------------------------------ case 3 (first: the pool is at its initial size)
@pytest.mark.parametrize("metric", [0, 1])
def test_nothing_hits_and_everything_hits_on_a_fresh_index(metric):
    n, d, nq = 50000, 768, 4
    x = _rows(n, d, 3)
    q = _queries(x, nq, 31)
    q[0] = x[123]                                          # equal to a row: L2 distance exactly 0
    ix = _index(d, metric, x)
    S, band = _truth(x, q, metric)
    none_r, all_r = (2.0, -2.0) if metric == 0 else (0.0, 5.0)
    # everything hits: 50 000 hits per query against an initial pool of a few thousand -> the one re-sweep
    res = ix.range_search(q, all_r)
    assert np.array_equal(np.diff(res[0]), [n] * nq)
    _check(res, S, band, all_r, metric, f"everything hits metric={metric}")
    # nothing hits; for L2 the row equal to the query has distance 0, and 0 < 0 is false (strictness)
    lims, D, I = ix.range_search(q, none_r)
    assert np.array_equal(lims, np.zeros(nq + 1, np.int64)) and D.shape == (0,) and I.shape == (0,)
    # ... while the smallest positive radius returns exactly that row for that query
    if metric == 1:
        lims, D, I = ix.range_search(q[:1], float(np.nextafter(np.float32(0), np.float32(1))))
        assert lims.tolist() == [0, 1] and I.tolist() == [123] and D.tolist() == [0.0]
    _same(ix.range_search(q, all_r), res, "second call with the grown pool")
    # no queries, and an empty index
    lims, D, I = ix.range_search(np.zeros((0, d), np.float32), all_r)
    assert lims.tolist() == [0] and D.shape == (0,) and I.shape == (0,)
    ix.close()
    empty = _index(d, metric)
    lims, D, I = empty.range_search(q, all_r)
    assert np.array_equal(lims, np.zeros(nq + 1, np.int64)) and D.shape == (0,) and I.shape == (0,)
    empty.close()


# ------------------------------------------------------------------ case 1
@pytest.mark.parametrize("d", [64, 100, 384, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_every_metric_dim_query_count_and_radius(metric, d):
    n = 100000
    x = _rows(n, d, 11)
    q = _queries(x, 100, 12)
    S, band = _truth(x, q, metric)
    ix = _index(d, metric, x)
    for radius in _radii(metric, d):
        for nq in (1, 3, 16, 17, 100):
            what = f"metric={metric} d={d} nq={nq} radius={radius:.4f}"
            res = ix.range_search(q[:nq], radius)
            hits, in_band = _check(res, S[:nq], band[:nq], radius, metric, what)
            _assert_cap(hits, in_band, what)
            assert hits > 0, what
    ix.close()


# ------------------------------------------------------------------ case 2
@pytest.mark.parametrize("metric", [0, 1])
def test_zero_band_radius_returns_exactly_the_fp64_top_10(metric):
    n, d, nq = 100000, 768, 100
    x = _rows(n, d, 11)
    q = _rows(nq, d, 13)
    S, band = _truth(x, q, metric)
    ix = _index(d, metric, x)
    ix.set_search_mode("exact_fp32")
    Dk, Ik = ix.search(q, 10)
    used = 0
    for j in range(nq):
        key = -S[j] if metric == 0 else S[j]
        top = np.lexsort((np.arange(n), key))[:11]
        s10, s11 = S[j, top[9]], S[j, top[10]]
        radius = np.float32((s10 + s11) / 2)
        b = band[j, top].max()
        if not (abs(s10 - float(radius)) > b and abs(float(radius) - s11) > b):
            continue                                       # radius +- band would touch a score: not a zero-band query
        used += 1
        lims, D, I = ix.range_search(q[j], float(radius))
        assert lims.tolist() == [0, 10] and I.tolist() == top[:10].tolist(), f"metric={metric} query {j}"
        assert (np.abs(D.astype(np.float64) - S[j, top[:10]]) <= band[j, top[:10]]).all()
        assert Ik[j].tolist() == I.tolist(), f"metric={metric} query {j}: search(q, 10) disagrees"
        assert (np.abs(Dk[j].astype(np.float64) - D.astype(np.float64)) <= 2 * band[j, top[:10]]).all()   # both within the band of fp64
    print(f"metric={metric}: {used} of {nq} queries have a zero-band radius")
    assert used >= nq // 2
    ix.close()


# ------------------------------------------------------------------ case 4
@pytest.mark.parametrize("metric", [0, 1])
def test_allow_masks_and_id_base(metric):
    n, d, nq = 60001, 384, 9
    x = _rows(n, d, 5)
    q = _queries(x, nq, 51)
    S, band = _truth(x, q, metric)
    radius = _radii(metric, d)[0]
    ix = _index(d, metric, x)
    rng = np.random.default_rng(6)
    half = rng.random(n) < 0.5
    res = ix.range_search(q, radius, allow=half)
    hits, in_band = _check(res, S, band, radius, metric, "random 50 % mask", allowed=half)
    _assert_cap(hits, in_band, f"random 50 % mask metric={metric}")
    assert hits > 100
    lims, D, I = ix.range_search(q, radius, allow=np.zeros(n, bool))
    assert lims[-1] == 0 and D.shape == (0,) and I.shape == (0,)
    one = np.zeros(n, bool)
    one[n - 1] = True
    everything = -2.0 if metric == 0 else 5.0
    lims, D, I = ix.range_search(q, everything, allow=one)
    assert np.array_equal(np.diff(lims), [1] * nq) and (I == n - 1).all()
    _check((lims, D, I), S, band, everything, metric, "one-row mask", allowed=one)
    ix.set_id_base(10 ** 9)
    based = ix.range_search(q, radius, allow=half)
    assert np.array_equal(based[0], res[0]) and np.array_equal(based[1], res[1]) and np.array_equal(based[2], res[2] + 10 ** 9)
    _check(ix.range_search(q, radius), S, band, radius, metric, "id base", id_base=10 ** 9)
    with pytest.raises(ValueError):
        ix.range_search(q, radius, allow=np.ones(n - 1, bool))
    ix.close()


# ------------------------------------------------------------------ case 5
@pytest.mark.parametrize("metric", [0, 1])
def test_result_does_not_depend_on_the_shadow_policy(metric):
    n, d, nq = 50000, 768, 17
    x = _rows(n, d, 7)
    q = _queries(x, nq, 71)
    radius = _radii(metric, d)[1]
    first = None
    for policy in POLICIES:
        ix = _index(d, metric, x, policy)
        for mode in ("auto", "exact_fp32", "coarse"):       # nor on the search mode
            ix.set_search_mode(mode)
            res = ix.range_search(q, radius)
            if first is None:
                first = res
                S, band = _truth(x, q, metric)
                hits, in_band = _check(res, S, band, radius, metric, f"shadow={policy}")
                _assert_cap(hits, in_band, f"shadow policies metric={metric}")
            _same(res, first, f"metric={metric} shadow={policy} mode={mode}")
        ix.close()


# ------------------------------------------------------------------ case 6
@pytest.mark.parametrize("metric", [0, 1])
def test_after_remove_ids_and_capacity_growth_equals_a_fresh_index(metric):
    n, d, nq = 40000, 768, 16
    x = _rows(n, d, 8)
    q = _queries(x, nq, 81)
    radius = _radii(metric, d)[0]
    ix = _index(d, metric)
    for r0 in range(0, n, 7000):                            # incremental adds: the capacity grows several times
        ix.add(x[r0:r0 + 7000])
        if r0 == 14000:
            ix.range_search(q, radius)                      # (a range search between two growths)
    fresh = _index(d, metric, x)
    S, band = _truth(x, q, metric)
    res = ix.range_search(q, radius)
    hits, in_band = _check(res, S, band, radius, metric, "after growth")
    _assert_cap(hits, in_band, f"after growth metric={metric}")
    _same(res, fresh.range_search(q, radius), "after capacity growth")
    fresh.close()
    gone = np.flatnonzero(np.random.default_rng(9).random(n) < 0.10)
    assert ix.remove_ids(gone) == gone.shape[0]
    surv = np.delete(x, gone, 0)
    fresh = _index(d, metric, surv)
    res = ix.range_search(q, radius)
    S, band = _truth(surv, q, metric)
    _check(res, S, band, radius, metric, "after remove_ids")
    _same(res, fresh.range_search(q, radius), "after remove_ids")
    ix.close()
    fresh.close()


# ------------------------------------------------------------------ case 7
def test_normalize_queries_on_the_device():
    n, d, nq = 30000, 768, 5
    x = _rows(n, d, 14)
    raw = (ko.synth_rows(nq, d, 15) * np.float32(3.7)).astype(np.float32)
    qn = ko.normalize_rows(raw)                             # q / (||q|| + 1e-8) in fp32, as the reference forms it
    S, band = _truth(x, qn, 0)
    ix = _index(d, 0, x)
    radius = 0.08
    res = ix.range_search(raw, radius, normalize=True)
    hits, in_band = _check(res, S, band, radius, 0, "normalize=True")
    _assert_cap(hits, in_band, "normalize=True")
    assert hits > 100
    ix.close()


# ------------------------------------------------------------------ case 8
@pytest.mark.parametrize("case", json.loads((GOLD / "knn_reference_cases.json").read_text())["cases"], ids=lambda c: c["name"])
def test_reference_known_answers(case):
    from claude_semantic_search_amd.flat_index import IndexFlatIP

    ix = IndexFlatIP(4)
    ix.add(np.array(case["rows"], np.float32), normalize=True)
    ids, sims = case["expected_ids"], case["expected_sims"]
    cuts = 0
    for c in range(1, len(ids)):
        if sims[c - 1] - sims[c] < 1e-4:
            continue
        cuts += 1
        lims, D, I = ix.range_search(np.array(case["query"], np.float32), (sims[c - 1] + sims[c]) / 2, normalize=True)
        assert lims.tolist() == [0, c] and I.tolist() == ids[:c]
        assert np.allclose(D, sims[:c], atol=1e-6)
    assert cuts > 0
    lims, D, I = ix.range_search(np.array(case["query"], np.float32), -2.0, normalize=True)
    assert I.tolist() == ids and np.allclose(D, sims, atol=1e-6)
    ix.close()


# ------------------------------------------------------------------ case 9
def test_errors():
    from claude_semantic_search_amd import _native as nat

    d = 64
    x = _rows(1000, d, 16)
    ix = _index(d, 0, x)
    with pytest.raises(nat.CssError) as e:
        ix.range_search(x[:2], float("nan"))
    assert e.value.code == nat.CSS_ERR_INVALID and "NaN" in str(e.value)
    with pytest.raises(ValueError):
        ix.range_search(np.zeros((2, d + 1), np.float32), 0.5)
    assert ix.range_search(x[:1], 0.999)[2].tolist() == [0]              # still usable after the errors
    assert ix.range_search(x[:1], float("inf"))[0].tolist() == [0, 0]    # infinite radii are ordinary floats
    assert ix.range_search(x[:1], float("-inf"))[0].tolist() == [0, 1000]
    ix.close()
    with pytest.raises(RuntimeError, match="freed"):
        ix.range_search(x[:1], 0.5)

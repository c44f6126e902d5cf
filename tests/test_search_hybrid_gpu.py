"""GPU: ``IndexFlat.set_terms`` / ``get_terms`` / ``term_stats`` / ``search_hybrid`` (``css_index_search_hybrid``; kernels
``k_lex_scores``, ``k_lex_df_add``, ``k_lex_len_add``, ``k_lex_move``, ``k_lex_stats``, ``k_lex_gather`` in front of and
behind ``k_scan_prior``).

Truth is computed here with numpy from the very fp32 rows, queries and weights handed to the index; the code under test
is never its own reference.  Rows, queries, bands, the fp64 ranking and the count of exempt slots are those of
``tests/test_search_prior_gpu.py`` (imported, so the fp64 rows are shared); the term lists come from
``synth.term_lists`` and their numpy statements from ``tests/lexical_fakes.py``.

    lex64   the BM25 column in float64 from the float32 weights and constants of the call
    lex32   the float32 restatement of the device arithmetic, the sum in query-term order
    inner product   F = S64 + alpha * lex64     larger is better
    squared L2      F = S64 - alpha * lex64     smaller is better

Rules.  Ids and order by ``knn_checks.assert_topk_matches(..., tie_eps=1e-6)``; ``|S - S64| <= band``;
``|D - F| <= band + 2^-24 |F| + |alpha| * 2^-21 * lex64`` (the last term: the handful of fp32 roundings of the lexical
sum); ``L == lex32[I]`` BIT FOR BIT, 0 in padded slots.  Every case asserts on the fp64 side that the slots exempt from
the id comparison are at most 5 % of the slots and prints the share.

Shapes.  The grid runs {IP, L2} x d {64, 100, 768} x k {1, 10, 128} x alpha {0.5, 2.0} x 24 (query, term set) pairs at
n = 100 003 rows (not a multiple of 4, of 64 or of 256: the last row group, wave and block are partial), one index per
(metric, d).  The list shapes of case 4 are the ones at which ``k_lex_scores`` takes another path: empty rows, a wave
whose 64 rows are all empty, a row longer than many strides of the wave, a saturated count, the largest term id, rows
beyond the lists, 32 query terms, query terms that share a slot of the kernel's term table.
"""
import ctypes
import functools

import numpy as np
import pytest

import knn_checks
import test_search_prior_gpu as tp
from claude_semantic_search_amd import synth
from claude_semantic_search_amd.lexical import bm25_weights
from lexical_fakes import Lists

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N = tp.N
FMAX = tp.FMAX
K1, B = 1.2, 0.75
NPAIR = 24


@functools.lru_cache(maxsize=3)
def _lists(n, seed):
    return Lists(*synth.term_lists(n, seed))


def _weights(ls, terms):
    return bm25_weights(ls.df(terms), ls.n, k1=K1, normalized=True)


def _index(d, metric, x=None, ls=None, policy="auto"):
    ix = tp._index(d, metric, x, policy)
    if ls is not None:
        ix.set_terms((ls.off, ls.tok))
    return ix


def _fused(S64, lex64, alpha, metric):
    a = np.float64(np.float32(alpha))
    return S64 + a * lex64 if metric == 0 else S64 - a * lex64


def _check(res, F, S64, band, lex64, lex32, alpha, k, metric, what, allowed=None, id_base=0):
    """(D, I, S, L) of nq single-query calls, stacked to [nq, k], by the rules of the module docstring.  Returns the
    number of slots exempt from the id comparison."""
    D, I, S, L = res
    nq, n = F.shape
    assert D.dtype == np.float32 and I.dtype == np.int64 and S.dtype == np.float32 and L.dtype == np.float32, what
    assert D.shape == I.shape == S.shape == L.shape == (nq, k), what
    I_ref, V, nxt = tp._topk64(F, k, metric, allowed)
    loc = np.where(I >= 0, I - id_base, -1)
    knn_checks.assert_topk_matches(D, loc, V.astype(np.float32), I_ref, V, what,
                                   D64_next=np.where(np.isnan(nxt), np.inf, nxt), tie_eps=1e-6)
    pad = np.float32(-FMAX if metric == 0 else FMAX)
    for j in range(nq):
        v = loc[j] >= 0
        i = loc[j][v]
        w = f"{what} query {j}"
        assert v[:i.size].all(), f"{w}: a pad in front of a result"
        assert (D[j][~v] == pad).all() and (S[j][~v] == pad).all() and (L[j][~v] == 0.0).all(), f"{w}: padded slots"
        assert ((i >= 0) & (i < n)).all() and np.unique(i).size == i.size, f"{w}: ids repeated or outside [0, n)"
        if allowed is not None:
            assert np.asarray(allowed, bool)[i].all(), f"{w}: a masked row was returned"
        d = D[j][v].astype(np.float64)
        step = np.diff(d)
        assert (step <= 0).all() if metric == 0 else (step >= 0).all(), f"{w}: D not best first"
        assert (np.diff(i)[step == 0] > 0).all(), f"{w}: equal values not by ascending id"
        errD = np.abs(d - F[j, i])
        tol = band[j, i] + U * np.abs(F[j, i]) + abs(alpha) * 2.0 ** -21 * lex64[j, i]
        assert (errD <= tol).all(), f"{w}: fused value error {errD.max():.3e} beyond the band"
        errS = np.abs(S[j][v].astype(np.float64) - S64[j, i])
        assert (errS <= band[j, i]).all(), f"{w}: raw score error {errS.max():.3e} beyond the band"
        assert np.array_equal(L[j][v].view(np.uint32), lex32[j, i].view(np.uint32)), \
            f"{w}: L differs from the float32 restatement in bits (max {np.abs(L[j][v] - lex32[j, i]).max():.3e})"
    return tp._exempt(I_ref, V, nxt)


def _run(ix, q, sets, ws, k, alpha, **kw):
    """One call per (query, term set) pair, stacked."""
    out = [ix.search_hybrid(q[j], sets[j], ws[j], k, alpha, k1=K1, b=B, **kw) for j in range(len(sets))]
    return tuple(np.concatenate([o[c] for o in out]) for c in range(4))


def _same(a, b, what):
    for u, v, name in zip(a, b, ("D", "I", "S", "L")):
        assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u.view(np.uint8), v.view(np.uint8)), \
            f"{what}: {name} differs"


def _columns(ls, sets, ws, avgdl):
    lex32 = np.stack([ls.f32(t, w, K1, B, avgdl) for t, w in zip(sets, ws)])
    lex64 = np.stack([ls.f64(t, w, K1, B, avgdl) for t, w in zip(sets, ws)])
    return lex32, lex64


# ------------------------------------------------------------------ case 1: the grid
@pytest.mark.parametrize("d", [64, 100, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_every_metric_dim_k_and_alpha(metric, d):
    x = tp._rows(N, d, 11)
    q = tp._queries(x, NPAIR, 12)
    ls = _lists(N, 101)
    sets = [synth.query_terms(j) for j in range(NPAIR)]
    ws = [_weights(ls, t) for t in sets]
    lex32, lex64 = _columns(ls, sets, ws, ls.avgdl())
    S64, band = tp._truth(x, q, metric)
    plain10, _, _ = tp._topk64(S64, 10, metric)
    ix = _index(d, metric, x, ls)
    for alpha in (0.5, 2.0):
        F = _fused(S64, lex64, alpha, metric)
        for k in (1, 10, 128):
            what = f"metric={metric} d={d} k={k} alpha={alpha}"
            res = _run(ix, q, sets, ws, k, alpha)           # avgdl=None: total_len / ndocs of the index
            exempt = _check(res, F, S64, band, lex64, lex32, alpha, k, metric, what)
            print(f"{what}: {exempt} of {NPAIR * k} slots exempt from the id comparison ({100.0 * exempt / (NPAIR * k):.2f} %)")
            assert exempt <= 0.05 * NPAIR * k, f"{what}: the tie rule exempts {exempt} of {NPAIR * k} slots"
            if k == 10:
                absent = sum(int((~np.isin(res[1][j], plain10[j])).sum()) for j in range(NPAIR))
                print(f"{what}: {absent} of {NPAIR * k} returned ids are absent from the plain fp64 top-10")
                assert absent >= 0.20 * NPAIR * k, f"{what}: only {absent} of {NPAIR * k} ids differ from the plain top-10"
    ix.close()


# ------------------------------------------------------------------ case 2: identities, in bits
@pytest.mark.parametrize("metric", [0, 1])
def test_identities_with_search_prior(metric):
    d, n = 100, 30011
    x = tp._rows(n, d, 21)
    q = tp._queries(x, 4, 22)
    ls = _lists(n, 102)
    terms = synth.query_terms(0)
    w = _weights(ls, terms)
    plain_ix = tp._index(d, metric, x)
    ix = _index(d, metric, x)
    for k in (10, 128):
        for j in range(4):
            plain = plain_ix.search_prior(q[j:j + 1], k, 0.0)
            for setup, args in (("no lists", (terms, w, k, 0.7)),):
                D, I, S, L = ix.search_hybrid(q[j], *args)
                _same((D, I, S), plain, f"metric={metric} k={k} query {j} {setup}")
                assert np.array_equal(S.view(np.uint32), D.view(np.uint32)) and (L == 0.0).all(), setup
    assert ix.term_stats(terms)[0].tolist() == [0] * len(terms) and ix.term_stats(())[1:] == (n, 0)
    ix.set_terms((ls.off, ls.tok))
    ix.set_priors(tp._priors(n, 23))                      # the stored priors play no part in a hybrid call
    for k in (10, 128):
        for j in range(4):
            plain = plain_ix.search_prior(q[j:j + 1], k, 0.0)
            for setup, args in (("m = 0", ((), (), k, 0.7)), ("alpha = 0", (terms, w, k, 0.0))):
                D, I, S, L = ix.search_hybrid(q[j], *args)
                _same((D, I, S), plain, f"metric={metric} k={k} query {j} {setup}")
                assert np.array_equal(S.view(np.uint32), D.view(np.uint32)) and (L == 0.0).all(), setup
    if metric == 0:
        # a zero query: the fused value IS the lexical value, so the rows come in descending lex (ties: lower row)
        lex32 = ls.f32(terms, w, K1, B, ls.avgdl())
        order = np.lexsort((np.arange(n), -lex32.astype(np.float64)))
        for k in (10, 128):
            D, I, S, L = ix.search_hybrid(np.zeros(d, np.float32), terms, w, k, 1.0, k1=K1, b=B)
            assert np.array_equal(I[0], order[:k]), f"k={k}: not the rows of descending lex"
            assert np.array_equal(D.view(np.uint32), L.view(np.uint32)) and (S == 0.0).all()
            assert np.array_equal(L[0].view(np.uint32), lex32[order[:k]].view(np.uint32))
    plain_ix.close()
    ix.close()


# ------------------------------------------------------------------ case 3: a keyword row far below any over-fetch
@pytest.mark.parametrize("metric", [0, 1])
def test_a_keyword_row_at_plain_rank_50000_comes_first(metric):
    d, k = 768, 10                                        # (at d = 64 the best plain scores exceed any normalised lex)
    x = tp._rows(N, d, 11)
    q = tp._queries(x, 1, 31)
    S64, band = tp._truth(x, q, metric)
    order0 = np.lexsort((np.arange(N), -S64[0] if metric == 0 else S64[0]))
    r = int(order0[50000])
    base = _lists(N, 101)
    key = 4095 + 7
    off = base.off.copy()
    off[r + 1:] += 1
    ls = Lists(off, np.insert(base.tok, base.off[r + 1], np.uint32(key)))
    assert ls.df([key]).tolist() == [1]
    w = _weights(ls, [key])
    ix = _index(d, metric, x, ls)
    res = ix.search_hybrid(q[0], [key], w, k, 1.0, k1=K1, b=B)
    D, I, S, L = res
    assert I[0, 0] == r, f"metric={metric}: the keyword row (plain rank 50000) is not first: {I[0].tolist()}"
    lex32, lex64 = _columns(ls, [[key]], [w], ls.avgdl())
    assert lex32[0, r] > 0.25 and np.count_nonzero(lex32) == 1
    F = _fused(S64, lex64, 1.0, metric)
    _check(res, F, S64, band, lex64, lex32, 1.0, k, metric, f"keyword row metric={metric}")
    I9, V9, nxt9 = tp._topk64(S64, k - 1, metric)
    knn_checks.assert_topk_matches(D[:, 1:], I[:, 1:], V9.astype(np.float32), I9, V9, "plain tail", D64_next=nxt9)
    assert np.array_equal(S[0, 1:].view(np.uint32), D[0, 1:].view(np.uint32)) and (L[0, 1:] == 0.0).all()
    ix.close()


# ------------------------------------------------------------------ case 4: shapes of the lists
def test_shapes_of_the_lists():
    d, n, T = 64, 10007, 6000
    x = tp._rows(n, d, 41)
    q = tp._queries(x, 4, 42)
    rng = np.random.default_rng(43)
    long_terms = rng.choice(1 << 20, size=5000, replace=False).astype(np.int64) + 5000
    rows = [np.floor(4096 * rng.random(int(rng.integers(1, 200))) ** 3).astype(np.int64) for _ in range(T)]
    for r in rng.choice(T, size=300, replace=False):
        rows[int(r)] = np.zeros(0, np.int64)                                   # scattered empty rows
    for r in range(1000, 1200):
        rows[r] = np.zeros(0, np.int64)                                        # a run that covers whole waves
    rows[0] = np.zeros(0, np.int64)
    rows[2500] = rng.permutation(long_terms)                                   # one row of 5000 distinct terms
    rows[2501] = np.full(300, 77, np.int64)                                    # one term 300 times: tf saturates at 255
    rows[2502] = np.array([(1 << 24) - 1, 3, (1 << 24) - 1], np.int64)         # the largest term id
    rows[2503] = np.array([100, 4196, 8292, 4196, 20580], np.int64)            # terms that share their low 12 bits
    rows[T - 1] = np.array([5, 5, 9], np.int64)
    ls_head = Lists(np.concatenate([[0], np.cumsum([len(r) for r in rows])]), np.concatenate(rows))
    full = Lists(np.concatenate([ls_head.off, np.full(n - T, ls_head.off[-1])]), ls_head.tok)   # rows >= T: empty
    ix = tp._index(d, 0, x)
    ix.set_terms(rows[:2500])
    ix.set_terms(rows[2500:])
    off, terms, tfs, dl = ix.get_terms()
    assert off.shape == (n + 1,) and np.array_equal(off, full.poff) and np.array_equal(terms, full.terms)
    assert np.array_equal(tfs, full.tfs) and np.array_equal(dl, full.dl)
    o1, t1, f1, d1 = ix.get_terms(2501, 2)
    assert o1.tolist() == [0, 1, 3] and t1.tolist() == [77, 3, (1 << 24) - 1] and f1.tolist() == [255, 1, 2] and d1.tolist() == [300, 3]
    assert (dl[T:] == 0).all() and off[T] == off[n]
    df, ndocs, total = ix.term_stats([77, (1 << 24) - 1, int(long_terms[0]), 4000000])
    assert df.tolist() == full.df([77, (1 << 24) - 1, int(long_terms[0]), 4000000]).tolist() and df[1] == 1 and df[3] == 0
    assert (ndocs, total) == (n, full.total_len)
    avgdl = full.avgdl()
    S64, band = tp._truth(x, q, 0)
    in_long = [int(t) for t in rows[2500][:32]]
    w_long = (0.001 * 1.23 ** np.arange(32)).astype(np.float32)                # (bm25 weights would all be equal: df = 1)
    queries = {"32 terms of the long row": (in_long, w_long), "the same reversed": (in_long[::-1], w_long[::-1]),
               "saturated": ([77, 5, 9], None), "largest id": ([(1 << 24) - 1, 3], None),
               "mixed": ([int(v) for v in synth.query_terms(3)] + [77, in_long[0]], None),
               "shared low bits": ([8292, 100, 12388, 20580, 4196], np.array([0.11, 0.07, 0.5, 0.03, 0.05], np.float32))}
    assert full.df([12388]).tolist() == [0] and full.df([100])[0] > 1 and full.df([4196, 8292, 20580]).tolist() == [1, 1, 1]
    cols = {}
    for name, (terms_q, w) in queries.items():
        if w is None:
            w = bm25_weights(full.df(terms_q), n, k1=K1, normalized=True)
        lex32, lex64 = _columns(full, [terms_q] * 4, [w] * 4, avgdl)
        cols[name] = lex32[0]
        assert (lex32[0, T:] == 0.0).all() and lex32[0, 1000:1200].max() == 0.0
        for k in (10, 128):
            res = _run(ix, q, [terms_q] * 4, [w] * 4, k, 1.0)
            _check(res, _fused(S64, lex64, 1.0, 0), S64, band, lex64, lex32, 1.0, k, 0, f"{name} k={k}")
        # the whole column through a zero query and a one-row mask: every row's L, in bits
        for r in (0, 1100, 2499, 2500, 2501, 2502, 2503, T - 1, T, n - 1):
            one = np.zeros(n, bool)
            one[r] = True
            D, I, S, L = ix.search_hybrid(np.zeros(d, np.float32), terms_q, w, 1, 1.0, k1=K1, b=B, allow=one)
            assert I[0, 0] == r and L[0, 0].view(np.uint32) == lex32[0, r].view(np.uint32), f"{name}: row {r}"
    assert cols["32 terms of the long row"][2500] > 0.0
    assert cols["32 terms of the long row"][2500].view(np.uint32) != cols["the same reversed"][2500].view(np.uint32), \
        "the order of the query terms must show in the bits of the sum"
    tf255 = np.float32(255.0)
    assert cols["saturated"][2501] > 0.0 and full.tfs[full.poff[2501]] == 255 and tf255 == 255.0
    assert cols["shared low bits"][2503] > 0.2 and np.count_nonzero(cols["shared low bits"]) == full.df([100])[0]
    ix.close()


# ------------------------------------------------------------------ case 5: the lists follow the rows
@pytest.mark.parametrize("metric", [0, 1])
def test_the_lists_follow_the_rows(metric):
    n, d, k, alpha = 40001, 64, 10, 0.5
    x = tp._rows(n, d, 8)
    q = tp._queries(x, 6, 81)
    ls = _lists(n, 103)
    sets = [synth.query_terms(j) for j in range(6)]
    every = np.arange(4096)

    def stats(index):
        df = np.concatenate([index.term_stats(every[c:c + 1024])[0] for c in range(0, 4096, 1024)])
        return df, index.term_stats(())[1:]

    def matches(index, want, nrows, what):
        off, terms, tfs, dl = index.get_terms()
        head = want.n
        assert off.shape == (nrows + 1,) and np.array_equal(off[:head + 1], want.poff) and (off[head:] == want.poff[-1]).all(), what
        assert np.array_equal(terms, want.terms) and np.array_equal(tfs, want.tfs), what
        assert np.array_equal(dl[:head], want.dl) and (dl[head:] == 0).all(), what
        df, (ndocs, total) = stats(index)
        assert np.array_equal(df, want.df(every)) and (ndocs, total) == (nrows, want.total_len), what

    ix = tp._index(d, metric)
    assert ix.get_terms()[0].tolist() == [0] and ix.term_stats([1])[0].tolist() == [0]
    ix.add(x[:7000])
    head = ls.rows(np.arange(5000))
    ix.set_terms((head.off[:3001], head.tok[:head.off[3000]]))                   # in pieces ...
    ix.set_terms((head.off[3000:] - head.off[3000], head.tok[head.off[3000]:]))
    matches(ix, head, 7000, "set_terms in pieces")
    for r0 in range(7000, n, 7000):                                             # the capacity grows several times
        ix.add(x[r0:r0 + 7000])
        matches(ix, head, min(r0 + 7000, n), "capacity growth")
    ix.set_terms((ls.rows(np.arange(5000, 9000)).off, ls.rows(np.arange(5000, 9000)).tok))
    matches(ix, ls.rows(np.arange(9000)), n, "appended lists")
    cut = ls.rows(np.arange(2000, 2500))
    ix.set_terms((cut.off, cut.tok), row0=4000)                                 # row0 < T truncates, then appends
    matches(ix, ls.rows(np.concatenate([np.arange(4000), np.arange(2000, 2500)])), n, "truncating set_terms")
    ix.set_terms([], row0=1000)                                                 # a pure truncation
    matches(ix, ls.rows(np.arange(1000)), n, "pure truncation")
    ix.set_terms((ls.off, ls.tok), row0=0)                                      # the rewrite
    matches(ix, ls, n, "rewrite")
    ws = [_weights(ls, t) for t in sets]
    S64, band = tp._truth(x, q, metric)
    lex32, lex64 = _columns(ls, sets, ws, ls.avgdl())
    _check(_run(ix, q, sets, ws, k, alpha), _fused(S64, lex64, alpha, metric), S64, band, lex64, lex32, alpha, k, metric, "after growth")
    gone = np.flatnonzero(np.random.default_rng(9).random(n) < 0.10)
    keep = np.ones(n, bool)
    keep[gone] = False
    assert ix.remove_ids(gone) == gone.shape[0]
    kept = ls.rows(keep)
    matches(ix, kept, kept.n, "remove_ids")
    fresh = _index(d, metric, x[keep], kept)
    matches(fresh, kept, kept.n, "fresh index")
    wk = [_weights(kept, t) for t in sets]
    for kk in (k, 128):
        _same(_run(ix, q, sets, wk, kk, alpha), _run(fresh, q, sets, wk, kk, alpha), f"after remove_ids k={kk}")
    S64, band = tp._truth(x[keep], q, metric)
    lex32, lex64 = _columns(kept, sets, wk, kept.avgdl())
    _check(_run(ix, q, sets, wk, k, alpha), _fused(S64, lex64, alpha, metric), S64, band, lex64, lex32, alpha, k, metric, "after remove_ids")
    fresh.close()
    ix.add(x[:100])                                                             # slots of removed rows are reused
    matches(ix, kept, kept.n + 100, "rows added after remove_ids have no list")
    tail = ls.rows(np.arange(100))
    ix.set_terms((tail.off, tail.tok))                                          # ... and lists append behind the kept ones
    matches(ix, ls.rows(np.concatenate([np.flatnonzero(keep), np.arange(100)])), kept.n + 100, "append after remove_ids")
    ix.reset()
    ix.add(x[:5000])
    off, terms, tfs, dl = ix.get_terms()
    assert off.tolist() == [0] * 5001 and terms.size == 0 and (dl == 0).all(), "reset must forget the lists"
    df, (ndocs, total) = stats(ix)
    assert not df.any() and (ndocs, total) == (5000, 0), "reset must zero the statistics"
    D, I, S, L = ix.search_hybrid(q[0], sets[0], ws[0], k, alpha)
    assert np.array_equal(D.view(np.uint32), S.view(np.uint32)) and (L == 0.0).all()
    ix.close()


# ------------------------------------------------------------------ case 6: masks and id base
@pytest.mark.parametrize("metric", [0, 1])
def test_allow_masks_and_id_base(metric):
    n, d, nq, k, alpha = 60001, 100, 6, 10, 0.5
    x = tp._rows(n, d, 5)
    q = tp._queries(x, nq, 51)
    ls = _lists(n, 104)
    sets = [synth.query_terms(j) for j in range(nq)]
    ws = [_weights(ls, t) for t in sets]
    S64, band = tp._truth(x, q, metric)
    lex32, lex64 = _columns(ls, sets, ws, ls.avgdl())
    F = _fused(S64, lex64, alpha, metric)
    ix = _index(d, metric, x, ls)
    half = np.random.default_rng(6).random(n) < 0.5
    res = _run(ix, q, sets, ws, k, alpha, allow=half)
    _check(res, F, S64, band, lex64, lex32, alpha, k, metric, "random 50 % mask", allowed=half)
    pad = np.float32(-FMAX if metric == 0 else FMAX)
    D, I, S, L = _run(ix, q, sets, ws, k, alpha, allow=np.zeros(n, bool))
    assert (I == -1).all() and (D == pad).all() and (S == pad).all() and (L == 0.0).all()
    one = np.zeros(n, bool)
    one[n - 1] = True
    D, I, S, L = _run(ix, q, sets, ws, k, alpha, allow=one)
    assert (I[:, 0] == n - 1).all() and (I[:, 1:] == -1).all() and (D[:, 1:] == pad).all() and (L[:, 1:] == 0.0).all()
    _check((D, I, S, L), F, S64, band, lex64, lex32, alpha, k, metric, "one-row mask", allowed=one)
    ix.set_id_base(10 ** 9)
    based = _run(ix, q, sets, ws, k, alpha, allow=half)
    assert all(np.array_equal(based[c], res[c]) for c in (0, 2, 3)) and np.array_equal(based[1], res[1] + 10 ** 9)
    _check(_run(ix, q, sets, ws, k, alpha), F, S64, band, lex64, lex32, alpha, k, metric, "id base", id_base=10 ** 9)
    with pytest.raises(ValueError):
        ix.search_hybrid(q[0], sets[0], ws[0], k, alpha, allow=np.ones(n - 1, bool))
    ix.close()


# ------------------------------------------------------------------ case 7: independence of shadow rows and search mode
@pytest.mark.parametrize("metric", [0, 1])
def test_result_does_not_depend_on_shadow_policy_or_search_mode(metric):
    n, d, nq, k, alpha = 50000, 768, 5, 10, 0.5
    x = tp._rows(n, d, 7)
    q = tp._queries(x, nq, 71)
    ls = _lists(n, 105)
    sets = [synth.query_terms(j) for j in range(nq)]
    ws = [_weights(ls, t) for t in sets]
    first = None
    for policy in tp.POLICIES:
        ix = _index(d, metric, x, ls, policy)
        for mode in ("auto", "exact_fp32", "coarse"):
            ix.set_search_mode(mode)
            res = _run(ix, q, sets, ws, k, alpha)
            if first is None:
                first = res
                S64, band = tp._truth(x, q, metric)
                lex32, lex64 = _columns(ls, sets, ws, ls.avgdl())
                _check(res, _fused(S64, lex64, alpha, metric), S64, band, lex64, lex32, alpha, k, metric, f"shadow={policy}")
            _same(res, first, f"metric={metric} shadow={policy} mode={mode}")
        ix.close()


# ------------------------------------------------------------------ case 8: errors
def test_errors():
    from claude_semantic_search_amd import _native as nat

    d, n = 64, 1000
    x = tp._rows(n, d, 16)
    ls = _lists(n, 106)
    ix = _index(d, 0, x, ls.rows(np.arange(600)))
    lib, h = nat.lib(), ix._handle()
    stored = ix.get_terms()
    terms = np.array([5, 9, 11], np.uint32)
    w = np.array([0.5, 0.25, 0.125], np.float32)

    def usable():
        now = ix.get_terms()
        assert all(np.array_equal(a, b) for a, b in zip(now, stored)), "a refused call changed the lists"
        assert ix.search_hybrid(x[0], terms, w, 1, 0.0)[1].tolist() == [[0]]

    def raw(k=5, alpha=0.5, t=terms, wt=w, m=None, k1=K1, b=B, avgdl=100.0):
        D, I = np.empty(129, np.float32), np.empty(129, np.int64)
        S, L = np.empty(129, np.float32), np.empty(129, np.float32)
        return lib.css_index_search_hybrid(h, x[:1].ctypes.data, k, alpha, t.ctypes.data, wt.ctypes.data, len(t) if m is None else m,
                                           k1, b, avgdl, 0, None, D.ctypes.data, I.ctypes.data, S.ctypes.data, L.ctypes.data)

    for k in (0, 129):
        with pytest.raises(ValueError):
            ix.search_hybrid(x[0], terms, w, k, 0.5)
        assert raw(k=k) == nat.CSS_ERR_INVALID and f"k={k}" in nat.last_error()
        usable()
    t33, w33 = np.arange(33, dtype=np.uint32), np.zeros(33, np.float32)
    with pytest.raises(ValueError):
        ix.search_hybrid(x[0], t33, w33, 5, 0.5)
    assert raw(t=t33, wt=w33) == nat.CSS_ERR_INVALID and "m=33" in nat.last_error()
    rep = np.array([5, 9, 5], np.uint32)
    with pytest.raises(ValueError, match="repeated"):
        ix.search_hybrid(x[0], rep, w, 5, 0.5)
    assert raw(t=rep) == nat.CSS_ERR_INVALID and "term 5 is repeated" in nat.last_error()
    big = np.array([1 << 24], np.uint32)
    assert raw(t=big, wt=w[:1]) == nat.CSS_ERR_INVALID and "2^24" in nat.last_error()
    usable()
    for bad, name in ((float("nan"), "NaN"), (float("inf"), "infinite"), (float("-inf"), "infinite")):
        for arg in ("alpha", "k1", "b", "avgdl"):
            with pytest.raises(ValueError):
                ix.search_hybrid(x[0], terms, w, 5, **{"alpha": 0.5, arg: bad})
            assert raw(**{arg: bad}) == nat.CSS_ERR_INVALID and arg in nat.last_error() and name in nat.last_error(), (arg, bad)
        wb = w.copy()
        wb[1] = bad
        with pytest.raises(ValueError):
            ix.search_hybrid(x[0], terms, wb, 5, 0.5)
        assert raw(wt=wb) == nat.CSS_ERR_INVALID and "weight of term 9" in nat.last_error() and name in nat.last_error()
        usable()
    for arg, bad in (("avgdl", 0.0), ("avgdl", -1.0), ("b", 1.5), ("b", -0.1), ("k1", -1.0)):
        with pytest.raises(ValueError):
            ix.search_hybrid(x[0], terms, w, 5, **{"alpha": 0.5, arg: bad})
        assert raw(**{arg: bad}) == nat.CSS_ERR_INVALID and arg in nat.last_error(), (arg, bad)
    usable()
    with pytest.raises(ValueError):
        ix.search_hybrid(x[:2], terms, w, 5, 0.5)                              # one query per call
    with pytest.raises(ValueError):
        ix.search_hybrid(np.zeros(d + 1, np.float32), terms, w, 5, 0.5)

    # set_terms: everything is checked before anything is written
    def set_raw(row0, off, tok):
        off, tok = np.asarray(off, np.int64), np.asarray(tok, np.uint32)
        return lib.css_index_set_terms(h, row0, off.shape[0] - 1, off.ctypes.data, tok.ctypes.data)

    with pytest.raises(ValueError, match="row 1"):
        ix.set_terms([[1, 2], [3, 1 << 24]])
    assert set_raw(600, [0, 2, 4], [1, 2, 3, 1 << 24]) == nat.CSS_ERR_INVALID and "row 601" in nat.last_error()
    assert set_raw(600, [0, 3, 2], [1, 2, 3]) == nat.CSS_ERR_INVALID and "decrease" in nat.last_error()
    assert set_raw(600, [1, 2], [1, 2]) == nat.CSS_ERR_INVALID and "start" in nat.last_error()
    assert set_raw(601, [0, 1], [1]) == nat.CSS_ERR_INVALID and "append-only" in nat.last_error()      # row0 > T
    assert set_raw(999, [0, 1, 2], [1, 2]) == nat.CSS_ERR_INVALID and "outside" in nat.last_error()    # beyond ntotal
    assert set_raw(-1, [0, 1], [1]) == nat.CSS_ERR_INVALID
    with pytest.raises(nat.CssError):
        ix.set_terms([[1]], row0=601)
    with pytest.raises(nat.CssError):
        ix.set_terms([[1]] * 401)                                               # 600 + 401 rows > ntotal
    with pytest.raises(nat.CssError):
        ix.set_terms((np.array([0, 2, 1]), np.array([1, 2], np.uint32)), row0=600)
    with pytest.raises(ValueError):
        ix.get_terms(990, 20)
    o = np.zeros(21, np.int64)
    assert lib.css_index_get_terms(h, 990, 20, o.ctypes.data, None, None) == nat.CSS_ERR_INVALID and "outside" in nat.last_error()
    with pytest.raises(ValueError):
        ix.term_stats([1 << 24])
    n64, t64 = ctypes.c_int64(0), ctypes.c_int64(0)
    df = np.zeros(1, np.int64)
    assert lib.css_index_term_stats(h, big.ctypes.data, 1, df.ctypes.data, ctypes.byref(n64), ctypes.byref(t64)) == nat.CSS_ERR_INVALID
    usable()
    ix.close()
    for call in (lambda: ix.search_hybrid(x[0], terms, w, 5, 0.5), lambda: ix.set_terms([[1]]), lambda: ix.get_terms(0, 0),
                 lambda: ix.term_stats([1])):
        with pytest.raises(RuntimeError, match="freed"):
            call()
    for metric, pad in ((0, -FMAX), (1, FMAX)):                                 # an empty index: padded rows
        empty = tp._index(d, metric)
        D, I, S, L = empty.search_hybrid(x[0], terms, w, 4, 0.5)
        assert (I == -1).all() and (D == np.float32(pad)).all() and (S == np.float32(pad)).all() and (L == 0.0).all()
        assert D.shape == (1, 4)
        empty.close()

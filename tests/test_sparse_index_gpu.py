"""GPU: sparse vectors on the flat index -- ``IndexFlat.set_sparse`` / ``get_sparse`` / ``sparse_rows`` /
``search_sparse`` / ``search_hybrid_sparse`` (``css_index_set_sparse`` ...; kernels ``k_sparse_scores`` in its two
instantiations, ``k_sparse_move``, ``k_sparse_topk`` and the part merge behind it, ``k_scan_prior`` for the hybrid).

Truth is numpy on the very arrays handed to the index (``tests/sparse_fakes.py``), never the code under test; the
inputs are those of ``tests/sparse_cases.py``, which ``tests/test_sparse_index_host.py`` proves binding on the CPU.

    sp32    the float32 restatement of the column, the sum in query-term order: D and L equal it BIT FOR BIT
    sp64    the same sum in float64 (the lattice cases: sp32 == sp64 exactly)

Pure search: ``I == lexsort((id, -sp32))`` over the hit rows, no tolerance and no exempt slots.  Hybrid: the rules of
``tests/test_search_hybrid_gpu.py`` with the last tolerance term ``|alpha| (m + 1) 2^-24 sum_j |w_j d_j|``, the
first-order bound of m rounded products summed recursively, taken from float64.  n = 20 003 rows (not a multiple of 64
or of 256), vocabulary 4096."""
import numpy as np
import pytest

import knn_checks
import sparse_cases as sc
import test_search_prior_gpu as tp
from claude_semantic_search_amd import synth
from sparse_fakes import Vectors, topk, topk_slice

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N = sc.N
FMAX = tp.FMAX
D_PURE = 64


def _index(vs=None, d=D_PURE, metric=0, x=None):
    ix = tp._index(d, metric, tp._rows(N, d, 11) if x is None else x)
    if vs is not None:
        ix.set_sparse(vs.csr)
    return ix


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b, what):
    for j, (u, v) in enumerate(zip(a, b)):
        assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(_bits(u), _bits(v)), f"{what}: array {j} differs"


def _shuffled(vs, seed):
    """The same vectors with the entries of every row in random order, as CSR."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(vs.n), np.diff(vs.off))
    order = np.lexsort((rng.random(rows.shape[0]), rows))
    return vs.off, vs.terms[order], vs.w[order]


def _matches(ix, want, nrows, what):
    off, terms, w = ix.get_sparse()
    assert off.shape == (nrows + 1,) and np.array_equal(off[:want.n + 1], want.off) and (off[want.n:] == want.off[-1]).all(), what
    assert terms.dtype == np.uint32 and w.dtype == np.float32, what
    assert np.array_equal(terms, want.terms) and np.array_equal(_bits(w), _bits(want.w)), what
    assert ix.sparse_rows == want.n, what


def _check_pure(res, sp32, hit, k, what, allowed=None, id_base=0):
    D, I = res
    Dw, Iw = topk(sp32, hit, k, allowed, id_base)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == I.shape == (1, k), what
    assert np.array_equal(I, Iw), f"{what}: ids differ from lexsort((id, -sp32)) over the hit rows: {I[0][:8]} vs {Iw[0][:8]}"
    assert np.array_equal(_bits(D), _bits(Dw)), f"{what}: D differs from the float32 restatement in bits"
    return int((I >= 0).sum())


# ------------------------------------------------------------------ storage: the vectors follow the rows
def test_vectors_round_trip_append_rewrite_grow_and_reset():
    x = tp._rows(N, D_PURE, 11)
    vs = sc.vectors(201)
    ls = synth.term_lists(N, 101)
    ix = tp._index(D_PURE, 0)
    assert ix.sparse_rows == 0 and ix.get_sparse()[0].tolist() == [0]
    ix.add(x[:7000])
    assert ix.sparse_rows == 0 and not ix.get_sparse()[0].any() and ix.get_sparse()[1].size == 0
    ix.set_terms((ls[0][:7001], ls[1][:ls[0][7000]]))                            # BM25 lists on the same index
    terms_before = ix.get_terms()
    head = vs.rows(np.arange(5000))
    off, t, w = _shuffled(head, 1)                                              # entries in any order: the library sorts
    ix.set_sparse((off[:3001].copy(), t[:off[3000]], w[:off[3000]]))            # in two pieces ...
    ix.set_sparse((off[3000:] - off[3000], t[off[3000]:], w[off[3000]:]))
    _matches(ix, head, 7000, "append in two pieces")
    one = _index(head, x=x[:7000])                                              # ... equals one call
    _same(ix.get_sparse(), one.get_sparse(), "two pieces against one call")
    one.close()
    o1, t1, w1 = ix.get_sparse(4999, 3)                                         # a range across the end of the vectors
    assert o1.tolist() == [0, int(head.off[5000] - head.off[4999])] + [int(head.off[5000] - head.off[4999])] * 2
    assert np.array_equal(t1, head.terms[head.off[4999]:]) and np.array_equal(w1, head.w[head.off[4999]:])
    for r0 in range(7000, N, 7000):                                             # the capacity grows several times
        ix.add(x[r0:r0 + 7000])
        _matches(ix, head, min(r0 + 7000, N), "capacity growth")
    ix.set_sparse(vs.rows(np.arange(5000, 9000)).csr)
    _matches(ix, vs.rows(np.arange(9000)), N, "appended vectors")
    ix.set_sparse(vs.rows(np.arange(2000, 2500)).csr, row0=4000)                # row0 < T drops, then appends
    _matches(ix, vs.rows(np.concatenate([np.arange(4000), np.arange(2000, 2500)])), N, "row0 < T")
    ix.set_sparse([], row0=1000)                                                # a pure truncation
    _matches(ix, vs.rows(np.arange(1000)), N, "pure truncation")
    ix.set_sparse(_shuffled(vs, 2), row0=0)                                     # the rewrite
    _matches(ix, vs, N, "rewrite")
    # the term lists never noticed, and the other way round
    now = ix.get_terms()
    assert np.array_equal(now[0][:7001], terms_before[0]) and np.array_equal(now[1], terms_before[1])
    assert np.array_equal(now[2], terms_before[2]) and np.array_equal(now[3][:7000], terms_before[3])
    ix.set_terms((ls[0], ls[1]), row0=0)
    _matches(ix, vs, N, "after set_terms")
    t_q, w_q = sc.query(4, 4)
    sp32, hit = vs.f32(t_q, w_q)
    _check_pure(ix.search_sparse(t_q, w_q, 10), sp32, hit, 10, "after growth and rewrite")
    ix.reset()
    ix.add(x[:5000])
    assert ix.sparse_rows == 0 and not ix.get_sparse()[0].any(), "reset must forget the vectors"
    D, I = ix.search_sparse(t_q, w_q, 10)
    assert (I == -1).all() and (D == np.float32(-FMAX)).all()
    ix.close()


def test_remove_ids_compacts_the_vectors_with_the_rows():
    x = tp._rows(N, D_PURE, 11)
    vs = sc.vectors(201)
    ix = _index(vs.rows(np.arange(15000)))                                      # rows 15 000 .. have no vector
    gone = np.flatnonzero(np.random.default_rng(9).random(N) < 1.0 / 3.0)       # a scattered third
    keep = np.ones(N, bool)
    keep[gone] = False
    assert ix.remove_ids(gone) == gone.shape[0]
    kept = vs.rows(np.flatnonzero(keep[:15000]))
    nk = int(keep.sum())
    _matches(ix, kept, nk, "remove_ids")
    fresh = _index(kept, x=x[keep])
    _same(ix.get_sparse(), fresh.get_sparse(), "get_sparse after remove_ids against a fresh index")
    full = kept.padded(nk)
    for name, (t, w) in sc.pure_queries(vs).items():
        sp32, hit = full.f32(t, w)
        for k in sc.KS:
            res = ix.search_sparse(t, w, k)
            _same(res, fresh.search_sparse(t, w, k), f"search_sparse after remove_ids, {name} k={k}")
            _check_pure(res, sp32, hit, k, f"after remove_ids, {name} k={k}")
    fresh.close()
    ix.add(x[:100])                                                             # rows added later have none
    _matches(ix, kept, nk + 100, "rows added after remove_ids")
    ix.remove_ids(np.arange(nk + 100))                                          # emptied: as reset
    assert ix.ntotal == 0 and ix.sparse_rows == 0
    ix.close()


# ------------------------------------------------------------------ pure search
def test_pure_search_is_the_float32_column_and_one_lexsort():
    vs = sc.vectors(201)
    half = sc.half_mask()
    ix = _index(vs)
    answers = {"full": 0, "short": 0, "none": 0}
    for name, (t, w) in sc.pure_queries(vs).items():
        sp32, hit = vs.f32(t, w)
        for k in sc.KS:
            for mask in (None, half):
                got = _check_pure(ix.search_sparse(t, w, k, allow=mask), sp32, hit, k, f"{name} k={k} mask={mask is not None}", mask)
                answers["full" if got == k else "none" if got == 0 else "short"] += 1
    assert min(answers.values()) >= 1, answers
    D, I = ix.search_sparse((), (), 5)                                          # m = 0: nothing can hit
    assert (I == -1).all() and (D == np.float32(-FMAX)).all() and D.shape == (1, 5)
    D, I = ix.search_sparse(*sc.query(4, 4), 10, allow=np.zeros(N, bool))
    assert (I == -1).all() and (D == np.float32(-FMAX)).all()
    ix.set_id_base(sc.ID_BASE)
    for m in (4, 33):
        t, w = sc.query(m, m)
        sp32, hit = vs.f32(t, w)
        _check_pure(ix.search_sparse(t, w, 10, allow=half), sp32, hit, 10, f"id base m={m}", half, sc.ID_BASE)
    with pytest.raises(ValueError):
        ix.search_sparse(*sc.query(4, 4), 10, allow=np.ones(N - 1, bool))
    ix.close()
    for metric in (0, 1):                                                       # larger is better on either metric
        ix = _index(vs, metric=metric)
        t, w = sc.query(32, 32)
        sp32, hit = vs.f32(t, w)
        _check_pure(ix.search_sparse(t, w, 128), sp32, hit, 128, f"metric={metric}")
        ix.close()
    empty = tp._index(D_PURE, 1)
    D, I = empty.search_sparse([3], [1.0], 4)
    assert (I == -1).all() and (D == np.float32(-FMAX)).all()
    empty.close()


def test_list_shapes_at_which_the_kernel_takes_another_path():
    vs, queries = sc.shapes()
    ix = _index()
    ix.set_sparse(vs.rows(np.arange(sc.SHAPES_T)).csr)                          # rows beyond T have none
    assert ix.sparse_rows == sc.SHAPES_T
    _matches(ix, vs.rows(np.arange(sc.SHAPES_T)), N, "shapes")
    for name, (t, w) in queries.items():
        sp32, hit = vs.f32(t, w)
        for k in sc.KS:
            _check_pure(ix.search_sparse(t, w, k), sp32, hit, k, f"{name} k={k}")
        # the column row by row through a one-row mask: the row's sp in bits, or no answer where it is no hit
        for r in (0, 1100, sc.LONG_ROW, sc.MAXTERM_ROW, sc.ALL64_ROW, sc.CHAIN_ROW, sc.CANCEL_ROW, sc.SHAPES_T - 1, sc.SHAPES_T, N - 1):
            one = np.zeros(N, bool)
            one[r] = True
            D, I = ix.search_sparse(t, w, 1, allow=one)
            if hit[r]:
                assert I[0, 0] == r and D[0, 0].view(np.uint32) == sp32[r].view(np.uint32), f"{name}: row {r}"
            else:
                assert I[0, 0] == -1 and D[0, 0] == np.float32(-FMAX), f"{name}: row {r} is no hit"
        # ... and as L of the hybrid search with a zero query (miss = 0 there)
        for r in (sc.LONG_ROW, sc.ALL64_ROW, sc.CHAIN_ROW, sc.CANCEL_ROW, sc.SHAPES_T):
            one = np.zeros(N, bool)
            one[r] = True
            D, I, S, L = ix.search_hybrid_sparse(np.zeros(D_PURE, np.float32), t, w, 1, 1.0, allow=one)
            assert I[0, 0] == r and L[0, 0].view(np.uint32) == sp32[r].view(np.uint32), f"{name}: L of row {r}"
    D, I = ix.search_sparse(*queries["no term occurs"], 10)
    assert (I == -1).all() and (D == np.float32(-FMAX)).all()
    D, I = ix.search_sparse(*queries["cancellation"], 10)
    assert I[0, :5].tolist() == [sc.CANCEL_ROW + 2, sc.CANCEL_ROW + 1, sc.CANCEL_ROW, sc.CANCEL_ROW + 3, -1]
    assert D[0, 2] == 0.0 and not np.signbit(D[0, 2])
    ix.close()


# ------------------------------------------------------------------ lattice: exact values, exact ties
def test_lattice_values_are_exact_and_ties_go_to_the_lower_id():
    vs = sc.vectors(202, lattice=True)
    # the blocks of k_sparse_topk start at multiples of the slice: from the launch geometry
    starts = np.arange(0, N, topk_slice(N))
    assert starts.tolist() == sc.slices().tolist() and len(starts) == 5
    ix = _index(vs)
    half = sc.half_mask()
    across = 0
    for name, (t, w) in sc.pure_queries(vs, lattice=True).items():
        sp64, _ = vs.f64(t, w)
        sp32, hit = vs.f32(t, w)
        for k in sc.KS:
            for mask in (None, half):
                D, I = ix.search_sparse(t, w, k, allow=mask)
                what = f"lattice {name} k={k} mask={mask is not None}"
                _check_pure((D, I), sp32, hit, k, what, mask)
                v = I[0] >= 0
                assert np.array_equal(D[0][v].astype(np.float64), sp64[I[0][v]]), f"{what}: D is not the float64 truth"
                if mask is None and v.all():
                    tied = np.flatnonzero(hit & (sp64 == sp64[I[0, k - 1]]))
                    if tied.size > np.count_nonzero(sp64[I[0]] == sp64[I[0, k - 1]]):   # the tie goes on beyond rank k
                        across += np.unique(np.searchsorted(starts, tied, side="right")).size >= 2
    assert across >= 6, f"only {across} answers cut a tie that spans slice boundaries"
    ix.close()


# ------------------------------------------------------------------ hybrid
@pytest.mark.parametrize("d", [64, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_hybrid_grid(metric, d):
    vs = sc.vectors(201)
    x, q, S64, band, sp32, sp64, mag, F = sc.hybrid_truth(tp, vs, d, metric)
    pairs = sc.hybrid_pairs()
    alpha = sc.HYBRID_ALPHA
    ix = _index(vs, d, metric, x)
    pad = np.float32(-FMAX if metric == 0 else FMAX)
    for k in sc.KS:
        what = f"metric={metric} d={d} k={k} alpha={alpha}"
        out = [ix.search_hybrid_sparse(q[j], t, w, k, alpha) for j, (t, w) in pairs]
        D, I, S, L = (np.concatenate([o[c] for o in out]) for c in range(4))
        assert D.dtype == S.dtype == L.dtype == np.float32 and I.dtype == np.int64 and D.shape == I.shape == S.shape == L.shape == (8, k)
        I_ref, V, nxt, exempt = sc.hybrid_exempt(tp, F, k, metric)
        knn_checks.assert_topk_matches(D, I, V.astype(np.float32), I_ref, V, what, D64_next=np.where(np.isnan(nxt), np.inf, nxt),
                                       tie_eps=1e-6)
        for j, (_, (t, w)) in enumerate(pairs):
            i = I[j]
            wj = f"{what} pair {j}"
            assert (i >= 0).all() and np.unique(i).size == k and (D[j] != pad).all(), wj
            dd = D[j].astype(np.float64)
            step = np.diff(dd)
            assert (step <= 0).all() if metric == 0 else (step >= 0).all(), f"{wj}: D not best first"
            assert (np.diff(i)[step == 0] > 0).all(), f"{wj}: equal values not by ascending id"
            errD = np.abs(dd - F[j, i])
            tol = band[j, i] + U * np.abs(F[j, i]) + abs(alpha) * (len(t) + 1) * U * mag[j, i]
            assert (errD <= tol).all(), f"{wj}: fused value error {errD.max():.3e} beyond the band"
            errS = np.abs(S[j].astype(np.float64) - S64[j, i])
            assert (errS <= band[j, i]).all(), f"{wj}: raw score error {errS.max():.3e} beyond the band"
            assert np.array_equal(L[j].view(np.uint32), sp32[j, i].view(np.uint32)), f"{wj}: L differs from the float32 restatement in bits"
        print(f"{what}: {exempt} of {8 * k} slots exempt from the id comparison ({100.0 * exempt / (8 * k):.2f} %)")
        assert exempt <= 0.05 * 8 * k, f"{what}: the tie rule exempts {exempt} of {8 * k} slots"
    ix.close()


# ------------------------------------------------------------------ neutrality
@pytest.mark.parametrize("metric", [0, 1])
def test_nothing_else_changes(metric):
    d = 64
    x = tp._rows(N, d, 11)
    q = tp._queries(x, 3, 12)
    vs = sc.vectors(201)
    ls = synth.term_lists(N, 101)
    t, w = sc.query(8, 8)
    plain = tp._index(d, metric, x)
    ix = tp._index(d, metric, x)
    ix.set_terms(ls)
    thresh = 0.3 if metric == 0 else 1.4
    before = (ix.search(q, 10), ix.search(q, 128), ix.search_hybrid(q[0], [11, 2550], [0.5, 0.25], 10, 0.5), ix.range_search(q, thresh))
    for k in (10, 128):                                                         # an index without vectors: search_prior
        for j in range(3):
            D, I, S, L = ix.search_hybrid_sparse(q[j], t, w, k, 0.7)
            _same((D, I, S), plain.search_prior(q[j:j + 1], k, 0.0), f"no vectors k={k}")
            assert np.array_equal(_bits(S), _bits(D)) and (L == 0.0).all()
    ix.set_sparse(vs.csr)
    ix.set_priors(tp._priors(N, 23))                                            # the stored priors play no part
    for k in (10, 128):
        for j in range(3):
            want = plain.search_prior(q[j:j + 1], k, 0.0)
            for setup, args in (("m = 0", ((), (), k, 0.7)), ("alpha = 0", (t, w, k, 0.0))):
                D, I, S, L = ix.search_hybrid_sparse(q[j], *args)
                _same((D, I, S), want, f"metric={metric} k={k} query {j} {setup}")
                assert np.array_equal(_bits(S), _bits(D)) and (L == 0.0).all(), setup
    ix.search_sparse(t, w, 128)
    ix.search_hybrid_sparse(q[0], t, w, 10, 0.5)
    ix.set_priors(np.zeros(N, np.float32))
    after = (ix.search(q, 10), ix.search(q, 128), ix.search_hybrid(q[0], [11, 2550], [0.5, 0.25], 10, 0.5), ix.range_search(q, thresh))
    for name, a, b in zip(("search k=10", "search k=128", "search_hybrid", "range_search"), before, after):
        _same(a, b, f"metric={metric} {name} before and after set_sparse and sparse searches")
    assert before[3][0][-1] > 0
    if metric == 0:
        # a zero query: the fused value IS the sparse value over ALL rows (misses at 0.0, ties to the lower row)
        sp32, hit = vs.f32(t, w)
        order = np.lexsort((np.arange(N), -sp32.astype(np.float64)))
        D, I, S, L = ix.search_hybrid_sparse(np.zeros(d, np.float32), t, w, 128, 1.0)
        assert np.array_equal(I[0], order[:128]) and np.array_equal(_bits(D), _bits(L)) and (S == 0.0).all()
    plain.close()
    ix.close()


# ------------------------------------------------------------------ errors at the library
def test_the_library_refuses_before_anything_is_written():
    from claude_semantic_search_amd import _native as nat

    vs = sc.vectors(201).rows(np.arange(600))
    x = tp._rows(N, D_PURE, 11)[:1000]
    ix = _index(vs, x=x)
    lib, h = nat.lib(), ix._handle()
    stored = ix.get_sparse()

    def unchanged():
        _same(ix.get_sparse(), stored, "a refused call changed the vectors")
        assert ix.sparse_rows == 600

    def set_raw(row0, off, t, w):
        off, t, w = np.asarray(off, np.int64), np.asarray(t, np.uint32), np.asarray(w, np.float32)
        return lib.css_index_set_sparse(h, row0, off.shape[0] - 1, off.ctypes.data, t.ctypes.data, w.ctypes.data)

    for bad_w, word in ((0.0, "zero"), (-1.0, "negative"), (float("nan"), "NaN"), (float("inf"), "infinite"), (65536.5, "too large")):
        assert set_raw(600, [0, 1, 3], [1, 2, 3], [1.0, 1.0, bad_w]) == nat.CSS_ERR_INVALID
        assert "row 601" in nat.last_error() and word in nat.last_error(), nat.last_error()
        unchanged()
    assert set_raw(600, [0, 1, 4], [1, 7, 3, 7], [1.0] * 4) == nat.CSS_ERR_INVALID and "term 7 is repeated in row 601" in nat.last_error()
    assert set_raw(600, [0, 1], [1 << 24], [1.0]) == nat.CSS_ERR_INVALID and "row 600" in nat.last_error() and "2^24" in nat.last_error()
    assert set_raw(600, [0, 3, 2], [1, 2, 3], [1.0] * 3) == nat.CSS_ERR_INVALID and "decrease at row 601" in nat.last_error()
    assert set_raw(600, [1, 2], [1, 2], [1.0] * 2) == nat.CSS_ERR_INVALID and "start" in nat.last_error()
    assert set_raw(601, [0, 1], [1], [1.0]) == nat.CSS_ERR_INVALID and "append-only" in nat.last_error()      # row0 > T
    assert set_raw(999, [0, 1, 2], [1, 2], [1.0] * 2) == nat.CSS_ERR_INVALID and "outside" in nat.last_error()
    assert set_raw(-1, [0, 1], [1], [1.0]) == nat.CSS_ERR_INVALID
    unchanged()
    assert set_raw(600, [0, 1], [3], [65536.0]) == nat.CSS_OK and ix.sparse_rows == 601                      # the largest weight
    ix.set_sparse([], row0=600)
    unchanged()

    def raw(t, w, k=5, m=None, hybrid=False):
        t, w = np.asarray(t, np.uint32), np.asarray(w, np.float32)
        D, I, S, L = np.empty(129, np.float32), np.empty(129, np.int64), np.empty(129, np.float32), np.empty(129, np.float32)
        m = len(t) if m is None else m
        if hybrid:
            return lib.css_index_search_hybrid_sparse(h, x[:1].ctypes.data, k, 0.5, t.ctypes.data, w.ctypes.data, m, 0, None,
                                                      D.ctypes.data, I.ctypes.data, S.ctypes.data, L.ctypes.data)
        return lib.css_index_search_sparse(h, t.ctypes.data, w.ctypes.data, m, k, None, D.ctypes.data, I.ctypes.data)

    for hybrid in (False, True):
        for k in (0, 129):
            assert raw([3], [1.0], k=k, hybrid=hybrid) == nat.CSS_ERR_INVALID and f"k={k}" in nat.last_error()
        assert raw(np.arange(65), np.ones(65), hybrid=hybrid) == nat.CSS_ERR_INVALID and "m=65" in nat.last_error()
        assert raw([5, 9, 5], [1.0] * 3, hybrid=hybrid) == nat.CSS_ERR_INVALID and "term 5 is repeated" in nat.last_error()
        assert raw([1 << 24], [1.0], hybrid=hybrid) == nat.CSS_ERR_INVALID and "2^24" in nat.last_error()
        for bad_w, word in ((0.0, "zero"), (float("nan"), "NaN"), (float("-inf"), "infinite"), (-65537.0, "too large")):
            assert raw([5, 9], [1.0, bad_w], hybrid=hybrid) == nat.CSS_ERR_INVALID
            assert "weight of term 9" in nat.last_error() and word in nat.last_error(), nat.last_error()
        assert raw(np.arange(64), -np.ones(64), hybrid=hybrid) == nat.CSS_OK
    unchanged()
    o = np.zeros(21, np.int64)
    assert lib.css_index_get_sparse(h, 990, 20, o.ctypes.data, None, None) == nat.CSS_ERR_INVALID and "outside" in nat.last_error()
    with pytest.raises(ValueError):
        ix.get_sparse(990, 20)
    with pytest.raises(nat.CssError):
        ix.set_sparse([([1], [1.0])], row0=700)
    ix.close()
    for call in (lambda: ix.search_sparse([3], [1.0], 5), lambda: ix.set_sparse([([1], [1.0])]), lambda: ix.get_sparse(0, 0),
                 lambda: ix.sparse_rows, lambda: ix.search_hybrid_sparse(x[0], [3], [1.0], 5, 0.5)):
        with pytest.raises(RuntimeError, match="freed"):
            call()

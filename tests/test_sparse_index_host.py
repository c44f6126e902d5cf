"""CPU: the host side of the sparse vectors on the flat index -- ``flat_index.sparse_args`` / ``sparse_as_csr`` (what the
library would refuse raises ``ValueError`` BEFORE the library is called: the index object here has no library handle at
all), ``synth.sparse_vectors``, the numpy restatements of ``tests/sparse_fakes.py``, and a proof, with numpy alone, that
the inputs of ``tests/test_sparse_index_gpu.py`` (``tests/sparse_cases.py``) make every one of its checks bind."""
import numpy as np
import pytest

import sparse_cases as sc
import test_search_prior_gpu as tp
from claude_semantic_search_amd import flat_index as fi
from claude_semantic_search_amd import synth
from claude_semantic_search_amd.sparse_encoder import SparseVector
from sparse_fakes import Vectors, topk, topk_slice


class _NoLibrary(fi.IndexFlat):
    """An ``IndexFlat`` without a library handle: every call that reaches the library raises ``RuntimeError``."""

    def __init__(self, d=8):
        self.d, self.metric_type, self.device, self._h, self._terms_rows = d, 0, 0, None, 0

    ntotal = 100
    sparse_rows = 0


NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("bad", [
    dict(terms=[3, 9, 3], weights=[1.0, 1.0, 1.0]),            # a repeated term
    dict(weights=[0.0]), dict(weights=[NAN]), dict(weights=[INF]), dict(weights=[65537.0]), dict(weights=[-65537.0]),
    dict(terms=list(range(65)), weights=[1.0] * 65),           # m = 65
    dict(k=129), dict(k=0),
    dict(terms=[[3, 9]], weights=[[1.0, 2.0]]),                # more than one query
    dict(terms=[1 << 24], weights=[1.0]), dict(terms=[-1], weights=[1.0]), dict(terms=[1, 2], weights=[1.0]),
])
def test_search_arguments_are_refused_before_the_library_is_called(bad):
    ix = _NoLibrary()
    args = dict(terms=[3], weights=[1.0], k=5)
    args.update(bad)
    with pytest.raises(ValueError):
        ix.search_sparse(args["terms"], args["weights"], args["k"])
    with pytest.raises(ValueError):
        ix.search_hybrid_sparse(np.zeros(8, np.float32), args["terms"], args["weights"], args["k"], 0.5)
    with pytest.raises(RuntimeError, match="freed"):           # (a good call does reach for the library)
        ix.search_sparse([3], [1.0], 5)


def test_hybrid_only_arguments_and_accepted_forms():
    ix = _NoLibrary()
    for alpha in (NAN, INF, -INF):
        with pytest.raises(ValueError, match="alpha"):
            ix.search_hybrid_sparse(np.zeros(8, np.float32), [3], [1.0], 5, alpha)
    with pytest.raises(ValueError, match="one query"):
        ix.search_hybrid_sparse(np.zeros((2, 8), np.float32), [3], [1.0], 5, 0.5)
    with pytest.raises(ValueError):
        ix.search_hybrid_sparse(np.zeros(9, np.float32), [3], [1.0], 5, 0.5)
    t, w, k, a = fi.sparse_args([7, 3], [-2.5, 65536.0], 128, 0.25)
    assert t.dtype == np.uint32 and t.tolist() == [7, 3] and w.dtype == np.float32 and w.tolist() == [-2.5, 65536.0]
    assert (k, a) == (128, 0.25)
    t, w, k, a = fi.sparse_args(SparseVector(np.array([5, 1], np.int32), np.array([0.5, 2.0], np.float32)), None, 1)
    assert t.tolist() == [5, 1] and w.tolist() == [0.5, 2.0] and a is None
    t, w, _, _ = fi.sparse_args((), (), 3)
    assert t.shape == (0,) and w.shape == (0,)
    assert len(fi.sparse_args(list(range(64)), [1.0] * 64, 1)[0]) == 64
    assert fi.MAX_SPARSE_QUERY_TERMS == 64 and fi.MAX_SPARSE_WEIGHT == 65536.0


@pytest.mark.parametrize("bad, names", [
    ([([3, 9], [1.0, 1.0]), ([4, 7, 4], [1.0, 1.0, 1.0])], "term 4 is repeated in row 1"),
    ([([3], [0.0])], "row 0"), ([([1], [1.0]), ([3], [-1.0])], "row 1"), ([([3], [NAN])], "row 0"),
    ([([3], [INF])], "row 0"), ([([3], [65536.5])], "row 0"), ([([1 << 24], [1.0])], "row 0"), ([([-1], [1.0])], "row 0"),
    ([([1, 2], [1.0])], "row 0"),
    ((np.array([0, 1, 3]), np.array([5, 6, 6]), np.array([1.0, 1.0, 1.0], np.float32)), "term 6 is repeated in row 1"),
    ((np.array([0, 2]), np.array([5, 6]), np.array([1.0], np.float32)), "weights"),
])
def test_set_sparse_arguments_are_refused_before_the_library_is_called(bad, names):
    with pytest.raises(ValueError, match=names):
        _NoLibrary().set_sparse(bad)
    with pytest.raises(ValueError, match=names):
        fi.sparse_as_csr(bad)


def test_sparse_as_csr_forms():
    off, t, w = fi.sparse_as_csr([SparseVector(np.array([9, 2], np.int32), np.array([0.5, 1.5], np.float32)), ([], []), ([7], [65536.0])])
    assert off.tolist() == [0, 2, 2, 3] and t.tolist() == [9, 2, 7] and w.tolist() == [0.5, 1.5, 65536.0]
    assert off.dtype == np.int64 and t.dtype == np.uint32 and w.dtype == np.float32
    o2, t2, w2 = fi.sparse_as_csr((off, t, w))
    assert o2.tolist() == off.tolist() and t2.tolist() == t.tolist() and w2.tolist() == w.tolist()
    assert fi.sparse_as_csr([])[0].tolist() == [0]
    with pytest.raises(ValueError, match="65537 entries"):
        fi.sparse_as_csr((np.array([0, 65537]), np.arange(65537), np.ones(65537, np.float32)))
    with pytest.raises(RuntimeError, match="freed"):
        _NoLibrary().set_sparse([([3], [1.0])])


# ------------------------------------------------------------------------------------------------ synth.sparse_vectors
def test_sparse_vectors_are_deterministic_sorted_and_skewed_like_term_lists():
    a, b = synth.sparse_vectors(3000, 5), synth.sparse_vectors(3000, 5)
    assert all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))
    off, t, w = a
    assert off.dtype == np.int64 and t.dtype == np.uint32 and w.dtype == np.float32 and off[0] == 0 and off[-1] == t.shape[0] == w.shape[0]
    assert not np.array_equal(synth.sparse_vectors(3000, 6)[1], t)
    rows = np.repeat(np.arange(3000), np.diff(off))
    assert (np.diff(rows.astype(np.int64) << 24 | t) > 0).all(), "terms must be distinct and ascending within a row"
    assert (w > 0).all() and np.isfinite(w).all() and w.max() <= 65536.0 and t.max() < 4096
    # the row sizes and terms are those of term_lists, de-duplicated
    loff, ltok = synth.term_lists(3000, 5)
    want = np.unique(np.repeat(np.arange(3000, dtype=np.int64), np.diff(loff)) << 24 | ltok)
    assert np.array_equal(rows.astype(np.int64) << 24 | t, want)
    assert synth.sparse_vectors(500, 5, vocab=64)[1].max() < 64


def test_the_lattice_form_is_exact():
    off, t, w = synth.sparse_vectors(3000, 7, lattice=True)
    assert np.array_equal(w * 8, np.round(w * 8)) and w.min() >= 0.125 and w.max() <= 4.0 and np.unique(w).size == 32
    vs = Vectors(off, t, w)
    for m in (1, 33, 64):
        qt, qw = sc.query(m, m, lattice=True, signed=(m == 33))
        assert np.array_equal(qw * 8, np.round(qw * 8)) and np.abs(qw).min() >= 0.125 and np.abs(qw).max() <= 4.0
        # every partial sum of 64 products is a multiple of 1/64 below 2^24 / 64: exact in float32 in any order
        sp64, mag = vs.f64(qt, qw)
        assert np.array_equal(sp64 * 64, np.round(sp64 * 64)) and mag.max() * 64 <= 64 * 16 * 64 < 2 ** 24
        sp32, hit = vs.f32(qt, qw)
        assert np.array_equal(sp32.astype(np.float64), sp64), "the float32 restatement must equal the float64 truth exactly"
        assert np.array_equal(vs.f32(qt[::-1], qw[::-1])[0], sp32)


def test_the_restatements_and_the_ranking():
    vs = Vectors(np.array([0, 2, 2, 5, 6]), np.array([9, 4, 1, 9, 4, 7]), np.array([0.5, 1.5, 2.0, 0.25, 1.0, 3.0], np.float32))
    assert vs.terms.tolist() == [4, 9, 1, 4, 9, 7] and vs.w.tolist() == [1.5, 0.5, 2.0, 1.0, 0.25, 3.0]      # the stored form
    sp, hit = vs.f32([9, 4], np.array([2.0, -1.0], np.float32))
    assert sp.tolist() == [-0.5, 0.0, -0.5, 0.0] and hit.tolist() == [True, False, True, False]
    sp64, mag = vs.f64([9, 4], np.array([2.0, -1.0], np.float32))
    assert sp64.tolist() == [-0.5, 0.0, -0.5, 0.0] and mag.tolist() == [2.5, 0.0, 1.5, 0.0]
    D, I = topk(sp, hit, 3)
    assert I.tolist() == [[0, 2, -1]] and D[0, :2].tolist() == [-0.5, -0.5] and D[0, 2] == -np.finfo(np.float32).max
    D, I = topk(sp, hit, 1, allowed=np.array([False, True, True, True]), id_base=10)
    assert I.tolist() == [[12]]
    sub = vs.rows(np.array([True, False, True, False]))
    assert sub.off.tolist() == [0, 2, 5] and sub.terms.tolist() == [4, 9, 1, 4, 9]
    assert vs.padded(6).off.tolist() == [0, 2, 2, 5, 6, 6, 6]
    assert topk_slice(20003) == 4096 and topk_slice(1 << 20) == 32768 and topk_slice(1) == 4096


# ------------------------------------------------------------------------------------- the GPU inputs make the checks bind
def test_pure_search_inputs_cover_full_short_and_empty_answers():
    vs = sc.vectors(201)
    half = sc.half_mask()
    full = short = none = 0
    for name, (t, w) in sc.pure_queries(vs).items():
        sp, hit = vs.f32(t, w)
        for mask in (None, half):
            nhit = int(np.count_nonzero(hit if mask is None else hit & mask))
            for k in sc.KS:
                full += nhit >= k
                short += 0 < nhit < k
                none += nhit == 0
    assert full > 0.6 * (full + short + none) and short >= 1 and none >= 1, (full, short, none)
    t, w = sc.pure_queries(vs)["signed m=8"]
    sp, hit = vs.f32(t, w)
    assert (sp[hit] < 0).any() and (sp[hit] > 0).any() and (w < 0).any()


def test_lattice_inputs_have_ties_across_rank_k_and_across_the_slices():
    vs = sc.vectors(202, lattice=True)
    starts = sc.slices()
    assert starts.tolist() == [0, 4096, 8192, 12288, 16384] and topk_slice(sc.N) == 4096
    straddle = {k: 0 for k in sc.KS}
    for name, (t, w) in sc.pure_queries(vs, lattice=True).items():
        sp, hit = vs.f32(t, w)
        sp64, _ = vs.f64(t, w)
        assert np.array_equal(sp.astype(np.float64), sp64), name
        ids = np.flatnonzero(hit)
        order = ids[np.lexsort((ids, -sp64[ids]))]
        for k in sc.KS:
            if order.size > k and sp64[order[k - 1]] == sp64[order[k]]:
                tied = ids[sp64[ids] == sp64[order[k - 1]]]
                # the tie at rank k has members in several slices of the column top-k: the part merge must pick by id
                if np.unique(np.searchsorted(starts, tied, side="right")).size >= 2:
                    straddle[k] += 1
    assert min(straddle.values()) >= 2, f"queries with a tie across rank k that spans slice boundaries, per k: {straddle}"


def test_shape_inputs_are_what_they_claim():
    vs, queries = sc.shapes()
    lens = np.diff(vs.off)
    assert vs.n == sc.N and (lens[sc.SHAPES_T:] == 0).all() and lens[0] == 0 and (lens[1024:1216] == 0).all()
    assert lens[sc.LONG_ROW] == 2000 and lens[sc.ALL64_ROW] == 64 and vs.terms.max() == sc.MAXTERM
    scattered = np.flatnonzero(lens[:sc.SHAPES_T] == 0)
    assert np.count_nonzero((scattered < 1024) | (scattered >= 1216)) >= 250     # empty rows among full ones
    t, w = queries["64 terms, one row holds them all"]
    sp, hit = vs.f32(t, w)
    sp_rev, _ = vs.f32(*queries["the same reversed"])
    assert len(t) == 64 and hit[sc.ALL64_ROW] and hit[sc.LONG_ROW] and not hit[sc.SHAPES_T:].any() and not hit[1024:1216].any()
    assert sp[sc.ALL64_ROW].view(np.uint32) != sp_rev[sc.ALL64_ROW].view(np.uint32), "the order of the query terms must show in the bits"
    assert len({int(v) & 4095 for v in sc.CHAIN}) == 1
    t, w = queries["shared low bits"]
    sp, hit = vs.f32(t, w)
    want = np.float32(np.float32(np.float32(np.float32(0.11) * np.float32(0.75)) + np.float32(0.07) * np.float32(0.5))
                      + np.float32(0.03) * np.float32(3.0))
    want = np.float32(want + np.float32(0.05) * np.float32(1.25))
    assert sp[sc.CHAIN_ROW] == want and np.count_nonzero(hit) == np.count_nonzero(vs.terms == 100)
    sp, hit = vs.f32(*queries["largest term id"])
    assert hit[sc.MAXTERM_ROW] and sp[sc.MAXTERM_ROW] == np.float32(1.125)
    assert not vs.f32(*queries["no term occurs"])[1].any()
    sp, hit = vs.f32(*queries["cancellation"])
    assert hit[sc.CANCEL_ROW] and sp[sc.CANCEL_ROW] == 0.0 and np.count_nonzero(hit) == 4
    D, I = topk(sp, hit, 10)
    # ... still a hit: behind the positive rows, in front of the negative one, and in front of no row that is not a hit
    assert I[0, :5].tolist() == [sc.CANCEL_ROW + 2, sc.CANCEL_ROW + 1, sc.CANCEL_ROW, sc.CANCEL_ROW + 3, -1]
    assert D[0, :4].tolist() == [2.0, 1.0, 0.0, -4.0]


@pytest.mark.parametrize("d", [64, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_hybrid_grid_exempts_at_most_five_percent_and_the_sparse_side_matters(metric, d):
    vs = sc.vectors(201)
    x, q, S64, band, sp32, sp64, mag, F = sc.hybrid_truth(tp, vs, d, metric)
    assert len(sc.hybrid_pairs()) == 8 and F.shape == (8, sc.N)
    plain10, _, _ = tp._topk64(S64, 10, metric)
    for k in sc.KS:
        I_ref, V, nxt, exempt = sc.hybrid_exempt(tp, F, k, metric)
        assert exempt <= 0.05 * 8 * k, f"metric={metric} d={d} k={k}: the tie rule exempts {exempt} of {8 * k} slots"
        if k == 10:
            absent = sum(int((~np.isin(I_ref[j], plain10[j])).sum()) for j in range(8))
            assert absent >= 0.20 * 8 * k, f"only {absent} of {8 * k} ids differ from the plain top-10"
    # the tolerance term of the sparse sum is far below the values it guards
    tol = abs(sc.HYBRID_ALPHA) * (np.array(sc.HYBRID_MS)[:, None] + 1) * 2.0 ** -24 * mag
    assert (np.abs(sp32.astype(np.float64) - sp64) <= (np.array(sc.HYBRID_MS)[:, None] + 1) * 2.0 ** -24 * mag).all()
    assert tol.max() < 1e-3

"""GPU: token matrices on the flat index -- ``IndexFlat.set_tokens`` / ``get_tokens`` / ``token_rows`` / ``token_dim`` /
``drop_tokens`` / ``search_maxsim`` / ``maxsim_ids`` (``css_index_set_tokens`` ...; kernels ``k_tok_scores<P, MT>``,
``k_tok_move_units``, ``k_sparse_topk`` and the part merge behind it).

Truth is numpy on the very arrays handed to the index (``tests/tokens_fakes.py``: float64 MaxSim, one ``lexsort``), never
the code under test; the inputs are those of ``tests/tokens_cases.py``, which ``tests/test_tokens_index_host.py`` proves
binding on the CPU.  The one exception is the exact Gaussian check, whose oracle is the library's EXISTING
``css_encoder_maxsim`` (``MpnetEncoder.maxsim``), which this index must equal in bits by construction.
N = 3 001 rows (not a multiple of 16, 64 or 256); doc lengths 0 .. 40 with 0, 1, 15, 16, 17, 63, 64, 65, 512 in front."""
import numpy as np
import pytest

import bert_reference as br
import test_search_prior_gpu as tp
import tokens_cases as tc
from claude_semantic_search_amd import synth
from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder
from tokens_fakes import topk

pytestmark = pytest.mark.gpu

N, D = tc.N, tc.D
FMAX = tp.FMAX


def _index(ms=None, x=None):
    ix = tp._index(D, 0, tp._rows(N, D, 11) if x is None else x)
    if ms is not None:
        ix.set_tokens(ms.csr)
    return ix


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b, what):
    for j, (u, v) in enumerate(zip(a, b)):
        assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(_bits(u), _bits(v)), f"{what}: array {j} differs"


def _matches(ix, want, nrows, what):
    off, tok = ix.get_tokens()
    assert off.shape == (nrows + 1,) and np.array_equal(off[:want.n + 1], want.off) and (off[want.n:] == want.off[-1]).all(), what
    assert tok.dtype == np.uint16 and tok.shape == want.tok.shape and np.array_equal(_bits(tok), _bits(want.tok)), what
    assert ix.token_rows == want.n and ix.token_dim == (want.P if want.n else 0), what


def _check(res, col, k, what, allowed=None, id_base=0):
    """D and I against the float64 column (exact in fp32 on lattice inputs) and ONE lexsort; no tolerance."""
    D_, I = res
    Dw, Iw = topk(col, k, allowed, id_base)
    assert D_.dtype == np.float32 and I.dtype == np.int64 and D_.shape == I.shape == (1, k), what
    assert np.array_equal(I, Iw), f"{what}: ids differ from lexsort((id, -score)) over the hit rows: {I[0][:8]} vs {Iw[0][:8]}"
    assert np.array_equal(_bits(D_), _bits(Dw)), f"{what}: D differs from the truth in bits"
    return int((I >= 0).sum())


# ------------------------------------------------------------------ storage: the matrices follow the rows
def test_matrices_round_trip_append_rewrite_grow_and_reset():
    x = tp._rows(N, D, 11)
    ms, qs = tc.lattice("E", 96)
    ls = synth.term_lists(N, 101)
    sv = synth.sparse_vectors(N, 201)
    ix = tp._index(D, 0)
    assert ix.token_rows == 0 and ix.token_dim == 0 and ix.get_tokens()[0].tolist() == [0]
    ix.add(x[:1000])
    assert ix.token_rows == 0 and not ix.get_tokens()[0].any() and ix.get_tokens()[1].size == 0
    ix.set_terms((ls[0][:1001], ls[1][:ls[0][1000]]))                            # BM25 lists and sparse vectors on the same index
    ix.set_sparse((sv[0][:1001], sv[1][:sv[0][1000]], sv[2][:sv[0][1000]]))
    terms_before, sparse_before = ix.get_terms(), ix.get_sparse()
    head = ms.rows(np.arange(700))
    ix.set_tokens(head.rows(np.arange(300)).mats())                             # in two pieces, the list form ...
    ix.set_tokens(head.rows(np.arange(300, 700)).csr)                           # ... and the CSR form
    _matches(ix, head, 1000, "append in two pieces")
    one = _index(head, x=x[:1000])                                              # ... equals one call
    _same(ix.get_tokens(), one.get_tokens(), "two pieces against one call")
    one.close()
    o1, t1 = ix.get_tokens(699, 3)                                              # a range across the end of the matrices
    assert o1.tolist() == [0] + [int(head.lens[699])] * 3 and np.array_equal(t1, head.mat(699))
    for r0 in range(1000, N, 1000):                                             # the capacity grows several times
        ix.add(x[r0:r0 + 1000])
        _matches(ix, head, min(r0 + 1000, N), "capacity growth")
    ix.set_tokens(ms.rows(np.arange(700, 1500)).csr)
    _matches(ix, ms.rows(np.arange(1500)), N, "appended matrices")
    ix.set_tokens(ms.rows(np.arange(200, 300)).csr, row0=600)                   # row0 < T drops, then appends
    _matches(ix, ms.rows(np.concatenate([np.arange(600), np.arange(200, 300)])), N, "row0 < T")
    ix.set_tokens([], row0=100)                                                 # a pure truncation
    _matches(ix, ms.rows(np.arange(100)), N, "pure truncation")
    ix.set_tokens(ms.csr, row0=0)                                               # the rewrite
    _matches(ix, ms, N, "rewrite")
    # the term lists and the sparse vectors never noticed
    now = ix.get_terms()
    assert np.array_equal(now[0][:1001], terms_before[0]) and np.array_equal(now[1], terms_before[1])
    now = ix.get_sparse()
    assert np.array_equal(now[0][:1001], sparse_before[0]) and np.array_equal(now[1], sparse_before[1])
    assert np.array_equal(_bits(now[2]), _bits(sparse_before[2]))
    _check(ix.search_maxsim(qs[4], 10), ms.scores64(qs[4]), 10, "after growth and rewrite")
    ix.set_tokens(tc.gaussian(32)[0].rows(np.arange(50)).csr, row0=0)           # another P, from row 0 only
    assert ix.token_dim == 32 and ix.token_rows == 50
    ix.drop_tokens()
    assert ix.token_rows == 0 and ix.token_dim == 0 and not ix.get_tokens()[0].any()
    ix.set_tokens(ms.rows(np.arange(10)).csr)
    ix.reset()
    ix.add(x[:500])
    assert ix.token_rows == 0 and ix.token_dim == 0 and not ix.get_tokens()[0].any(), "reset must forget the matrices"
    D_, I = ix.search_maxsim(qs[0], 10)
    assert (I == -1).all() and (D_ == np.float32(-FMAX)).all()
    assert (ix.maxsim_ids(qs[0], [0, 499]) == -np.inf).all()
    ix.close()


def test_remove_ids_compacts_the_matrices_with_the_rows():
    x = tp._rows(N, D, 11)
    ms, qs = tc.lattice("E", 64)
    ix = _index(ms.rows(np.arange(tc.T_PART)))                                  # rows T_PART .. have no matrix
    ls = synth.term_lists(N, 101)
    ix.set_terms(ls)
    gone = np.flatnonzero(np.random.default_rng(9).random(N) < 1.0 / 3.0)       # a scattered third
    keep = np.ones(N, bool)
    keep[gone] = False
    assert ix.remove_ids(gone) == gone.shape[0]
    kept = ms.rows(np.flatnonzero(keep[:tc.T_PART]))
    nk = int(keep.sum())
    _matches(ix, kept, nk, "remove_ids")
    fresh = _index(kept, x=x[keep])
    _same(ix.get_tokens(), fresh.get_tokens(), "get_tokens after remove_ids against a fresh index")
    full = kept.padded(nk)
    for j, q in enumerate(qs):
        col = full.scores64(q)
        for k in tc.KS:
            res = ix.search_maxsim(q, k)
            _same(res, fresh.search_maxsim(q, k), f"search_maxsim after remove_ids, query {j} k={k}")
            _check(res, col, k, f"after remove_ids, query {j} k={k}")
    fresh.close()
    ix.add(x[:100])                                                             # rows added later have none
    _matches(ix, kept, nk + 100, "rows added after remove_ids")
    ix.remove_ids(np.arange(nk + 100))                                          # emptied: as reset
    assert ix.ntotal == 0 and ix.token_rows == 0 and ix.token_dim == 0
    ix.close()


def test_the_library_refuses_before_anything_is_written():
    from claude_semantic_search_amd import _native as nat

    ms, qs = tc.gaussian(64)
    ix = _index(ms.rows(np.arange(600)), x=tp._rows(N, D, 11)[:1000])
    lib, h = nat.lib(), ix._handle()
    stored = ix.get_tokens()

    def unchanged():
        _same(ix.get_tokens(), stored, "a refused call changed the matrices")
        assert ix.token_rows == 600 and ix.token_dim == 64

    def set_raw(row0, off, tok, P=64):
        off, tok = np.asarray(off, np.int64), np.ascontiguousarray(tok, np.uint16)
        return lib.css_index_set_tokens(h, row0, off.shape[0] - 1, off.ctypes.data, tok.ctypes.data, P)

    ok = np.full((3, 64), 0x3F80, np.uint16)
    for bits, word in ((0x7FC0, "NaN"), (0x7F80, "infinite"), (0xFF80, "infinite")):
        bad = ok.copy()
        bad[2, 5] = bits
        assert set_raw(600, [0, 1, 3], bad) == nat.CSS_ERR_INVALID
        assert "row 601" in nat.last_error() and word in nat.last_error(), nat.last_error()
        unchanged()
    assert set_raw(600, [0, 1, 514], np.full((514, 64), 0x3F80, np.uint16)) == nat.CSS_ERR_INVALID
    assert "row 601 has 513 tokens (at most 512)" in nat.last_error(), nat.last_error()
    assert set_raw(601, [0, 1], ok) == nat.CSS_ERR_INVALID and "row0=601" in nat.last_error() and "append-only" in nat.last_error()
    assert set_raw(600, [0, 1], np.full((1, 32), 0x3F80, np.uint16), P=32) == nat.CSS_ERR_INVALID
    assert "P=32" in nat.last_error() and "P=64" in nat.last_error()           # a second P
    assert set_raw(600, [0, 1], ok, P=48) == nat.CSS_ERR_INVALID and "P=48" in nat.last_error()
    assert set_raw(600, [0, 3, 2], ok) == nat.CSS_ERR_INVALID and "decrease at row 601" in nat.last_error()
    assert set_raw(600, [1, 2], ok) == nat.CSS_ERR_INVALID and "start" in nat.last_error()
    assert set_raw(999, [0, 1, 2], ok) == nat.CSS_ERR_INVALID and "outside" in nat.last_error()
    assert set_raw(-1, [0, 1], ok) == nat.CSS_ERR_INVALID
    unchanged()
    assert set_raw(600, [0, 512], np.full((512, 64), 0x3F80, np.uint16)) == nat.CSS_OK and ix.token_rows == 601   # the longest row
    ix.set_tokens([], row0=600)
    unchanged()

    def raw(q, k=5, mq=None, P=64):
        q = np.ascontiguousarray(q, np.uint16)
        D_, I = np.empty(129, np.float32), np.empty(129, np.int64)
        return lib.css_index_search_maxsim(h, q.ctypes.data, q.shape[0] if mq is None else mq, P, k, None, D_.ctypes.data, I.ctypes.data)

    for k in (0, 129):
        assert raw(qs[1], k=k) == nat.CSS_ERR_INVALID and f"k={k}" in nat.last_error()
    assert raw(qs[1], mq=0) == nat.CSS_ERR_INVALID and "mq=0" in nat.last_error()
    assert raw(np.zeros((65, 64), np.uint16)) == nat.CSS_ERR_INVALID and "mq=65" in nat.last_error()
    assert raw(tc.gaussian(32)[1][1], P=32) == nat.CSS_ERR_INVALID and "P=32" in nat.last_error() and "P=64" in nat.last_error()
    bad = qs[1].copy()
    bad[7, 3] = 0x7FC0
    assert raw(bad) == nat.CSS_ERR_INVALID and "query token 7" in nat.last_error() and "NaN" in nat.last_error()
    assert raw(qs[5]) == nat.CSS_OK
    with pytest.raises(nat.CssError, match=r"position 2"):
        ix.maxsim_ids(qs[1], [5, 6, 1000, 7])
    with pytest.raises(nat.CssError, match=r"position 0"):
        ix.maxsim_ids(qs[1], [-1])
    unchanged()
    o = np.zeros(21, np.int64)
    assert lib.css_index_get_tokens(h, 990, 20, o.ctypes.data, None) == nat.CSS_ERR_INVALID and "outside" in nat.last_error()
    with pytest.raises(ValueError):
        ix.get_tokens(990, 20)
    with pytest.raises(nat.CssError):
        ix.set_tokens([ok], row0=700)
    ix.close()
    for call in (lambda: ix.search_maxsim(qs[0], 5), lambda: ix.set_tokens([ok]), lambda: ix.get_tokens(0, 0),
                 lambda: ix.token_rows, lambda: ix.token_dim, lambda: ix.maxsim_ids(qs[0], [1]), lambda: ix.drop_tokens()):
        with pytest.raises(RuntimeError, match="freed"):
            call()


# ------------------------------------------------------------------ lattice inputs: exact, ties to the lower id
@pytest.mark.parametrize("P", tc.WIDTHS)
@pytest.mark.parametrize("family", tc.FAMILIES)
def test_lattice_scores_are_exact_and_ties_go_to_the_lower_id(family, P):
    ms, qs = tc.lattice(family, P)
    ix = _index(ms)
    allow = tc.half_mask()
    for j, q in enumerate(qs):
        col = ms.scores64(q)
        for k in tc.KS:
            got = _check(ix.search_maxsim(q, k), col, k, f"{family} P={P} query {j} k={k}")
            assert got == k
        _check(ix.search_maxsim(q, 10, allow=allow), col, 10, f"{family} P={P} query {j} masked", allowed=allow)
    ix.set_token_blocks(2)                                                      # many docs through one wave, 16 per turn
    for j, q in enumerate(qs):
        _check(ix.search_maxsim(q, 128), ms.scores64(q), 128, f"{family} P={P} query {j} on two blocks")
    ix.set_token_blocks(0)
    q = qs[tc.PLANT_QUERY]
    col = ms.scores64(q)
    D_, I = ix.search_maxsim(q, 1)
    assert I[0, 0] == tc.PLANTS[0]                                              # the planted tie at rank 1
    D_, I = ix.search_maxsim(q, 10, allow=np.zeros(N, bool))                    # a mask that masks every row
    assert (I == -1).all() and (D_ == np.float32(-FMAX)).all()
    few = np.zeros(N, bool)
    few[[3, 0, 1, tc.PLANTS[0], 8]] = True                                              # row 0 is empty: 4 hits, then padding
    assert _check(ix.search_maxsim(q, 10, allow=few), col, 10, "fewer than k hits", allowed=few) == 4
    ix.set_id_base(tc.ID_BASE)
    _check(ix.search_maxsim(q, 128), col, 128, "id_base", id_base=tc.ID_BASE)
    got = ix.maxsim_ids(q, np.array([5, 0, 8, 5]) + tc.ID_BASE)
    assert np.array_equal(got, col[[5, 0, 8, 5]].astype(np.float32)) and got[1] == -np.inf
    ix.set_id_base(0)
    ix.set_tokens(ms.rows(np.arange(tc.T_PART)).csr, row0=0)                    # rows >= T are misses
    part = ms.rows(np.arange(tc.T_PART)).padded(N).scores64(q)
    assert (part[tc.T_PART:] == -np.inf).all()
    _check(ix.search_maxsim(q, 128), part, 128, "rows >= T")
    ix.close()


@pytest.mark.parametrize("P", (32, 128))
def test_a_query_whose_every_dot_is_negative(P):
    ms, q = tc.negative_case(P)
    ix = _index(ms)
    col = ms.scores64(q)
    assert (col[ms.lens > 0] < 0).all()
    for k in tc.KS:
        assert _check(ix.search_maxsim(q, k), col, k, f"negative P={P} k={k}") == k
    ix.close()


@pytest.mark.parametrize("P", tc.WIDTHS)
def test_the_bits_do_not_depend_on_the_grid(P):
    ms, qs = tc.gaussian(P)
    ix = _index(ms)
    ids = np.arange(N)
    for q in (qs[1], qs[5]):
        want = (ix.search_maxsim(q, 128), ix.maxsim_ids(q, ids))
        for blocks in (1, 3, 0, 0):                                             # (0 twice: a second call)
            ix.set_token_blocks(blocks)
            _same(ix.search_maxsim(q, 128), want[0], f"P={P} blocks={blocks}: search_maxsim")
            _same([ix.maxsim_ids(q, ids)], [want[1]], f"P={P} blocks={blocks}: maxsim_ids")
    ix.close()


# ------------------------------------------------------------------ Gaussian unit rows rounded to bf16
@pytest.fixture(scope="module")
def enc():
    cfg = br.BertCfg(num_layers=2, vocab=1000, **br.SMALL)
    e = MpnetEncoder(synthetic_seed=1, cfg_overrides=cfg.encoder_overrides())
    yield e
    e.close()


@pytest.mark.parametrize("P", tc.WIDTHS)
def test_gaussian_rows_within_the_derived_bound_and_equal_to_css_encoder_maxsim(enc, P):
    """(i) |D - truth64(I)| <= 2^-23 mq (P + mq) c, the derived bound of tests/test_maxsim_gpu.py; every returned id's
    truth is at least the k-th truth minus twice the bound, every other hit row's at most the k-th truth plus twice
    the bound.  (ii) no row left out: the score of every non-empty row through the EXISTING css_encoder_maxsim on the
    same matrices, then I == lexsort((id, -that)) and D equal to it in bits."""
    ms, qs = tc.gaussian(P)
    ix = _index(ms)
    live = np.flatnonzero(ms.lens > 0)
    d_mats = [ms.mat(int(r)) for r in live]
    worst = 0.0
    for j, q in enumerate(qs):
        t64 = ms.scores64(q)
        b = tc.bound(q, ms)
        oracle = np.full(N, -np.inf)
        oracle[live] = enc.maxsim([q], d_mats).astype(np.float64)
        for k in tc.KS:
            D_, I = ix.search_maxsim(q, k)
            what = f"P={P} query {j} k={k}"
            assert (I >= 0).all() and np.unique(I).size == k, what
            err = np.abs(D_[0].astype(np.float64) - t64[I[0]])
            worst = max(worst, float((err / b[I[0]]).max()))
            assert (err <= b[I[0]]).all(), (what, err.max())
            kth = np.sort(t64[live])[::-1][k - 1]
            slack = 2.0 * b.max()
            assert (t64[I[0]] >= kth - slack).all(), what
            rest = np.setdiff1d(live, I[0])
            assert (t64[rest] <= kth + slack).all(), what
            _check((D_, I), oracle, k, f"{what} against css_encoder_maxsim")
        got = ix.maxsim_ids(q, np.arange(N))
        assert np.array_equal(_bits(got), _bits(oracle.astype(np.float32))), f"P={P} query {j}: maxsim_ids of every row"
    print(f"[tokens gaussian] P={P}: largest |D - truth| / bound = {worst:.3e}")
    ix.close()


@pytest.mark.parametrize("P", (32, 96))
def test_maxsim_ids_equals_the_search_and_takes_any_order(P):
    ms, qs = tc.gaussian(P)
    ix = _index(ms.rows(np.arange(tc.T_PART)))
    ix.set_id_base(tc.ID_BASE)
    for q in qs:
        D_, I = ix.search_maxsim(q, 128)
        got = ix.maxsim_ids(q, I[0])
        assert np.array_equal(_bits(got), _bits(D_[0]))
        order = np.random.default_rng(3).permutation(128)
        ids = np.concatenate([I[0][order], I[0][:7], [tc.ID_BASE, tc.ID_BASE + tc.T_PART, tc.ID_BASE + N - 1]])
        got = ix.maxsim_ids(q, ids)
        assert np.array_equal(_bits(got[:128]), _bits(D_[0][order])) and np.array_equal(_bits(got[128:135]), _bits(D_[0][:7]))
        assert (got[135:] == -np.inf).all()                                     # an empty row, rows >= T
    assert ix.maxsim_ids(qs[0], []).shape == (0,)
    ix.close()

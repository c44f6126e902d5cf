"""GPU: the batched MaxSim search -- ``IndexFlat.search_maxsim_batch`` / ``last_maxsim_passes``
(``css_index_search_maxsim_batch``; kernels ``k_tok_scores_b<P, MT, NB, G>``, ``k_sparse_topk_cols`` and the part merge
behind it; a group of one query runs ``k_tok_scores``).

Truth is the float64 column and ONE ``lexsort`` of ``tests/tokens_fakes.py`` on the very arrays handed to the index,
never the code under test; the single call ``search_maxsim`` is checked IN ADDITION for byte equality.  The inputs are
those of ``tests/tokens_cases.py`` (N = 3 001 rows) and ``tests/tokens_codec_cases.py`` (N = 500);
``tests/test_tokens_batch_host.py`` proves on the CPU that the six queries of a lattice case have pairwise different
truths, so a batch that mixes up its slots fails here."""
import numpy as np
import pytest

import test_search_prior_gpu as tp
import test_tokens_codec_gpu as tcg
import tokens_cases as tc
import tokens_codec_cases as cc
from claude_semantic_search_amd import flat_index as fi
from tokens_fakes import topk

pytestmark = pytest.mark.gpu

N, D = tc.N, tc.D
FMAX = tp.FMAX
G = fi.MAXSIM_BATCH_GROUP


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


def _check_rows(res, cols, k, what, allowed=None, id_base=0):
    """Every row of D and I against its float64 column (exact in fp32 on lattice inputs) and ONE lexsort; no tolerance."""
    D_, I = res
    assert D_.dtype == np.float32 and I.dtype == np.int64 and D_.shape == I.shape == (len(cols), k), what
    hits = []
    for b, col in enumerate(cols):
        Dw, Iw = topk(col, k, allowed, id_base)
        assert np.array_equal(I[b:b + 1], Iw), f"{what} row {b}: ids differ from lexsort((id, -score)): {I[b][:8]} vs {Iw[0][:8]}"
        assert np.array_equal(_bits(D_[b:b + 1]), _bits(Dw)), f"{what} row {b}: D differs from the truth in bits"
        hits.append(int((I[b] >= 0).sum()))
    return hits


def _equals_single_calls(ix, res, qs, k, what, allow=None):
    for b, q in enumerate(qs):
        _same((res[0][b:b + 1], res[1][b:b + 1]), ix.search_maxsim(q, k, allow=allow), f"{what} row {b} against search_maxsim")


def _several_groups(qs):
    """The six queries tiled and permuted to nq = 2 G + 1: two full groups and a remainder of one."""
    nq = 2 * G + 1
    pick = np.random.default_rng(12).permutation(np.arange(nq) % len(qs))
    return pick, [qs[i] for i in pick]


# ------------------------------------------------------------------ lattice inputs: exact, one batch of mixed lengths
@pytest.mark.parametrize("P", tc.WIDTHS)
@pytest.mark.parametrize("family", tc.FAMILIES)
def test_lattice_batch_is_exact_and_equals_the_single_calls(family, P):
    ms, qs = tc.lattice(family, P)
    assert len(qs) % G != 0 and [q.shape[0] for q in qs] == list(tc.QUERY_LENS)   # mixed MT, an empty slot
    ix = _index(ms)
    cols = [ms.scores64(q) for q in qs]
    for k in tc.KS:
        res = ix.search_maxsim_batch(qs, k)
        assert _check_rows(res, cols, k, f"{family} P={P} k={k}") == [k] * len(qs)
        assert ix.last_maxsim_passes == -(-len(qs) // G)
        _equals_single_calls(ix, res, qs, k, f"{family} P={P} k={k}")
    ix.close()


@pytest.mark.parametrize("P", (32, 128))
def test_several_groups_and_a_remainder_of_one(P):
    ms, qs = tc.lattice("E", P)
    ix = _index(ms)
    pick, batch = _several_groups(qs)
    nq = len(batch)
    cols = [ms.scores64(q) for q in batch]
    for k in (10, 128):
        res = ix.search_maxsim_batch(batch, k)
        assert ix.last_maxsim_passes == -(-nq // G) == 3                         # a loop of single calls would scan nq times
        _check_rows(res, cols, k, f"P={P} k={k} nq={nq}")
        _equals_single_calls(ix, res, batch, k, f"P={P} k={k} nq={nq}")
        for a in range(nq):                                                     # equal queries in different slots and groups
            for b in range(a + 1, nq):
                if pick[a] == pick[b]:
                    _same((res[0][a], res[1][a]), (res[0][b], res[1][b]), f"P={P} k={k}: rows {a} and {b} hold the same query")
        back = ix.search_maxsim_batch(batch[::-1], k)
        _same(back, (res[0][::-1].copy(), res[1][::-1].copy()), f"P={P} k={k}: the reversed batch")
    for nq2 in (1, 2, G - 1, G, G + 1):                                         # every split into groups around G
        res = ix.search_maxsim_batch(batch[:nq2], 10)
        assert ix.last_maxsim_passes == -(-nq2 // G)
        _check_rows(res, cols[:nq2], 10, f"P={P} nq={nq2}")
    ix.close()


@pytest.mark.parametrize("P", (64, 96))
def test_one_mask_and_the_edge_cases(P):
    ms, qs = tc.lattice("T", P)
    ix = _index(ms)
    cols = [ms.scores64(q) for q in qs]
    allow = tc.half_mask()
    res = ix.search_maxsim_batch(qs, 10, allow=allow)
    _check_rows(res, cols, 10, f"P={P} masked", allowed=allow)
    _equals_single_calls(ix, res, qs, 10, f"P={P} masked", allow=allow)
    D_, I = ix.search_maxsim_batch(qs, 10, allow=np.zeros(N, bool))             # a mask that masks every row
    assert (I == -1).all() and (D_ == np.float32(-FMAX)).all()
    few = np.zeros(N, bool)
    few[[3, 0, 1, tc.PLANTS[0], 8]] = True                                      # row 0 is empty: 4 hits, then padding, in every row
    assert _check_rows(ix.search_maxsim_batch(qs, 10, allow=few), cols, 10, f"P={P} fewer than k hits", allowed=few) == [4] * len(qs)
    ix.set_id_base(tc.ID_BASE)
    res = ix.search_maxsim_batch(qs, 128)
    _check_rows(res, cols, 128, f"P={P} id_base", id_base=tc.ID_BASE)
    _equals_single_calls(ix, res, qs, 128, f"P={P} id_base")
    ix.set_id_base(0)
    ix.set_tokens(ms.rows(np.arange(tc.T_PART)).csr, row0=0)                    # rows >= T are misses
    part = ms.rows(np.arange(tc.T_PART)).padded(N)
    pcols = [part.scores64(q) for q in qs]
    assert all((c[tc.T_PART:] == -np.inf).all() for c in pcols)
    res = ix.search_maxsim_batch(qs, 128, allow=allow)
    _check_rows(res, pcols, 128, f"P={P} rows >= T", allowed=allow)
    _equals_single_calls(ix, res, qs, 128, f"P={P} rows >= T", allow=allow)
    ix.close()
    ms, q = tc.negative_case(P)                                                 # every dot negative
    ix = _index(ms)
    batch = [q, q[:1], q[1:], q]
    cols = [ms.scores64(b) for b in batch]
    assert all((c[ms.lens > 0] < 0).all() for c in cols)
    for k in tc.KS:
        assert _check_rows(ix.search_maxsim_batch(batch, k), cols, k, f"negative P={P} k={k}") == [k] * 4
    ix.close()


def test_an_index_without_matrices_and_an_empty_index_pad():
    ms, qs = tc.lattice("E", 64)
    ix = _index(ms)
    ix.search_maxsim_batch(qs, 10)
    assert ix.last_maxsim_passes == 1
    ix.drop_tokens()
    res = ix.search_maxsim_batch(qs, 10)
    assert (res[1] == -1).all() and (res[0] == np.float32(-FMAX)).all() and res[0].shape == (len(qs), 10)
    assert ix.last_maxsim_passes == 0
    _equals_single_calls(ix, res, qs, 10, "no matrices")
    ix.close()
    ix = tp._index(D, 0)                                                        # no rows at all
    res = ix.search_maxsim_batch(qs, 128)
    assert (res[1] == -1).all() and (res[0] == np.float32(-FMAX)).all() and res[1].shape == (len(qs), 128)
    assert ix.last_maxsim_passes == 0
    ix.close()


# ------------------------------------------------------------------ Gaussian unit rows: the single call's bytes
@pytest.mark.parametrize("P", tc.WIDTHS)
def test_gaussian_rows_equal_the_single_calls_on_every_grid(P):
    """The single call is pinned to css_encoder_maxsim by tests/test_tokens_index_gpu.py; the batch must give its bytes
    -- whatever the grid of k_tok_scores_b."""
    ms, qs = tc.gaussian(P)
    ix = _index(ms)
    _, batch = _several_groups(qs)
    want = [ix.search_maxsim(q, 128) for q in batch]
    want = (np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want]))
    allow = tc.half_mask()
    want_m = [ix.search_maxsim(q, 10, allow=allow) for q in qs]
    want_m = (np.concatenate([w[0] for w in want_m]), np.concatenate([w[1] for w in want_m]))
    for blocks in (0, 1, 2, 3, 0):
        ix.set_token_blocks(blocks)
        _same(ix.search_maxsim_batch(batch, 128), want, f"P={P} blocks={blocks}")
        _same(ix.search_maxsim_batch(qs, 10, allow=allow), want_m, f"P={P} blocks={blocks} masked")
    ix.close()


# ------------------------------------------------------------------ the compressed store
@pytest.mark.parametrize("C", (17, 300))
@pytest.mark.parametrize("nbits", cc.BITS)
@pytest.mark.parametrize("P", cc.WIDTHS)
def test_compressed_batch_is_exact_and_equals_the_single_calls(P, nbits, C):
    codec, ms, qs = cc.lattice(P, nbits, C)
    _, _, dec = tcg._double(codec, ms)
    ix = tcg._index(codec, ms)
    what = f"P={P} nbits={nbits} C={C}"
    cols = [dec.scores64(q) for q in qs]
    allow = cc.half_mask()
    for k in (10, 128):
        res = ix.search_maxsim_batch(qs, k)
        assert _check_rows(res, cols, k, f"{what} k={k}") == [k] * len(qs)
        _equals_single_calls(ix, res, qs, k, f"{what} k={k}")
    res = ix.search_maxsim_batch(qs, 10, allow=allow)
    _check_rows(res, cols, 10, f"{what} masked", allowed=allow)
    _equals_single_calls(ix, res, qs, 10, f"{what} masked", allow=allow)
    batch = [qs[i] for i in (4, 0, 3, 1, 2, 2, 0, 4, 1, 3, 4, 0, 2, 1, 3, 3, 0)][:2 * G + 1]
    bcols = [dec.scores64(q) for q in batch]
    want = ix.search_maxsim_batch(batch, 128)
    assert ix.last_maxsim_passes == -(-len(batch) // G)
    _check_rows(want, bcols, 128, f"{what} nq={len(batch)}")
    for blocks in (1, 2, 3, 0):
        ix.set_token_blocks(blocks)
        _same(ix.search_maxsim_batch(batch, 128), want, f"{what} blocks={blocks}")
    ix.close()


# ------------------------------------------------------------------ the library refuses before anything is enqueued
def test_the_library_refuses_and_the_index_stays_usable():
    from claude_semantic_search_amd import _native as nat

    ms, qs = tc.lattice("E", 64)
    ix = _index(ms)
    lib, h = nat.lib(), ix._handle()
    cols = [ms.scores64(q) for q in qs]

    def raw(mats, k=5, nq=None, P=64, off=None):
        o = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64) if off is None else np.asarray(off, np.int64)
        t = np.ascontiguousarray(np.concatenate(mats), np.uint16)
        n = len(mats) if nq is None else nq
        D_, I = np.empty(max(n, 1) * 129, np.float32), np.empty(max(n, 1) * 129, np.int64)
        return lib.css_index_search_maxsim_batch(h, t.ctypes.data, o.ctypes.data, n, P, k, None, D_.ctypes.data, I.ctypes.data)

    def usable():
        _check_rows(ix.search_maxsim_batch(qs, 10), cols, 10, "after a refused call")

    assert raw(qs, nq=0) == nat.CSS_ERR_INVALID and "nq=0" in nat.last_error(), nat.last_error()
    usable()
    big = [qs[0]] * 1025
    assert raw(big) == nat.CSS_ERR_INVALID and "nq=1025" in nat.last_error(), nat.last_error()
    usable()
    q32 = tc.lattice("E", 32)[1]
    assert raw(q32, P=32) == nat.CSS_ERR_INVALID and "P=32" in nat.last_error() and "P=64" in nat.last_error(), nat.last_error()
    usable()
    for k in (0, 129):
        assert raw(qs, k=k) == nat.CSS_ERR_INVALID and f"k={k}" in nat.last_error()
    assert raw(qs, P=48) == nat.CSS_ERR_INVALID and "P=48" in nat.last_error()
    assert raw([qs[0], qs[1]], off=[0, 1, 1]) == nat.CSS_ERR_INVALID and "query 1 has 0 tokens" in nat.last_error(), nat.last_error()
    assert raw([qs[0], np.zeros((65, 64), np.uint16)]) == nat.CSS_ERR_INVALID and "query 1 has 65 tokens" in nat.last_error()
    assert raw([qs[0], qs[1]], off=[1, 2, 16]) == nat.CSS_ERR_INVALID and "start" in nat.last_error()
    bad = qs[3].copy()
    bad[7, 3] = 0x7FC0
    assert raw([qs[0], qs[1], bad]) == nat.CSS_ERR_INVALID
    assert "token 7 of query 2" in nat.last_error() and "NaN" in nat.last_error(), nat.last_error()
    usable()
    assert raw([qs[5]] * 1024, k=1) == nat.CSS_OK and ix.last_maxsim_passes == -(-1024 // G)   # the largest batch
    ix.close()
    with pytest.raises(RuntimeError, match="freed"):
        ix.search_maxsim_batch(qs, 5)

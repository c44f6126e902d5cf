"""GPU: candidate generation for MaxSim on the codes -- ``IndexFlat.maxsim_candidates`` / ``search_maxsim_pruned``
(kernels ``k_tok_ctable<P>``, ``k_tok_ci<WP>``, the radix select ``k_sel_hist`` / ``k_sel_count`` / ``k_sel_write``, then
the existing ``k_tok_scores<P, MT, NB>`` over the candidate list).

Lattice inputs (tests/tokens_prune_cases.py; tests/test_tokens_prune_host.py proves that rows tie on the approximate
score across rank ncand, within and across the select's slices, that pruned answers differ from and equal the
exhaustive one, and that exact scores tie across rank k): no tolerance anywhere -- the candidate ids equal the double's
in bytes, ``approx`` and ``D`` equal the float64 truth in bits, ``I`` is ONE lexsort.  Arbitrary inputs: the oracle of
``approx`` is the library's EXISTING ``css_encoder_maxsim`` of ``centroids[codes]`` and ``maxsim_ids`` of an
uncompressed index that holds those matrices."""
import ctypes

import numpy as np
import pytest

import bert_reference as br
import test_search_prior_gpu as tp
import tokens_codec_cases as cc
import tokens_prune_cases as pc
from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd import flat_index as fi
from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder
from tokens_fakes import Matrices

pytestmark = pytest.mark.gpu

N, D = cc.N, cc.D
FMAX = tp.FMAX


def _index(codec=None, ms=None, n=N):
    ix = tp._index(D, 0, tp._rows(N, D, 11)[:n])
    if codec is not None:
        ix.set_token_codec(codec)
    if ms is not None:
        ix.set_tokens(ms.csr)
    return ix


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b, what):
    for j, (u, v) in enumerate(zip(a, b)):
        assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(_bits(u), _bits(v)), f"{what}: array {j} differs"


def _check_cands(got, a64, ncand, what, allowed=None, id_base=0):
    """ids in bytes against ONE lexsort of the float64 column, approx in bits against it."""
    ids, approx = got
    want = pc.candidates64(a64, ncand, allowed)
    assert ids.dtype == np.int64 and approx.dtype == np.float32 and ids.shape == approx.shape, what
    assert np.array_equal(ids, want + id_base), f"{what}: {ids.size} candidate ids differ from the double's {want.size}"
    assert np.array_equal(_bits(approx), _bits(a64[want].astype(np.float32))), f"{what}: approx differs from the truth in bits"
    return ids.size


def _check_pruned(ix, q, a64, e64, k, ncand, what, allowed=None, id_base=0):
    D_, I = ix.search_maxsim_pruned(q, k, ncand, allow=allowed)
    Dw, Iw = pc.pruned64(a64, e64, k, ncand, allowed, id_base)
    assert D_.dtype == np.float32 and I.dtype == np.int64 and D_.shape == I.shape == (1, k), what
    assert np.array_equal(I, Iw), f"{what}: ids differ from the lexsort over the candidates: {I[0][:8]} vs {Iw[0][:8]}"
    assert np.array_equal(_bits(D_), _bits(Dw)), f"{what}: D differs from the truth in bits"
    hit = I[0] >= 0
    if hit.any():
        assert np.array_equal(_bits(D_[0][hit]), _bits(ix.maxsim_ids(q, I[0][hit]))), f"{what}: D is not maxsim_ids(q, I)"
    return D_, I


# ------------------------------------------------------------------ lattice inputs: bytes and bits, no tolerance
@pytest.mark.parametrize("C", cc.CENTROIDS)
@pytest.mark.parametrize("nbits", cc.BITS)
@pytest.mark.parametrize("P", cc.WIDTHS)
def test_lattice_candidates_and_pruned_answers_are_exact(P, nbits, C):
    codec, ms, qs, codes, res = pc.lattice_codes(P, nbits, C)
    ix = _index(codec, ms)
    _same(ix.get_token_codes(), (ms.off, codes, res), "the device's codes are the double's")
    what = f"P={P} nbits={nbits} C={C}"
    allow = cc.half_mask()
    cols = [(pc.approx64(codec, ms.off, codes, q), pc.exact64(codec, ms, codes, res, q)) for q in qs]
    for j, q in enumerate(qs):
        a64, e64 = cols[j]
        live = int((a64 > -np.inf).sum())
        a32 = fi.token_codec_approx(codec, ms.off, codes, q)
        for ncand in (1, 10) + pc.NCANDS:
            got = ix.maxsim_candidates(q, ncand)
            assert _check_cands(got, a64, ncand, f"{what} query {j} ncand={ncand}") == min(ncand, live)
            _same(got, fi.maxsim_candidates_numpy(a32, ncand), f"{what} query {j} ncand={ncand}: the numpy double")
        _check_cands(ix.maxsim_candidates(q, 100, allow=allow), a64, 100, f"{what} query {j} masked", allowed=allow)
        for k in pc.KS:
            for ncand in sorted({k, 16, 100, 499, 500, 65536}):
                if ncand < k:
                    continue
                res_p = _check_pruned(ix, q, a64, e64, k, ncand, f"{what} query {j} k={k} ncand={ncand}")
                _same(res_p, fi.search_maxsim_pruned_numpy(codec, ms.off, codes, res, q, k, ncand),
                      f"{what} query {j} k={k} ncand={ncand}: the numpy double")
                if ncand >= live:
                    _same(res_p, ix.search_maxsim(q, k), f"{what} query {j} k={k} ncand={ncand}: search_maxsim")
        _check_pruned(ix, q, a64, e64, 10, 16, f"{what} query {j} masked", allowed=allow)
        _same(ix.search_maxsim_pruned(q, 10, 500, allow=allow), ix.search_maxsim(q, 10, allow=allow),
              f"{what} query {j} masked, every allowed row a candidate")
    ix.close()


def test_the_same_bytes_whatever_the_grid():
    for P, nbits, C in ((32, 1, 17), (128, 2, 300), (96, 4, 256)):
        codec, ms, qs, codes, res = pc.lattice_codes(P, nbits, C)
        ix = _index(codec, ms)
        for j, q in enumerate(qs):
            a64, e64 = pc.approx64(codec, ms.off, codes, q), pc.exact64(codec, ms, codes, res, q)
            for blocks in (1, 2, 3, 0):
                ix.set_token_blocks(blocks)
                _check_cands(ix.maxsim_candidates(q, 65536), a64, 65536, f"P={P} query {j} on {blocks} blocks")
                _check_cands(ix.maxsim_candidates(q, 100), a64, 100, f"P={P} query {j} on {blocks} blocks")
                _check_pruned(ix, q, a64, e64, 128, 128, f"P={P} query {j} on {blocks} blocks")
        ix.close()


def test_masks_id_base_rows_without_matrices_and_padding():
    P, nbits, C = 64, 2, 17
    codec, ms, qs, codes, res = pc.lattice_codes(P, nbits, C)
    ix = _index(codec, ms)
    q = qs[2]
    a64, e64 = pc.approx64(codec, ms.off, codes, q), pc.exact64(codec, ms, codes, res, q)
    none = np.zeros(N, bool)                                                    # a mask that masks every row
    ids, approx = ix.maxsim_candidates(q, 100, allow=none)
    assert ids.shape == (0,) and approx.shape == (0,)
    D_, I = ix.search_maxsim_pruned(q, 10, 100, allow=none)
    assert (I == -1).all() and (D_ == np.float32(-FMAX)).all()
    few = np.zeros(N, bool)
    few[[3, 0, 1, 6, 5]] = True                                                 # row 0 is empty: 4 candidates, then padding
    assert _check_cands(ix.maxsim_candidates(q, 100, allow=few), a64, 100, "fewer than ncand", allowed=few) == 4
    D_, I = _check_pruned(ix, q, a64, e64, 10, 100, "fewer than k candidates", allowed=few)
    assert int((I >= 0).sum()) == 4 and (D_[0][4:] == np.float32(-FMAX)).all()
    D_, I = _check_pruned(ix, q, a64, e64, 10, 10, "k = ncand", allowed=few)
    ix.set_id_base(cc.ID_BASE)
    _check_cands(ix.maxsim_candidates(q, 16), a64, 16, "id_base", id_base=cc.ID_BASE)
    _check_pruned(ix, q, a64, e64, 128, 499, "id_base", id_base=cc.ID_BASE)
    ix.set_id_base(0)
    ix.set_tokens(ms.rows(np.arange(cc.T_PART)).csr, row0=0)                    # rows >= T are misses
    part = Matrices(ms.off[:cc.T_PART + 1], ms.tok[:ms.off[cc.T_PART]]).padded(N)
    pcodes, pres = codes[:ms.off[cc.T_PART]], res[:ms.off[cc.T_PART]]
    pa, pe = pc.approx64(codec, part.off, pcodes, q), pc.exact64(codec, part, pcodes, pres, q)
    assert (pa[cc.T_PART:] == -np.inf).all()
    n = _check_cands(ix.maxsim_candidates(q, 65536), pa, 65536, "rows >= T")
    assert n == int((part.lens > 0).sum())
    _check_pruned(ix, q, pa, pe, 100, 100, "rows >= T")
    _same(ix.search_maxsim_pruned(q, 128, 65536), ix.search_maxsim(q, 128), "rows >= T, every row a candidate")
    ix.close()


@pytest.mark.parametrize("nbits", cc.BITS)
@pytest.mark.parametrize("P", (32, 128))
def test_a_query_whose_every_dot_is_negative(P, nbits):
    codec, ms, q = cc.negative_case(P, nbits)
    codes, res = fi.token_codec_encode(codec, ms.tok)
    ix = _index(codec, ms)
    a64, e64 = pc.approx64(codec, ms.off, codes, q), pc.exact64(codec, ms, codes, res, q)
    assert (a64[ms.lens > 0] < 0).all() and (e64[ms.lens > 0] < 0).all()
    for ncand in (1, 16, 100, 65536):
        _check_cands(ix.maxsim_candidates(q, ncand), a64, ncand, f"negative P={P} nbits={nbits} ncand={ncand}")
    for k in pc.KS:
        _check_pruned(ix, q, a64, e64, k, 128, f"negative P={P} nbits={nbits} k={k}")
        _same(ix.search_maxsim_pruned(q, k, 500), ix.search_maxsim(q, k), "negative: every row a candidate")
    ix.close()


def test_a_codec_without_matrices_and_an_index_without_a_codec():
    codec, ms, qs = cc.lattice(64, 2, 17)
    q = qs[2]
    ix = _index(codec)                                                          # a codec, no matrices
    ids, approx = ix.maxsim_candidates(q, 100)
    assert ids.shape == (0,) and approx.shape == (0,)
    D_, I = ix.search_maxsim_pruned(q, 10, 100)
    assert (I == -1).all() and (D_ == np.float32(-FMAX)).all()
    lib, h = nat.lib(), ix._handle()
    Dk, Ik = np.zeros(10, np.float32), np.zeros(10, np.int64)
    for k, ncand, word in ((10, 0, "ncand=0"), (10, 65537, "ncand=65537"), (0, 10, "k=0"), (129, 1000, "k=129"),
                           (10, 9, "k=10 exceeds ncand=9")):
        rc = lib.css_index_search_maxsim_pruned(h, q.ctypes.data, q.shape[0], 64, k, ncand, None, Dk.ctypes.data, Ik.ctypes.data, None)
        assert rc == nat.CSS_ERR_INVALID and word in nat.last_error(), nat.last_error()
    rc = lib.css_index_search_maxsim_pruned(h, q.ctypes.data, q.shape[0] // 2, 32, 10, 10, None, Dk.ctypes.data, Ik.ctypes.data, None)
    assert rc == nat.CSS_ERR_INVALID and "P=32" in nat.last_error(), nat.last_error()
    with pytest.raises(ValueError, match="ncand"):
        ix.maxsim_candidates(q, 0)
    with pytest.raises(ValueError, match="exceeds ncand"):
        ix.search_maxsim_pruned(q, 11, 10)
    ix.close()
    plain = _index(None, ms)                                                    # matrices, no codec
    for call in (lambda: plain.maxsim_candidates(q, 100), lambda: plain.search_maxsim_pruned(q, 10, 100)):
        with pytest.raises(ValueError, match="no token codec"):
            call()
    h = plain._handle()
    n = ctypes.c_int64(7)
    ids, ap = np.zeros(100, np.int64), np.zeros(100, np.float32)
    rc = lib.css_index_maxsim_candidates(h, q.ctypes.data, q.shape[0], 64, 100, None, ids.ctypes.data, ap.ctypes.data, ctypes.byref(n))
    assert rc == nat.CSS_ERR_INVALID and "has no token codec" in nat.last_error(), nat.last_error()
    rc = lib.css_index_search_maxsim_pruned(h, q.ctypes.data, q.shape[0], 64, 10, 100, None, Dk.ctypes.data, Ik.ctypes.data, None)
    assert rc == nat.CSS_ERR_INVALID and "has no token codec" in nat.last_error(), nat.last_error()
    plain.close()


# ------------------------------------------------------------------ the wide case: the select over ten slices
def test_the_wide_case_selects_the_doubles_candidates():
    codec, ms, q, codes, res = pc.wide()
    ix = tp._index(D, 0, tp._rows(pc.WIDE_N, D, 12))
    ix.set_token_codec(codec)
    ix.set_token_codes(ms.off, codes, res)
    a64 = pc.approx64(codec, ms.off, codes, q)
    live = int((a64 > -np.inf).sum())
    allow = np.random.default_rng(3).random(pc.WIDE_N) < 0.7
    for ncand in pc.WIDE_NCANDS:
        got = ix.maxsim_candidates(q, ncand)
        assert _check_cands(got, a64, ncand, f"wide ncand={ncand}") == min(ncand, live)
        _check_cands(ix.maxsim_candidates(q, ncand, allow=allow), a64, ncand, f"wide masked ncand={ncand}", allowed=allow)
    e64 = pc.exact64(codec, ms, codes, res, q)
    _check_pruned(ix, q, a64, e64, 128, 4097, "wide k=128 ncand=4097")
    _same(ix.search_maxsim_pruned(q, 128, 65536), ix.search_maxsim(q, 128), "wide: every row a candidate")
    ix.close()


# ------------------------------------------------------------------ arbitrary inputs with a trained codec
@pytest.fixture(scope="module")
def enc():
    cfg = br.BertCfg(num_layers=2, vocab=1000, **br.SMALL)
    e = MpnetEncoder(synthetic_seed=1, cfg_overrides=cfg.encoder_overrides())
    yield e
    e.close()


@pytest.mark.parametrize("P", cc.WIDTHS)
@pytest.mark.parametrize("kind", ("clustered", "gaussian"))
def test_arbitrary_approx_equals_css_encoder_maxsim_of_the_centroid_matrices(enc, kind, P):
    """approx of every non-empty row equals, in bits, (a) the EXISTING css_encoder_maxsim of centroids[codes] and (b)
    maxsim_ids of an uncompressed index that holds those matrices; the pruned D equals maxsim_ids in bits; the
    candidate set is the double's, given the device's approx column."""
    ms, qs = cc.arbitrary(kind, P)
    codec = fi.train_token_codec(ms.csr, 256, nbits=2, niter=5, seed=3)
    ix = _index(codec, ms)
    off, codes, res = ix.get_token_codes()
    cm = Matrices(off, fi.f32_to_bf16_rne(codec.centroids[codes]))              # the matrices centroids[codes]
    live = np.flatnonzero(ms.lens > 0)
    c_mats = [cm.mat(int(r)) for r in live]
    plain = _index(None, cm)
    for j, q in enumerate(qs):
        ids, approx = ix.maxsim_candidates(q, 65536)
        assert np.array_equal(ids, live), f"query {j}: every non-empty row is a candidate, ascending"
        oracle = enc.maxsim([q], c_mats)
        assert np.array_equal(_bits(approx), _bits(oracle)), f"query {j}: approx against css_encoder_maxsim of centroids[codes]"
        assert np.array_equal(_bits(approx), _bits(plain.maxsim_ids(q, live))), f"query {j}: against the uncompressed index"
        col = np.full(N, -np.inf, np.float32)
        col[live] = approx
        for ncand in (1, 16, 100):
            _same(ix.maxsim_candidates(q, ncand), fi.maxsim_candidates_numpy(col, ncand), f"query {j} ncand={ncand}")
            D_, I = ix.search_maxsim_pruned(q, 10, max(ncand, 10))
            cand, _ = fi.maxsim_candidates_numpy(col, max(ncand, 10))
            sc = ix.maxsim_ids(q, cand)
            order = np.lexsort((cand, -sc))[:10]
            assert np.array_equal(I[0], cand[order]) and np.array_equal(_bits(D_[0]), _bits(sc[order])), f"query {j} ncand={ncand}"
            assert np.array_equal(_bits(D_[0]), _bits(ix.maxsim_ids(q, I[0])))
        _same(ix.search_maxsim_pruned(q, 128, 500), ix.search_maxsim(q, 128), f"query {j}: every row a candidate")
    plain.close()
    ix.close()


# ------------------------------------------------------------------ life cycle
def test_after_remove_ids_and_after_appending_rows_the_answer_is_a_fresh_index():
    P, nbits, C = 96, 2, 300
    codec, ms, qs, codes, res = pc.lattice_codes(P, nbits, C)
    x = tp._rows(N, D, 11)
    ix = tp._index(D, 0, x[:300])
    ix.set_token_codec(codec)
    ix.set_tokens(ms.rows(np.arange(300)).csr)
    for q in qs[1:4]:
        ix.search_maxsim_pruned(q, 10, 16)                                      # the workspaces are in use before the growth
    ix.add(x[300:])
    ix.set_tokens(ms.rows(np.arange(300, N)).csr)
    fresh = _index(codec, ms)
    for j, q in enumerate(qs):
        for ncand in (16, 100, 65536):
            _same(ix.maxsim_candidates(q, ncand), fresh.maxsim_candidates(q, ncand), f"appended, query {j} ncand={ncand}")
            _same(ix.search_maxsim_pruned(q, 10, ncand), fresh.search_maxsim_pruned(q, 10, ncand), f"appended, query {j}")
    fresh.close()
    gone = np.flatnonzero(np.random.default_rng(9).random(N) < 1.0 / 3.0)
    keep = np.ones(N, bool)
    keep[gone] = False
    assert ix.remove_ids(gone) == gone.shape[0]
    fresh = tp._index(D, 0, x[keep])
    fresh.set_token_codec(codec)
    fresh.set_tokens(ms.rows(np.flatnonzero(keep)).csr)
    for j, q in enumerate(qs):
        for ncand in (16, 100, 65536):
            _same(ix.maxsim_candidates(q, ncand), fresh.maxsim_candidates(q, ncand), f"removed, query {j} ncand={ncand}")
            _same(ix.search_maxsim_pruned(q, 10, ncand), fresh.search_maxsim_pruned(q, 10, ncand), f"removed, query {j}")
    fresh.close()
    ix.close()

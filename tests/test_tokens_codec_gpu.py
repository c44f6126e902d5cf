"""GPU: compressed token matrices on the flat index -- ``IndexFlat.set_token_codec`` / ``get_token_codec`` /
``token_codec_bits`` / ``get_token_codes`` / ``set_token_codes`` and ``set_tokens`` / ``get_tokens`` / ``search_maxsim`` /
``maxsim_ids`` / ``remove_ids`` on an index with a codec (kernels ``k_tok_encode<P>``, ``k_tok_decode``,
``k_tok_scores<P, MT, NB>``, ``k_tok_move_units``).

Lattice inputs (tests/tokens_codec_cases.py; tests/test_tokens_codec_host.py proves that they contain tied centroids,
residuals on cutoffs and scores tied across rank k): no tolerance anywhere -- codes and decoded tokens equal the numpy
double in bytes, D equals the float64 truth in bits, I is ONE lexsort.  Arbitrary inputs: the oracle is the library's
EXISTING ``css_encoder_maxsim`` over ``get_tokens()`` and an uncompressed index filled with ``get_tokens()``."""
import numpy as np
import pytest

import bert_reference as br
import test_search_prior_gpu as tp
import tokens_codec_cases as cc
from claude_semantic_search_amd import flat_index as fi
from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder
from tokens_fakes import Matrices, topk

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


def _check(res, col, k, what, allowed=None, id_base=0):
    """D and I against the float64 column (exact in fp32 on lattice inputs) and ONE lexsort; no tolerance."""
    D_, I = res
    Dw, Iw = topk(col, k, allowed, id_base)
    assert D_.dtype == np.float32 and I.dtype == np.int64 and D_.shape == I.shape == (1, k), what
    assert np.array_equal(I, Iw), f"{what}: ids differ from lexsort((id, -score)) over the hit rows: {I[0][:8]} vs {Iw[0][:8]}"
    assert np.array_equal(_bits(D_), _bits(Dw)), f"{what}: D differs from the truth in bits"
    return int((I >= 0).sum())


def _double(codec, ms):
    """(codes, res, decoded Matrices) of the numpy double."""
    codes, res = fi.token_codec_encode(codec, ms.tok)
    return codes, res, Matrices(ms.off, fi.token_codec_decode(codec, codes, res))


# ------------------------------------------------------------------ lattice inputs: bytes and bits, no tolerance
@pytest.mark.parametrize("C", cc.CENTROIDS)
@pytest.mark.parametrize("nbits", cc.BITS)
@pytest.mark.parametrize("P", cc.WIDTHS)
def test_lattice_codes_tokens_and_scores_are_exact(P, nbits, C):
    codec, ms, qs = cc.lattice(P, nbits, C)
    codes, res, dec = _double(codec, ms)
    ix = _index(codec, ms)
    what = f"P={P} nbits={nbits} C={C}"
    assert ix.token_codec_bits == nbits and ix.token_rows == N and ix.token_dim == P
    got = ix.get_token_codec()
    _same([got.centroids, got.cutoffs, got.weights], [codec.centroids, codec.cutoffs, codec.weights], f"{what}: get_token_codec")
    assert got.nbits == nbits
    _same(ix.get_token_codes(), (ms.off, codes, res), f"{what}: get_token_codes against the numpy double")
    _same(ix.get_tokens(), (dec.off, dec.tok), f"{what}: get_tokens against the numpy decode")
    o1, c1, r1 = ix.get_token_codes(5, 3)                                       # a range
    assert o1.tolist() == (ms.off[5:9] - ms.off[5]).tolist() and np.array_equal(c1, codes[ms.off[5]:ms.off[8]])
    assert np.array_equal(r1, res[ms.off[5]:ms.off[8]])
    allow = cc.half_mask()
    cols = [dec.scores64(q) for q in qs]
    for j, q in enumerate(qs):
        for k in cc.KS:
            assert _check(ix.search_maxsim(q, k), cols[j], k, f"{what} query {j} k={k}") == k
        _check(ix.search_maxsim(q, 10, allow=allow), cols[j], 10, f"{what} query {j} masked", allowed=allow)
    for blocks in (1, 2, 3, 0):                                                 # the same bits whatever the grid
        ix.set_token_blocks(blocks)
        for j, q in enumerate(qs):
            _check(ix.search_maxsim(q, 128), cols[j], 128, f"{what} query {j} on {blocks} blocks")
    q, col = qs[2], cols[2]
    D_, I = ix.search_maxsim(q, 10, allow=np.zeros(N, bool))                    # a mask that masks every row
    assert (I == -1).all() and (D_ == np.float32(-FMAX)).all()
    few = np.zeros(N, bool)
    few[[3, 0, 1, 6, 5]] = True                                                 # row 0 is empty: 4 hits, then padding
    assert _check(ix.search_maxsim(q, 10, allow=few), col, 10, f"{what}: fewer than k hits", allowed=few) == 4
    ix.set_id_base(cc.ID_BASE)
    _check(ix.search_maxsim(q, 128), col, 128, f"{what}: id_base", id_base=cc.ID_BASE)
    ids = np.array([5, 0, 8, 5, N - 1, 6, 3, 499, 7, 7, 2])                     # repeats, out of order, an empty row
    got = ix.maxsim_ids(q, ids + cc.ID_BASE)
    assert np.array_equal(_bits(got), _bits(col[ids].astype(np.float32))) and got[1] == -np.inf, f"{what}: maxsim_ids"
    ix.set_id_base(0)
    # the codes into a fresh index with the same codec: the same search bytes
    fresh = _index(codec)
    fresh.set_token_codes(*ix.get_token_codes())
    _same(fresh.get_token_codes(), (ms.off, codes, res), f"{what}: set_token_codes round trip")
    for j, q in enumerate(qs):
        _same(fresh.search_maxsim(q, 128), ix.search_maxsim(q, 128), f"{what} query {j}: an index loaded from codes")
    fresh.close()
    ix.set_tokens(ms.rows(np.arange(cc.T_PART)).csr, row0=0)                    # rows >= T are misses
    part = Matrices(dec.off[:cc.T_PART + 1], dec.tok[:dec.off[cc.T_PART]]).padded(N).scores64(q)
    assert (part[cc.T_PART:] == -np.inf).all()
    _check(ix.search_maxsim(q, 128), part, 128, f"{what}: rows >= T")
    ix.close()


@pytest.mark.parametrize("nids", (1, 5, 70))
def test_maxsim_ids_of_a_few_rows_equals_search_maxsim_over_them(nids):
    """A list so short that a wave's turn is ONE row (the default grid has more waves than 70 rows; one wave, five
    waves, more than one block), on the codes: the same bits as the scan, whose turns are 16 rows, gives those rows."""
    codec, ms, qs = cc.lattice(32, 2, 17)
    ix = _index(codec, ms)
    ids = np.random.default_rng(nids).permutation(N)[:nids]
    allow = np.zeros(N, bool)
    allow[ids] = True
    for j, q in enumerate(qs):
        D_, I = ix.search_maxsim(q, 128, allow=allow)
        want = np.full(N, -np.inf, np.float32)
        want[I[I >= 0]] = D_[I >= 0]
        assert (I >= 0).sum() == (ms.lens[ids] > 0).sum()
        assert np.array_equal(_bits(ix.maxsim_ids(q, ids)), _bits(want[ids])), f"query {j}, {nids} ids"
    ix.close()


@pytest.mark.parametrize("nbits", cc.BITS)
@pytest.mark.parametrize("P", (32, 128))
def test_a_query_whose_every_dot_is_negative(P, nbits):
    codec, ms, q = cc.negative_case(P, nbits)
    _, _, dec = _double(codec, ms)
    ix = _index(codec, ms)
    col = dec.scores64(q)
    assert (col[ms.lens > 0] < 0).all()
    for k in cc.KS:
        assert _check(ix.search_maxsim(q, k), col, k, f"negative P={P} nbits={nbits} k={k}") == k
    ix.close()


# ------------------------------------------------------------------ arbitrary inputs with a trained codec
@pytest.fixture(scope="module")
def enc():
    cfg = br.BertCfg(num_layers=2, vocab=1000, **br.SMALL)
    e = MpnetEncoder(synthetic_seed=1, cfg_overrides=cfg.encoder_overrides())
    yield e
    e.close()


@pytest.mark.parametrize("nbits", cc.BITS)
@pytest.mark.parametrize("P", cc.WIDTHS)
@pytest.mark.parametrize("kind", ("clustered", "gaussian"))
def test_arbitrary_rows_equal_css_encoder_maxsim_and_an_uncompressed_index_of_the_decoded_matrices(enc, kind, P, nbits):
    """The score of every non-empty row over the compressed store equals, in bits, (a) the EXISTING css_encoder_maxsim
    over get_tokens() and (b) search_maxsim / maxsim_ids of an uncompressed index filled with get_tokens().  Given the
    device's codes, the buckets and the decoded values equal the numpy double in bytes.

    The codes are checked by a bound, not by equality.  Both operands of a dot are bf16, so the P products are exact in
    fp32; an fp32 dot of P exact products in any order errs by at most 2^-23 P c, with c = ||d|| ||c|| bounding every
    sum of |products| (the per-dot bound of tests/test_maxsim_gpu.py).  The device picks the largest fp32 dot, so its
    exact (float64) dot falls short of the exact maximum by at most one such error on each of the two dots compared:
    2 * 2^-23 P ||d|| max ||c|| -- 3.1e-5 for unit operands at P = 128 (``tokens_codec_cases.assign_bound``).
    Measured on these inputs (MI355X, all 24 cases of about 10 500 tokens each): the device's shortfall is 0 for every
    token, the numpy float32 restatement (``token_codec_assign``, another summation order) needs 0 as well, and the two
    agree on every code -- the best and the second-best centroid of a unit token are never within 3e-5 here.  The slack
    each needs is printed."""
    ms, qs = cc.arbitrary(kind, P)
    codec = fi.train_token_codec(ms.csr, 256, nbits=nbits, niter=5, seed=3)
    assert codec.centroids.shape == (256, P) and codec.nbits == nbits
    ix = _index(codec, ms)
    off, codes, res = ix.get_token_codes()
    assert np.array_equal(off, ms.off) and codes.max() < 256
    _, want_res = fi.token_codec_encode(codec, ms.tok, codes=codes)
    assert np.array_equal(res, want_res), "buckets: the device against the numpy double, given the device's codes"
    doff, dtok = ix.get_tokens()
    assert np.array_equal(doff, ms.off) and np.array_equal(dtok, fi.token_codec_decode(codec, codes, res)), "decoded values"
    # the codes by the derived bound
    d64 = cc.dots64(codec, ms.tok)
    b = cc.assign_bound(P, ms.tok, codec)
    short = d64.max(axis=1) - d64[np.arange(d64.shape[0]), codes]
    short_np = d64.max(axis=1) - d64[np.arange(d64.shape[0]), fi.token_codec_assign(codec, ms.tok)]
    print(f"[tokens codec] {kind} P={P} nbits={nbits}: shortfall / bound: device {float((short / b).max()):.3e}, "
          f"numpy float32 restatement {float((short_np / b).max()):.3e}; codes differing from numpy: "
          f"{int((codes != fi.token_codec_assign(codec, ms.tok)).sum())} of {codes.shape[0]}")
    assert (short >= 0).all() and (short <= b).all(), float((short / b).max())
    # the scores
    dec = Matrices(doff, dtok)
    live = np.flatnonzero(ms.lens > 0)
    d_mats = [dec.mat(int(r)) for r in live]
    plain = _index(None, dec)
    assert plain.token_codec_bits == 0
    for j, q in enumerate(qs):
        oracle = np.full(N, -np.inf)
        oracle[live] = enc.maxsim([q], d_mats).astype(np.float64)
        got = ix.maxsim_ids(q, np.arange(N))
        assert np.array_equal(_bits(got), _bits(oracle.astype(np.float32))), f"query {j}: maxsim_ids against css_encoder_maxsim"
        assert np.array_equal(_bits(got), _bits(plain.maxsim_ids(q, np.arange(N)))), f"query {j}: against the uncompressed index"
        for k in (10, 128):
            res_c = ix.search_maxsim(q, k)
            _check(res_c, oracle, k, f"query {j} k={k} against css_encoder_maxsim")
            _same(res_c, plain.search_maxsim(q, k), f"query {j} k={k} against the uncompressed index")
    plain.close()
    ix.close()


# ------------------------------------------------------------------ life cycle
def test_the_codec_is_refused_while_matrices_exist_and_survives_drop_and_reset():
    from claude_semantic_search_amd import _native as nat

    codec, ms, qs = cc.lattice(64, 2, 17)
    other = cc.lattice_codec(64, 4, 300)
    ix = _index(None, ms)                                                       # raw matrices: no codec may come
    with pytest.raises(nat.CssError, match="rows have token matrices"):
        ix.set_token_codec(codec)
    with pytest.raises(ValueError, match="no token codec"):
        ix.get_token_codes()
    assert ix.token_codec_bits == 0 and ix.get_token_codec() is None
    ix.drop_tokens()
    ix.set_token_codec(codec)
    ix.set_tokens(ms.csr)
    for c in (other, None):                                                      # ... nor go, nor change
        with pytest.raises(nat.CssError, match="rows have token matrices"):
            ix.set_token_codec(c)
    assert ix.token_codec_bits == 2
    with pytest.raises(nat.CssError, match="codec has P=64"):
        ix.set_tokens(cc.lattice(32, 2, 17)[1].rows(np.arange(5)).csr, row0=0)
    assert ix.token_rows == N
    off, codes, res = ix.get_token_codes()
    bad = codes.copy()
    r = 9 + int(np.flatnonzero(ms.lens[9:] > 0)[0])
    bad[int(off[r])] = 17                                                       # the first token of row r
    with pytest.raises(ValueError, match=f"row {r} "):
        ix.set_token_codes(off, bad, res, row0=0)
    lib, h = nat.lib(), ix._handle()
    assert lib.css_index_set_token_codes(h, 0, N, off.ctypes.data, bad.ctypes.data, res.ctypes.data) == nat.CSS_ERR_INVALID
    assert f"token 0 of row {r} has code 17" in nat.last_error(), nat.last_error()
    _same(ix.get_token_codes(), (off, codes, res), "a refused call changed the codes")
    cent = codec.centroids.copy()
    ix.drop_tokens()
    assert ix.token_codec_bits == 2 and ix.token_rows == 0, "drop_tokens keeps the codec"
    for badc, word in (((cent, 3, codec.cutoffs, codec.weights), "nbits=3"), ((cent[:, :48], 2, codec.cutoffs, codec.weights), "P=48")):
        c, nb, cut, w = badc
        c = np.ascontiguousarray(c)
        rc = lib.css_index_set_token_codec(h, c.ctypes.data, c.shape[0], c.shape[1], nb, cut.ctypes.data, w.ctypes.data)
        assert rc == nat.CSS_ERR_INVALID and word in nat.last_error(), nat.last_error()
    notbf = cent.copy()
    notbf[1, 2] = np.float32(1.0 + 2.0 ** -12)
    assert lib.css_index_set_token_codec(h, notbf.ctypes.data, 17, 64, 2, codec.cutoffs.ctypes.data,
                                         codec.weights.ctypes.data) == nat.CSS_ERR_INVALID
    assert "component 2 of centroid 1 is not a bf16 value" in nat.last_error(), nat.last_error()
    desc = np.array([0.1, 0.0, 0.2], np.float32)
    assert lib.css_index_set_token_codec(h, cent.ctypes.data, 17, 64, 2, desc.ctypes.data,
                                         codec.weights.ctypes.data) == nat.CSS_ERR_INVALID and "ascend" in nat.last_error()
    assert lib.css_index_set_token_codec(h, cent.ctypes.data, 0, 64, 2, codec.cutoffs.ctypes.data,
                                         codec.weights.ctypes.data) == nat.CSS_ERR_INVALID and "C=0" in nat.last_error()
    assert ix.token_codec_bits == 2                                             # refused calls changed nothing
    ix.set_tokens(ms.csr)
    _same(ix.get_token_codes(), (off, codes, res), "after drop_tokens: the same codec encodes the same bytes")
    ix.reset()
    assert ix.token_codec_bits == 2 and ix.token_rows == 0, "reset keeps the codec"
    ix.add(tp._rows(N, D, 11))
    ix.set_tokens(ms.csr)
    _same(ix.get_token_codes(), (off, codes, res), "after reset")
    ix.drop_tokens()
    ix.set_token_codec(other)                                                   # no matrices: the codec may change ...
    assert ix.token_codec_bits == 4 and ix.get_token_codec().centroids.shape == (300, 64)
    ix.set_token_codec(None)                                                    # ... and go: raw storage again
    assert ix.token_codec_bits == 0
    ix.set_tokens(ms.csr)
    _same(ix.get_tokens(), (ms.off, ms.tok), "an index whose codec was cleared stores raw matrices")
    ix.close()


def test_append_growth_and_rewrite_from_row_0():
    codec, ms, qs = cc.lattice(96, 2, 300)
    codes, res, dec = _double(codec, ms)
    x = tp._rows(N, D, 11)
    ix = tp._index(D, 0, x[:200])
    ix.set_token_codec(codec)
    ix.set_tokens(ms.rows(np.arange(60)).mats())                                # in pieces, the list form ...
    ix.set_tokens(ms.rows(np.arange(60, 150)).csr)                              # ... and the CSR form
    want = (ms.off[:151], codes[:ms.off[150]], res[:ms.off[150]])
    got = ix.get_token_codes(0, 150)
    _same(got, want, "append in two pieces")
    assert ix.get_token_codes()[0].shape == (201,) and ix.token_rows == 150
    for r0 in range(200, N, 100):                                               # the capacity grows; the codes stay
        ix.add(x[r0:r0 + 100])
        _same(ix.get_token_codes(0, 150), want, "capacity growth")
    ix.set_tokens(ms.rows(np.arange(150, N)).csr)                               # a long append: the buffers grow
    _same(ix.get_token_codes(), (ms.off, codes, res), "appended")
    ix.set_tokens(ms.rows(np.arange(20, 40)).csr, row0=100)                     # row0 < T drops, then appends
    sel = np.concatenate([np.arange(100), np.arange(20, 40)])
    sub = ms.rows(sel)
    c2, r2, _ = _double(codec, sub)
    _same(ix.get_token_codes(0, 120), (sub.off, c2, r2), "row0 < T")
    assert ix.token_rows == 120
    ix.set_tokens([], row0=10)                                                  # a pure truncation
    assert ix.token_rows == 10
    ix.set_tokens(ms.csr, row0=0)                                               # the rewrite
    _same(ix.get_token_codes(), (ms.off, codes, res), "rewrite")
    _check(ix.search_maxsim(qs[3], 10), dec.scores64(qs[3]), 10, "after growth and rewrite")
    ix.close()


def test_remove_ids_compacts_the_codes_with_the_rows():
    for P, nbits in ((32, 1), (128, 4), (96, 2)):                               # packed rows of 4, 64 and 24 bytes
        codec, ms, qs = cc.lattice(P, nbits, 17)
        ix = _index(codec, ms.rows(np.arange(cc.T_PART)))                       # rows T_PART .. have no matrix
        gone = np.flatnonzero(np.random.default_rng(9).random(N) < 1.0 / 3.0)
        keep = np.ones(N, bool)
        keep[gone] = False
        assert ix.remove_ids(gone) == gone.shape[0]
        kept = ms.rows(np.flatnonzero(keep[:cc.T_PART]))
        nk = int(keep.sum())
        fresh = tp._index(D, 0, tp._rows(N, D, 11)[keep])
        fresh.set_token_codec(codec)
        fresh.set_tokens(kept.csr)
        _same(ix.get_token_codes(), fresh.get_token_codes(), f"P={P} nbits={nbits}: get_token_codes after remove_ids")
        c, r, dec = _double(codec, kept)
        _same(ix.get_token_codes(0, kept.n), (kept.off, c, r), "... and the numpy double of the kept rows")
        assert ix.token_rows == kept.n and ix.token_codec_bits == nbits and ix.ntotal == nk
        for j, q in enumerate(qs):
            _check(ix.search_maxsim(q, 128), dec.padded(nk).scores64(q), 128, f"P={P} nbits={nbits} query {j} after remove_ids")
        fresh.close()
        ix.remove_ids(np.arange(nk))                                            # emptied: as reset, the codec stays
        assert ix.ntotal == 0 and ix.token_rows == 0 and ix.token_codec_bits == nbits
        ix.close()


def test_an_index_without_a_codec_stores_the_bytes_it_was_given():
    ms, qs = cc.arbitrary("gaussian", 64)
    ix = _index(None, ms)
    assert ix.token_codec_bits == 0 and ix.get_token_codec() is None
    _same(ix.get_tokens(), (ms.off, ms.tok), "raw storage")
    col = ix.maxsim_ids(qs[2], np.arange(N))
    t64 = ms.scores64(qs[2])
    live = ms.lens > 0
    assert np.abs(col[live] - t64[live]).max() < 1e-4 and (col[~live] == -np.inf).all()
    ix.close()


# ------------------------------------------------------------------ the trainer
def test_the_trainer_gives_the_same_bytes_twice():
    ms, _ = cc.arbitrary("clustered", 64)
    for nbits in cc.BITS:
        a = fi.train_token_codec(ms.csr, 200, nbits=nbits, niter=4, seed=7)
        b = fi.train_token_codec(ms.mats(), 200, nbits=nbits, niter=4, seed=7)
        _same([a.centroids, a.cutoffs, a.weights], [b.centroids, b.cutoffs, b.weights], f"nbits={nbits}: two calls")
        assert a.nbits == nbits and a.centroids.shape == (200, 64) and a.centroids.dtype == np.float32
        assert not (a.centroids.view(np.uint32) & 0xFFFF).any() and np.isfinite(a.centroids).all()   # bf16 values
        assert (np.diff(a.cutoffs) > 0).all() and (np.diff(a.weights) >= 0).all()
        assert a.cutoffs.shape == ((1 << nbits) - 1,) and a.weights.shape == (1 << nbits,)
        fi.token_codec_args(*a, P=64)
    c = fi.train_token_codec(ms.csr, 200, nbits=2, niter=4, seed=8)
    assert not np.array_equal(c.centroids, a.centroids)                         # another seed, another codec
    # a trained codec finds the clusters: a token lies at cosine 1 / sqrt(1 + 0.25^2) = 0.97 from its centre, and the
    # decoded tokens are about that close to the stored ones where k-means found the centre (0.9: some are missed)
    ix = _index(c, ms)
    dec = fi.bf16_to_f32(ix.get_tokens()[1])
    cos = (dec * fi.bf16_to_f32(ms.tok)).sum(axis=1) / np.linalg.norm(dec, axis=1)
    print(f"[tokens codec] trained codec, clustered tokens: mean cosine of decoded and stored tokens {float(cos.mean()):.4f}")
    assert cos.mean() > 0.9, float(cos.mean())
    ix.close()

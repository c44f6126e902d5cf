"""CPU: the token codec's host side -- every refusal of ``token_codec_args``, the canonical packing, the numpy double of
encode / decode against a float64 restatement on lattice inputs, and a proof that the lattice cases of
tests/tokens_codec_cases.py contain what makes the exact GPU checks bind: tokens whose best centroid is tied between
two ids, residuals exactly on a cutoff, and scores tied on both sides of rank k."""
import numpy as np
import pytest

import tokens_codec_cases as cc
from claude_semantic_search_amd import flat_index as fi
from tokens_fakes import Matrices, ties_at


def _codec(P=64, nbits=2, C=17):
    return cc.lattice_codec(P, nbits, C)


def test_every_refusal_of_token_codec_args():
    c = _codec()
    ok = fi.token_codec_args(*c, P=64)
    assert ok.nbits == 2 and ok.P == 64 and ok.res_bytes == 16 and ok.centroids.dtype == np.float32
    for nbits in (0, 3, 8, 2.5, "2", None):
        with pytest.raises(ValueError, match="nbits"):
            fi.token_codec_args(c.centroids, nbits, c.cutoffs, c.weights)
    with pytest.raises(ValueError, match="ascending"):
        fi.token_codec_args(c.centroids, 2, [0.0, 0.0, 0.125], c.weights)
    with pytest.raises(ValueError, match="ascending"):
        fi.token_codec_args(c.centroids, 2, [0.125, 0.0, -0.125], c.weights)
    with pytest.raises(ValueError, match="cutoffs for nbits=2"):
        fi.token_codec_args(c.centroids, 2, [0.0], c.weights)
    with pytest.raises(ValueError, match="weights for nbits=2"):
        fi.token_codec_args(c.centroids, 2, c.cutoffs, [0.0, 1.0])
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="cutoff is NaN or infinite"):
            fi.token_codec_args(c.centroids, 2, [-0.125, bad, 0.125], c.weights)
        with pytest.raises(ValueError, match="weight is NaN or infinite"):
            fi.token_codec_args(c.centroids, 2, c.cutoffs, [0.0, bad, 0.0, 0.0])
        cent = c.centroids.copy()
        cent[3, 5] = bad
        with pytest.raises(ValueError, match="centroid 3 has a NaN or infinite"):
            fi.token_codec_args(cent, 2, c.cutoffs, c.weights)
    cent = c.centroids.copy()
    cent[2, 1] = np.float32(1.0) + np.float32(2.0 ** -10)                       # a float32 value that is no bf16 value
    with pytest.raises(ValueError, match="not bf16 values"):
        fi.token_codec_args(cent, 2, c.cutoffs, c.weights)
    with pytest.raises(ValueError, match="float32"):
        fi.token_codec_args(c.centroids.astype(np.float64), 2, c.cutoffs, c.weights)
    with pytest.raises(ValueError, match=r"C=0 outside"):
        fi.token_codec_args(np.zeros((0, 64), np.float32), 2, c.cutoffs, c.weights)
    with pytest.raises(ValueError, match=r"C=65537 outside"):
        fi.token_codec_args(np.zeros((65537, 32), np.float32), 2, c.cutoffs, c.weights)
    fi.token_codec_args(np.zeros((65536, 32), np.float32), 2, c.cutoffs, c.weights)
    for P in (16, 48, 160):
        with pytest.raises(ValueError, match=f"P={P} must be"):
            fi.token_codec_args(np.zeros((4, P), np.float32), 2, c.cutoffs, c.weights)
    with pytest.raises(ValueError, match="P=64, the token matrices P=128"):
        fi.token_codec_args(*c, P=128)
    with pytest.raises(ValueError, match="shape"):
        fi.token_codec_args(c.centroids[0], 2, c.cutoffs, c.weights)
    with pytest.raises(ValueError, match="nbits"):
        fi.train_token_codec([np.zeros((4, 32), np.uint16)], 2, nbits=3)
    with pytest.raises(ValueError, match="ncentroids"):
        fi.train_token_codec([np.zeros((4, 32), np.uint16)], 4097)


def test_token_codes_as_csr_refuses_what_the_library_would():
    c = _codec(C=17)
    codes = np.arange(6, dtype=np.uint16)
    res = np.zeros((6, c.res_bytes), np.uint8)
    off, k, r = fi.token_codes_as_csr([0, 2, 2, 6], codes, res, c)
    assert off.dtype == np.int64 and k.dtype == np.uint16 and r.shape == (6, 16)
    bad = codes.copy()
    bad[4] = 17
    with pytest.raises(ValueError, match=r"token 2 of row 2 \(of this call\) has code 17"):
        fi.token_codes_as_csr([0, 2, 2, 6], bad, res, c)
    with pytest.raises(ValueError, match="offsets"):
        fi.token_codes_as_csr([0, 2, 5], codes, res, c)
    with pytest.raises(ValueError, match="bytes of buckets"):
        fi.token_codes_as_csr([0, 6], codes, res[:, :8], c)


@pytest.mark.parametrize("nbits", cc.BITS)
def test_canonical_pack_and_unpack_round_trip(nbits):
    rng = np.random.default_rng(nbits)
    for P in cc.WIDTHS:
        b = rng.integers(0, 1 << nbits, size=(37, P)).astype(np.uint8)
        r = fi.pack_buckets(b, nbits)
        assert r.dtype == np.uint8 and r.shape == (37, P * nbits // 8)
        assert np.array_equal(fi.unpack_buckets(r, nbits), b)
        # the layout, component by component: bits [nbits (j % (8 / nbits)), +nbits) of byte j nbits / 8
        per = 8 // nbits
        for j in range(P):
            got = (r[:, j * nbits // 8] >> (nbits * (j % per))) & ((1 << nbits) - 1)
            assert np.array_equal(got, b[:, j])
        r2 = rng.integers(0, 256, size=(5, P * nbits // 8)).astype(np.uint8)    # ... and from bytes back to bytes
        assert np.array_equal(fi.pack_buckets(fi.unpack_buckets(r2, nbits), nbits), r2)


def test_bf16_rounding_is_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -2.0, 3.4e38], np.float32)
    want = np.array([0x3F80, 0x3F80, 0x3F82, 0x3F81, 0xC000, 0x7F80], np.uint16)   # ties to even; overflow to inf
    assert np.array_equal(fi.f32_to_bf16_rne(x), want)
    assert np.array_equal(fi.bf16_to_f32(want[:3]), np.array([1.0, 1.0, 1.0 + 2.0 ** -6], np.float32))


@pytest.mark.parametrize("C", cc.CENTROIDS)
@pytest.mark.parametrize("nbits", cc.BITS)
@pytest.mark.parametrize("P", (32, 128))
def test_numpy_double_equals_the_float64_restatement_on_lattice_inputs(P, nbits, C):
    codec, ms, _ = cc.lattice(P, nbits, C)
    codes, res = fi.token_codec_encode(codec, ms.tok)
    codes64, buckets64 = cc.encode64(codec, ms.tok)
    assert codes.dtype == np.uint16 and np.array_equal(codes, codes64)
    assert np.array_equal(fi.unpack_buckets(res, nbits), buckets64)
    dec = fi.token_codec_decode(codec, codes, res)
    d64 = cc.decode64(codec, codes64, buckets64)
    assert np.array_equal(fi.bf16_to_f32(dec).astype(np.float64), d64)           # exact: no rounding happened
    assert np.abs(d64).max() <= 2.0 and np.array_equal(d64 * 8, np.round(d64 * 8))
    _, res2 = fi.token_codec_encode(codec, ms.tok, codes=codes)                   # the residual half alone
    assert np.array_equal(res2, res)


@pytest.mark.parametrize("C", cc.CENTROIDS)
@pytest.mark.parametrize("nbits", cc.BITS)
@pytest.mark.parametrize("P", cc.WIDTHS)
def test_the_lattice_cases_contain_the_ties_that_make_the_gpu_checks_bind(P, nbits, C):
    codec, ms, qs = cc.lattice(P, nbits, C)
    assert ms.n == cc.N and ms.lens[:len(cc.EDGE)].tolist() == list(cc.EDGE) and ms.lens[len(cc.EDGE):-1].max() <= 40
    assert ms.lens[-1] == 512 and np.array_equal(ms.mat(cc.N - 1), ms.mat(cc.EDGE.index(512)))   # the longest doc's twin
    # (i) tokens whose best centroid is tied between two ids (no two ids when C = 1)
    d = cc.dots64(codec, ms.tok)
    tied = (d == d.max(axis=1, keepdims=True)).sum(axis=1) > 1
    if C > 1:
        assert tied.sum() >= 100, f"only {tied.sum()} tokens have a tied best centroid"
        codes, _ = cc.encode64(codec, ms.tok)
        assert (d[tied][np.arange(tied.sum()), codes[tied]] == d[tied].max(axis=1)).all()
        first = (d[tied] == d[tied].max(axis=1, keepdims=True)).argmax(axis=1)
        assert np.array_equal(codes[tied], first)                                 # ... and the truth takes the lower id
    else:
        assert not tied.any()
    # (ii) residuals that fall exactly on a cutoff: `<` and `<=` give different buckets there
    codes, buckets = cc.encode64(codec, ms.tok)
    r = fi.bf16_to_f32(ms.tok) - codec.centroids[codes]
    on = (r[:, :, None] == codec.cutoffs[None, None, :]).any(axis=2)
    assert on.sum() >= 1000
    le = (codec.cutoffs[None, None, :] <= r[:, :, None]).sum(axis=2)
    assert (le[on] == buckets[on] + 1).all() and np.array_equal(le[~on], buckets[~on])
    # (iii) scores tied on both sides of rank k, for every k that the GPU tests ask for
    dec = Matrices(ms.off, fi.token_codec_decode(codec, *fi.token_codec_encode(codec, ms.tok)))
    for j, q in enumerate(qs):
        col = dec.scores64(q)
        assert np.array_equal(col[col > -np.inf], col[col > -np.inf].astype(np.float32))   # exact in fp32
    for k in cc.KS:
        assert any(ties_at(dec.scores64(q), k) for q in qs), f"no query has a tie across rank {k}"


def test_the_negative_case_is_negative_and_the_assignment_bound_is_small():
    for nbits in cc.BITS:
        codec, ms, q = cc.negative_case(32, nbits)
        dec = Matrices(ms.off, fi.token_codec_decode(codec, *fi.token_codec_encode(codec, ms.tok)))
        col = dec.scores64(q)
        assert (col[ms.lens > 0] < 0).all()
    ms, _ = cc.arbitrary("clustered", 128)
    codec = fi.TokenCodec(fi.bf16_to_f32(ms.tok[:256]), 2, cc.CUTOFFS[2], cc.WEIGHTS[2])
    assert cc.assign_bound(128, ms.tok, codec).max() < 3.2e-5                     # unit operands: 2 * 128 * 2^-23


def test_residual_quantiles_ascend_and_split_evenly():
    r = np.random.default_rng(0).standard_normal(100000).astype(np.float32) * 0.05
    for nbits in cc.BITS:
        cut, w = fi.residual_quantiles(r, nbits)
        assert cut.dtype == w.dtype == np.float32 and cut.shape == ((1 << nbits) - 1,) and w.shape == (1 << nbits,)
        assert (np.diff(cut) > 0).all() and (np.diff(w) > 0).all()
        counts = np.bincount(np.searchsorted(cut, r, side="left"), minlength=1 << nbits)
        assert np.abs(counts / r.size - 1.0 / (1 << nbits)).max() < 0.01
    cut, _ = fi.residual_quantiles(np.zeros(100, np.float32), 2)                # no spread: still strictly ascending
    assert (np.diff(cut) > 0).all()

"""CPU: the argument rules of ``maxsim_candidates`` / ``search_maxsim_pruned``, the numpy double of the candidate stage
(``flat_index.token_centroid_scores`` / ``token_codec_approx`` / ``maxsim_candidates_numpy`` / ``token_codec_scores`` /
``search_maxsim_pruned_numpy``) against a float64 restatement, and the proof, with numpy alone, that the inputs of
tests/test_tokens_prune_gpu.py (tests/tokens_prune_cases.py) make its exact checks bind."""
import numpy as np
import pytest

import tokens_codec_cases as cc
import tokens_prune_cases as pc
from claude_semantic_search_amd import flat_index as fi

CASES = ((32, 1, 1), (64, 2, 17), (96, 4, 256), (128, 2, 300), (32, 2, 300), (128, 4, 17))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_every_refusal_of_the_argument_checkers():
    assert fi.prune_args(10, 10) == (10, 10) and fi.prune_args(None, 65536, "maxsim_candidates") == (None, 65536)
    assert fi.prune_args(np.int64(128), np.int64(4096)) == (128, 4096)
    for ncand in (0, -1, 65537, 2.5, "many", None):
        with pytest.raises(ValueError, match="ncand"):
            fi.prune_args(1, ncand)
        with pytest.raises(ValueError, match="maxsim_candidates: ncand"):
            fi.prune_args(None, ncand, "maxsim_candidates")
    for k in (0, -3, 129):
        with pytest.raises(ValueError, match=r"k=-?\d+ outside \[1, 128\]"):
            fi.prune_args(k, 1000)
    with pytest.raises(ValueError, match="k=17 exceeds ncand=16"):
        fi.prune_args(17, 16)
    # the query matrix is checked by maxsim_args, under the caller's name
    with pytest.raises(ValueError, match="search_maxsim_pruned: P=48"):
        fi.maxsim_args(np.zeros((3, 48), np.uint16), what="search_maxsim_pruned")
    with pytest.raises(ValueError, match="maxsim_candidates: 65 query tokens"):
        fi.maxsim_args(np.zeros((65, 32), np.uint16), what="maxsim_candidates")
    with pytest.raises(ValueError, match="ncand"):
        fi.maxsim_candidates_numpy(np.zeros(4, np.float32), 0)


@pytest.mark.parametrize("P,nbits,C", CASES)
def test_the_numpy_double_equals_the_float64_restatement_on_lattice_cases(P, nbits, C):
    codec, ms, qs, codes, res = pc.lattice_codes(P, nbits, C)
    allow = cc.half_mask()
    for j, q in enumerate(qs):
        S = fi.token_centroid_scores(codec, q)
        S64 = codec.centroids.astype(np.float64) @ fi.bf16_to_f32(q).astype(np.float64).T
        assert S.dtype == np.float32 and S.shape == (C, q.shape[0]) and np.array_equal(S.astype(np.float64), S64)
        a64, e64 = pc.approx64(codec, ms.off, codes, q), pc.exact64(codec, ms, codes, res, q)
        a = fi.token_codec_approx(codec, ms.off, codes, q)
        assert np.array_equal(_bits(a), _bits(a64.astype(np.float32))) and np.array_equal(a.astype(np.float64), a64)
        assert ((a == -np.inf) == (ms.lens == 0)).all()
        e = fi.token_codec_scores(codec, ms.off, codes, res, q)
        assert np.array_equal(_bits(e), _bits(e64.astype(np.float32))) and np.array_equal(e.astype(np.float64), e64)
        sub = np.array([7, 0, 499, 7, 3])
        assert np.array_equal(_bits(fi.token_codec_scores(codec, ms.off, codes, res, q, rows=sub)), _bits(e[sub]))
        for ncand in (1, 16, 100, 499, 500, 65536):
            for al in (None, allow):
                ids, ap = fi.maxsim_candidates_numpy(a, ncand, al, id_base=cc.ID_BASE)
                want = pc.candidates64(a64, ncand, al)
                assert np.array_equal(ids, want + cc.ID_BASE) and np.array_equal(_bits(ap), _bits(a[want]))
                assert (np.diff(ids) > 0).all()
                for k in (1, 10, 128):
                    if k > ncand:
                        continue
                    got = fi.search_maxsim_pruned_numpy(codec, ms.off, codes, res, q, k, ncand, al, id_base=cc.ID_BASE)
                    Dw, Iw = pc.pruned64(a64, e64, k, ncand, al, id_base=cc.ID_BASE)
                    assert np.array_equal(got[1], Iw) and np.array_equal(_bits(got[0]), _bits(Dw)), (j, ncand, k)


def test_the_approximate_score_is_the_exact_score_of_the_centroid_matrices():
    """Definition 2: A[r] is the MaxSim of the matrix centroids[codes of r]."""
    from tokens_fakes import Matrices

    for P, nbits, C in CASES[:4]:
        codec, ms, qs, codes, res = pc.lattice_codes(P, nbits, C)
        cm = Matrices(ms.off, cc.to_bits(codec.centroids[codes]))
        for q in qs:
            assert np.array_equal(pc.approx64(codec, ms.off, codes, q), cm.scores64(q))


def test_the_lattice_cases_bind():
    """Ties on A on both sides of rank ncand, pruned answers that differ from and equal the exhaustive one, exact
    scores tied across rank k inside the candidate set."""
    tied = {nc: 0 for nc in (1, 10, 16, 100, 128)}
    differ = same = ktied = masked_tied = 0
    allow = cc.half_mask()
    for P, nbits, C in CASES:
        codec, ms, qs, codes, res = pc.lattice_codes(P, nbits, C)
        for q in qs:
            a64, e64 = pc.approx64(codec, ms.off, codes, q), pc.exact64(codec, ms, codes, res, q)
            live = int((a64 > -np.inf).sum())
            assert 16 < live <= 499, "ncand = 500 and 65536 take every live row, 16 and 100 do not"
            for nc in tied:
                tied[nc] += pc.ties_across(a64, nc)
            masked_tied += pc.ties_across(a64, 16, allow)
            full = pc.pruned64(a64, e64, 10, 65536)
            assert np.array_equal(full[1], pc.pruned64(a64, e64, 10, 500)[1])
            for nc in (10, 16, 100):
                got = pc.pruned64(a64, e64, 10, nc)
                differ += not np.array_equal(got[1], full[1])
                same += np.array_equal(got[1], full[1]) and np.array_equal(_bits(got[0]), _bits(full[0]))
                rows = pc.candidates64(a64, nc)
                s = np.sort(-e64[rows])
                ktied += bool(s.shape[0] > 10 and s[9] == s[10])
    assert all(v > 0 for v in tied.values()), tied
    assert masked_tied > 0 and differ > 0 and same > 0 and ktied > 0, (masked_tied, differ, same, ktied)


def test_the_wide_case_binds():
    codec, ms, q, codes, res = pc.wide()
    assert ms.n == pc.WIDE_N and 55000 < ms.off[-1] < 65000 and int(ms.lens.max()) == 3 and (ms.lens == 0).any()
    a64 = pc.approx64(codec, ms.off, codes, q)
    a = fi.token_codec_approx(codec, ms.off, codes, q)
    assert np.array_equal(a.astype(np.float64), a64)
    live = int((a64 > -np.inf).sum())
    assert 4097 < live < pc.WIDE_N and np.unique(a64).size < 200, "thousands of rows tie on A"
    assert pc.WIDE_N > 9 * pc.SLICE, "the compaction runs ten blocks"
    for nc in pc.WIDE_NCANDS:
        cand = pc.candidates64(a64, nc)
        assert cand.size == min(nc, live)
        if nc >= live:
            continue
        assert pc.ties_across(a64, nc), nc
        thr = np.sort(-a64[a64 > -np.inf])[nc - 1] * -1.0
        eq = np.flatnonzero(a64 == thr)
        took, left = np.intersect1d(eq, cand), np.setdiff1d(eq, cand)
        assert took.size >= 1 and left.size >= 1
        # the tie quota is cut inside the row order: rows equal to the threshold are left in several later slices, and
        # for the larger ncand the taken ones span more than one slice
        assert np.unique(left // pc.SLICE).size > 1 and took.max() < left.min()
        if nc >= 128:
            assert np.unique(took // pc.SLICE).size > 1, nc

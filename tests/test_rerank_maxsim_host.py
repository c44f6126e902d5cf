"""CPU: the argument helper and the numpy doubles of the two-stage search (``flat_index.rerank_args``,
``maxsim_lists_numpy``, ``search_rerank_maxsim_numpy``), and the proofs that the inputs of
tests/test_rerank_maxsim_gpu.py (tests/rerank_cases.py) make its exact checks bind: late scores tie across rank k inside
a pool, so that the position rule decides; the pools of different queries differ; some pool entries are misses."""
import numpy as np
import pytest

import rerank_cases as rc
import tokens_cases as tc
import tokens_codec_cases as cc
from claude_semantic_search_amd import flat_index as fi


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------------ the argument helper
def test_rerank_args_accepts_and_resolves():
    _, qs = tc.lattice("T", 32)
    x, Q = rc.dense(500)
    a, off, tok, k, fetch, floor, ids = fi.rerank_args(Q[:6], qs, 10, 50, None, d=rc.D)
    assert a.dtype == np.float32 and a.shape == (6, rc.D) and off.tolist() == [0, 1, 16, 32, 49, 81, 145]
    assert tok.shape == (145, 32) and (k, fetch) == (10, 50) and floor != floor and ids is None
    assert fi.rerank_args(Q[:6], qs, 50, 50, 0.25, d=rc.D)[5] == 0.25                        # k == fetch is allowed
    assert fi.rerank_args(Q[:6], qs, 128, 2048, None, d=rc.D)[3:5] == (128, 2048)
    _, off, tok, k, f, _, ids = fi.rerank_args(None, qs[:2], None, None, ids=[[1, 2, 3], [4, 5, -1]], what="maxsim_ids_batch")
    assert k is None and f == 3 and ids.dtype == np.int64 and ids.shape == (2, 3)


def test_every_refusal_of_rerank_args_is_a_value_error():
    _, qs = tc.lattice("T", 32)
    _, qs64 = tc.lattice("T", 64)
    x, Q = rc.dense(500)
    nan_q = qs[1].copy()
    nan_q[3, 5] = 0x7FC0
    bad = [
        (dict(q=Q[:6], q_mats=qs, k=0, fetch=50), "k=0 outside"),
        (dict(q=Q[:6], q_mats=qs, k=51, fetch=50), r"k=51 outside \[1, min\(fetch=50, 128\)\]"),
        (dict(q=Q[:6], q_mats=qs, k=129, fetch=200), "k=129 outside"),
        (dict(q=Q[:6], q_mats=qs, k=1.5, fetch=50), "k=1.5 outside"),
        (dict(q=Q[:6], q_mats=qs, k="x", fetch=50), "no integer"),
        (dict(q=Q[:6], q_mats=qs, k=1, fetch=0), r"fetch=0 outside \[1, 2048\]"),
        (dict(q=Q[:6], q_mats=qs, k=1, fetch=2049), "fetch=2049 outside"),
        (dict(q=Q[:6], q_mats=qs, k=1, fetch=None), "no integer"),
        (dict(q=Q[:5], q_mats=qs, k=1, fetch=50), "5 dense queries for 6 query matrices"),
        (dict(q=Q[:6, :32], q_mats=qs, k=1, fetch=50), "expected shape"),
        (dict(q=Q[:6], q_mats=qs, k=1, fetch=50, floor="low"), "floor='low' is no number"),
        (dict(q=Q[:0], q_mats=[], k=1, fetch=50), r"0 queries outside \[1, 1024\]"),
        (dict(q=Q[:1], q_mats=[qs[0]] * 1025, k=1, fetch=50), "1025 queries outside"),
        (dict(q=Q[:2], q_mats=[qs[0], np.zeros((65, 32), np.uint16)], k=1, fetch=50), "query 1: 65 query tokens"),
        (dict(q=Q[:2], q_mats=[qs[0], np.zeros((0, 32), np.uint16)], k=1, fetch=50), "query 1: 0 query tokens"),
        (dict(q=Q[:2], q_mats=[qs[0], qs64[0]], k=1, fetch=50), "query 1 has P=64"),
        (dict(q=Q[:2], q_mats=[qs[0], np.zeros((2, 48), np.uint16)], k=1, fetch=50), "query 1: P=48"),
        (dict(q=Q[:2], q_mats=[qs[0], nan_q], k=1, fetch=50), "query 1: query token 3 has a NaN"),
        (dict(q=Q[:2], q_mats=[qs[0], np.zeros((2, 32), np.float64)], k=1, fetch=50), "query 1: the query matrix must be uint16"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            fi.rerank_args(d=rc.D, **kw)
    for ids, msg in (([1, 2, 3], "expected"), ([[1, 2]], r"ids of shape \(1, 2\) for 2 queries"), ([[], []], r"f=0 outside"),
                     (np.zeros((2, 2049), np.int64), "f=2049 outside"), ([["a"], ["b"]], "integer array")):
        with pytest.raises(ValueError, match=msg):
            fi.rerank_args(None, qs[:2], None, None, ids=ids, what="maxsim_ids_batch")


# ------------------------------------------------------------------ the doubles against float64
@pytest.mark.parametrize("family,P", (("T", 32), ("E", 128)))
def test_list_double_equals_float64_on_a_raw_store(family, P):
    ms, qs = tc.lattice(family, P)
    part = ms.rows(np.arange(tc.T_PART))
    _, mats = rc.batch(qs, 9)
    ids = rc.id_lists(9, 50, tc.N, tc.T_PART, 3, id_base=tc.ID_BASE)
    want = rc.lists64(part, mats, ids, tc.N, tc.ID_BASE)
    got = fi.maxsim_lists_numpy(part.off, mats, ids, tok=part.tok, id_base=tc.ID_BASE)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
    assert (want == -np.inf).any() and (want > -np.inf).any()
    one = fi.token_scores(ms.off, ms.tok, qs[4])
    assert np.array_equal(_bits(one), _bits(ms.scores64(qs[4]).astype(np.float32)))


@pytest.mark.parametrize("nbits", cc.BITS)
def test_list_double_equals_float64_on_a_compressed_store(nbits):
    codec, ms, qs = cc.lattice(64, nbits, 17)
    dec = rc.decoded(codec, ms)
    codes = fi.token_codec_assign(codec, ms.tok)
    codes, res = fi.token_codec_encode(codec, ms.tok, codes)
    _, mats = rc.batch(qs, 7)
    ids = rc.id_lists(7, 17, cc.N, cc.N, 5)
    got = fi.maxsim_lists_numpy(ms.off, mats, ids, codec=codec, codes=codes, res=res)
    assert np.array_equal(_bits(got), _bits(rc.lists64(dec, mats, ids, cc.N)))


def test_ranking_double_equals_the_restatement():
    ms, qs = tc.lattice("T", 32)
    x, Q = rc.dense(tc.N)
    _, mats = rc.batch(qs, 9)
    for metric in (0, 1):
        for fetch, k, floor in ((50, 10, None), (128, 128, None), (17, 1, 3.0), (50, 10, float("nan"))):
            want, (S0, I0, late) = rc.truth(x, Q[:9], ms, mats, k, fetch, metric, floor)
            got = fi.search_rerank_maxsim_numpy(S0, I0, late, k, floor)
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), (metric, fetch, k, floor)
    # a pool with padding, a miss in the middle, a floor at a pool score, a tie that the position decides
    S0 = np.array([[9, 7, 7, 5, 3, -rc.FMAX]], np.float32)
    I0 = np.array([[4, 8, 2, 6, 1, -1]], np.int64)
    late = np.array([[1.0, 2.0, -np.inf, 2.0, 5.0, -np.inf]], np.float32)
    D_, I, S, R = fi.search_rerank_maxsim_numpy(S0, I0, late, 4, floor=5.0)
    assert I.tolist() == [[8, 6, 4, -1]] and R.tolist() == [[1, 3, 0, -1]] and D_[0, :3].tolist() == [2.0, 2.0, 1.0]
    assert S[0, :3].tolist() == [7.0, 5.0, 9.0] and D_[0, 3] == S[0, 3] == np.float32(-rc.FMAX) and R.dtype == np.int32


# ------------------------------------------------------------------ the GPU file's inputs are what they claim
def test_late_scores_tie_across_rank_k_inside_a_pool():
    x, Q = rc.dense(tc.N)
    ms, qs = tc.lattice("T", 32)
    _, mats = rc.batch(qs, 9)
    for fetch, k in ((50, 10), (128, 10), (17, 1)):
        _, (S0, I0, late) = rc.truth(x, Q[:9], ms, mats, k, fetch)
        tied = [b for b in range(9) if rc.tie_across(late[b], S0[b], I0[b], k)]
        assert tied, (fetch, k)
    codec, cms, cqs = cc.lattice(64, 2, 17)                     # the docs are drawn from 60 matrices: ties at every rank
    xc, Qc = rc.dense(cc.N)
    _, cmats = rc.batch(cqs, 5)
    for k in rc.KS:
        _, (S0, I0, late) = rc.truth(xc, Qc[:5], rc.decoded(codec, cms), cmats, k, 500)
        assert any(rc.tie_across(late[b], S0[b], I0[b], k) for b in range(5)), k
    # ... and the tied entries stand in an order that no sort by id gives: the position rule is what is checked
    (D_, I, S, R), _ = rc.truth(xc, Qc[:5], rc.decoded(codec, cms), cmats, 128, 500)
    assert any((np.diff(I[b][D_[b] == D_[b, 0]]) < 0).any() for b in range(5))


def test_pools_of_different_queries_differ_and_hold_misses():
    x, Q = rc.dense(tc.N)
    S0, I0 = rc.pool64(x, Q[:9], 50)
    assert len({tuple(r) for r in I0.tolist()}) == 9
    ms, qs = tc.lattice("T", 32)
    part = ms.rows(np.arange(tc.T_PART))
    _, mats = rc.batch(qs, 9)
    late = rc.lists64(part, mats, I0, tc.N)
    assert ((I0 >= tc.T_PART) & (late == -np.inf)).any()                                   # rows >= T
    xc, Qc = rc.dense(cc.N)
    codec, cms, cqs = cc.lattice(64, 2, 17)
    S0, I0 = rc.pool64(xc, Qc[:5], 600)                                                    # fetch above ntotal
    assert (I0[:, 500:] == -1).all() and (I0[:, :500] >= 0).all()                          # -1 padding
    late = rc.lists64(cms, rc.batch(cqs, 5)[1], I0, cc.N)
    empty = np.flatnonzero(cms.lens == 0)
    assert empty.size and all((late[b][np.isin(I0[b], empty)] == -np.inf).all() for b in range(5))   # empty rows
    # a floor at a pool score cuts in the middle of a pool
    S0, I0 = rc.pool64(x, Q[:9], 50)
    floor = float(S0[0, 25])
    assert 0 < (S0[0] < floor).sum() < 50 and (S0[0] == floor).any()

"""GPU: MaxSim over per-query row lists and the two-stage search -- ``IndexFlat.maxsim_ids_batch``
(``css_index_maxsim_rows_batch``; kernel ``k_tok_scores_l<P, MT, NB>``) and ``IndexFlat.search_rerank_maxsim``
(``css_index_search_rerank_maxsim``; the pool search, ``k_rr_lists``, ``k_tok_scores_l``, ``k_sparse_topk_cols`` by
position and ``k_rr_out``).

Truth is the float64 restatement of tests/rerank_cases.py on the very arrays handed to the index -- exact in fp32 on the
lattice inputs, so every comparison is one of bits -- never the code under test; byte equality with the library's own
single calls (``search`` of the same call shape, ``maxsim_ids``) is checked IN ADDITION.
tests/test_rerank_maxsim_host.py proves on the CPU that these inputs hold late-score ties across rank k inside a pool,
pools that differ between queries, and pool entries that are misses."""
import re

import numpy as np
import pytest

import rerank_cases as rc
import test_search_prior_gpu as tp
import tokens_cases as tc
import tokens_codec_cases as cc
from claude_semantic_search_amd import _native as nat

pytestmark = pytest.mark.gpu

FMAX = rc.FMAX


def _index(n, ms=None, codec=None, metric=0):
    x, _ = rc.dense(n)
    ix = tp._index(rc.D, metric, x)
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


def _loop_of_single_calls(ix, mats, ids, n, id_base=0):
    """[nq, f] from ``maxsim_ids``, one call per query over the ids the single call accepts; -inf elsewhere."""
    out = np.full(ids.shape, -np.inf, np.float32)
    for b, q in enumerate(mats):
        ok = (ids[b] >= id_base) & (ids[b] < id_base + n)
        out[b, ok] = ix.maxsim_ids(q, ids[b, ok])
    return out


# ------------------------------------------------------------------ maxsim_ids_batch, in bits
@pytest.mark.parametrize("nq", rc.NQS)
@pytest.mark.parametrize("f", rc.FS)
def test_lists_equal_float64_and_the_single_calls(f, nq):
    ms, qs = tc.lattice("E", 64)
    part = ms.rows(np.arange(tc.T_PART))                                         # rows >= T are misses
    ix = _index(tc.N, part)
    pick, mats = rc.batch(qs, nq)                                                # nq >= 6: all six lengths in ONE call
    ids = rc.id_lists(nq, f, tc.N, tc.T_PART, 100 * f + nq)
    got = ix.maxsim_ids_batch(mats, ids)
    want = rc.lists64(part, mats, ids, tc.N)
    assert got.dtype == np.float32 and got.shape == (nq, f)
    assert np.array_equal(_bits(got), _bits(want)), f"f={f} nq={nq}: {(got != want).sum()} scores differ from float64"
    sub = slice(0, nq) if nq <= 9 else slice(nq - 13, nq)                        # (the long batch: its last 13 lists)
    assert np.array_equal(_bits(got[sub]), _bits(_loop_of_single_calls(ix, mats[sub], ids[sub], tc.N)))
    if f >= 15:
        assert (want == -np.inf).any() and (want > -np.inf).any()
    if nq > 6:                                                                   # equal queries at different positions
        same = ix.maxsim_ids_batch(mats, np.broadcast_to(ids[0], ids.shape).copy())
        for b in range(6, nq, 97):
            assert np.array_equal(_bits(same[b]), _bits(same[pick[b]]))
    ix.close()


@pytest.mark.parametrize("P", tc.WIDTHS)
@pytest.mark.parametrize("family", tc.FAMILIES)
def test_lists_on_every_width_grid_and_id_base(family, P):
    ms, qs = tc.lattice(family, P)
    ix = _index(tc.N, ms)
    _, mats = rc.batch(qs, 9)
    ids = rc.id_lists(9, 50, tc.N, tc.N, P)
    want = rc.lists64(ms, mats, ids, tc.N)
    ref = ix.maxsim_ids_batch(mats, ids)
    assert np.array_equal(_bits(ref), _bits(want))
    for blocks in (1, 2, 3, 0):                                                  # the grid does not change a bit
        ix.set_token_blocks(blocks)
        assert np.array_equal(_bits(ix.maxsim_ids_batch(mats, ids)), _bits(want)), f"blocks={blocks}"
    ix.set_id_base(tc.ID_BASE)
    based = rc.id_lists(9, 50, tc.N, tc.N, P, id_base=tc.ID_BASE)
    got = ix.maxsim_ids_batch(mats, based)
    assert np.array_equal(_bits(got), _bits(rc.lists64(ms, mats, based, tc.N, tc.ID_BASE)))
    assert np.array_equal(_bits(got), _bits(_loop_of_single_calls(ix, mats, based, tc.N, tc.ID_BASE)))
    assert (ix.maxsim_ids_batch(mats, ids) == -np.inf).all()                     # the unbased ids now name no row
    ix.close()


@pytest.mark.parametrize("C", (17, 300))
@pytest.mark.parametrize("nbits", cc.BITS)
def test_lists_on_a_compressed_store(nbits, C):
    for P in (64, 128):
        codec, ms, qs = cc.lattice(P, nbits, C)
        ix = _index(cc.N, ms, codec)
        _, mats = rc.batch(qs, 9)
        ids = rc.id_lists(9, 50, cc.N, cc.N, C + nbits)
        got = ix.maxsim_ids_batch(mats, ids)
        assert np.array_equal(_bits(got), _bits(rc.lists64(rc.decoded(codec, ms), mats, ids, cc.N))), f"P={P}"
        assert np.array_equal(_bits(got), _bits(_loop_of_single_calls(ix, mats, ids, cc.N))), f"P={P}"
        ix.set_token_blocks(2)
        assert np.array_equal(_bits(ix.maxsim_ids_batch(mats, ids)), _bits(got))
        ix.close()


def test_lists_without_matrices_and_their_refusals():
    ms, qs = tc.lattice("T", 32)
    ix = _index(tc.N)
    assert (ix.maxsim_ids_batch(qs, np.zeros((6, 3), np.int64)) == -np.inf).all()
    ix.set_tokens(ms.csr)
    lib, h = nat.lib(), ix._handle()
    off = np.array([0, 1, 16], np.int64)
    tok = np.concatenate([qs[0], qs[1]])
    ids, out = np.zeros((2, 4), np.int64), np.zeros((2, 4), np.float32)

    def call(off=off, tok=tok, nq=2, P=32, f=4):
        return lib.css_index_maxsim_rows_batch(h, tok.ctypes.data, off.ctypes.data, nq, P, ids.ctypes.data, f, out.ctypes.data)

    nan = tok.copy()
    nan[9, 2] = 0x7F80
    for kw, msg in ((dict(nq=0), r"nq=0 outside \[1, 1024\]"), (dict(f=0), r"f=0 outside \[1, 2048\]"), (dict(f=2049), "f=2049"),
                    (dict(P=48), "P=48"), (dict(off=np.array([1, 2, 3], np.int64)), "start at 1"),
                    (dict(off=np.array([0, 1, 70], np.int64)), "query 1 has 69 tokens"),
                    (dict(off=np.array([0, 1, 1], np.int64)), "query 1 has 0 tokens"),
                    (dict(tok=nan), "component 2 of token 8 of query 1 is infinite")):
        assert call(**kw) != 0
        assert re.search(msg, nat.last_error()), (msg, nat.last_error())
    _, qs64 = tc.lattice("T", 64)
    with pytest.raises(nat.CssError, match="the stored matrices P=32"):
        ix.maxsim_ids_batch(qs64, np.zeros((6, 3), np.int64))
    got = ix.maxsim_ids_batch(qs[:2], [[5, 6, 7, 8], [5, 6, 7, 8]])              # the index is as usable as before
    assert np.array_equal(_bits(got), _bits(rc.lists64(ms, qs[:2], np.array([[5, 6, 7, 8]] * 2), tc.N)))
    ix.close()


# ------------------------------------------------------------------ search_rerank_maxsim against the oracle sentence
def _composed(ix, Q, mats, k, fetch, floor=None, allow=None, n=None, id_base=0):
    """The oracle sentence from the library's own single calls: ``search`` of the same nq and fetch, ``maxsim_ids``."""
    S0, I0 = ix.search(Q, fetch, allow=allow)
    return rc.rank(S0, I0, _loop_of_single_calls(ix, mats, I0, n, id_base), k, floor)


def _check(ix, x, Q, ms, mats, k, fetch, what, metric=0, floor=None, allow=None, id_base=0):
    got = ix.search_rerank_maxsim(Q, mats, k, fetch, floor=floor, allow=allow)
    want, pool = rc.truth(x, Q, ms, mats, k, fetch, metric, floor, allow, id_base)
    assert [a.dtype for a in got] == [np.float32, np.int64, np.float32, np.int32], what
    _same(got, want, f"{what} against float64")
    _same(got, _composed(ix, Q, mats, k, fetch, floor, allow, x.shape[0], id_base), f"{what} against search + maxsim_ids")
    return got, pool


@pytest.mark.parametrize("k", rc.KS)
@pytest.mark.parametrize("metric", (0, 1))
def test_two_stage_search_equals_the_oracle(metric, k):
    ms, qs = tc.lattice("T", 32)
    part = ms.rows(np.arange(tc.T_PART))
    x, Q = rc.dense(tc.N)
    ix = _index(tc.N, part, metric=metric)
    ties = 0
    for nq, fetch in ((1, max(k, 17)), (9, max(k, 50)), (9, 128), (2, 300)):    # (300: the pool search takes passes)
        _, mats = rc.batch(qs, nq)
        (D_, I, S, R), (S0, I0, late) = _check(ix, x, Q[:nq], part, mats, k, fetch, f"metric={metric} k={k} nq={nq} fetch={fetch}",
                                               metric)
        ties += sum(rc.tie_across(late[b], S0[b], I0[b], k) for b in range(nq))
        assert (I[:, 0] >= 0).all() and (np.diff(D_.astype(np.float64), axis=1) <= 0).all()   # (padding is -FLT_MAX: last)
    assert ties > 0 or k == 128                                                  # ties across rank k: the position decided
    ix.close()


def test_two_stage_search_floors_masks_and_id_base():
    ms, qs = tc.lattice("T", 32)
    x, Q = rc.dense(tc.N)
    ix = _index(tc.N, ms)
    _, mats = rc.batch(qs, 9)
    S0, _ = rc.pool64(x, Q[:9], 50)
    floor = float(S0[0, 25])                                                     # equal to a pool score, in the middle of a pool
    (D_, I, S, R), _ = _check(ix, x, Q[:9], ms, mats, 50, 50, "floor", floor=floor)
    assert (S[0][I[0] >= 0] >= floor).all() and (S[0] == floor).any() and 0 < (I[0] >= 0).sum() < 50
    _check(ix, x, Q[:9], ms, mats, 10, 50, "floor above every score", floor=1e9)
    _check(ix, x, Q[:9], ms, mats, 10, 50, "NaN floor", floor=float("nan"))
    allow = tc.half_mask()
    (D_, I, S, R), _ = _check(ix, x, Q[:9], ms, mats, 10, 50, "masked", allow=allow)
    assert allow[I[I >= 0]].all()
    _check(ix, x, Q[:9], ms, mats, 10, 50, "masked and floored", floor=floor, allow=allow)
    few = np.zeros(tc.N, bool)
    few[[3, 0, 1, 8]] = True                                                     # row 0 is empty: three entries, then padding
    (D_, I, S, R), _ = _check(ix, x, Q[:9], ms, mats, 10, 50, "fewer than k", allow=few)
    assert ((I >= 0).sum(axis=1) == 3).all() and (R[:, 3:] == -1).all() and (D_[:, 3:] == np.float32(-FMAX)).all()
    for blocks in (1, 3, 0):
        ix.set_token_blocks(blocks)
        _check(ix, x, Q[:9], ms, mats, 10, 128, f"blocks={blocks}")
    ix.set_id_base(tc.ID_BASE)
    _check(ix, x, Q[:9], ms, mats, 10, 50, "id_base", id_base=tc.ID_BASE)
    ix.close()


@pytest.mark.parametrize("nbits", cc.BITS)
def test_two_stage_search_on_a_compressed_store_around_ntotal(nbits):
    codec, ms, qs = cc.lattice(64, nbits, 17)
    dec = rc.decoded(codec, ms)
    x, Q = rc.dense(cc.N)
    ix = _index(cc.N, ms, codec)
    _, mats = rc.batch(qs, 5)
    for fetch in (cc.N - 1, cc.N, cc.N + 100):                                   # below, at and above ntotal
        for k in (10, 128):
            (D_, I, S, R), (S0, I0, late) = _check(ix, x, Q[:5], dec, mats, k, fetch, f"nbits={nbits} fetch={fetch} k={k}")
            assert any(rc.tie_across(late[b], S0[b], I0[b], k) for b in range(5))
    assert (I0[:, cc.N:] == -1).all()
    ix.close()


def test_two_stage_search_pads_without_matrices_and_without_rows():
    ms, qs = tc.lattice("T", 32)
    x, Q = rc.dense(tc.N)
    for ix in (_index(tc.N), tp._index(rc.D, 0)):
        D_, I, S, R = ix.search_rerank_maxsim(Q[:6], qs, 10, 50)
        assert (D_ == np.float32(-FMAX)).all() and (S == np.float32(-FMAX)).all() and (I == -1).all() and (R == -1).all()
        assert R.dtype == np.int32 and D_.shape == (6, 10)
        ix.close()


def test_c_level_refusals_leave_the_index_usable():
    ms, qs = tc.lattice("T", 32)
    x, Q = rc.dense(tc.N)
    ix = _index(tc.N, ms)
    lib, h = nat.lib(), ix._handle()
    off = np.array([0, 1, 16], np.int64)
    tok = np.concatenate([qs[0], qs[1]])
    q = np.ascontiguousarray(Q[:2])
    D_, I, S, R = np.zeros((2, 128), np.float32), np.zeros((2, 128), np.int64), np.zeros((2, 128), np.float32), np.zeros((2, 128), np.int32)

    def call(off=off, tok=tok, nq=2, P=32, fetch=50, k=10):
        return lib.css_index_search_rerank_maxsim(h, q.ctypes.data, 0, tok.ctypes.data, off.ctypes.data, nq, P, fetch, k,
                                                  float("nan"), None, D_.ctypes.data, I.ctypes.data, S.ctypes.data, R.ctypes.data)

    nan = tok.copy()
    nan[0, 31] = 0x7FC1
    for kw, msg in ((dict(nq=0), r"nq=0 outside"), (dict(nq=1025), "nq=1025"), (dict(fetch=0), r"fetch=0 outside \[1, 2048\]"),
                    (dict(fetch=2049), "fetch=2049"), (dict(k=0), "k=0 outside"), (dict(k=51), r"k=51 outside \[1, min\(fetch=50, 128\)\]"),
                    (dict(k=129, fetch=200), "k=129"), (dict(P=16), "P=16"), (dict(off=np.array([0, 65, 66], np.int64)), "query 0 has 65 tokens"),
                    (dict(tok=nan), "component 31 of token 0 of query 0 is NaN")):
        assert call(**kw) != 0
        assert re.search(msg, nat.last_error()), (msg, nat.last_error())
    _, qs64 = tc.lattice("T", 64)
    with pytest.raises(nat.CssError, match="the stored matrices P=32"):
        ix.search_rerank_maxsim(Q[:6], qs64, 10, 50)
    with pytest.raises(ValueError, match="k=51 outside"):
        ix.search_rerank_maxsim(Q[:6], qs, 51, 50)
    assert call() == 0
    _, mats = rc.batch(qs, 2)
    _check(ix, x, Q[:2], ms, mats, 10, 50, "after the refusals")
    ix.close()

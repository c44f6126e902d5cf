"""CPU: the host side of the diversified search -- ``flat_index.mmr_select`` against a loop-written statement
(``diverse_fakes.mmr_loop``: ties, pads, both metrics) and against two cases worked by hand, the argument rules, and
``HybridStorage.search_diverse`` over the numpy double ``diverse_fakes.FakeDiverseIndex``."""
import numpy as np
import pytest

from claude_semantic_search_amd import flat_index as fi
from claude_semantic_search_amd.chunk import Chunk
from claude_semantic_search_amd.storage import HybridStorage, SearchConfig, StorageConfig
from diverse_fakes import FakeDiverseIndex, mmr_loop
from related_fakes import FakeIndex

FLT_MAX = np.finfo(np.float32).max


# ---------------------------------------------------------------------------------------------------------- mmr_select
@pytest.mark.parametrize("metric", [0, 1])
def test_mmr_select_equals_the_loop(metric):
    """Rows of multiples of 1/8 with a third of them copies, scores on a coarse grid, weights that are multiples of
    1/4: every quantity is exact in float32, ties are plentiful, and the two statements must agree bit for bit."""
    rng = np.random.default_rng(2)
    for nq, m, d, k in ((1, 32, 6, 10), (6, 128, 8, 10), (2, 128, 5, 128), (4, 17, 7, 17), (3, 1, 4, 1), (5, 64, 8, 3)):
        X = (rng.integers(-8, 9, size=(nq, m, d)) / 8.0).astype(np.float32)
        X[:, m - m // 3:] = X[:, :m // 3]                                    # copies: sim = the row's own norm / 0
        s = rng.integers(-8, 9, size=(nq, m)) / 8.0                          # a coarse grid: ties
        S = (np.sort(s, axis=1)[:, ::-1] if metric == 0 else np.sort(s + 1.0, axis=1)).astype(np.float32)
        I = np.stack([rng.permutation(1000)[:m] for _ in range(nq)]).astype(np.int64)
        npad = rng.integers(0, m + 1, size=nq)
        npad[0] = 0
        for j in range(nq):                                                  # pads at the tail (a whole row of them too)
            if npad[j]:
                I[j, m - npad[j]:], S[j, m - npad[j]:] = -1, (-FLT_MAX if metric == 0 else FLT_MAX)
        for lam in (0.0, 0.25, 0.5, 0.75, 1.0):
            got = fi.mmr_select(S, I, X, k, lam, metric)
            want = mmr_loop(S, I, X, k, lam, metric)
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and a.shape == b.shape
                assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                      b.view(np.uint32) if b.dtype == np.float32 else b), (nq, m, d, k, lam)
            if lam == 1.0:                                                   # the first k entries of the pool
                assert np.array_equal(got[1], I[:, :k]) and np.array_equal(got[0], S[:, :k])
            npicks = np.minimum(k, m - npad)
            for j in range(nq):                                              # a permutation of pool entries, then pads
                ids = got[1][j, :npicks[j]]
                assert len(set(ids.tolist())) == npicks[j] and np.isin(ids, I[j, :m - npad[j]]).all()
                assert (got[1][j, npicks[j]:] == -1).all()
                assert (got[0][j, npicks[j]:] == (-FLT_MAX if metric == 0 else FLT_MAX)).all()


def test_mmr_select_by_hand_inner_product():
    # q = (1, 0).  A and B are copies; C points elsewhere; D is short.
    X = np.array([[[1, 1], [1, 1], [0.5, -1], [0.25, 0], [9, 9]]], np.float32)
    S = np.array([[1.0, 1.0, 0.5, 0.25, -FLT_MAX]], np.float32)
    I = np.array([[0, 4, 2, 1, -1]], np.int64)
    # step 1 (last = A): sim = 2, -0.5, 0.25 -> v = 0.5 - 1, 0.25 + 0.25, 0.125 - 0.125 = -0.5, 0.5, 0   -> C
    # step 2 (last = C): pen_B = max(2, -0.5), pen_D = max(0.25, 0.125) -> v = -0.5, 0                   -> D, then B
    D_, I_ = fi.mmr_select(S, I, X, 5, 0.5, 0)
    assert I_.tolist() == [[0, 2, 1, 4, -1]]
    assert D_[0, :4].tolist() == [1.0, 0.5, 0.25, 1.0] and D_[0, 4] == -FLT_MAX
    assert fi.mmr_select(S, I, X, 3, 0.5, 0)[1].tolist() == [[0, 2, 1]]
    assert fi.mmr_select(S, I, X, 3, 1.0, 0)[1].tolist() == [[0, 4, 2]]
    # lam = 0: relevance plays no part.  After A: pen = 2, -0.5, 0.25 -> C; then pen_B = 2, pen_D = 0.25 -> D
    assert fi.mmr_select(S, I, X, 4, 0.0, 0)[1].tolist() == [[0, 2, 1, 4]]


def test_mmr_select_by_hand_l2():
    # the same rows under L2, q = (1, 0): squared distances D 0.5625, A 1, B 1, C 1.25 -> best first D, A, B, C
    X = np.array([[[0.25, 0], [1, 1], [1, 1], [0.5, -1]]], np.float32)
    S = np.array([[0.5625, 1.0, 1.0, 1.25]], np.float32)
    I = np.array([[1, 0, 4, 2]], np.int64)
    # step 1 (last = D): sim = -1.5625, -1.5625, -1.0625 -> v = -0.5 + 0.78125 (twice), -0.625 + 0.53125: A on the tie
    # step 2 (last = A): sim(B, A) = 0 exactly -> v_B = -0.5; pen_C = max(-1.0625, -4.25) -> v_C = -0.09375 -> C, then B
    D_, I_ = fi.mmr_select(S, I, X, 4, 0.5, 1)
    assert I_.tolist() == [[1, 0, 2, 4]] and D_.tolist() == [[0.5625, 1.0, 1.25, 1.0]]
    assert fi.mmr_select(S, I, X, 2, 1.0, 1)[1].tolist() == [[1, 0]]


def test_mmr_select_of_nothing():
    S = np.full((2, 4), -FLT_MAX, np.float32)
    I = np.full((2, 4), -1, np.int64)
    D_, I_ = fi.mmr_select(S, I, np.zeros((2, 4, 3), np.float32), 3, 0.5, 0)
    assert (I_ == -1).all() and (D_ == -FLT_MAX).all() and D_.shape == (2, 3)
    D_, I_ = fi.mmr_select(S[:0], I[:0], np.zeros((0, 4, 3), np.float32), 3, 0.5, 1)
    assert D_.shape == (0, 3) and I_.shape == (0, 3)


# ------------------------------------------------------------------------------------------------------ argument rules
def test_argument_rules():
    assert fi.diverse_args(8, 0, 0.5) == (8, 32, 0.5)
    assert fi.diverse_args(9, 0, 0) == (9, 128, 0.0)
    assert fi.diverse_args(1, 1, 1) == (1, 1, 1.0)
    assert fi.diverse_args(128, 0, 1.0) == (128, 128, 1.0)
    assert fi.diverse_args(32, 32, 0.25) == (32, 32, 0.25)
    for k, fetch, lam, word in ((0, 0, 0.5, "k="), (0, 32, 0.5, "k="), (33, 32, 0.5, "k="), (129, 0, 0.5, "k="),
                                (1, 129, 0.5, "fetch="), (1, -1, 0.5, "fetch="), (5, 0, -0.1, "lam="),
                                (5, 0, 1.5, "lam="), (5, 0, float("nan"), "lam=")):
        with pytest.raises(ValueError, match=word):
            fi.diverse_args(k, fetch, lam)


def test_index_methods_check_their_arguments_before_they_touch_the_device():
    ix = object.__new__(fi.IndexFlat)      # no device: the handle is never reached by a refused call
    ix.d, ix._h = 4, None
    q = np.zeros((2, 4), np.float32)
    for kw in (dict(k=0), dict(k=33, fetch=32), dict(k=5, fetch=129), dict(k=5, lam=-0.1), dict(k=5, lam=1.5),
               dict(k=5, lam=float("nan"))):
        with pytest.raises(ValueError):
            ix.search_diverse(q, **kw)
        with pytest.raises(ValueError):
            ix.search_diverse_dev(0, 2, kw.pop("k"), 0, 0, **kw)
    with pytest.raises(ValueError):
        ix.search_diverse(np.zeros((2, 5), np.float32), 3)           # wrong dimension
    with pytest.raises(RuntimeError, match="freed"):
        ix.search_diverse(q, 3)                                      # accepted arguments reach the handle


# ------------------------------------------------------------------------------------------------------ search_diverse
D_ = 4
Q = [1.0, 0.5, 0.0, 0.0]
# c0, c4 and c7 are one passage pasted into three sessions; the others are distinct
ROWS = [[1, 0.5, 0.5, 0], [1, 0, -0.5, 0], [0.5, 1, 0, 0.5], [0.75, 0.25, 0, -1], [1, 0.5, 0.5, 0], [0, 1, 0, 1],
        [0.5, 0, 1, 0], [1, 0.5, 0.5, 0], [0.25, 0.5, -0.5, 0.25], [-0.5, 0.25, 0, 0], [0.5, 0.5, 0.5, 0.5], [0, 0.25, 1, -1]]
SESS = ["a", "a", "b", "c", "b", "c", "a", "d", "d", "b", "e", "e"]
SCORE = [float(np.dot(np.array(r, np.float64), np.array(Q, np.float64))) for r in ROWS]


def _use(monkeypatch, cls):
    monkeypatch.setattr(fi, "IndexFlat", cls)
    monkeypatch.setattr(fi, "IndexFlatIP", lambda d, device=0: cls(d, 0, device))
    monkeypatch.setattr(fi, "IndexFlatL2", lambda d, device=0: cls(d, 1, device))


def _chunks(lo, hi):
    return [Chunk(f"c{i}", f"text {i}", {"project_name": "proj", "has_code": i % 2 == 0, "session_id": SESS[i]},
                  np.array(ROWS[i], np.float32)) for i in range(lo, hi)]


def _storage(tmp_path, pushdown=False, n=len(ROWS)):
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=D_, normalize_embeddings=True,
                                    auto_save=False, filter_pushdown=pushdown))
    s.initialize()
    if n:
        s.add_chunks(_chunks(0, n))
    return s


def _ids(res):
    return [r.chunk_id for r in res]


def _restated(cfg, lam=0.5, k=None, pool=lambda i: True, keep=lambda i: True):
    """The pool is every row that passes ``pool`` (12 rows: any fetch holds them all), best first; k picks by the loop
    statement; then threshold, ``keep`` and the cut at top_k, in pick order."""
    rows = sorted((i for i in range(len(ROWS)) if pool(i)), key=lambda i: (-SCORE[i], i))
    k = cfg.top_k if k is None else k
    S = np.array([[SCORE[i] for i in rows]], np.float32)
    I = np.array([rows], np.int64)
    X = np.array([[ROWS[i] for i in rows]], np.float32)
    Dp, Ip = mmr_loop(S, I, X, min(k, 128), lam, 0)
    out = [f"c{i}" for s, i in zip(Dp[0].tolist(), Ip[0].tolist()) if i >= 0 and s >= cfg.similarity_threshold and keep(i)]
    return out[:cfg.top_k]


@pytest.mark.parametrize("pushdown", [False, True])
def test_the_pasted_passage_comes_once_then_distinct_chunks(tmp_path, monkeypatch, pushdown):
    _use(monkeypatch, FakeDiverseIndex)
    s = _storage(tmp_path, pushdown)
    assert _ids(s.search(Q))[:3] == ["c0", "c4", "c7"]                       # search(): the three copies lead
    res = s.search_diverse(Q, SearchConfig(top_k=5))
    assert _ids(res) == _restated(SearchConfig(top_k=5))
    assert _ids(res)[0] == "c0" and not {"c4", "c7"} & set(_ids(res)[:3])
    assert s.faiss_index.calls[-1] == ("search_diverse", 5, False)
    by_id = {r.chunk_id: r.similarity for r in s.search(Q, SearchConfig(top_k=12, max_results=12))}
    assert all(r.similarity == by_id[r.chunk_id] for r in res)              # the ordinary score of every pick
    assert [r.similarity for r in res] != sorted((r.similarity for r in res), reverse=True)   # pick order, not score order
    # lam = 1 is search()
    assert _ids(s.search_diverse(Q, SearchConfig(top_k=5), lam=1.0)) == _ids(s.search(Q, SearchConfig(top_k=5)))
    for lam in (0.0, 0.25, 0.75):
        assert _ids(s.search_diverse(Q, SearchConfig(top_k=6), lam=lam)) == _restated(SearchConfig(top_k=6), lam=lam)
    s.close()


@pytest.mark.parametrize("pushdown", [False, True])
def test_the_threshold_is_applied_in_pick_order(tmp_path, monkeypatch, pushdown):
    _use(monkeypatch, FakeDiverseIndex)
    s = _storage(tmp_path, pushdown)
    full = s.search_diverse(Q, SearchConfig(top_k=8))
    thr = sorted(r.similarity for r in full)[3]                              # a value some picks fall below
    cfg = SearchConfig(top_k=8, similarity_threshold=thr)
    got = s.search_diverse(Q, cfg)
    assert _ids(got) == [r.chunk_id for r in full if r.similarity >= thr] == _restated(cfg)
    assert 0 < len(got) < len(full)
    s.close()


@pytest.mark.parametrize("pushdown", [False, True])
def test_tombstones_are_masked_out_in_both_modes(tmp_path, monkeypatch, pushdown):
    _use(monkeypatch, FakeDiverseIndex)
    s = _storage(tmp_path, pushdown)
    assert s.delete_chunk("c0") and s.delete_chunk("c3")
    res = s.search_diverse(Q, SearchConfig(top_k=5))
    assert _ids(res) == _restated(SearchConfig(top_k=5), pool=lambda i: i not in (0, 3))
    assert _ids(res)[0] == "c4" and "c7" not in _ids(res)[:3]                # the next copy leads, the third still waits
    assert s.faiss_index.calls[-1] == ("search_diverse", 5, True)
    s.close()


def test_filters_with_and_without_pushdown(tmp_path, monkeypatch):
    _use(monkeypatch, FakeDiverseIndex)
    odd = {"has_code": False}                                                # chunks with an odd number
    is_odd = lambda i: i % 2 == 1   # noqa: E731
    # pushed down: the pool holds matching chunks only, top_k picks
    s = _storage(tmp_path / "a", True)
    cfg = SearchConfig(top_k=4)
    assert _ids(s.search_diverse(Q, cfg, filters=odd)) == _restated(cfg, pool=is_odd)
    assert s.faiss_index.calls[-1] == ("search_diverse", 4, True)
    s.close()
    # not pushed down: max(top_k, max_results) picks over every chunk, filtered in pick order
    s = _storage(tmp_path / "b", False)
    cfg = SearchConfig(top_k=4, max_results=9)
    assert _ids(s.search_diverse(Q, cfg, filters=odd)) == _restated(cfg, k=9, keep=is_odd)
    assert s.faiss_index.calls[-1] == ("search_diverse", 9, False)
    assert _ids(s.search_diverse(Q, SearchConfig(top_k=4, max_results=1000), filters=odd)) == \
        _restated(SearchConfig(top_k=4), k=128, keep=is_odd)
    assert s.faiss_index.calls[-1] == ("search_diverse", 128, False)         # never more than the pool limit
    assert _ids(s.search_diverse(Q, cfg)) == _restated(cfg)
    assert s.faiss_index.calls[-1] == ("search_diverse", 4, False)           # no filter: top_k picks are enough
    s.close()


def test_an_index_without_diversified_search_raises(tmp_path, monkeypatch):
    _use(monkeypatch, FakeIndex)
    s = _storage(tmp_path)
    with pytest.raises(NotImplementedError):
        s.search_diverse(Q)
    assert _ids(s.search(Q))[:3] == ["c0", "c4", "c7"]
    s.close()


def test_empty_storage(tmp_path, monkeypatch):
    _use(monkeypatch, FakeDiverseIndex)
    s = _storage(tmp_path, n=0)
    assert s.search_diverse(Q) == []
    s.add_chunks(_chunks(0, 3))
    assert s.search_diverse(Q, SearchConfig(top_k=0)) == []
    s.close()

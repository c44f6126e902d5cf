"""CPU: the host side of the grouped search -- ``flat_index.collapse_groups`` against a loop-written statement (ties,
pads, negative labels), label validation, and ``HybridStorage.search_sessions`` over the numpy double
``grouped_fakes.FakeGroupedIndex`` (which states the operation as per-group maxima, with no passes)."""
import numpy as np
import pytest

from claude_semantic_search_amd import flat_index as fi
from claude_semantic_search_amd.chunk import Chunk
from claude_semantic_search_amd.storage import HybridStorage, SearchConfig, StorageConfig
from grouped_fakes import FakeGroupedIndex
from related_fakes import FakeIndex

FLT_MAX = np.finfo(np.float32).max


# ------------------------------------------------------------------------------------------------------ collapse_groups
def _collapse_loop(D, I, G, k, metric):
    nq = I.shape[0]
    Do = np.full((nq, k), -FLT_MAX if metric == 0 else FLT_MAX, np.float32)
    Io = np.full((nq, k), -1, np.int64)
    Go = np.full((nq, k), -1, np.int32)
    for j in range(nq):
        seen, m = set(), 0
        for s, i, g in zip(D[j], I[j], G[j]):
            if i < 0 or m == k:
                continue
            if g >= 0:
                if int(g) in seen:
                    continue
                seen.add(int(g))
            Do[j, m], Io[j, m], Go[j, m] = s, i, max(int(g), -1)
            m += 1
    return Do, Io, Go


@pytest.mark.parametrize("metric", [0, 1])
def test_collapse_groups_equals_the_loop(metric):
    rng = np.random.default_rng(1)
    for nq, kk, ngroups, k in ((1, 32, 5, 10), (7, 128, 40, 10), (3, 128, 3, 128), (5, 17, 100, 17), (2, 1, 1, 1), (4, 64, 8, 3)):
        s = rng.integers(-8, 9, size=(nq, kk)) / 8.0                       # a coarse grid: ties
        D = (np.sort(s, axis=1)[:, ::-1] if metric == 0 else np.sort(s, axis=1)).astype(np.float32)
        I = np.stack([rng.permutation(1000)[:kk] for _ in range(nq)]).astype(np.int64)
        G = rng.integers(-3, ngroups, size=(nq, kk)).astype(np.int32)      # -3 .. -1: ungrouped
        npad = rng.integers(0, kk + 1, size=nq)
        for j in range(nq):                                                # pads at the tail
            if npad[j]:
                I[j, kk - npad[j]:], D[j, kk - npad[j]:], G[j, kk - npad[j]:] = -1, (-FLT_MAX if metric == 0 else FLT_MAX), -1
        got = fi.collapse_groups(D, I, G, k, metric)
        want = _collapse_loop(D, I, G, k, metric)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b), (nq, kk, ngroups, k)


def test_collapse_groups_by_hand():
    D = np.array([[0.9, 0.9, 0.8, 0.7, 0.7, 0.1, -FLT_MAX]], np.float32)
    I = np.array([[4, 9, 2, 7, 8, 1, -1]], np.int64)
    G = np.array([[5, 5, -1, -1, 6, 5, -1]], np.int32)
    Do, Io, Go = fi.collapse_groups(D, I, G, 5, 0)
    assert Io.tolist() == [[4, 2, 7, 8, -1]] and Go.tolist() == [[5, -1, -1, 6, -1]]
    assert Do[0, :4].tolist() == [np.float32(0.9), np.float32(0.8), np.float32(0.7), np.float32(0.7)] and Do[0, 4] == -FLT_MAX
    Do, Io, Go = fi.collapse_groups(D, I, G, 2, 0)
    assert Io.tolist() == [[4, 2]] and Go.tolist() == [[5, -1]]


# ----------------------------------------------------------------------------------------------------- label validation
def test_label_validation():
    assert fi.labels_as_int32([3, -7, 0]).dtype == np.int32
    assert fi.labels_as_int32(np.array([2 ** 31 - 1, -2 ** 31], np.int64)).tolist() == [2 ** 31 - 1, -2 ** 31]
    assert fi.labels_as_int32(np.zeros(0, np.int64)).shape == (0,)
    for bad in (np.zeros(3, np.float32), np.zeros(3, np.bool_), ["a"], np.zeros((2, 2), np.int32),
                np.array([2 ** 31], np.int64), np.array([-2 ** 31 - 1], np.int64), np.array([2 ** 63], np.uint64)):
        with pytest.raises(ValueError):
            fi.labels_as_int32(bad)


# ------------------------------------------------------------------------------------------------------ search_sessions
D_ = 4
# chunk i: score against Q = ROWS[i]; sessions of very unequal size; c3 and c9 have no session
ROWS = [1.0, 0.875, 0.875, 0.75, 0.625, 0.5, 0.5, 0.375, 0.25, 0.125, 0.0, -0.125]
SESS = ["big", "big", "big", None, "big", "mid", "big", "mid", "one", None, "big", "mid"]
Q = [1.0, 0.0, 0.0, 0.0]


def _use(monkeypatch, cls):
    monkeypatch.setattr(fi, "IndexFlat", cls)
    monkeypatch.setattr(fi, "IndexFlatIP", lambda d, device=0: cls(d, 0, device))
    monkeypatch.setattr(fi, "IndexFlatL2", lambda d, device=0: cls(d, 1, device))


def _chunks(lo, hi):
    out = []
    for i in range(lo, hi):
        e = np.zeros(D_, np.float32)
        e[0] = ROWS[i]
        md = {"project_name": "proj", "has_code": i % 2 == 0}
        if SESS[i] is not None:
            md["session_id"] = SESS[i]
        out.append(Chunk(f"c{i}", f"text {i}", md, e))
    return out


def _storage(tmp_path, pushdown=False, l2=False, n=len(ROWS)):
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=D_, normalize_embeddings=not l2,
                                    auto_save=False, filter_pushdown=pushdown))
    s.initialize()
    if n:
        s.add_chunks(_chunks(0, n))
    return s


def _ids(res):
    return [r.chunk_id for r in res]


def _restated(cfg, dead=(), keep=lambda i: True, n=len(ROWS), l2=False):
    """Per session the best live chunk that passes ``keep`` (a chunk without a session stands for itself), then
    threshold, rank order, cut at top_k."""
    score = (lambda i: (1.0 - ROWS[i]) ** 2) if l2 else (lambda i: ROWS[i])
    best = {}
    for i in range(n):
        if i in dead or not keep(i):
            continue
        key = SESS[i] if SESS[i] is not None else ("own", i)
        rank = (score(i) if l2 else -score(i), i)
        if key not in best or rank < best[key]:
            best[key] = rank
    reps = sorted(best.values())
    return [f"c{i}" for _, i in reps if score(i) >= cfg.similarity_threshold][:cfg.top_k]


@pytest.mark.parametrize("pushdown", [False, True])
def test_one_chunk_per_session_in_rank_order(tmp_path, monkeypatch, pushdown):
    _use(monkeypatch, FakeGroupedIndex)
    s = _storage(tmp_path, pushdown)
    cfg = SearchConfig()
    res = s.search_sessions(Q)
    assert _ids(res) == ["c0", "c3", "c5", "c8", "c9"] == _restated(cfg)
    assert [r.similarity for r in res] == [1.0, 0.75, 0.5, 0.25, 0.125]
    assert res[0].metadata["session_id"] == "big" and res[1].metadata.get("session_id") is None
    assert _ids(s.search_sessions(Q, SearchConfig(top_k=2))) == ["c0", "c3"]
    assert _ids(s.search_sessions(Q, SearchConfig(similarity_threshold=0.3))) == ["c0", "c3", "c5"]
    # search() is what it was: ten chunks, seven of them of one session
    assert _ids(s.search(Q)) == [f"c{i}" for i in range(10)]
    # the labels: dense, in order of first appearance by faiss_id; pushed once
    assert s.faiss_index.get_groups().tolist() == [0, 0, 0, -1, 0, 1, 0, 1, 2, -1, 0, 1]
    assert [c for c in s.faiss_index.calls if c[0] == "set_groups"] == [("set_groups", 0, 12)]
    s.close()


@pytest.mark.parametrize("pushdown", [False, True])
def test_labels_are_pushed_lazily_tail_after_adds_everything_after_a_rebuild(tmp_path, monkeypatch, pushdown):
    _use(monkeypatch, FakeGroupedIndex)
    s = _storage(tmp_path, pushdown, n=6)
    assert not [c for c in s.faiss_index.calls if c[0] == "set_groups"]          # add_chunks makes no new call
    assert _ids(s.search_sessions(Q)) == _restated(SearchConfig(), n=6)
    s.add_chunks(_chunks(6, 12))
    assert _ids(s.search(Q)) == [f"c{i}" for i in range(10)]
    assert not [c for c in s.faiss_index.calls if c[0] == "set_groups" and c[1] == 6]   # ... nor does search
    assert _ids(s.search_sessions(Q)) == ["c0", "c3", "c5", "c8", "c9"]
    assert [c for c in s.faiss_index.calls if c[0] == "set_groups"] == [("set_groups", 0, 6), ("set_groups", 6, 6)]
    # tombstones never stand for their session; the next best chunk does
    assert s.delete_chunk("c0") and s.delete_chunk("c5") and s.delete_chunk("c8")
    dead = {0, 5, 8}
    assert _ids(s.search_sessions(Q)) == ["c1", "c3", "c7", "c9"] == _restated(SearchConfig(), dead)
    # compaction renumbers the rows: every label is pushed again
    s.optimize()
    assert s.faiss_index.ntotal == 9
    assert _ids(s.search_sessions(Q)) == ["c1", "c3", "c7", "c9"]
    assert [c for c in s.faiss_index.calls if c[0] == "set_groups"][-1] == ("set_groups", 0, 9)
    # a new index object (clear_all_data) starts over
    s.clear_all_data()
    assert s.search_sessions(Q) == []
    s.add_chunks(_chunks(4, 8))
    assert _ids(s.search_sessions(Q)) == ["c4", "c5"]
    assert s.faiss_index.get_groups().tolist() == [0, 1, 0, 1]
    s.close()


def test_filters_with_and_without_pushdown(tmp_path, monkeypatch):
    _use(monkeypatch, FakeGroupedIndex)
    odd = {"has_code": False}                       # chunks with an odd number
    # pushed down: every session is represented by its best MATCHING chunk
    s = _storage(tmp_path / "a", True)
    assert _ids(s.search_sessions(Q, filters=odd)) == ["c1", "c3", "c5", "c9"] == _restated(SearchConfig(), keep=lambda i: i % 2 == 1)
    assert s.faiss_index.calls[-1] == ("search_grouped", 10, True)
    s.close()
    # not pushed down: groups whose best row fails the filter are dropped on the host (big -> c0 and one -> c8 fail)
    s = _storage(tmp_path / "b", False)
    assert _ids(s.search_sessions(Q, filters=odd)) == ["c3", "c5", "c9"]
    assert s.faiss_index.calls[-1] == ("search_grouped", 12, False)       # min(max_results, ntotal) groups fetched
    assert _ids(s.search_sessions(Q)) == ["c0", "c3", "c5", "c8", "c9"]
    assert s.faiss_index.calls[-1] == ("search_grouped", 10, False)       # no filter: top_k groups are enough
    s.close()


def test_l2_storage_ranks_sessions_by_distance(tmp_path, monkeypatch):
    _use(monkeypatch, FakeGroupedIndex)
    s = _storage(tmp_path, l2=True)
    res = s.search_sessions(Q, SearchConfig(top_k=3))
    assert _ids(res) == ["c0", "c3", "c5"] == _restated(SearchConfig(top_k=3), l2=True)
    assert [r.similarity for r in res] == [0.0, 0.0625, 0.25]
    s.close()


def test_an_index_without_grouped_search_raises(tmp_path, monkeypatch):
    _use(monkeypatch, FakeIndex)
    s = _storage(tmp_path)
    with pytest.raises(NotImplementedError):
        s.search_sessions(Q)
    assert _ids(s.search(Q)) == [f"c{i}" for i in range(10)]
    s.close()


def test_empty_storage(tmp_path, monkeypatch):
    _use(monkeypatch, FakeGroupedIndex)
    s = _storage(tmp_path, n=0)
    assert s.search_sessions(Q) == []
    s.close()

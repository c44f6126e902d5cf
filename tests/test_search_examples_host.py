"""CPU: the host side of the search by examples -- the argument rules of ``IndexFlat.search_examples``
(``flat_index.example_args`` / ``example_vectors``), ``flat_index.fuse_example_scores`` against an fp64 statement, and
``HybridStorage.search_like`` over the numpy double ``examples_fakes.FakeExamplesIndex``.  Embeddings are multiples of
1/8, so every fused value is exact and the expected order is restated here in plain Python."""
import numpy as np
import pytest

from claude_semantic_search_amd import flat_index as fi
from claude_semantic_search_amd.chunk import Chunk
from claude_semantic_search_amd.storage import HybridStorage, SearchConfig, StorageConfig
from examples_fakes import FakeExamplesIndex
from related_fakes import FakeIndex

D_ = 8


# ------------------------------------------------------------------------------------------------- argument rules
def test_argument_validation():
    assert fi.MAX_EXAMPLES == 16 and fi.MAX_EXAMPLES_K == 128
    assert fi.example_args(10, 0.5, 1, 1) == (10, 0.5)
    assert fi.example_args(np.int64(128), 0, 3, 16) == (128, 0.0)
    for k in (0, -1, 129):
        with pytest.raises(ValueError, match="k="):
            fi.example_args(k, 0.5, 1, 1)
    for g in (float("nan"), float("inf"), -0.5, float("-inf")):
        with pytest.raises(ValueError, match="gamma"):
            fi.example_args(5, g, 1, 2)
    with pytest.raises(ValueError, match="positive"):
        fi.example_args(5, 0.5, 0, 3)
    with pytest.raises(ValueError, match="16"):
        fi.example_args(5, 0.5, 9, 17)
    assert fi.example_vectors(None, D_).shape == (0, D_)
    assert fi.example_vectors([], D_).shape == (0, D_)
    assert fi.example_vectors(np.zeros((0, D_)), D_).shape == (0, D_)
    one = fi.example_vectors(np.arange(D_), D_)
    assert one.shape == (1, D_) and one.dtype == np.float32 and one.flags["C_CONTIGUOUS"]
    assert fi.example_vectors(np.ones((3, D_), np.float64)[::2], D_).shape == (2, D_)
    for bad in (np.zeros(D_ + 1), np.zeros((2, D_ - 1)), np.zeros((2, 2, D_))):
        with pytest.raises(ValueError):
            fi.example_vectors(bad, D_)


# ------------------------------------------------------------------------------------------------- the fusion rule
@pytest.mark.parametrize("metric", [0, 1])
def test_fuse_example_scores_against_fp64(metric):
    rng = np.random.default_rng(3 + metric)
    n = 5000
    ext = np.max if metric == 0 else np.min
    for npos, nneg in ((1, 0), (3, 0), (1, 1), (4, 5), (1, 15)):
        Sp = rng.standard_normal((npos, n)).astype(np.float32) * (1 if metric == 0 else 3) ** 2
        Sn = rng.standard_normal((nneg, n)).astype(np.float32)
        if metric == 1:
            Sp, Sn = np.abs(Sp), np.abs(Sn)
        for gamma in (0.0, 0.5, 1.0, 0.3):
            F, P = fi.fuse_example_scores(Sp, Sn, gamma, metric)
            assert F.dtype == P.dtype == np.float32 and F.shape == P.shape == (n,)
            P64 = ext(Sp.astype(np.float64), axis=0)
            assert np.array_equal(P.astype(np.float64), P64), "an extremum of float32 values is exact"
            if nneg == 0:
                assert np.array_equal(F.view(np.uint32), P.view(np.uint32)), "no negative: F is P, bit for bit"
                continue
            F64 = P64 - np.float64(np.float32(gamma)) * ext(Sn.astype(np.float64), axis=0)
            # one rounding of the exact value: within half a float32 ulp of it, and exactly its float32 rounding
            assert np.array_equal(F, F64.astype(np.float32))
            assert (np.abs(F.astype(np.float64) - F64) <= 2.0 ** -24 * np.abs(F64) + 1e-45).all()
            if gamma == 0.0:
                assert np.array_equal(F.view(np.uint32), P.view(np.uint32)), "gamma 0: F is P"
    # small exact cases, both metrics' direction
    F, P = fi.fuse_example_scores([[1.0, 0.25], [0.5, 0.75]], [[0.5, 1.0]], 0.5, 0)
    assert P.tolist() == [1.0, 0.75] and F.tolist() == [0.75, 0.25]
    F, P = fi.fuse_example_scores([[1.0, 0.25], [0.5, 0.75]], [[0.5, 1.0], [2.0, 0.125]], 2.0, 1)
    assert P.tolist() == [0.5, 0.25] and F.tolist() == [-0.5, 0.0]
    F, P = fi.fuse_example_scores(np.ones((2, 3)), np.zeros((0, 3)), 0.5, 0)
    assert F.tolist() == P.tolist() == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError):
        fi.fuse_example_scores(np.zeros((0, 3)), np.zeros((1, 3)), 0.5, 0)
    with pytest.raises(ValueError):
        fi.fuse_example_scores(np.zeros((1, 3)), np.zeros((1, 4)), 0.5, 0)


# ------------------------------------------------------------------------------------------------- search_like
# twelve chunks in eight dimensions, coordinates in eighths; c0..c2 point along axis 0, c3..c5 along axis 1, the rest mix
E = np.array([[8, 0, 0, 0, 0, 0, 0, 0], [7, 1, 0, 0, 0, 0, 0, 0], [6, 0, 2, 0, 0, 0, 0, 0], [0, 8, 0, 0, 0, 0, 0, 0],
              [1, 7, 0, 0, 0, 0, 0, 0], [0, 6, 0, 2, 0, 0, 0, 0], [4, 4, 0, 0, 0, 0, 0, 0], [5, 3, 1, 0, 0, 0, 0, 0],
              [3, 5, 0, 1, 0, 0, 0, 0], [2, 2, 4, 0, 0, 0, 0, 0], [0, 0, 8, 0, 0, 0, 0, 0], [4, 0, 4, 0, 0, 0, 0, 0]],
             np.float32) / 8.0
N_ = E.shape[0]


def _use(monkeypatch, cls):
    monkeypatch.setattr(fi, "IndexFlat", cls)
    monkeypatch.setattr(fi, "IndexFlatIP", lambda d, device=0: cls(d, 0, device))
    monkeypatch.setattr(fi, "IndexFlatL2", lambda d, device=0: cls(d, 1, device))


def _storage(tmp_path, pushdown=False, l2=False, n=N_):
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=D_, normalize_embeddings=not l2,
                                    auto_save=False, filter_pushdown=pushdown))
    s.initialize()
    if n:
        s.add_chunks([Chunk(f"c{i}", f"text {i}", {"project_name": "proj", "has_code": i % 2 == 0}, E[i].copy()) for i in range(n)])
    return s


def _ids(res):
    return [r.chunk_id for r in res]


def _score(a, b, l2):
    return float(((a - b) ** 2).sum()) if l2 else float((a * b).sum())


def _restated(cfg, liked, disliked=(), query=None, gamma=0.5, dead=(), keep=lambda i: True, l2=False, fetch=None):
    """Every live chunk that is no example and passes ``keep``, ranked by the fused value (ties: lower row); of the
    first ``fetch`` (default: top_k, what the index is asked for) those that pass the threshold on the RAW best-liked
    similarity, cut at top_k."""
    pos = [E[i] for i in liked] + ([np.asarray(query, np.float32)] if query is not None else [])
    best = min if l2 else max
    rows = []
    for i in range(N_):
        if i in dead or i in liked or i in disliked or not keep(i):
            continue
        p = best(_score(E[i], e, l2) for e in pos)
        f = p - gamma * best(_score(E[i], E[j], l2) for j in disliked) if disliked else p
        rows.append((f if l2 else -f, i, p))
    rows.sort()
    rows = rows[:cfg.top_k if fetch is None else fetch]
    return [(f"c{i}", p) for _, i, p in rows if p >= cfg.similarity_threshold][:cfg.top_k]


@pytest.mark.parametrize("pushdown", [False, True])
def test_fused_order_raw_similarity_examples_left_out(tmp_path, monkeypatch, pushdown):
    _use(monkeypatch, FakeExamplesIndex)
    s = _storage(tmp_path, pushdown)
    cfg = SearchConfig()
    for liked, disliked, query, gamma in (([0], [], None, 0.5), ([0, 3], [], None, 0.5), ([0], [3], None, 0.5),
                                          ([0], [3], None, 1.0), ([0, 10], [3, 5], None, 0.25), ([], [3], E[0], 0.5),
                                          ([10], [4], E[6], 0.5), ([0], [3], None, 0.0)):
        res = s.search_like([f"c{i}" for i in liked], [f"c{i}" for i in disliked], query_embedding=query, gamma=gamma)
        want = _restated(cfg, liked, disliked, query, gamma)
        what = (liked, disliked, gamma)
        assert _ids(res) == [c for c, _ in want] and [r.similarity for r in res] == [v for _, v in want], what
        assert not {f"c{i}" for i in liked + disliked} & set(_ids(res)), what     # examples are never returned
        call = s.faiss_index.calls[-1]
        assert call[0] == "search_examples" and call[3:] == (len(liked) + (query is not None), len(disliked), True), what
    # the negatives reorder: without them c1 leads the chunks like c0, with c4 disliked... c6 (half axis 1) falls behind c2
    assert _ids(s.search_like(["c0"]))[:3] == ["c1", "c2", "c7"]
    assert _ids(s.search_like(["c0"], ["c3"], gamma=1.0))[:3] == ["c1", "c2", "c11"]
    # a string is one chunk id; similarity is the RAW best-liked score, to which the threshold applies
    assert _ids(s.search_like("c0", "c3")) == _ids(s.search_like(["c0"], ["c3"]))
    got = s.search_like(["c0"], ["c3"], config=SearchConfig(similarity_threshold=0.6), gamma=1.0)
    assert _ids(got) == [c for c, _ in _restated(SearchConfig(similarity_threshold=0.6), [0], [3], gamma=1.0)]
    assert all(r.similarity >= 0.6 for r in got) and len(got) < len(s.search_like(["c0"], ["c3"], gamma=1.0))
    top3 = s.search_like(["c0", "c3"], config=SearchConfig(top_k=3))
    assert _ids(top3) == [c for c, _ in _restated(SearchConfig(top_k=3), [0, 3])] and len(top3) == 3
    assert s.faiss_index.calls[-1][1] == 3
    s.close()


@pytest.mark.parametrize("pushdown", [False, True])
def test_tombstones_always_go_into_the_mask(tmp_path, monkeypatch, pushdown):
    _use(monkeypatch, FakeExamplesIndex)
    s = _storage(tmp_path, pushdown)
    for c in ("c1", "c7"):
        s.delete_chunk(c)
    res = s.search_like(["c0"], ["c3"])
    assert _ids(res) == [c for c, _ in _restated(SearchConfig(), [0], [3], dead=(1, 7))]
    assert s.faiss_index.calls[-1][2] is True                                  # a mask in both modes
    with pytest.raises(KeyError):
        s.search_like(["c1"])                                                  # a deleted chunk is no example
    with pytest.raises(KeyError):
        s.search_like(["c0"], ["c7"])
    s.close()


def test_filters_with_and_without_pushdown(tmp_path, monkeypatch):
    _use(monkeypatch, FakeExamplesIndex)
    odd = {"has_code": False}                       # chunks with an odd number
    s = _storage(tmp_path / "a", True)
    res = s.search_like(["c0"], ["c3"], config=SearchConfig(top_k=3), filters=odd)
    assert _ids(res) == [c for c, _ in _restated(SearchConfig(top_k=3), [0], [3], keep=lambda i: i % 2 == 1)]
    assert s.faiss_index.calls[-1][:3] == ("search_examples", 3, True)          # the filter is in the mask: top_k rows
    s.close()
    s = _storage(tmp_path / "b", False)
    res = s.search_like(["c0"], ["c3"], config=SearchConfig(top_k=3), filters=odd)
    assert _ids(res) == [c for c, _ in _restated(SearchConfig(top_k=3), [0], [3], keep=lambda i: i % 2 == 1)]
    assert s.faiss_index.calls[-1][:3] == ("search_examples", 100, False)       # max(top_k, max_results) rows, filtered in rank order
    s.search_like(["c0"], config=SearchConfig(top_k=3, max_results=500), filters=odd)
    assert s.faiss_index.calls[-1][:3] == ("search_examples", 128, False)       # ... at most 128
    res = s.search_like(["c0"], ["c3"], config=SearchConfig(top_k=3, max_results=2), filters=odd)
    assert s.faiss_index.calls[-1][:3] == ("search_examples", 3, False)
    first3 = [c for c, _ in _restated(SearchConfig(top_k=3), [0], [3])]
    assert _ids(res) == [c for c in first3 if int(c[1:]) % 2 == 1]              # of the fused top-3, the odd ones
    s.search_like(["c0"], config=SearchConfig(top_k=3))
    assert s.faiss_index.calls[-1][:3] == ("search_examples", 3, False)         # no filter: top_k rows are enough
    s.close()


def test_l2_storage_ranks_by_nearest_liked_minus_nearest_disliked(tmp_path, monkeypatch):
    _use(monkeypatch, FakeExamplesIndex)
    s = _storage(tmp_path, l2=True)
    cfg = SearchConfig(top_k=5, similarity_threshold=-1.0)
    res = s.search_like(["c0", "c10"], ["c3"], config=cfg, gamma=0.5)
    want = _restated(cfg, [0, 10], [3], l2=True)
    assert _ids(res) == [c for c, _ in want] and [r.similarity for r in res] == [v for _, v in want]
    s.close()


def test_argument_errors_and_an_index_without_the_method(tmp_path, monkeypatch):
    _use(monkeypatch, FakeExamplesIndex)
    s = _storage(tmp_path / "a")
    with pytest.raises(ValueError, match="positive"):
        s.search_like([])
    with pytest.raises(ValueError, match="positive"):
        s.search_like([], ["c3"])
    for g in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="gamma"):
            s.search_like(["c0"], ["c3"], gamma=g)
    with pytest.raises(ValueError, match="16"):
        s.search_like([f"c{i}" for i in range(9)] , [f"c{i}" for i in range(4)] * 2)
    for liked, disliked in ((["nope"], []), (["c0", "nope"], []), (["c0"], ["nope"])):
        with pytest.raises(KeyError):
            s.search_like(liked, disliked)
    assert not [c for c in s.faiss_index.calls if c[0] == "search_examples"]    # nothing reached the index
    assert s.search_like(["c0"], config=SearchConfig(top_k=0)) == []
    assert len(s.search_like(["c0"])) == 10                                     # the defaults
    s.close()
    _use(monkeypatch, FakeIndex)
    s = _storage(tmp_path / "b")
    with pytest.raises(NotImplementedError):
        s.search_like(["c0"])
    s.close()
    _use(monkeypatch, FakeExamplesIndex)
    s = _storage(tmp_path / "c", n=0)
    assert s.search_like(["c0"]) == [] and s.search_like([], query_embedding=E[0]) == []   # an empty index
    with pytest.raises(ValueError):
        s.search_like([])
    s.close()

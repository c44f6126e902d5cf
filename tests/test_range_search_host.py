"""CPU: ``HybridStorage.search_range`` over a numpy TEST DOUBLE of the device index that implements ``range_search``
(strict comparison, best first, ties by id -- the contract of ``css_index_range_search``).  The double lives here in
tests/ only; the product never falls back to it.

Rows are built from multiples of 1/8 so that every score is exact in float32 and float64 alike and thresholds can sit
exactly ON a score: that is what tells ``>=`` from ``>``."""
import numpy as np
import pytest

from claude_semantic_search_amd import flat_index as fi
from claude_semantic_search_amd.chunk import Chunk
from claude_semantic_search_amd.storage import HybridStorage, SearchConfig, StorageConfig


class _FakeRangeIndex:
    calls = []   # (radius, allow is not None) of every range_search, newest last

    def __init__(self, d, metric=0, device=0):
        self.d, self.metric_type, self.device = int(d), int(metric), device
        self._x = np.zeros((0, self.d), np.float32)

    ntotal = property(lambda self: self._x.shape[0])

    def add(self, x, normalize=False):   # (`normalize` is the device's business, tested on the GPU: rows stay as given)
        self._x = np.concatenate([self._x, np.asarray(x, np.float32).reshape(-1, self.d)])

    def _scores(self, q):
        if self.metric_type == 0:
            return (q[:, None, :] * self._x[None, :, :]).sum(-1, dtype=np.float32)
        return ((q[:, None, :] - self._x[None, :, :]) ** 2).sum(-1, dtype=np.float32)

    def search(self, q, k, normalize=False, allow=None):
        raise AssertionError("search_range must not go through the top-k search")

    def range_search(self, q, thresh, normalize=False, allow=None):
        _FakeRangeIndex.calls.append((np.float32(thresh), allow is not None))
        q = np.asarray(q, np.float32).reshape(-1, self.d)
        s = self._scores(q)
        r = np.float32(thresh)
        lims, D, I = [0], [], []
        for j in range(q.shape[0]):
            hit = s[j] > r if self.metric_type == 0 else s[j] < r       # strict, as the library
            if allow is not None:
                hit &= np.asarray(allow, bool)
            ids = np.flatnonzero(hit)
            order = np.lexsort((ids, -s[j, ids] if self.metric_type == 0 else s[j, ids]))
            D.append(s[j, ids][order])
            I.append(ids[order].astype(np.int64))
            lims.append(lims[-1] + ids.size)
        return np.array(lims, np.int64), np.concatenate(D).astype(np.float32), np.concatenate(I)

    def reconstruct_n(self, row0=0, n=None):
        n = self.ntotal - row0 if n is None else n
        return self._x[row0:row0 + n].copy()

    def reserve(self, n):
        pass

    def close(self):
        pass


@pytest.fixture(autouse=True)
def fake_device_index(monkeypatch):
    _FakeRangeIndex.calls = []
    monkeypatch.setattr(fi, "IndexFlat", _FakeRangeIndex)
    monkeypatch.setattr(fi, "IndexFlatIP", lambda d, device=0: _FakeRangeIndex(d, 0, device))
    monkeypatch.setattr(fi, "IndexFlatL2", lambda d, device=0: _FakeRangeIndex(d, 1, device))


D_ = 4


def _storage(tmp_path, rows, l2=False, pushdown=False, name="s"):
    """Row i = (rows[i], 0, 0, 0) (the double stores it as given): IP score with q = (1, 0, 0, 0) is rows[i], L2 distance (rows[i] - 1)^2."""
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / name), embedding_dim=D_, normalize_embeddings=not l2,
                                    auto_save=False, filter_pushdown=pushdown))
    s.initialize()
    chunks = []
    for i, v in enumerate(rows):
        e = np.zeros(D_, np.float32)
        e[0] = v
        chunks.append(Chunk(f"c{i}", f"text {i}", {"session_id": f"s{i % 3}", "project_name": "proj", "has_code": i % 2 == 0}, e))
    if chunks:
        s.add_chunks(chunks)
    return s


Q = [1.0, 0.0, 0.0, 0.0]
ROWS = [0.125 * i for i in range(-8, 9)]          # scores -1.0 .. 1.0 in steps of 1/8, chunk c(i) has score (i - 8) / 8


def _ids(res):
    return [r.chunk_id for r in res]


def test_greater_or_equal_at_an_exactly_representable_threshold(tmp_path):
    s = _storage(tmp_path, ROWS)
    res = s.search_range(np.array(Q, np.float32), threshold=0.5)
    assert _ids(res) == ["c16", "c15", "c14", "c13", "c12"]           # 1.0, .875, .75, .625 and 0.5 ITSELF
    assert [r.similarity for r in res] == [1.0, 0.875, 0.75, 0.625, 0.5]
    # the index was asked strictly, with the float32 just below the threshold
    assert _FakeRangeIndex.calls[-1][0] == np.nextafter(np.float32(0.5), np.float32(-np.inf))
    # a threshold a hair above the score excludes it; one that float32 cannot represent is not rounded down past a score
    assert _ids(s.search_range(Q, threshold=float(np.nextafter(np.float32(0.5), np.float32(1))))) == ["c16", "c15", "c14", "c13"]
    assert _ids(s.search_range(Q, threshold=0.5 + 1e-12)) == ["c16", "c15", "c14", "c13"]
    assert _ids(s.search_range(Q, threshold=0.5 - 1e-12)) == ["c16", "c15", "c14", "c13", "c12"]
    with pytest.raises(ValueError):
        s.search_range(Q, threshold=float("nan"))
    s.close()


def test_threshold_defaults_to_the_config_and_results_carry_the_usual_fields(tmp_path):
    s = _storage(tmp_path, ROWS)
    res = s.search_range(Q, config=SearchConfig(similarity_threshold=0.875))
    assert _ids(res) == ["c16", "c15"]
    assert res[0].text == "text 16" and res[0].metadata["session_id"] == "s1" and res[0].chunk.id == "c16"
    bare = s.search_range(Q, threshold=0.875, config=SearchConfig(include_text=False, include_metadata=False))
    assert _ids(bare) == ["c16", "c15"] and bare[0].text is None and bare[0].metadata is None and bare[0].chunk is None
    assert len(s.search_range(Q)) == 9                                  # default threshold 0.0: scores 0 .. 1
    s.close()


def test_list_input_empty_index_and_limit(tmp_path):
    empty = _storage(tmp_path, [], name="e")
    assert empty.search_range(Q, threshold=-1.0) == []
    empty.close()
    s = _storage(tmp_path, ROWS)
    assert _ids(s.search_range(list(Q), threshold=0.75)) == ["c16", "c15", "c14"]
    assert _ids(s.search_range(Q, threshold=-1.0, limit=4)) == ["c16", "c15", "c14", "c13"]
    assert s.search_range(Q, threshold=-1.0, limit=0) == []
    assert len(s.search_range(Q, threshold=-1.0, limit=1000)) == len(ROWS)
    s.close()


def test_not_capped_by_max_results_or_top_k(tmp_path):
    rows = [0.5 + (i % 64) / 128 for i in range(300)]                  # 300 rows, all scores in [0.5, 1)
    s = _storage(tmp_path, rows)
    cfg = SearchConfig(top_k=10, max_results=100)
    res = s.search_range(Q, threshold=0.5, config=cfg)
    assert len(res) == 300 > cfg.max_results
    sims = [r.similarity for r in res]
    assert sims == sorted(sims, reverse=True)
    ties = [int(r.chunk_id[1:]) for r in res if r.similarity == sims[0]]
    assert ties == sorted(ties) and len(ties) > 1                      # equal scores by ascending row id
    s.close()


@pytest.mark.parametrize("pushdown", [False, True])
def test_filters_and_tombstones_with_and_without_pushdown(tmp_path, pushdown):
    s = _storage(tmp_path, ROWS, pushdown=pushdown)
    assert s.delete_chunk("c15") and s.delete_chunk("c2")
    assert s.faiss_index.ntotal == len(ROWS)                            # tombstones: the rows are still in the index
    assert _ids(s.search_range(Q, threshold=0.5)) == ["c16", "c14", "c13", "c12"]
    assert _FakeRangeIndex.calls[-1][1] is pushdown                     # the mask is used exactly when pushed down
    assert _ids(s.search_range(Q, threshold=0.0, filters={"session_id": "s1"})) == ["c16", "c13", "c10"]
    assert _ids(s.search_range(Q, threshold=0.0, filters={"has_code": True, "session_id": ["s0", "s2"]})) == ["c14", "c12", "c8"]
    assert _ids(s.search_range(Q, threshold=0.0, filters={"session_id": "s1"}, limit=2)) == ["c16", "c13"]
    assert s.search_range(Q, threshold=0.0, filters={"session_id": "nobody"}) == []
    s.close()


def test_l2_storage_means_distance_at_most_threshold(tmp_path):
    s = _storage(tmp_path, ROWS, l2=True)
    assert s.faiss_index.metric_type == fi.METRIC_L2
    # distance to q is ((i - 8) / 8 - 1)^2: 0 (c16), 1/64 (c15), 4/64 (c14), 9/64 (c13) ...
    res = s.search_range(Q, threshold=0.0625)
    assert _ids(res) == ["c16", "c15", "c14"] and [r.similarity for r in res] == [0.0, 0.015625, 0.0625]
    assert _FakeRangeIndex.calls[-1][0] == np.nextafter(np.float32(0.0625), np.float32(np.inf))
    assert _ids(s.search_range(Q, threshold=0.0625 - 1e-12)) == ["c16", "c15"]
    assert _ids(s.search_range(Q, threshold=0.0)) == ["c16"]            # distance 0 <= 0
    assert s.search_range(Q, threshold=-1.0) == []
    s.close()


def test_search_is_untouched(tmp_path):
    """``search()`` still goes through the top-k call (the double's ``search`` raises)."""
    s = _storage(tmp_path, ROWS)
    with pytest.raises(AssertionError, match="top-k"):
        s.search(Q)
    s.close()

"""CPU: ``HybridStorage.search_related`` over the numpy test double of the device index (``related_fakes.FakeIndex``,
patched in the way ``test_range_search_host.py`` does it).

Row i = (ROWS[i], 0, 0, 0) with ROWS multiples of 1/8, stored as given: with the inner product the score of chunk i
against anchor a is ROWS[i] * ROWS[a], exact in float32.  Chunk i belongs to session ``s{i % 3}``."""
import numpy as np
import pytest

from claude_semantic_search_amd import flat_index as fi
from claude_semantic_search_amd.chunk import Chunk
from claude_semantic_search_amd.storage import HybridStorage, SearchConfig, StorageConfig
from related_fakes import FakeIndex


@pytest.fixture(autouse=True)
def fake_device_index(monkeypatch):
    monkeypatch.setattr(fi, "IndexFlat", FakeIndex)
    monkeypatch.setattr(fi, "IndexFlatIP", lambda d, device=0: FakeIndex(d, 0, device))
    monkeypatch.setattr(fi, "IndexFlatL2", lambda d, device=0: FakeIndex(d, 1, device))


D_ = 4
ROWS = [0.125 * i for i in range(-8, 9)]          # c0 = -1.0 .. c16 = 1.0; against c16 the score of chunk i is ROWS[i]
Q = [1.0, 0.0, 0.0, 0.0]


def _storage(tmp_path, rows, l2=False, pushdown=False, name="s"):
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


def _ids(res):
    return [r.chunk_id for r in res]


def _restated(rows, anchor, cfg, same_session=False, dead=(), keep=lambda i: True):
    """What ``search_related`` must return when ``max_results`` does not bind: every other live chunk that passes the
    threshold, the filter ``keep`` and the session rule, best score first, lower row first on ties, cut at ``top_k``."""
    cand = [(-(rows[i] * rows[anchor]), i) for i in range(len(rows))
            if i != anchor and i not in dead and keep(i) and (same_session or i % 3 != anchor % 3)
            and rows[i] * rows[anchor] >= cfg.similarity_threshold]
    return [f"c{i}" for _, i in sorted(cand)[:cfg.top_k]]


@pytest.mark.parametrize("pushdown", [False, True])
def test_session_rule_in_both_settings(tmp_path, pushdown):
    s = _storage(tmp_path, ROWS, pushdown=pushdown)
    cfg = SearchConfig()
    res = s.search_related("c16")
    assert _ids(res) == ["c15", "c14", "c12", "c11", "c9", "c8"] == _restated(ROWS, 16, cfg)     # c13 and c10 share s1
    assert [r.similarity for r in res] == [0.875, 0.75, 0.5, 0.375, 0.125, 0.0]
    assert res[0].text == "text 15" and res[0].metadata["session_id"] == "s0" and res[0].chunk.id == "c15"
    mates = s.search_related("c16", same_session=True)
    assert _ids(mates) == ["c15", "c14", "c13", "c12", "c11", "c10", "c9", "c8"] == _restated(ROWS, 16, cfg, True)
    # the index was asked by id, with the anchor excluded there; the mask exactly when pushed down
    assert s.faiss_index.calls[-1][0] == "search_by_ids" and s.faiss_index.calls[-1][2] is pushdown
    assert all(c[0] == "search_by_ids" for c in s.faiss_index.calls)
    # an anchor in the middle: a negative row turns the order round
    assert _ids(s.search_related("c0", same_session=True)) == _restated(ROWS, 0, cfg, True)[:10]
    assert _ids(s.search_related("c0"))[:3] == ["c1", "c2", "c4"]
    # the keys the reference puts into `filters` stay ignored there
    assert _ids(s.search_related("c16", filters={"related_to": "c3", "same_session": True})) == _ids(res)
    s.close()


@pytest.mark.parametrize("pushdown", [False, True])
def test_filters_and_tombstones_with_and_without_pushdown(tmp_path, pushdown):
    s = _storage(tmp_path, ROWS, pushdown=pushdown)
    assert s.delete_chunk("c15") and s.delete_chunk("c2")
    assert s.faiss_index.ntotal == len(ROWS)                            # tombstones: the rows are still in the index
    cfg = SearchConfig()
    dead = (15, 2)
    assert _ids(s.search_related("c16")) == ["c14", "c12", "c11", "c9", "c8"] == _restated(ROWS, 16, cfg, dead=dead)
    assert _ids(s.search_related("c16", filters={"has_code": True})) == ["c14", "c12", "c8"]
    assert _ids(s.search_related("c16", filters={"has_code": True}, same_session=True)) == ["c14", "c12", "c10", "c8"]
    assert _ids(s.search_related("c16", filters={"session_id": ["s0", "s1"]})) == ["c12", "c9"]   # s1 is the anchor's own
    assert _ids(s.search_related("c16", filters={"session_id": "s1"}, same_session=True)) == ["c13", "c10"]
    assert s.search_related("c16", filters={"session_id": "nobody"}) == []
    low = SearchConfig(top_k=3, similarity_threshold=-1.0)
    assert _ids(s.search_related("c16", config=low, filters={"has_code": False})) == \
        _restated(ROWS, 16, low, dead=dead, keep=lambda i: i % 2 == 1) == ["c11", "c9", "c5"]
    s.close()


def test_pushdown_returns_the_true_filtered_top_k_where_max_results_binds(tmp_path):
    cfg = SearchConfig(top_k=2, max_results=4, similarity_threshold=-1.0)
    got = {}
    for pushdown in (False, True):
        s = _storage(tmp_path, ROWS, pushdown=pushdown, name=f"p{pushdown}")
        got[pushdown] = _ids(s.search_related("c16", config=cfg, filters={"has_code": False}))
        assert s.faiss_index.calls[-1][1] == (2 if pushdown else 4)     # k: top_k pushed down, max_results otherwise
        s.close()
    assert got[True] == ["c15", "c11"]                # the filtered top 2
    assert got[False] == ["c15"]                      # the reference's over-fetch: c15 c14 c13 c12 fetched, one survives


def test_unknown_and_deleted_chunks_raise_key_error(tmp_path):
    s = _storage(tmp_path, ROWS)
    with pytest.raises(KeyError):
        s.search_related("nobody")
    assert s.delete_chunk("c5")
    with pytest.raises(KeyError):
        s.search_related("c5")
    s.close()


@pytest.mark.parametrize("pushdown", [False, True])
def test_empty_storage_and_a_storage_holding_only_the_anchor(tmp_path, pushdown):
    empty = _storage(tmp_path, [], pushdown=pushdown, name="e")
    assert empty.search_related("c0") == []
    empty.close()
    one = _storage(tmp_path, [1.0], pushdown=pushdown, name="o")
    assert one.search_related("c0") == [] and one.search_related("c0", same_session=True) == []
    assert one.faiss_index.calls == []                                  # nothing to ask the index for
    one.close()


def test_threshold(tmp_path):
    s = _storage(tmp_path, ROWS)
    assert _ids(s.search_related("c16", config=SearchConfig(similarity_threshold=0.5))) == ["c15", "c14", "c12"]
    assert _ids(s.search_related("c16", config=SearchConfig(similarity_threshold=0.5), same_session=True)) == \
        ["c15", "c14", "c13", "c12"]
    assert s.search_related("c16", config=SearchConfig(similarity_threshold=0.9)) == []
    assert len(s.search_related("c16", config=SearchConfig(similarity_threshold=-2.0, top_k=100), same_session=True)) == 16
    s.close()


def test_l2_storage_ranks_by_distance(tmp_path):
    s = _storage(tmp_path, ROWS, l2=True)
    assert s.faiss_index.metric_type == fi.METRIC_L2
    res = s.search_related("c8", config=SearchConfig(top_k=4), same_session=True)      # c8 = 0.0: distance ROWS[i]^2
    assert _ids(res) == ["c7", "c9", "c6", "c10"] and [r.similarity for r in res] == [0.015625, 0.015625, 0.0625, 0.0625]
    s.close()


@pytest.mark.parametrize("pushdown", [False, True])
def test_search_is_untouched(tmp_path, pushdown):
    """``search()`` still goes through the top-k call and returns what it returned before its result loop moved into
    the helper it now shares with ``search_related``."""
    s = _storage(tmp_path, ROWS, pushdown=pushdown)
    res = s.search(Q)
    assert _ids(res) == [f"c{i}" for i in range(16, 7, -1)]             # scores 1.0 .. 0.0, threshold 0.0, top_k 10
    assert [r.similarity for r in res] == [0.125 * i for i in range(8, -1, -1)]
    assert res[0].text == "text 16" and res[0].metadata["session_id"] == "s1" and res[0].chunk.id == "c16"
    assert s.faiss_index.calls == [("search", 17, False)]              # k' = min(max_results, ntotal); no mask without need
    assert _ids(s.search(Q, SearchConfig(top_k=3))) == ["c16", "c15", "c14"]
    assert _ids(s.search(Q, filters={"session_id": "s1"})) == ["c16", "c13", "c10"]
    assert s.faiss_index.calls[-1] == ("search", 10 if pushdown else 17, pushdown)
    assert s.delete_chunk("c15")
    assert _ids(s.search(Q, SearchConfig(similarity_threshold=0.75))) == ["c16", "c14"]
    bare = s.search(Q, SearchConfig(include_text=False, include_metadata=False, top_k=1))
    assert _ids(bare) == ["c16"] and bare[0].text is None and bare[0].metadata is None and bare[0].chunk is None
    assert all(c[0] == "search" for c in s.faiss_index.calls)
    s.close()

"""GPU, end to end: ``HybridStorage.search_late_many`` equals ``search_late`` query by query -- chunk ids and
similarity BITS -- with and without filters, on a raw token store, with ``token_codec_bits=2`` and with
``late_candidates > 0`` (where it runs the single pruned calls).  A spy counts the calls: one ``encode_queries`` and one
``search_maxsim_batch`` per ``search_late_many``.  The model and texts are those of tests/test_tokens_storage_gpu.py."""
import pytest

import test_tokens_storage_gpu as ts
from claude_semantic_search_amd import flat_index as fi
from test_tokens_storage_gpu import late  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

NCH, D_, LOW = ts.NCH, ts.D_, ts.LOW


class _QuerySpy:
    """The model as the storage sees it: query encodings counted."""
    model_name = "synthetic-late-7"

    def __init__(self, late):  # noqa: F811
        self.late, self.query_calls = late, []

    def __getattr__(self, name):
        return getattr(self.late, name)

    def encode_queries(self, texts, **kw):
        self.query_calls.append(len(texts))
        return self.late.encode_queries(texts, **kw)


def _storage(tmp_path, pushdown=False, **kw):
    from claude_semantic_search_amd import HybridStorage, StorageConfig

    return HybridStorage(StorageConfig(data_dir=str(tmp_path / "store"), embedding_dim=D_, auto_save=False, filter_pushdown=pushdown, **kw))


def _queries(texts):
    """11 queries of mixed lengths, one of them twice and one empty: more than one group, a remainder."""
    qs = [texts[3], "wave lane bank " + texts[17][:40], "fence", texts[8], "", texts[30][:25], "grid tile", texts[3],
          "rank score query dense sparse weight vocab token chunk index merge shard mask fault page sector cache", texts[39], "item7"]
    assert len(qs) == 11
    return qs


def _pairs(res):
    return [(r.chunk_id, ts._bits([r.similarity])[0]) for r in res]


def _equal_to_the_loop(st, spy, queries, cfg, filters=None):
    calls = []
    real = st.faiss_index.search_maxsim_batch
    st.faiss_index.search_maxsim_batch = lambda *a, **k: (calls.append(len(a[0])), real(*a, **k))[1]
    try:
        spy.query_calls.clear()
        many = st.search_late_many(queries, spy, cfg, filters)
        assert spy.query_calls == [len(queries)], "search_late_many must encode its queries in ONE call"
    finally:
        del st.faiss_index.search_maxsim_batch
    assert len(many) == len(queries)
    for i, q in enumerate(queries):
        one = st.search_late(q, spy, cfg, filters)
        assert _pairs(many[i]) == _pairs(one), (i, q)
    assert any(many), "every result list is empty: the case does not bind"
    return many, calls


@pytest.mark.parametrize("pushdown", [False, True])
def test_search_late_many_equals_search_late(tmp_path, late, pushdown):  # noqa: F811
    from claude_semantic_search_amd import SearchConfig, synth

    texts = ts._texts()
    emb = synth.rows(NCH + 2, D_, 9)
    spy = _QuerySpy(late)
    wide = SearchConfig(top_k=NCH, similarity_threshold=LOW, max_results=NCH)
    few = SearchConfig(top_k=5, similarity_threshold=LOW)
    queries = _queries(texts)
    with _storage(tmp_path, pushdown) as st:
        assert st.search_late_many(queries, spy) == [[] for _ in queries]                        # an empty storage
        assert st.search_late_many([], spy) == []
        st.add_chunks(ts._chunks(texts, emb))
        many, calls = _equal_to_the_loop(st, spy, queries, wide)
        assert calls == [len(queries)], "one search_maxsim_batch call for the batch"
        assert st.faiss_index.last_maxsim_passes == -(-len(queries) // fi.MAXSIM_BATCH_GROUP)
        assert many[0][0].chunk_id == "c3" and _pairs(many[0]) == _pairs(many[7]) and _pairs(many[0]) != _pairs(many[1])
        assert all(len(m) == NCH for m in many)
        _equal_to_the_loop(st, spy, queries, few)
        got, _ = _equal_to_the_loop(st, spy, queries, wide, filters={"has_code": True})
        assert all(int(r.chunk_id[1:]) % 2 == 0 for m in got for r in m) and all(len(m) == NCH // 2 for m in got)
        assert st.delete_chunk("c3") and st.delete_chunk("c20")                                  # tombstones
        got, _ = _equal_to_the_loop(st, spy, queries, wide)
        assert all(r.chunk_id not in ("c3", "c20") for m in got for r in m)
        assert st.search_late_many(queries, spy, SearchConfig(top_k=0)) == [[] for _ in queries]


@pytest.mark.parametrize("cands", [0, 12])
def test_search_late_many_on_a_compressed_store(tmp_path, late, cands):  # noqa: F811
    from claude_semantic_search_amd import SearchConfig, synth

    texts = ts._texts()
    emb = synth.rows(NCH + 2, D_, 9)
    spy = _QuerySpy(late)
    wide = SearchConfig(top_k=NCH, similarity_threshold=LOW, max_results=NCH)
    queries = _queries(texts)
    with _storage(tmp_path, token_codec_bits=2, token_codec_centroids=64, late_candidates=cands) as st:
        st.add_chunks(ts._chunks(texts, emb))
        assert st.index_tokens(late) == NCH and st.faiss_index.token_codec_bits == 2
        many, calls = _equal_to_the_loop(st, spy, queries, wide)
        assert calls == ([len(queries)] if cands == 0 else []), "late_candidates > 0 runs the single pruned calls"
        _equal_to_the_loop(st, spy, queries, SearchConfig(top_k=5, similarity_threshold=LOW), filters={"has_code": False})

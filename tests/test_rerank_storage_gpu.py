"""GPU, end to end: ``HybridStorage.search_late_reranked_many`` equals ``search_late_reranked`` query by query -- chunk
ids, late score BITS and ``rank_before`` -- on a raw token store and with ``token_codec_bits=2``, with filters, and
with tombstones, where the documented difference (a deleted row never takes a place of the pool) is asserted.  A spy
counts the calls: one ``encode_queries`` and one ``search_rerank_maxsim`` per call, no ``search`` and no ``maxsim_ids``.
The model and texts are those of tests/test_tokens_storage_gpu.py."""
import numpy as np
import pytest

import test_tokens_storage_gpu as ts
from test_tokens_batch_storage_gpu import _QuerySpy, _queries, _storage
from test_tokens_storage_gpu import late  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

NCH, D_, LOW = ts.NCH, ts.D_, ts.LOW


def _embeddings(emb, nq):
    """One dense query per text query: stored rows and fresh ones in turn."""
    from claude_semantic_search_amd import synth

    fresh = synth.rows(nq, D_, 10)
    return np.stack([emb[(7 * i) % NCH] if i % 2 == 0 else fresh[i] for i in range(nq)]).astype(np.float32)


def _unit(x):
    """Float64 unit rows: what the storage's normalisation makes of the embeddings, closely enough to rank them."""
    x = np.asarray(x, np.float64)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _triples(res):
    return [(r.result.chunk_id, ts._bits([r.score])[0], r.rank_before) for r in res]


def _many(st, spy, queries, Q, cfg, filters=None, fetch=50):
    """The call under test, with its index calls counted."""
    calls = []
    ix = st.faiss_index
    real = {name: getattr(ix, name) for name in ("search_rerank_maxsim", "search", "maxsim_ids")}
    for name, fn in real.items():
        setattr(ix, name, lambda *a, _n=name, _f=fn, **k: (calls.append(_n), _f(*a, **k))[1])
    try:
        spy.query_calls.clear()
        many = st.search_late_reranked_many(queries, Q, spy, cfg, filters, fetch=fetch)
        assert spy.query_calls == [len(queries)], "search_late_reranked_many must encode its queries in ONE call"
        assert calls == ["search_rerank_maxsim"], f"one index call for the batch, got {calls}"
    finally:
        for name in real:
            delattr(ix, name)
    assert len(many) == len(queries)
    return many


def _equal_to_the_loop(st, spy, queries, Q, cfg, filters=None, fetch=50):
    many = _many(st, spy, queries, Q, cfg, filters, fetch)
    for i, q in enumerate(queries):
        one = st.search_late_reranked(q, Q[i], spy, cfg, filters, fetch=fetch)
        assert _triples(many[i]) == _triples(one), (i, q)
        assert all(r.result.text is not None for r in many[i])
    assert any(many), "every result list is empty: the case does not bind"
    return many


@pytest.mark.parametrize("bits", [0, 2])
def test_search_late_reranked_many_equals_the_loop(tmp_path, late, bits):  # noqa: F811
    from claude_semantic_search_amd import SearchConfig, synth

    texts = ts._texts()
    emb = synth.rows(NCH + 2, D_, 9)
    spy = _QuerySpy(late)
    queries = _queries(texts)
    Q = _embeddings(emb, len(queries))
    kw = dict(token_codec_bits=2, token_codec_centroids=64) if bits else {}
    with _storage(tmp_path, pushdown=True, **kw) as st:
        assert st.search_late_reranked_many(queries, Q, spy) == [[] for _ in queries]            # an empty storage
        assert st.search_late_reranked_many([], Q[:0], spy) == []
        st.add_chunks(ts._chunks(texts, emb))
        assert st.index_tokens(late) == NCH and st.faiss_index.token_codec_bits == bits
        cfg = SearchConfig(top_k=5, similarity_threshold=LOW)
        many = _equal_to_the_loop(st, spy, queries, Q, cfg, fetch=12)                            # the pool is a part of the store
        assert all(len(m) == 5 for m in many) and any(r.rank_before >= 5 for m in many for r in m), "re-ranking changed nothing"
        assert _triples(many[0]) != _triples(many[1])
        _equal_to_the_loop(st, spy, queries, Q, SearchConfig(top_k=NCH, similarity_threshold=LOW, max_results=NCH))   # fetch above ntotal
        s0 = np.sort(_unit(emb[:NCH]) @ _unit(Q[0]))[::-1]
        thr = float((s0[6] + s0[7]) / 2)                                                         # a threshold inside the pools
        cut = _equal_to_the_loop(st, spy, queries, Q, SearchConfig(top_k=10, similarity_threshold=thr), fetch=12)
        assert len(cut[0]) == 7 and all(r.result.similarity >= thr for m in cut for r in m)
        got = _equal_to_the_loop(st, spy, queries, Q, cfg, filters={"has_code": True}, fetch=12)  # pushed down in both
        assert all(int(r.result.chunk_id[1:]) % 2 == 0 for m in got for r in m)
        assert st.search_late_reranked_many(queries, Q, spy, SearchConfig(top_k=0)) == [[] for _ in queries]


def test_tombstones_never_enter_the_pool(tmp_path, late):  # noqa: F811
    from claude_semantic_search_amd import SearchConfig, synth

    texts = ts._texts()
    emb = synth.rows(NCH + 2, D_, 9)
    spy = _QuerySpy(late)
    unit = _unit(emb[:NCH])
    far = next(j for j in range(NCH) if not np.isin(np.argsort(-(unit @ unit[j]), kind="stable")[:15], (3, 20)).any())
    queries = [texts[3], "fence", texts[far]]
    Q = np.stack([emb[3], emb[20], emb[far]]).astype(np.float32)                                 # c3 and c20 lead their pools
    cfg = SearchConfig(top_k=5, similarity_threshold=LOW, max_results=12)
    with _storage(tmp_path, pushdown=False) as st:
        st.add_chunks(ts._chunks(texts, emb))
        _equal_to_the_loop(st, spy, queries, Q, cfg, fetch=12)
        assert st.delete_chunk("c3") and st.delete_chunk("c20")
        many = _many(st, spy, queries, Q, cfg, fetch=12)
        assert all(r.result.chunk_id not in ("c3", "c20") for m in many for r in m)
        ones = [st.search_late_reranked(q, Q[i], spy, cfg, fetch=12) for i, q in enumerate(queries)]
        # the documented difference: without push-down the single call lets a deleted row take a place of its pool of 12
        # and re-ranks the live rows left; the batched call re-ranks 12 live rows.  So the single call equals the
        # batched one with a pool smaller by the deleted rows among the query's 12 best ...
        dead = [int(np.isin(np.argsort(-(unit @ _unit(Q[i])), kind="stable")[:12], (3, 20)).sum()) for i in range(3)]
        assert dead[0] >= 1 and dead[1] >= 1 and dead[2] == 0
        for i in (0, 1):
            assert _triples(ones[i]) == _triples(_many(st, spy, queries, Q, cfg, fetch=12 - dead[i])[i]), i
        # ... and a query whose pool holds no deleted row is answered alike by both
        assert _triples(ones[2]) == _triples(many[2])
    with _storage(tmp_path / "pd", pushdown=True) as st:                                         # with push-down both mask alike
        st.add_chunks(ts._chunks(texts, emb))
        assert st.delete_chunk("c3") and st.delete_chunk("c20")
        _equal_to_the_loop(st, spy, queries, Q, cfg, fetch=12)

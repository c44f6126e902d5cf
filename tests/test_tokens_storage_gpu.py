"""GPU, end to end: ``HybridStorage.index_tokens`` / ``search_late`` / ``search_late_reranked`` with a synthetic-seed
``LateInteraction`` (2 layers, hidden 384, P = 96, hash tokeniser, one word on the skiplist) over 40 chunks.  Truth is
the library's existing late-interaction path on the very texts: ``late.score`` over ``encode_documents`` of the live
texts (``css_encoder_maxsim``) for the first stage, ``search_reranked(reranker=late)`` (a text forward pass per hit)
for the re-rank stage -- both must be met in order and in score BITS, and a spy counts the forward passes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D_ = 64
NCH = 40
WORDS = ("kernel launch stream event graph wave lane bank block grid tile ring queue fence barrier cache sector "
         "page fault mask shard merge index chunk token vocab weight sparse dense query score rank").split()
LOW = -1.0e9


def _texts(n=NCH, seed=5):
    rng = np.random.default_rng(seed)
    return [" ".join(rng.choice(WORDS, size=int(rng.integers(6, 30)), replace=True)) + f" item{i} part{i * 7}" for i in range(n)]


class _Spy:
    """The model as the storage sees it: document encodings and forward passes counted."""
    model_name = "synthetic-late-7"

    def __init__(self, late):
        self.late, self.doc_calls, self.doc_texts, self.forward_docs = late, 0, 0, 0

    def __getattr__(self, name):
        return getattr(self.late, name)

    def encode_documents(self, texts, batch_size=32):
        self.doc_calls += 1
        self.doc_texts += len(texts)
        return self.late.encode_documents(texts, batch_size=batch_size)

    def predict(self, pairs, **kw):
        self.forward_docs += len(pairs)
        return self.late.predict(pairs, **kw)


def _storage(tmp_path, pushdown=False):
    from claude_semantic_search_amd import HybridStorage, StorageConfig

    return HybridStorage(StorageConfig(data_dir=str(tmp_path / "store"), embedding_dim=D_, auto_save=False, filter_pushdown=pushdown))


def _chunks(texts, emb, lo=0):
    from claude_semantic_search_amd import Chunk

    return [Chunk(f"c{lo + i}", t, {"project_name": "p", "has_code": (lo + i) % 2 == 0}, emb[lo + i]) for i, t in enumerate(texts)]


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32).tolist()


def _truth(late, query, texts, ids):
    """[(chunk id, score)] of the live texts by late.score over encode_documents, ranked by lexsort((id, -score))."""
    q_mats, _ = late.encode_queries([query])
    d_mats, keep = late.encode_documents(texts)
    scores = late.score(q_mats, d_mats, keep=keep)
    order = np.lexsort((np.asarray(ids), -scores.astype(np.float64)))
    return [(f"c{ids[i]}", scores[i]) for i in order]


@pytest.fixture(scope="module")
def late():
    from claude_semantic_search_amd.late_interaction import LateInteraction

    # (pad_id = 1: the hash tokeniser of the synthetic weights opens a text with id 0, BERT's own pad id)
    with LateInteraction(None, synthetic_seed=7, cfg_overrides={"num_layers": 2, "pad_id": 1}, projection_dim=96,
                         query_marker_id=3, document_marker_id=2, document_length=64) as li:
        li.skip_ids = frozenset({li.encoder.tokenize(["lane"])[0][1]})          # one word on the skiplist
        assert li.token_dim == 96 and int(li.cfg["hidden"]) == 384
        yield li


@pytest.mark.parametrize("pushdown", [False, True])
def test_index_tokens_search_late_save_load_and_optimize(tmp_path, late, pushdown):
    from claude_semantic_search_amd import SearchConfig, synth

    texts = _texts()
    emb = synth.rows(NCH + 2, D_, 9)
    spy = _Spy(late)
    wide = SearchConfig(top_k=NCH, similarity_threshold=LOW, max_results=NCH)
    with _storage(tmp_path, pushdown) as st:
        assert st.search_late(texts[0], spy) == [] and st.index_tokens(spy) == 0                 # an empty storage
        st.add_chunks(_chunks(texts[:30], emb))
        assert st.index_tokens(spy) == 30 and (spy.doc_calls, spy.doc_texts) == (1, 30)          # each text once
        assert st.index_tokens(spy) == 0 and spy.doc_calls == 1                                  # a second call encodes nothing
        st.add_chunks(_chunks(texts[30:], emb, lo=30))
        assert st.index_tokens(spy) == 10 and (spy.doc_calls, spy.doc_texts) == (2, 40)          # later chunks only themselves
        ix = st.faiss_index
        assert ix.token_rows == NCH and ix.token_dim == 96
        off, tok = ix.get_tokens()
        d_mats, keep = late.encode_documents(texts)
        assert any((k == 0).any() for k in keep), "the skiplist drops nothing: the case does not bind"
        for i in range(NCH):                                                                     # kept tokens only, in bits
            assert np.array_equal(tok[off[i]:off[i + 1]], d_mats[i][keep[i] != 0]), i
        # the first stage equals late.score over encode_documents, ranked by lexsort
        for query in (texts[3], "wave lane bank " + texts[17][:40], "fence"):
            res = st.search_late(query, spy, wide)
            want = _truth(late, query, texts, list(range(NCH)))
            assert [r.chunk_id for r in res] == [c for c, _ in want], query
            assert _bits([r.similarity for r in res]) == _bits([s for _, s in want]), query
        assert st.search_late(texts[3], spy, SearchConfig(top_k=5, similarity_threshold=LOW))[0].chunk_id == "c3"
        assert spy.doc_calls == 2
        # the re-rank stage equals search_reranked(reranker=late) and runs no document forward pass
        q = emb[3] + 0.5 * emb[8]
        cfg = SearchConfig(top_k=10, similarity_threshold=LOW)
        for fetch in (25, 5):
            ref = st.search_reranked(texts[8], q, spy, cfg, fetch=fetch)
            passes = spy.forward_docs
            assert passes > 0
            got = st.search_late_reranked(texts[8], q, spy, cfg, fetch=fetch)
            assert spy.forward_docs == passes and spy.doc_calls == 2, "search_late_reranked sent a text through the encoder"
            assert [(g.result.chunk_id, g.rank_before) for g in got] == [(r.result.chunk_id, r.rank_before) for r in ref]
            assert _bits([g.score for g in got]) == _bits([r.score for r in ref])
            assert [g.result.similarity for g in got] == [r.result.similarity for r in ref]
        assert [g.result.chunk_id for g in got] != [r.chunk_id for r in st.search(q, cfg)][:len(got)], "re-ranking changed nothing"
        # filters and tombstones as in search_sparse
        before = [(r.chunk_id, r.similarity) for r in st.search_late(texts[3], spy, wide)]
        res = st.search_late(texts[3], spy, wide, filters={"has_code": True})
        assert res and [r.chunk_id for r in res] == [c for c, _ in before if int(c[1:]) % 2 == 0]
        assert st.delete_chunk("c3") and st.delete_chunk("c20")
        res = st.search_late(texts[3], spy, wide)
        after_delete = [b for b in before if b[0] not in ("c3", "c20")]
        assert [(r.chunk_id, r.similarity) for r in res] == after_delete
        assert "c3" not in [g.result.chunk_id for g in st.search_late_reranked(texts[3], emb[3], spy, cfg)]
        st.save_index()
        assert st.tokens_path.exists() and spy.doc_calls == 2
        stamp = st.tokens_path.stat().st_mtime_ns
        st.save_index()                                                                          # nothing changed: no write
        assert st.tokens_path.stat().st_mtime_ns == stamp
    # load: the matrices come back from the file, no text is encoded again
    fresh = _Spy(late)
    with _storage(tmp_path, pushdown) as st:
        assert st.faiss_index.token_rows == NCH and st.faiss_index.token_dim == 96
        res = st.search_late(texts[3], fresh, wide)
        assert [(r.chunk_id, r.similarity) for r in res] == after_delete and fresh.doc_calls == 0
        new_text = "fence barrier queue ring item99 part99"
        st.add_chunks(_chunks([new_text], emb, lo=NCH))                                          # only the new row is encoded
        assert st.index_tokens(fresh) == 1 and (fresh.doc_calls, fresh.doc_texts) == (1, 1)
        assert st.search_late(new_text, fresh, SearchConfig(top_k=3, similarity_threshold=LOW))[0].chunk_id == f"c{NCH}"
        # compaction renumbers the rows; the index compacts the matrices with them and nothing is encoded again
        st.optimize()
        live = [i for i in range(NCH + 1) if i not in (3, 20)]
        assert st.faiss_index.ntotal == len(live) and st.faiss_index.token_rows == len(live) and not st.tokens_path.exists()
        res = st.search_late(texts[3], fresh, wide)
        assert fresh.doc_calls == 1
        # ... and equals a fresh storage of the live chunks
        all_texts = texts + [new_text]
        want = _truth(late, texts[3], [all_texts[i] for i in live], live)
        assert [r.chunk_id for r in res] == [c for c, _ in want] and _bits([r.similarity for r in res]) == _bits([s for _, s in want])
        off, tok = st.faiss_index.get_tokens()
        d_mats, keep = late.encode_documents([all_texts[i] for i in live])
        assert np.array_equal(tok, np.concatenate([m[k != 0] for m, k in zip(d_mats, keep)]))
        st.save_index()
        assert st.tokens_path.exists()
        path = st.tokens_path
    # a file that speaks of another number of rows is ignored: the lazy sync encodes again
    with np.load(str(path)) as z:
        parts = {name: z[name] for name in z.files}
    assert parts["offsets"].shape == (len(live) + 1,) and int(parts["rows"]) == len(live) and int(parts["P"]) == 96
    assert str(parts["model"]) == _Spy.model_name and parts["tokens"].dtype == np.uint16
    parts["offsets"] = parts["offsets"][:-1]
    np.savez(str(path), **parts)
    again = _Spy(late)
    with _storage(tmp_path, pushdown) as st:
        assert st.faiss_index.ntotal == len(live) and st.faiss_index.token_rows == 0
        res = st.search_late(texts[3], again, wide)
        assert [r.chunk_id for r in res] == [c for c, _ in want]
        assert (again.doc_calls, again.doc_texts) == (1, len(live))

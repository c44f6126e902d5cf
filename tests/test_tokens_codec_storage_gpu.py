"""GPU, end to end: ``HybridStorage`` with ``StorageConfig.token_codec_bits`` -- ``index_tokens`` trains a codec on the
first batch and stores the chunks' token matrices compressed, ``save_index`` writes codec and codes (never decoded
matrices), a fresh ``HybridStorage`` on the same directory answers ``search_late`` with the same ids and score bits
without a forward pass.  The model and texts are those of tests/test_tokens_storage_gpu.py.  Truth for the scores is
the library's existing ``late.score`` (``css_encoder_maxsim``) over the index's DECODED matrices."""
import numpy as np
import pytest

import test_tokens_storage_gpu as ts
from test_tokens_storage_gpu import late  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

NCH, D_, LOW = ts.NCH, ts.D_, ts.LOW


def _storage(tmp_path, bits, name="store"):
    from claude_semantic_search_amd import HybridStorage, StorageConfig

    return HybridStorage(StorageConfig(data_dir=str(tmp_path / name), embedding_dim=D_, auto_save=False, token_codec_bits=bits,
                                       token_codec_centroids=64))


def _decoded_truth(late, ix, query):
    """[(chunk id, score)] by late.score over the index's decoded matrices, ranked by lexsort((id, -score))."""
    off, tok = ix.get_tokens()
    live = [i for i in range(off.shape[0] - 1) if off[i + 1] > off[i]]
    q_mats, _ = late.encode_queries([query])
    scores = late.score(q_mats, [tok[off[i]:off[i + 1]] for i in live])
    order = np.lexsort((np.asarray(live), -scores.astype(np.float64)))
    return [(f"c{live[i]}", scores[i]) for i in order]


def test_compressed_token_matrices_through_index_save_and_load(tmp_path, late):  # noqa: F811
    from claude_semantic_search_amd import SearchConfig, synth
    from claude_semantic_search_amd import flat_index as fi

    texts = ts._texts()
    emb = synth.rows(NCH + 2, D_, 9)
    spy = ts._Spy(late)
    wide = SearchConfig(top_k=NCH, similarity_threshold=LOW, max_results=NCH)
    queries = (texts[3], "wave lane bank " + texts[17][:40], "fence")
    with _storage(tmp_path, 2) as st:
        st.add_chunks(ts._chunks(texts[:30], emb))
        assert st.index_tokens(spy) == 30 and spy.doc_calls == 1                                 # trains, then stores compressed
        ix = st.faiss_index
        codec = ix.get_token_codec()
        assert ix.token_codec_bits == 2 and codec.P == 96 and 2 <= codec.centroids.shape[0] <= 64
        st.add_chunks(ts._chunks(texts[30:], emb, lo=30))
        assert st.index_tokens(spy) == 10 and spy.doc_calls == 2                                 # the same codec from then on
        again = ix.get_token_codec()
        assert all(np.array_equal(a, b) for a, b in zip(codec, again)), "the codec was trained a second time"
        assert ix.token_rows == NCH and ix.token_dim == 96
        # the stored codes are those of the numpy double's residual half on the model's kept tokens
        d_mats, keep = late.encode_documents(texts)
        kept = np.concatenate([m[k != 0] for m, k in zip(d_mats, keep)])
        off, codes, res = ix.get_token_codes()
        assert off[-1] == kept.shape[0] and np.array_equal(res, fi.token_codec_encode(codec, kept, codes=codes)[1])
        assert not np.array_equal(ix.get_tokens()[1], kept), "the matrices were not compressed"
        results = {}
        for query in queries:
            got = st.search_late(query, spy, wide)
            want = _decoded_truth(late, ix, query)
            assert [r.chunk_id for r in got] == [c for c, _ in want], query
            assert ts._bits([r.similarity for r in got]) == ts._bits([s for _, s in want]), query
            results[query] = [(r.chunk_id, ts._bits([r.similarity])[0]) for r in got]
        reranked = [(g.result.chunk_id, ts._bits([g.score])[0])
                    for g in st.search_late_reranked(texts[8], emb[3] + 0.5 * emb[8], spy, SearchConfig(top_k=10, similarity_threshold=LOW), fetch=25)]
        assert len(reranked) == 10 and spy.doc_calls == 2
        st.save_index()
        path = st.tokens_path
        ntok = int(off[-1])
    # the file: the COMPRESSED form, within the derived size
    with np.load(str(path)) as z:
        names = set(z.files)
        assert {"offsets", "codes", "res", "centroids", "cutoffs", "weights", "nbits", "P", "rows", "model"} <= names
        assert "tokens" not in names, "the decoded matrices were written"
        assert z["codes"].dtype == np.uint16 and z["codes"].shape == (ntok,)
        assert z["res"].dtype == np.uint8 and z["res"].shape == (ntok, 96 * 2 // 8)
        assert int(z["nbits"]) == 2 and int(z["P"]) == 96 and int(z["rows"]) == NCH
        C = z["centroids"].shape[0]
    # 2 + P nbits / 8 bytes per token, 8 per offset, the codec (bf16 centroids, 3 cutoffs, 4 weights), and per array of
    # the archive a 128-byte .npy header plus zip's local and central entries (below 400 bytes for each of the 10)
    bound = ntok * (2 + 96 * 2 // 8) + 8 * (NCH + 1) + C * 96 * 2 + 7 * 4 + 10 * 400
    assert path.stat().st_size <= bound, (path.stat().st_size, bound)
    assert path.stat().st_size < ntok * 96 * 2 / 4, "no smaller than a quarter of the raw matrices"
    # a fresh storage on the same directory: the same ids and score bits, no forward pass
    fresh = ts._Spy(late)
    with _storage(tmp_path, 2) as st:
        assert st.faiss_index.token_rows == NCH and st.faiss_index.token_codec_bits == 2
        for query in queries:
            got = st.search_late(query, fresh, wide)
            assert [(r.chunk_id, ts._bits([r.similarity])[0]) for r in got] == results[query], query
        got = [(g.result.chunk_id, ts._bits([g.score])[0])
               for g in st.search_late_reranked(texts[8], emb[3] + 0.5 * emb[8], fresh, SearchConfig(top_k=10, similarity_threshold=LOW), fetch=25)]
        assert got == reranked
        assert fresh.doc_calls == 0 and fresh.forward_docs == 0, "a loaded storage sent a text through the encoder"
        new_text = "fence barrier queue ring item99 part99"
        st.add_chunks(ts._chunks([new_text], emb, lo=NCH))                                       # a later chunk: the loaded codec
        assert st.index_tokens(fresh) == 1 and (fresh.doc_calls, fresh.doc_texts) == (1, 1)
        assert st.faiss_index.token_codec_bits == 2 and st.faiss_index.token_rows == NCH + 1
        assert st.search_late(new_text, fresh, SearchConfig(top_k=3, similarity_threshold=LOW))[0].chunk_id == f"c{NCH}"


def test_with_bits_0_the_file_and_the_results_are_unchanged(tmp_path, late):  # noqa: F811
    from claude_semantic_search_amd import SearchConfig, synth

    texts = ts._texts()
    emb = synth.rows(NCH + 2, D_, 9)
    spy = ts._Spy(late)
    wide = SearchConfig(top_k=NCH, similarity_threshold=LOW, max_results=NCH)
    with _storage(tmp_path, 0) as st:
        st.add_chunks(ts._chunks(texts, emb))
        assert st.index_tokens(spy) == NCH and st.faiss_index.token_codec_bits == 0
        got = st.search_late(texts[3], spy, wide)
        want = ts._truth(late, texts[3], texts, list(range(NCH)))
        assert [r.chunk_id for r in got] == [c for c, _ in want]
        assert ts._bits([r.similarity for r in got]) == ts._bits([s for _, s in want])
        st.save_index()
        with np.load(str(st.tokens_path)) as z:
            assert set(z.files) == {"offsets", "tokens", "P", "rows", "model"} and z["tokens"].dtype == np.uint16
    # a file of that shape loads into an index without a codec, whatever the configuration asks of LATER encodings
    fresh = ts._Spy(late)
    with _storage(tmp_path, 2) as st:
        assert st.faiss_index.token_rows == NCH and st.faiss_index.token_codec_bits == 0
        got2 = st.search_late(texts[3], fresh, wide)
        assert [(r.chunk_id, r.similarity) for r in got2] == [(r.chunk_id, r.similarity) for r in got] and fresh.doc_calls == 0

"""GPU, end to end: ``HybridStorage.search_late`` with ``StorageConfig.late_candidates`` on an index with a token codec.
0 is the exhaustive search as before; a value of at least the chunk count gives the same ids and score bits through
``IndexFlat.search_maxsim_pruned``; a small value returns chunks from the candidate set alone, with scores that are
``maxsim_ids`` of the returned chunks in bits.  The model and texts are those of tests/test_tokens_storage_gpu.py."""
import numpy as np
import pytest

import test_tokens_storage_gpu as ts
from test_tokens_codec_storage_gpu import _decoded_truth
from test_tokens_storage_gpu import late  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

NCH, D_, LOW = ts.NCH, ts.D_, ts.LOW


def _storage(tmp_path, cands, bits=2, name="store"):
    from claude_semantic_search_amd import HybridStorage, StorageConfig

    return HybridStorage(StorageConfig(data_dir=str(tmp_path / name), embedding_dim=D_, auto_save=False, token_codec_bits=bits,
                                       token_codec_centroids=64, late_candidates=cands))


def test_late_candidates_through_search_late(tmp_path, late):  # noqa: F811
    from claude_semantic_search_amd import SearchConfig, StorageConfig, synth

    assert StorageConfig().late_candidates == 0
    texts = ts._texts()
    emb = synth.rows(NCH + 2, D_, 9)
    wide = SearchConfig(top_k=NCH, similarity_threshold=LOW, max_results=NCH)
    queries = (texts[3], "wave lane bank " + texts[17][:40], "fence")
    results = {}
    with _storage(tmp_path, 0) as st:                                           # exhaustive: the present results
        st.add_chunks(ts._chunks(texts, emb))
        assert st.index_tokens(late) == NCH and st.faiss_index.token_codec_bits == 2
        for query in queries:
            got = st.search_late(query, late, wide)
            want = _decoded_truth(late, st.faiss_index, query)
            assert [r.chunk_id for r in got] == [c for c, _ in want], query
            assert ts._bits([r.similarity for r in got]) == ts._bits([s for _, s in want]), query
            results[query] = [(r.chunk_id, ts._bits([r.similarity])[0]) for r in got]
        st.save_index()
    for cands in (NCH, 1000, 65536, 10 ** 6):                                   # every chunk a candidate: the same bytes
        with _storage(tmp_path, cands) as st:
            assert st.faiss_index.token_rows == NCH
            for query in queries:
                got = st.search_late(query, late, wide)
                assert [(r.chunk_id, ts._bits([r.similarity])[0]) for r in got] == results[query], (cands, query)
    few = SearchConfig(top_k=3, similarity_threshold=LOW)
    with _storage(tmp_path, 5) as st:                                           # five candidates, three results
        ix = st.faiss_index
        for query in queries:
            got = st.search_late(query, late, few)
            q_mat = late.encode_queries([query])[0][0]
            cand, _ = ix.maxsim_candidates(q_mat, 5)
            assert len(got) == 3 and cand.shape == (5,)
            rows = np.array([int(r.chunk_id[1:]) for r in got])
            assert set(rows.tolist()) <= set(cand.tolist()), "a result from outside the candidate set"
            assert ts._bits([r.similarity for r in got]) == ts._bits(ix.maxsim_ids(q_mat, rows)), query
            sc = ix.maxsim_ids(q_mat, cand)
            assert rows.tolist() == cand[np.lexsort((cand, -sc))][:3].tolist(), query
        got = st.search_late(queries[0], late, SearchConfig(top_k=8, similarity_threshold=LOW))   # top_k above the setting
        assert len(got) == 8
    with _storage(tmp_path, 5, bits=0, name="plain") as st:                     # no codec: the setting is not used
        st.add_chunks(ts._chunks(texts, emb))
        assert st.index_tokens(late) == NCH and st.faiss_index.token_codec_bits == 0
        got = st.search_late(texts[3], late, wide)
        want = ts._truth(late, texts[3], texts, list(range(NCH)))
        assert [r.chunk_id for r in got] == [c for c, _ in want]
        assert ts._bits([r.similarity for r in got]) == ts._bits([s for _, s in want])

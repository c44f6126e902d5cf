"""GPU, end to end: ``HybridStorage.index_sparse`` / ``search_sparse`` / ``search_hybrid_sparse`` with a synthetic-seed
``SparseEncoder`` (2 layers, hash tokeniser) over a dozen chunks.  Truth is numpy on the very vectors the encoder handed
to the storage (a wrapper records them and counts the calls); the dot products are restated in float64
(``SparseEncoder.score``) and the device value must lie within the fp32-versus-float64 summation bound
``(m + 1) 2^-24 sum_j |w_j d_j|`` of it, plus the one rounding of the restated score to float32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
D_ = 64
WORDS = ("kernel launch stream event graph wave lane bank block grid tile ring queue fence barrier cache sector "
         "page fault mask shard merge index chunk token vocab weight sparse dense query score rank").split()


def _texts():
    rng = np.random.default_rng(5)
    return [" ".join(rng.choice(WORDS, size=int(rng.integers(8, 14)), replace=False)) + f" item{i} part{i * 7}" for i in range(12)]


class _Counting:
    """The encoder as the storage sees it: the calls counted, the vectors it handed out kept."""
    model_name = "synthetic-seed-7"

    def __init__(self, enc):
        self.enc, self.doc_calls, self.doc_texts, self.vectors, self.query = enc, 0, 0, {}, None

    def encode_documents(self, texts, batch_size=32, **kw):
        out = self.enc.encode_documents(texts, batch_size=batch_size, **kw)
        self.doc_calls += 1
        self.doc_texts += len(texts)
        self.vectors.update(zip(texts, out))
        return out

    def encode_queries(self, texts, **kw):
        out = self.enc.encode_queries(texts, **kw)
        self.query = out[0]
        return out


def _storage(tmp_path, pushdown=False):
    from claude_semantic_search_amd import HybridStorage, StorageConfig

    return HybridStorage(StorageConfig(data_dir=str(tmp_path / "store"), embedding_dim=D_, auto_save=False, filter_pushdown=pushdown))


def _chunks(texts, emb, lo=0):
    from claude_semantic_search_amd import Chunk

    return [Chunk(f"c{lo + i}", t, {"project_name": "p", "has_code": (lo + i) % 2 == 0}, emb[lo + i]) for i, t in enumerate(texts)]


def _check_scores(res, enc, wrapped, texts, what):
    """Every result's similarity against the float64 dot product of the recorded vectors; returns the restated scores
    of ALL texts."""
    q = wrapped.query
    docs = [wrapped.vectors[t] for t in texts]
    ref = enc.score([q], docs).astype(np.float64)
    for r in res:
        i = int(r.chunk_id[1:])
        _, qi, di = np.intersect1d(q.terms, docs[i].terms, assume_unique=True, return_indices=True)
        mag = float(np.abs(q.weights[qi].astype(np.float64) * docs[i].weights[di].astype(np.float64)).sum())
        tol = (len(q.terms) + 1) * U * mag + U * abs(ref[i])
        err = abs(float(r.similarity) - ref[i])
        print(f"{what}: {r.chunk_id} similarity {r.similarity:.6f} restated {ref[i]:.6f} error {err:.2e} (bound {tol:.2e})")
        assert err <= tol, f"{what}: {r.chunk_id} differs from SparseEncoder.score by {err:.3e} (bound {tol:.3e})"
    return ref


@pytest.mark.parametrize("pushdown", [False, True])
def test_index_sparse_search_save_and_load(tmp_path, pushdown):
    from claude_semantic_search_amd import SearchConfig, SparseEncoder, synth

    texts = _texts()
    emb = synth.rows(13, D_, 9)
    # (pad_id = 1: the hash tokeniser of the synthetic weights opens a text with id 0, BERT's own pad id)
    with SparseEncoder(None, synthetic_seed=7, cfg_overrides={"num_layers": 2, "pad_id": 1}) as enc:
        wrapped = _Counting(enc)
        with _storage(tmp_path, pushdown) as st:
            assert st.search_sparse(texts[0], wrapped) == [] and st.index_sparse(wrapped) == 0      # an empty storage
            st.add_chunks(_chunks(texts, emb))
            assert st.index_sparse(wrapped) == 12 and (wrapped.doc_calls, wrapped.doc_texts) == (1, 12)
            assert st.index_sparse(wrapped) == 0 and wrapped.doc_calls == 1 and st.faiss_index.sparse_rows == 12
            for i, t in enumerate(texts):                                                            # a chunk's own text finds it
                res = st.search_sparse(t, wrapped, SearchConfig(top_k=5))
                ref = _check_scores(res, enc, wrapped, texts, f"own text {i}")
                assert res[0].chunk_id == f"c{i}", f"text {i}: {[r.chunk_id for r in res]}"
                order = np.lexsort((np.arange(12), -ref))
                sims = [r.similarity for r in res]
                hits = sum(1 for u in texts if np.intersect1d(wrapped.query.terms, wrapped.vectors[u].terms).size)
                assert sims == sorted(sims, reverse=True) and len(res) == min(5, hits)
                assert all(ref[int(r.chunk_id[1:])] >= ref[order[4]] - 1e-4 for r in res)
            assert wrapped.doc_calls == 1
            before = [(r.chunk_id, r.similarity) for r in st.search_sparse(texts[3], wrapped, SearchConfig(top_k=12))]
            # filters hold
            res = st.search_sparse(texts[3], wrapped, SearchConfig(top_k=12), filters={"has_code": True})
            assert res and all(int(r.chunk_id[1:]) % 2 == 0 for r in res)
            assert [r.chunk_id for r in res] == [c for c, _ in before if int(c[1:]) % 2 == 0]
            # the sparse leg of the hybrid search: fused order, raw similarities
            q = emb[3] + 0.5 * emb[8]
            hyb = st.search_hybrid_sparse(texts[5], q, wrapped, alpha=0.3, config=SearchConfig(top_k=12, similarity_threshold=-10.0))
            sp = enc.score([wrapped.query], [wrapped.vectors[t] for t in texts]).astype(np.float64)
            x = emb[:12].astype(np.float64)
            cos = (x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-8)) @ (q.astype(np.float64) / (np.linalg.norm(q) + 1e-8))
            fused = cos + float(np.float32(0.3)) * sp
            got = [int(r.chunk_id[1:]) for r in hyb]
            assert sorted(got) == list(range(12)) and np.abs(np.array([r.similarity for r in hyb]) - cos[got]).max() < 1e-5
            assert (np.diff(fused[got]) <= 1e-5).all(), "the hybrid results are not in fused order"
            print(f"hybrid: fused order {got}, plain order {np.argsort(-cos).tolist()}, sp {np.round(sp, 3).tolist()}")
            assert got != np.argsort(-cos).tolist(), "the sparse leg changed nothing"
            plain = st.search_hybrid_sparse(texts[5], q, wrapped, alpha=0.0, config=SearchConfig(top_k=12, similarity_threshold=-10.0))
            assert [r.chunk_id for r in plain] == [r.chunk_id for r in st.search(q, SearchConfig(top_k=12, similarity_threshold=-10.0))]
            with pytest.raises(ValueError, match="alpha"):
                st.search_hybrid_sparse(texts[5], q, wrapped, alpha=float("nan"))
            # a deleted chunk is never returned
            assert st.delete_chunk("c3")
            res = st.search_sparse(texts[3], wrapped, SearchConfig(top_k=12))
            assert [(r.chunk_id, r.similarity) for r in res] == [b for b in before if b[0] != "c3"]
            assert "c3" not in [r.chunk_id for r in st.search_hybrid_sparse(texts[3], emb[3], wrapped, config=SearchConfig(top_k=12, similarity_threshold=-10.0))]
            after_delete = [(r.chunk_id, r.similarity) for r in res]
            st.save_index()
            assert st.sparse_path.exists() and wrapped.doc_calls == 1
        # load: the vectors come back from the file, no text is encoded again
        fresh = _Counting(enc)
        with _storage(tmp_path, pushdown) as st:
            assert st.faiss_index.sparse_rows == 12
            res = st.search_sparse(texts[3], fresh, SearchConfig(top_k=12))
            assert [(r.chunk_id, r.similarity) for r in res] == after_delete and fresh.doc_calls == 0
            st.add_chunks(_chunks(["fence barrier queue ring item99 part99"], emb, lo=12))             # only the new row is encoded
            assert st.index_sparse(fresh) == 1 and (fresh.doc_calls, fresh.doc_texts) == (1, 1)
            assert st.search_sparse("fence barrier queue ring item99 part99", fresh, SearchConfig(top_k=3))[0].chunk_id == "c12"
            # compaction renumbers the rows; the index compacts the vectors with them and nothing is encoded again
            st.optimize()
            assert st.faiss_index.ntotal == 12 and st.faiss_index.sparse_rows == 12 and not st.sparse_path.exists()
            res = st.search_sparse(texts[3], fresh, SearchConfig(top_k=12))
            assert [(r.chunk_id, r.similarity) for r in res if r.chunk_id != "c12"] == after_delete and fresh.doc_calls == 1
            st.save_index()
            assert st.sparse_path.exists()
            path = st.sparse_path
        # a file that speaks of another number of rows is ignored: the lazy sync encodes again
        with np.load(str(path)) as z:
            parts = {name: z[name] for name in z.files}
        assert parts["offsets"].shape == (13,) and int(parts["rows"]) == 12 and str(parts["model"]) == _Counting.model_name
        parts["offsets"] = parts["offsets"][:-1]
        np.savez(str(path), **parts)
        again = _Counting(enc)
        with _storage(tmp_path, pushdown) as st:
            assert st.faiss_index.ntotal == 12 and st.faiss_index.sparse_rows == 0
            res = st.search_sparse(texts[3], again, SearchConfig(top_k=12))
            assert [r.chunk_id for r in res if r.chunk_id != "c12"] == [c for c, _ in after_delete]
            assert (again.doc_calls, again.doc_texts) == (1, 12)

"""GPU: ``HybridStorage.facets`` on the HIP index over the corpus of ``facets_fakes`` -- 240 chunks whose projects,
sessions, timestamps over sixteen months and NULLs are laid out so that every expected count is known by construction
(``facets_fakes.expected`` restates the rule without the product's bucket arithmetic).  Similarities sit at six levels
0.2 apart, so every threshold used here is either far from all of them or EXACTLY a chunk's similarity as the index
reports it (``search_range`` runs the same fp32 chain)."""
import numpy as np
import pytest

from claude_semantic_search_amd.storage import HybridStorage, SearchConfig, StorageConfig
from facets_fakes import D_, LEVELS, N, Q, as_tuples, corpus, expected

pytestmark = pytest.mark.gpu

BYS = ("project_name", "session_id", "chunk_type", "has_code", "has_tools", "day", "week", "month")


def _storage(tmp_path, pushdown=False, l2=False, n=N):
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=D_, normalize_embeddings=not l2,
                                    auto_save=False, filter_pushdown=pushdown))
    s.initialize()
    s.add_chunks(corpus(0, n))
    return s


def test_every_by_thresholds_top_and_the_inclusive_threshold(tmp_path):
    s = _storage(tmp_path)
    for by in BYS:
        for thr in (0.4, 0.0, -1.0, 0.95):
            assert as_tuples(s.facets(Q, by=by, threshold=thr)) == expected(by, thr), (by, thr)
        res = s.facets(Q, by=by, config=SearchConfig(similarity_threshold=0.6, include_text=False))
        assert as_tuples(res) == expected(by, 0.6)
        for f in res.buckets:
            assert abs(f.best.similarity - LEVELS[int(f.best.chunk_id[1:]) % 6]) < 1e-6 and f.best.text is None
    for top in (1, 3, 100):
        assert as_tuples(s.facets(Q, by="week", threshold=0.2, top=top)) == expected("week", 0.2, top=top)
    # the threshold at exactly a chunk's similarity counts that chunk (>=); the next float32 leaves its level out
    hits = s.search_range(Q, threshold=0.6)
    at = min(r.similarity for r in hits)                                          # a chunk of the 0.7 level, as reported
    assert abs(at - 0.7) < 1e-6 and len(hits) == N // 3
    assert s.facets(Q, by="has_code", threshold=at).total == N // 3
    above = float(np.nextafter(np.float32(max(r.similarity for r in hits if r.similarity < 0.8)), np.float32(1)))
    assert s.facets(Q, by="has_code", threshold=above).total == N // 6
    assert as_tuples(s.facets(Q, by="project_name", threshold=at)) == expected("project_name", 0.7)
    s.close()


@pytest.mark.parametrize("pushdown", [False, True])
def test_tombstones_filters_session_labels_and_optimize(tmp_path, pushdown):
    s = _storage(tmp_path, pushdown)
    dead = {0, 6, 7, 100, 239}
    for i in dead:
        assert s.delete_chunk(f"c{i}")
    for by in BYS:
        assert as_tuples(s.facets(Q, by=by, threshold=0.2)) == expected(by, 0.2, dead=dead), by
    # filters go into the mask with and without filter_pushdown: both storages give the restated answer
    got = s.facets(Q, by="project_name", threshold=0.2, filters={"has_code": True})
    assert as_tuples(got) == expected("project_name", 0.2, dead=dead, keep=lambda i: i % 2 == 0)
    got = s.facets(Q, by="month", threshold=0.2, filters={"chunk_type": ["code", "tool"], "project_name": "ALPH"})
    assert as_tuples(got) == expected("month", 0.2, dead=dead, keep=lambda i: i % 3 != 0 and (i // 6) % 4 == 0)
    # by="session_id" counts over the stored labels: buckets=None reaches the index, no column is uploaded
    seen = []
    real = s.faiss_index.facets
    s.faiss_index.facets = lambda q, r, **kw: (seen.append(kw), real(q, r, **kw))[1]
    assert as_tuples(s.facets(Q, by="session_id", threshold=0.2)) == expected("session_id", 0.2, dead=dead)
    assert len(seen) == 1 and seen[0]["buckets"] is None and seen[0]["nbuckets"] == 8 and seen[0]["allow"] is not None
    s.facets(Q, by="project_name", threshold=0.2)
    assert seen[1]["buckets"] is not None and seen[1]["buckets"].shape == (N,) and seen[1]["nbuckets"] == 3
    del s.faiss_index.facets
    # consistent after a compaction: rows renumbered, labels and bucket ids rebuilt
    before = {by: as_tuples(s.facets(Q, by=by, threshold=0.2)) for by in BYS}
    s.optimize()
    assert s.faiss_index.ntotal == N - len(dead)
    for by in BYS:
        assert as_tuples(s.facets(Q, by=by, threshold=0.2)) == before[by] == expected(by, 0.2, dead=dead), by
    s.close()


def test_l2_storage(tmp_path):
    s = _storage(tmp_path, l2=True)
    for by in ("project_name", "month", "session_id", "has_tools"):
        for thr in (0.7, 1.0, 5.0, 0.1):                                          # 2 - 2 cos: 0.2, 0.6, 1.0, 1.4, 1.8, 2.4
            assert as_tuples(s.facets(Q, by=by, threshold=thr)) == expected(by, thr, l2=True), (by, thr)
    res = s.facets(Q, by="has_code", threshold=0.7)
    assert res.total == N // 3 and [round(f.best.similarity, 5) for f in res.buckets] == [0.2, 0.6]
    at = max(r.similarity for r in s.search_range(Q, threshold=0.7))              # a chunk at distance 0.6, as reported
    assert s.facets(Q, by="has_code", threshold=at).total == N // 3               # distance <= threshold
    below = float(np.nextafter(np.float32(min(r.similarity for r in s.search_range(Q, threshold=0.7) if r.similarity > 0.4)),
                               np.float32(0)))
    assert s.facets(Q, by="has_code", threshold=below).total == N // 6
    s.close()

"""GPU: ``HybridStorage.search_hybrid`` on the HIP index (no test double): 300 chunks at d = 64 whose texts are drawn
from a small vocabulary; two chunks far from the query hold the word asked for, and one of them is deleted.  Against
a restatement in fp64 -- inner products (or squared distances) of the rows AS STORED with the query as the index sees
it, plus / minus ``alpha`` times the BM25 value of ``lexical.terms_of`` of the chunks' own texts with
``lexical.bm25_weights``.  The order must equal the fp64 ranking wherever neighbouring fused values differ by more than
1e-5 (fp32 sums of 64 terms round at ~1e-7, the lexical sum of a few terms at ~1e-7 of a value below 1);
``similarity`` fields are the RAW ones.  The lists are pushed once, only the tail after an add, and all again after
``optimize()``, which also takes the deleted chunk out of the statistics."""
import numpy as np
import pytest

from oracle import knn_oracle as ko

pytestmark = pytest.mark.gpu

D_ = 64
N = 300
DEAD = 17
KEYROW = 201
KEY = "hipErrorIllegalAddress"
K1, B = 1.2, 0.75


def _data():
    rng = np.random.default_rng(5)
    q = ko.synth_rows(1, D_, 61)[0]
    raw = ko.synth_rows(N + 20, D_, 62)
    for i in range(0, N, 3):                              # a third of the chunks resemble the query, at falling similarity
        raw[i] = q + (0.5 + 0.01 * i) * raw[i]
    vocab = [f"word{j}" for j in range(50)]
    texts = [" ".join(vocab[int(v)] for v in np.floor(50 * rng.random(int(rng.integers(5, 40))) ** 2)) for _ in range(N + 20)]
    texts[KEYROW] = f"launch failed: {KEY} in kernel word3"
    texts[DEAD] += f" {KEY}"                              # the deleted chunk holds the word too: it must not come back
    return ko.normalize_rows(q[None, :])[0], ko.normalize_rows(raw), texts


def _storage(tmp_path, raw, texts, l2, sharded, record):
    from claude_semantic_search_amd import flat_index as fi
    from claude_semantic_search_amd.chunk import Chunk
    from claude_semantic_search_amd.storage import HybridStorage, StorageConfig

    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=D_, auto_save=False, normalize_embeddings=not l2,
                                    sharded=sharded))
    s.initialize()
    assert isinstance(s.faiss_index, fi.IndexFlat) != sharded
    s.add_chunks([Chunk(f"c{i}", texts[i], {"project_name": "p", "has_code": i % 2 == 0}, raw[i]) for i in range(N)])
    _record(s, record)
    return s


def _record(s, record):
    """A thin recorder around the CURRENT index object's own method."""
    inner = s.faiss_index.set_terms
    if getattr(inner, "recorder", False):                 # (optimize() may keep the index object)
        return

    def recording(lists, row0=None):
        record.append((row0, len(lists)))
        return inner(lists, row0=row0)
    recording.recorder = True
    s.faiss_index.set_terms = recording


def _expect(scores, texts, rows, indexed, query, alpha, l2, top_k, keep=lambda i: True):
    """fp64 ranking of the chunks ``rows``: [(chunk number, fused value)] best first, cut at top_k + 1.  The statistics
    are those of the chunks ``indexed`` (every chunk whose list is in the index, deleted or not)."""
    from claude_semantic_search_amd.lexical import bm25_weights, terms_of

    docs = {i: terms_of(texts[i]) for i in indexed}
    avgdl = float(np.float32(sum(len(d) for d in docs.values()) / len(indexed)))
    qt = [t for t in dict.fromkeys(terms_of(query)) if any(t in d for d in docs.values())]
    w = bm25_weights([sum(t in d for d in docs.values()) for t in qt], len(indexed), k1=K1).astype(np.float64)
    k1 = float(np.float32(K1))
    fused = {}
    for i in rows:
        if not keep(i):
            continue
        K = k1 * (1.0 - B) + k1 * B * len(docs[i]) / avgdl
        lex = sum(wj * min(docs[i].count(t), 255) * (k1 + 1.0) / (min(docs[i].count(t), 255) + K) for t, wj in zip(qt, w) if t in docs[i])
        fused[i] = scores[i] - alpha * lex if l2 else scores[i] + alpha * lex
    order = sorted(fused, key=lambda i: (fused[i] if l2 else -fused[i], i))
    return [(i, fused[i]) for i in order[:top_k + 1]]


def _check(res, want, scores, what):
    """``want`` carries one rank more than ``res`` may hold, so that the last rank has both neighbours."""
    got = [int(r.chunk_id[1:]) for r in res]
    assert len(got) == len(want) - 1, what
    for pos, (g, (i, f)) in enumerate(zip(got, want)):
        near = [abs(f - want[p][1]) <= 1e-5 for p in (pos - 1, pos + 1) if 0 <= p < len(want)]
        assert g == i or any(near), f"{what}: rank {pos} is c{g}, fp64 says c{i}"
    for r in res:
        i = int(r.chunk_id[1:])
        assert abs(r.similarity - scores[i]) <= 4 * 64 * 2.0 ** -24, f"{what}: similarity of c{i} is not the raw one"


@pytest.mark.parametrize("sharded", [False, True], ids=["one_index", "facade"])
@pytest.mark.parametrize("l2", [False, True], ids=["ip", "l2"])
def test_search_hybrid_ranks_by_similarity_plus_bm25(tmp_path, l2, sharded):
    from claude_semantic_search_amd.chunk import Chunk
    from claude_semantic_search_amd.storage import SearchConfig

    q, raw, texts = _data()
    record = []
    s = _storage(tmp_path, raw, texts, l2, sharded, record)

    def stored_scores(n):
        x = s.faiss_index.reconstruct_n(0, n).astype(np.float64)            # the rows as stored
        return ((x - q.astype(np.float64)[None, :]) ** 2).sum(1) if l2 else x @ q.astype(np.float64)

    scores = stored_scores(N)
    cfg = SearchConfig(similarity_threshold=-1e30)
    alpha = 4.0 if l2 else 2.0                            # (squared distances of unit rows spread twice as wide)
    live = [i for i in range(N) if i != DEAD]
    assert not record
    # both holders of the word lead; then one is deleted: its list stays in the index, and it never comes back
    res = s.search_hybrid(KEY, q, cfg, alpha=alpha, k1=K1, b=B)
    _check(res, _expect(scores, texts, range(N), range(N), KEY, alpha, l2, 10), scores, "two holders")
    assert {r.chunk_id for r in res[:2]} == {f"c{KEYROW}", f"c{DEAD}"}
    assert record == [(0, N)]
    assert s.delete_chunk(f"c{DEAD}")
    plain = [r.chunk_id for r in s.search(q, cfg)]
    assert f"c{KEYROW}" not in plain
    res = s.search_hybrid(KEY, q, cfg, alpha=alpha, k1=K1, b=B)
    _check(res, _expect(scores, texts, live, range(N), KEY, alpha, l2, 10), scores, "keyword")
    assert res[0].chunk_id == f"c{KEYROW}" and f"c{DEAD}" not in [r.chunk_id for r in res]
    assert record == [(0, N)]
    # frequent words reorder within reach of their small weights; the lists are not pushed again
    for query in ("word3 word40 word41", "word49, WORD48; word47 word46 word45", f"{KEY} word12 unknownword"):
        res = s.search_hybrid(query, q, cfg, alpha=alpha, k1=K1, b=B)
        _check(res, _expect(scores, texts, live, range(N), query, alpha, l2, 10), scores, query)
    res = s.search_hybrid("word49 word48 word47", q, cfg, alpha=alpha, k1=K1, b=B)
    assert [r.chunk_id for r in res] != plain, "the lexical term changed nothing: the case shows nothing"
    assert record == [(0, N)]
    # top_k and a filter (not pushed down: max_results rows are fetched and filtered in rank order)
    res = s.search_hybrid("word49 word48", q, SearchConfig(top_k=4, similarity_threshold=-1e30), filters={"has_code": False},
                          alpha=alpha, k1=K1, b=B)
    _check(res, _expect(scores, texts, live, range(N), "word49 word48", alpha, l2, 4, keep=lambda i: i % 2 == 1), scores, "filter")
    # no usable term, and alpha 0: the plain search
    assert [r.chunk_id for r in s.search_hybrid("", q, cfg, alpha=alpha)] == plain
    assert [r.chunk_id for r in s.search_hybrid("unknownword", q, cfg, alpha=alpha)] == plain
    assert [r.chunk_id for r in s.search_hybrid(KEY, q, cfg, alpha=0.0)] == plain
    # an add pushes only the tail
    s.add_chunks([Chunk(f"c{i}", texts[i], {"project_name": "p", "has_code": i % 2 == 0}, raw[i]) for i in range(N, N + 20)])
    scores = stored_scores(N + 20)
    res = s.search_hybrid("word49 word48 word47", q, cfg, alpha=alpha, k1=K1, b=B)
    _check(res, _expect(scores, texts, live + list(range(N, N + 20)), range(N + 20), "word49 word48 word47", alpha, l2, 10), scores,
           "after an add")
    assert record == [(0, N), (N, 20)]
    # optimize() compacts the rows: every list is pushed again, and the deleted chunk leaves the statistics
    s.optimize()
    _record(s, record)
    assert s.faiss_index.ntotal == N + 19
    rows = live + list(range(N, N + 20))
    dense = stored_scores(N + 19)
    scores = {i: dense[p] for p, i in enumerate(rows)}
    res = s.search_hybrid(KEY, q, cfg, alpha=alpha, k1=K1, b=B)
    _check(res, _expect(scores, texts, rows, rows, KEY, alpha, l2, 10), scores, "after optimize")
    assert res[0].chunk_id == f"c{KEYROW}" and record[2:] == [(0, N + 19)]
    from claude_semantic_search_amd.lexical import terms_of

    df, ndocs, _ = s.faiss_index.term_stats(terms_of(KEY))
    assert df.tolist() == [1] and ndocs == N + 19
    s.close()

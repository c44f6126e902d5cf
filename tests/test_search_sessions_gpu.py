"""GPU: ``HybridStorage.search_sessions`` on the HIP index (no test double): 3 sessions of very unequal size (45, 8 and
1 chunks) plus 6 chunks without a session at d = 768; the big session's chunks are near-copies of the query, so
``search()`` returns ten chunks of that one session.  Against a numpy restatement -- fp64 inner products of the rows AS
STORED with the normalised query, per session the best live (and, pushed down, matching) chunk, best first.  Scores of
different chunks are >= 1e-3 apart here, so the order is compared exactly and the scores to ``knn_checks.SCORE_TOL``."""
import numpy as np
import pytest

from knn_checks import SCORE_TOL
from oracle import knn_oracle as ko

pytestmark = pytest.mark.gpu

D_ = 768
SESS = ["big"] * 45 + ["mid"] * 8 + ["one"] + [None] * 6
N = len(SESS)


def _raw():
    q = ko.synth_rows(1, D_, 41)[0]
    raw = ko.synth_rows(N, D_, 42)
    for i in range(45):                                   # the big session: near-copies at falling similarity
        raw[i] = q + (0.2 + 0.02 * i) * raw[i]
    order = np.random.default_rng(43).permutation(N)      # sessions interleaved in faiss_id order
    return q, raw[order], [SESS[i] for i in order]


def _storage(tmp_path, name, raw, sess, pushdown, sharded):
    from claude_semantic_search_amd.chunk import Chunk
    from claude_semantic_search_amd.storage import HybridStorage, StorageConfig

    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / name), embedding_dim=D_, auto_save=False,
                                    filter_pushdown=pushdown, sharded=sharded))
    s.initialize()
    chunks = []
    for i in range(N):
        md = {"project_name": "p", "has_code": i % 2 == 0}
        if sess[i] is not None:
            md["session_id"] = sess[i]
        chunks.append(Chunk(f"c{i}", f"t{i}", md, raw[i]))
    s.add_chunks(chunks[:25])                             # two adds: the labels of the second arrive as a tail
    assert len(s.search_sessions(raw[0])) > 0
    s.add_chunks(chunks[25:])
    return s


def _restated(scores, sess, top_k, live, keep=lambda i: True, host_filter=None):
    """``live``: chunk numbers still there.  ``keep``: what the index may return (pushed-down filter).  ``host_filter``:
    applied to each session's representative afterwards (filters without push-down)."""
    best = {}
    for i in live:
        if not keep(i):
            continue
        key = sess[i] if sess[i] is not None else ("own", i)
        if key not in best or (-scores[i], i) < (-scores[best[key]], best[key]):
            best[key] = i
    reps = sorted(best.values(), key=lambda i: (-scores[i], i))
    if host_filter is not None:
        reps = [i for i in reps if host_filter(i)]
    return [i for i in reps if scores[i] >= 0.0][:top_k]


def _check(res, want, scores, what):
    assert [r.chunk_id for r in res] == [f"c{i}" for i in want], what
    assert all(abs(r.similarity - scores[i]) <= SCORE_TOL for r, i in zip(res, want)), what


@pytest.mark.parametrize("sharded", [False, True], ids=["one_index", "facade"])
@pytest.mark.parametrize("pushdown", [False, True])
def test_search_sessions_returns_one_chunk_per_session(tmp_path, pushdown, sharded):
    from claude_semantic_search_amd.storage import SearchConfig

    q, raw, sess = _raw()
    s = _storage(tmp_path, "s", raw, sess, pushdown, sharded)
    x = s.faiss_index.reconstruct_n(0, N).astype(np.float64)
    scores = x @ ko.normalize_rows(q[None, :])[0].astype(np.float64)
    gaps = np.diff(np.sort(scores))
    assert gaps.min() > 1e-6
    live = list(range(N))
    before = [(r.chunk_id, r.similarity) for r in s.search(q)]
    assert {sess[int(c[1:])] for c, _ in before} == {"big"}          # what search() answers: one conversation, ten times

    want = _restated(scores, sess, 10, live)
    res = s.search_sessions(q)
    _check(res, want, scores, "plain")
    assert sess[want[0]] == "big" and len({sess[i] for i in want if sess[i]}) == len([i for i in want if sess[i]])
    assert res[0].chunk.id == res[0].chunk_id and res[0].text.startswith("t")
    _check(s.search_sessions(q, SearchConfig(top_k=3)), want[:3], scores, "top_k")
    # a filter: pushed down, the best MATCHING chunk stands for its session; otherwise groups whose best row fails go
    odd = lambda i: i % 2 == 1                                         # noqa: E731
    if pushdown:
        want_f = _restated(scores, sess, 10, live, keep=odd)
    else:
        want_f = _restated(scores, sess, 10, live, host_filter=odd)
    _check(s.search_sessions(q, filters={"has_code": False}), want_f, scores, "filter")
    # tombstones: the best chunk of the big session and the single chunk of "one" go
    dead = [want[0], sess.index("one")]
    for i in dead:
        assert s.delete_chunk(f"c{i}")
    live = [i for i in live if i not in dead]
    want_d = _restated(scores, sess, 10, live)
    res = s.search_sessions(q)
    _check(res, want_d, scores, "tombstones")
    assert not {f"c{i}" for i in dead} & {r.chunk_id for r in res} and sess[want_d[0]] == "big"
    assert "one" not in [sess[i] for i in want_d]
    # compaction renumbers the rows; the answer stays
    s.optimize()
    assert s.faiss_index.ntotal == N - 2
    _check(s.search_sessions(q), want_d, scores, "after optimize")
    if pushdown:
        _check(s.search_sessions(q, filters={"has_code": False}), _restated(scores, sess, 10, live, keep=odd), scores, "filter after optimize")
    # search() of the same storage returns what it returned before, minus the tombstone
    after = [(r.chunk_id, r.similarity) for r in s.search(q)]
    assert [c for c, _ in after][:9] == [c for c, _ in before if c != f"c{dead[0]}"]
    s.close()

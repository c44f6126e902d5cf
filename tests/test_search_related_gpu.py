"""GPU: ``HybridStorage.search_related`` on the HIP index (no test double): a storage of 40 chunks in 3 sessions at
d = 768, against a numpy restatement -- fp64 inner products of the rows AS STORED (``reconstruct_n``) with the anchor's
stored row, the anchor, its session mates (unless ``same_session``), tombstones and filtered chunks taken out, best
first.  Random 768-d rows: neighbouring scores are ~1e-2 apart, so the order is compared exactly and the scores to the
suite's 1e-3 (``knn_checks.SCORE_TOL``)."""
import numpy as np
import pytest

from knn_checks import SCORE_TOL
from oracle import knn_oracle as ko

pytestmark = pytest.mark.gpu

N, D_ = 40, 768


def _storage(tmp_path, name, raw, pushdown=False, sharded=False):
    from claude_semantic_search_amd.chunk import Chunk
    from claude_semantic_search_amd.storage import HybridStorage, StorageConfig

    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / name), embedding_dim=D_, auto_save=False,
                                    filter_pushdown=pushdown, sharded=sharded))
    s.initialize()
    s.add_chunks([Chunk(f"c{i}", f"t{i}", {"session_id": f"s{i % 3}", "project_name": "p", "has_code": i % 2 == 0}, raw[i])
                  for i in range(raw.shape[0])])
    return s


def _restated(x, anchor, top_k, thr=0.0, same_session=False, dead=(), keep=lambda i: True):
    s = x.astype(np.float64) @ x[anchor].astype(np.float64)
    cand = [i for i in range(x.shape[0]) if i != anchor and i not in dead and keep(i)
            and (same_session or i % 3 != anchor % 3) and s[i] >= thr]
    cand.sort(key=lambda i: (-s[i], i))
    return cand[:top_k], s


def _check(res, want, s, what):
    assert [r.chunk_id for r in res] == [f"c{i}" for i in want], what
    assert all(abs(r.similarity - s[i]) <= SCORE_TOL for r, i in zip(res, want)), what


@pytest.mark.parametrize("sharded", [False, True], ids=["one_index", "facade"])
@pytest.mark.parametrize("pushdown", [False, True])
def test_search_related_matches_the_numpy_restatement(tmp_path, pushdown, sharded):
    from claude_semantic_search_amd.storage import SearchConfig

    raw = ko.synth_rows(N, D_, 17)
    s = _storage(tmp_path, "s", raw, pushdown=pushdown, sharded=sharded)
    x = s.faiss_index.reconstruct_n(0, N)
    assert np.allclose(np.linalg.norm(x, axis=1), 1.0, atol=1e-5)
    wide = SearchConfig(top_k=100, similarity_threshold=-1.0)
    for anchor in (0, 17, 39):
        for same in (False, True):
            want, sc = _restated(x, anchor, 10, same_session=same)
            _check(s.search_related(f"c{anchor}", same_session=same), want, sc, f"anchor {anchor} same_session={same}")
            want, sc = _restated(x, anchor, 100, thr=-1.0, same_session=same)
            assert len(want) == (N - 1 if same else N - len(range(anchor % 3, N, 3)))
            _check(s.search_related(f"c{anchor}", config=wide, same_session=same), want, sc, f"anchor {anchor}, everything")
    res = s.search_related("c17", config=wide, same_session=True)
    assert res[0].text.startswith("t") and res[0].chunk.id == res[0].chunk_id and "c17" not in [r.chunk_id for r in res]
    # filters, a threshold inside the list, tombstones
    want, sc = _restated(x, 5, 4, thr=-1.0, keep=lambda i: i % 2 == 0)
    _check(s.search_related("c5", config=SearchConfig(top_k=4, similarity_threshold=-1.0), filters={"has_code": True}), want, sc, "filter")
    every, sc = _restated(x, 5, 100, thr=-1.0, same_session=True)
    thr = float(sc[every[6]] + sc[every[7]]) / 2
    want, _ = _restated(x, 5, 100, thr=thr, same_session=True)
    assert want == every[:7]
    _check(s.search_related("c5", config=SearchConfig(top_k=100, similarity_threshold=thr), same_session=True), want, sc, "threshold")
    dead = (every[0], every[3])
    for i in dead:
        assert s.delete_chunk(f"c{i}")
    want, sc = _restated(x, 5, 10, thr=-1.0, same_session=True, dead=dead)
    _check(s.search_related("c5", config=SearchConfig(similarity_threshold=-1.0), same_session=True), want, sc, "tombstones")
    with pytest.raises(KeyError):
        s.search_related(f"c{dead[0]}")
    with pytest.raises(KeyError):
        s.search_related("nobody")
    s.close()


def test_a_storage_holding_only_the_anchor(tmp_path):
    s = _storage(tmp_path, "one", ko.synth_rows(1, D_, 3))
    assert s.search_related("c0") == [] and s.search_related("c0", same_session=True) == []
    s.close()

"""GPU: ``HybridStorage.topics`` on the HIP index (no test double): 300 chunks of three planted subjects of unequal size
(150, 100, 50) at d = 768, chunks of two projects interleaved, with a deleted chunk and a project filter."""
import numpy as np
import pytest

from kmeans_fakes import planted

pytestmark = pytest.mark.gpu

D_ = 768
SIZES = (150, 100, 50)


def _storage(tmp_path):
    from claude_semantic_search_amd.chunk import Chunk
    from claude_semantic_search_amd.storage import HybridStorage, StorageConfig

    lab = np.random.default_rng(3).permutation(np.repeat([0, 1, 2], SIZES))
    C = planted(3, D_, 3, seed=0)[2]
    x = (C[lab] + np.random.default_rng(4).integers(-2, 3, size=(lab.shape[0], D_)) / 8.0).astype(np.float32)
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "t"), embedding_dim=D_, auto_save=False))
    s.initialize()
    s.add_chunks([Chunk(f"c{i}", f"text {i}", {"project_name": "alpha" if i % 3 else "beta", "session_id": f"s{lab[i]}"}, x[i])
                  for i in range(lab.shape[0])])
    return s, lab, x


def _seed(rows, lab):
    from claude_semantic_search_amd import flat_index as fi

    # (a start with one chunk of every subject: Lloyd's steps recover a planted partition from such a start)
    return next(sd for sd in range(64) if len(set(lab[fi.kmeans_init_ids(rows, 3, sd)].tolist())) == 3)


def test_topics_of_three_planted_subjects(tmp_path):
    from claude_semantic_search_amd.storage import Topic

    s, lab, x = _storage(tmp_path)
    n = lab.shape[0]
    xn = x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-8)
    topics = s.topics(n_topics=3, seed=_seed(np.arange(n), lab), examples=3)
    assert [t.size for t in topics] == [150, 100, 50] and all(isinstance(t, Topic) for t in topics)
    for t, subject in zip(topics, (0, 1, 2)):
        members = np.flatnonzero(lab == subject)
        assert sorted(t.chunk_ids, key=lambda c: int(c[1:])) == [f"c{i}" for i in members]
        assert t.representative is t.examples[0] and len(t.examples) == 3
        assert all(e.chunk_id in t.chunk_ids for e in t.examples)
        sims = [e.similarity for e in t.examples]
        assert sims == sorted(sims, reverse=True)
        # the similarity is the cosine to the (unit) centroid of the subject's normalised chunks
        cent = xn[members].astype(np.float64).mean(axis=0)
        cent /= np.linalg.norm(cent)
        best = np.sort(xn[members].astype(np.float64) @ cent)[::-1][:3]
        assert np.abs(np.array(sims) - best).max() <= 2.0 * D_ * 2.0 ** -24   # (fp32 dot products of unit vectors, twice)
    # a deleted chunk is in no topic
    victim = f"c{int(np.flatnonzero(lab == 0)[0])}"
    assert s.delete_chunk(victim)
    live = np.array([i for i in range(n) if f"c{i}" != victim])
    topics = s.topics(n_topics=3, seed=_seed(live, lab))
    assert [t.size for t in topics] == [149, 100, 50] and not any(victim in t.chunk_ids for t in topics)
    # a project filter clusters those chunks only
    beta = np.array([i for i in live if i % 3 == 0])
    topics = s.topics(n_topics=3, filters={"project_name": "beta"}, seed=_seed(beta, lab))
    assert sorted(c for t in topics for c in t.chunk_ids) == sorted(f"c{i}" for i in beta)
    assert [t.size for t in topics] == sorted(np.bincount(lab[beta]).tolist(), reverse=True)
    # one topic, and more topics than chunks
    assert [t.size for t in s.topics(n_topics=1)] == [299]
    few = s.topics(n_topics=40, filters={"session_id": "s2", "project_name": "beta"})
    assert sum(t.size for t in few) == int(((lab[beta] == 2)).sum()) and len(few) <= 40
    s.close()

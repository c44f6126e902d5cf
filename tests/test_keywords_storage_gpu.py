"""GPU: ``HybridStorage.keywords`` on the HIP index (no test double), one index and the one-rank facade: 200 short texts
at d = 16 drawn from a small vocabulary; the chunks of one group share two planted words.  Expected counts come from
``lexical.terms_of`` of the chunks' own texts, expected scores from Python floats; everything is compared exactly.  A
deleted chunk counts neither in the selection nor in the background, before and after ``optimize()``."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D_ = 16
N = 200
GROUP = [5, 6, 64, 65, 66, 130, 131, 190, 199]
OUTSIDE = 77          # holds one of the two words without belonging to the group
DEAD = (64, 77)


def _h(word):
    return zlib.crc32(word.encode("utf-8")) & 0xFFFFFF


def _texts():
    rng = np.random.default_rng(13)
    vocab = [f"word{j}" for j in range(40)]
    texts = [" ".join(vocab[int(v)] for v in np.floor(40 * rng.random(int(rng.integers(4, 20))) ** 2)) for _ in range(N)]
    for i in GROUP:
        texts[i] += " Occupancy wavefront, occupancy!"
    texts[OUTSIDE] += " wavefront"
    return texts


def _jlh(fg, FG, bg, BG):
    p, q = float(fg) / float(FG), float(bg) / float(BG)
    return (p - q) * (p / q)


def _expected(texts, chosen, live, n, min_count):
    """(word, term, fg, bg, score) of every qualifying term, best first: sets of terms per chunk, Python arithmetic."""
    from claude_semantic_search_amd.lexical import terms_of

    docs = {i: set(terms_of(texts[i])) for i in live}
    FG, BG = len(chosen), len(live)
    out = []
    for t in set().union(*(docs[i] for i in chosen)):
        fg, bg = sum(t in docs[i] for i in chosen), sum(t in docs[i] for i in live)
        if fg >= min_count and fg * BG > bg * FG:
            out.append((-_jlh(fg, FG, bg, BG), t, fg, bg))
    out.sort()
    return [(t, fg, bg, -s) for s, t, fg, bg in out[:n]]


def _check(kw, want, what):
    assert [(k.term, k.count, k.background_count, k.score) for k in kw] == want, what
    assert all(_h(k.word) == k.term for k in kw), what


@pytest.mark.parametrize("sharded", [False, True], ids=["one_index", "facade"])
def test_keywords_name_a_group_of_chunks(tmp_path, sharded):
    from claude_semantic_search_amd import flat_index as fi
    from claude_semantic_search_amd.chunk import Chunk
    from claude_semantic_search_amd.storage import HybridStorage, StorageConfig

    texts = _texts()
    x = np.random.default_rng(3).standard_normal((N, D_)).astype(np.float32)
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=D_, auto_save=False, normalize_embeddings=True,
                                    sharded=sharded))
    s.initialize()
    assert isinstance(s.faiss_index, fi.IndexFlat) != sharded
    s.add_chunks([Chunk(f"c{i}", texts[i], {"project_name": "even" if i % 2 == 0 else "odd"}, x[i]) for i in range(N)])
    ids = [f"c{i}" for i in GROUP]
    everyone = list(range(N))

    kw = s.keywords(chunk_ids=ids, n=10, min_count=2)
    _check(kw, _expected(texts, GROUP, everyone, 10, 2), "the group")
    assert [(k.word, k.count, k.background_count) for k in kw[:2]] == [("occupancy", 9, 9), ("wavefront", 9, 10)]
    assert kw[0].score == _jlh(9, 9, 9, N) and kw[1].score == _jlh(9, 9, 10, N)
    for n, mc in ((1, 1), (3, 1), (256, 1), (256, 5)):
        _check(s.keywords(chunk_ids=ids, n=n, min_count=mc), _expected(texts, GROUP, everyone, n, mc), f"n={n} min_count={mc}")
    # filters cut the selection, not the background
    odd = [i for i in GROUP if i % 2 == 1]
    _check(s.keywords(chunk_ids=ids, filters={"project_name": "odd"}, n=5, min_count=1), _expected(texts, odd, everyone, 5, 1), "filter")
    half = [i for i in everyone if i % 2 == 0]
    _check(s.keywords(filters={"project_name": "even"}, n=20, min_count=2), _expected(texts, half, everyone, 20, 2), "filter alone")
    assert s.keywords() == [] and s.keywords(chunk_ids=["nope"]) == []

    # deleted chunks count nowhere
    for i in DEAD:
        assert s.delete_chunk(f"c{i}")
    live = [i for i in everyone if i not in DEAD]
    group = [i for i in GROUP if i not in DEAD]
    kw = s.keywords(chunk_ids=ids, n=10, min_count=2)
    _check(kw, _expected(texts, group, live, 10, 2), "after the deletions")
    assert sorted((k.word, k.count, k.background_count) for k in kw[:2]) == [("occupancy", 8, 8), ("wavefront", 8, 8)]
    s.optimize()
    _check(s.keywords(chunk_ids=ids, n=10, min_count=2), _expected(texts, group, live, 10, 2), "after optimize")
    s.close()

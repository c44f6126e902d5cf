"""CPU: the host side of significant terms -- ``lexical.jlh`` / ``significant_from_counts`` / ``words_of_terms`` against a
float64 loop written here in plain Python, the tie and equality rules, the argument checks, and
``HybridStorage.keywords`` over the numpy double ``sigterms_fakes.FakeSigIndex``."""
import struct
import zlib

import numpy as np
import pytest

from claude_semantic_search_amd import flat_index as fi
from claude_semantic_search_amd import lexical as lx
from claude_semantic_search_amd.chunk import Chunk
from claude_semantic_search_amd.storage import HybridStorage, Keyword, StorageConfig
from lexical_fakes import FakeLexIndex, pack
from sigterms_fakes import FakeSigIndex, subset_counts


def _h(word):
    return zlib.crc32(word.encode("utf-8")) & 0xFFFFFF


def _bits(x):
    return struct.pack("<d", float(x))


def _loop(terms, fg, bg, FG, BG, m, min_count):
    """Qualify, score and order, one term at a time: Python ints for the comparison (exact), Python floats (IEEE
    float64, one rounding per operation) for the score, and a sort on ``(-score, term)``."""
    rows = []
    for t, f, b in zip(terms, fg, bg):
        t, f, b = int(t), int(f), int(b)
        if f >= min_count and f * BG > b * FG:
            p = float(f) / float(FG)
            q = float(b) / float(BG)
            rows.append((-((p - q) * (p / q)), t, f, b))
    rows.sort()
    return rows[:m]


def _same(res, rows):
    assert res.terms.dtype == np.uint32 and res.fg.dtype == np.int64 and res.bg.dtype == np.int64 and res.score.dtype == np.float64
    assert res.terms.tolist() == [r[1] for r in rows]
    assert res.fg.tolist() == [r[2] for r in rows] and res.bg.tolist() == [r[3] for r in rows]
    assert [_bits(s) for s in res.score] == [_bits(-r[0]) for r in rows]


def test_jlh_and_the_ranking_against_a_float64_loop():
    rng = np.random.default_rng(5)
    for FG, BG in ((7, 1000), (333, 1000), (1, 3), (999, 1000), (1 << 20, (1 << 31) + 12345)):
        n = 400
        terms = rng.choice(1 << 24, size=n, replace=False).astype(np.uint32)
        terms[:2] = (0, (1 << 24) - 1)
        fg = rng.integers(1, FG + 1, size=n)
        bg = np.minimum(fg + rng.integers(0, BG - FG + 1, size=n), BG)
        one = [(float(f) / float(FG) - float(b) / float(BG)) * ((float(f) / float(FG)) / (float(b) / float(BG)))
               for f, b in zip(fg.tolist(), bg.tolist())]
        assert [_bits(v) for v in lx.jlh(fg, FG, bg, BG)] == [_bits(v) for v in one]
        for m, mc in ((1, 1), (20, 2), (256, 1), (256, 50)):
            res = lx.significant_from_counts(terms, fg, bg, FG, BG, m, mc)
            _same(res, _loop(terms, fg, bg, FG, BG, m, mc))
            assert (res.n_fg, res.n_bg) == (FG, BG)


def test_ties_equality_and_short_answers():
    # equal (fg, bg) give equal scores: the smaller term first, wherever it stands in the input
    res = lx.significant_from_counts([90, 7, 50, 8], [5, 5, 5, 6], [10, 10, 10, 10], 10, 100, 3, 1)
    assert res.terms.tolist() == [8, 7, 50] and res.score[1] == res.score[2]
    # fg * BG == bg * FG is no over-representation; neither is less
    res = lx.significant_from_counts([1, 2, 3], [5, 5, 5], [50, 49, 51], 10, 100, 20, 1)
    assert res.terms.tolist() == [2]
    # products beyond 2^63 that differ only below float64's spacing are still told apart (all four factors below 2^32)
    FG, BG = 4000000007, 4294967291
    f, b = 3999909380, 4294869981
    assert 0 < b * FG - f * BG < 300 and f * BG >= 1 << 63 and float(f * BG) == float(b * FG)
    assert lx.significant_from_counts([4], [f], [b], FG, BG, 5, 1).terms.size == 0
    assert lx.significant_from_counts([4], [f], [b - 1], FG, BG, 5, 1).terms.tolist() == [4]
    # min_count, fewer than m, nothing at all, an empty selection
    res = lx.significant_from_counts([1, 2], [1, 2], [1, 2], 2, 100, 20, 2)
    assert res.terms.tolist() == [2] and res.fg.tolist() == [2]
    res = lx.significant_from_counts([], [], [], 4, 9, 20, 1)
    assert res.terms.shape == (0,) and res.score.dtype == np.float64 and (res.n_fg, res.n_bg) == (4, 9)
    res = lx.significant_from_counts([], [], [], 0, 9, 20, 1)
    assert res.terms.shape == (0,) and (res.n_fg, res.n_bg) == (0, 0)
    for bad in (dict(m=0), dict(m=257), dict(min_count=0), dict(min_count=-3)):
        args = dict(m=5, min_count=1)
        args.update(bad)
        with pytest.raises(ValueError):
            lx.significant_from_counts([1], [1], [1], 1, 2, **args)
    assert lx.MAX_SIG_TERMS == 256


def test_words_of_terms():
    texts = ["Alpha beta, gamma!", None, "beta BETA delta alpha", "epsilon"]
    got = lx.words_of_terms(texts, [_h("beta"), _h("delta"), _h("alpha"), 12345])
    assert got == {_h("beta"): "beta", _h("delta"): "delta", _h("alpha"): "alpha"}
    assert lx.words_of_terms(texts, []) == {}
    seen = []

    def lazily():
        for t in texts:
            seen.append(t)
            yield t

    assert lx.words_of_terms(lazily(), [_h("gamma")]) == {_h("gamma"): "gamma"}
    assert len(seen) <= 2                                   # the scan stops when every term has its word
    assert lx.words_of_terms(["Café cafe"], [_h("cafe")]) == {_h("cafe"): "cafe"}       # the word as terms_of hashes it


def test_the_double_counts_like_a_bincount():
    rng = np.random.default_rng(11)
    lists = [rng.integers(0, 40, size=int(rng.integers(0, 30))) for _ in range(90)]
    ix = FakeSigIndex(4)
    ix.add(np.zeros((100, 4), np.float32))
    ix.set_terms(lists)
    off, tok = lx.lists_as_csr(lists)
    poff, terms, _, _ = pack(off, tok)
    for sel in (None, rng.random(100) < 0.3, np.zeros(100, bool), np.arange(100) >= 90):
        t, f = ix.subset_terms(sel)
        wt, wf = subset_counts(poff, terms, np.ones(90, bool) if sel is None else sel[:90])
        assert t.tolist() == wt.tolist() and f.tolist() == wf.tolist()
    with pytest.raises(ValueError):
        ix.subset_terms(np.ones(99, bool))
    back = np.arange(100) % 2 == 0
    with pytest.raises(ValueError, match="row 1 "):
        ix.significant_terms(allow=np.arange(100) < 5, background=back)
    res = ix.significant_terms(allow=np.zeros(100, bool))
    assert res.terms.size == 0 and (res.n_fg, res.n_bg) == (0, 0)


# ------------------------------------------------------------------------------------------------------ keywords
D_ = 4
N = 40
GROUP = [3, 4, 10, 11, 12, 30]


def _texts():
    out = [f"chunk number {i} talks about kernels and launches" for i in range(N)]
    for i in GROUP:
        out[i] += " Wavefront occupancy"
    out[12] = "OCCUPANCY first, then the wavefront; chunk kernels"
    out[20] += " wavefront"                                  # one holder outside the group
    return out


def _use(monkeypatch, cls):
    monkeypatch.setattr(fi, "IndexFlat", cls)
    monkeypatch.setattr(fi, "IndexFlatIP", lambda d, device=0: cls(d, 0, device))
    monkeypatch.setattr(fi, "IndexFlatL2", lambda d, device=0: cls(d, 1, device))


def _storage(tmp_path, texts):
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=D_, normalize_embeddings=True, auto_save=False))
    s.initialize()
    chunks = []
    for i, text in enumerate(texts):
        e = np.zeros(D_, np.float32)
        e[i % D_] = 1.0
        chunks.append(Chunk(f"c{i}", text, {"project_name": "even" if i % 2 == 0 else "odd"}, e))
    s.add_chunks(chunks)
    return s


def test_keywords_over_the_double(tmp_path, monkeypatch):
    _use(monkeypatch, FakeSigIndex)
    s = _storage(tmp_path, _texts())
    ids = [f"c{i}" for i in GROUP]
    kw = s.keywords(chunk_ids=ids + ["no-such-chunk"], n=5, min_count=2)
    assert all(isinstance(k, Keyword) for k in kw)
    # "occupancy" is in the 6 chunks of the group only, "wavefront" in one more: both beat every common word
    assert [(k.word, k.term, k.count, k.background_count) for k in kw[:2]] == [
        ("occupancy", _h("occupancy"), 6, 6), ("wavefront", _h("wavefront"), 6, 7)]
    assert kw[0].score == (6 / 6 - 6 / 40) * ((6 / 6) / (6 / 40)) and kw[0].score > kw[1].score
    assert all(k.count >= 2 and k.count * 40 > k.background_count * 6 for k in kw)
    assert ("set_terms", 0, N) in s.faiss_index.calls                     # the lists were synced first
    # the word comes from the first selected chunk in faiss_id order that holds it, as that text's word
    # (c12's own words "first", "then", "the" are in one chunk of two and in no other: equal scores, the smallest term)
    assert s.keywords(chunk_ids=["c12", "c30"], n=1, min_count=1)[0].word == min(("first", "then", "the"), key=_h)
    assert s.keywords(chunk_ids=["c30", "c12"], n=9, min_count=2)[0].word == "OCCUPANCY".lower()
    # filters and chunk_ids intersect; the background stays the live chunks
    kw = s.keywords(chunk_ids=ids, filters={"project_name": "even"}, n=2, min_count=1)
    assert [(k.word, k.count, k.background_count) for k in kw] == [("occupancy", 4, 6), ("wavefront", 4, 7)]
    # the whole corpus against itself: nothing is over-represented; an empty or unknown selection: nothing
    assert s.keywords() == [] and s.keywords(chunk_ids=[]) == [] and s.keywords(chunk_ids=["nope"]) == []
    # a tombstoned chunk counts nowhere
    assert s.delete_chunk("c3") and s.delete_chunk("c20")
    kw = s.keywords(chunk_ids=ids, n=2, min_count=2)
    assert [(k.word, k.count, k.background_count) for k in kw] == [(w, 5, 5) for w in sorted(("occupancy", "wavefront"), key=_h)]
    assert kw[0].score == kw[1].score
    for bad in (dict(n=0), dict(n=257), dict(min_count=0)):
        with pytest.raises(ValueError):
            s.keywords(chunk_ids=ids, **bad)
    s.close()


def test_keywords_needs_an_index_that_counts(tmp_path, monkeypatch):
    _use(monkeypatch, FakeLexIndex)
    s = _storage(tmp_path, _texts())
    with pytest.raises(NotImplementedError, match="significant_terms"):
        s.keywords(chunk_ids=["c3", "c4"])
    s.close()


def test_keywords_of_an_empty_storage(tmp_path, monkeypatch):
    _use(monkeypatch, FakeSigIndex)
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=D_, auto_save=False))
    s.initialize()
    assert s.keywords() == [] and s.keywords(chunk_ids=["c1"]) == []
    s.close()

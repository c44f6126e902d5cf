"""CPU: the host side of the hybrid search -- ``lexical.terms_of`` / ``bm25_weights`` / ``lists_as_csr``,
``flat_index.hybrid_args`` and ``HybridStorage.search_hybrid`` over the numpy double ``lexical_fakes.FakeLexIndex`` (one
fp64 ranking of every allowed row).  Similarities are multiples of 1/8; the expected order is restated here in plain
Python floats from the chunks' texts."""
import math
import zlib

import numpy as np
import pytest

from claude_semantic_search_amd import flat_index as fi
from claude_semantic_search_amd import lexical as lx
from claude_semantic_search_amd.chunk import Chunk
from claude_semantic_search_amd.storage import HybridStorage, SearchConfig, StorageConfig
from lexical_fakes import FakeLexIndex, bm25_f32, bm25_f64, pack
from prior_fakes import FakePriorIndex


def _h(word):
    return zlib.crc32(word.encode("utf-8")) & 0xFFFFFF


# ------------------------------------------------------------------------------------------------------ terms_of
def test_terms_of():
    assert lx.terms_of("") == [] and lx.terms_of(None) == [] and lx.terms_of(" ... !? ") == []
    assert lx.terms_of("hipErrorIllegalAddress") == [_h("hiperrorillegaladdress")]              # lower-cased, one word
    # punctuation splits and is dropped; an underscore is punctuation; repeats stay, in text order
    assert lx.terms_of("rc = css_index_add(ix, x); css_index_add!") == [
        _h(w) for w in ("rc", "css", "index", "add", "ix", "x", "css", "index", "add")]
    assert lx.terms_of("--offload-arch=gfx950 file.hip") == [_h(w) for w in ("offload", "arch", "gfx950", "file", "hip")]
    assert lx.terms_of("Café NAÏVE cafe") == [_h("cafe"), _h("naive"), _h("cafe")]               # accents stripped
    assert lx.terms_of("検索 abc") == [_h("検"), _h("索"), _h("abc")]                             # CJK one by one
    assert lx.terms_of("a\tb\nc\x00d") == [_h("a"), _h("b"), _h("cd")]
    assert all(0 <= t < lx.TERM_SPACE for t in lx.terms_of("the quick brown fox 123 4.5"))
    assert lx.TERM_SPACE == 1 << 24 and lx.MAX_QUERY_TERMS == fi.MAX_QUERY_TERMS == 32 and fi.MAX_HYBRID_K == 128


# -------------------------------------------------------------------------------------------------- bm25_weights
def test_bm25_weights_against_the_formula():
    N, k1 = 1000, 1.2
    df = [0, 1, 10, 500, 1000]
    idf = [math.log(1.0 + (N - d + 0.5) / (d + 0.5)) for d in df]
    w = lx.bm25_weights(df, N, k1=k1, normalized=False)
    assert w.dtype == np.float32 and w.tolist() == [float(np.float32(v)) for v in idf]
    assert idf[0] > idf[1] > idf[2] > idf[3] > idf[4] > 0.0                                      # df = N is still positive
    wn = lx.bm25_weights(df, N, k1=k1, normalized=True)
    assert wn.tolist() == [float(np.float32(v / (sum(idf) * (k1 + 1.0)))) for v in idf]
    assert abs(float(wn.astype(np.float64).sum()) * (k1 + 1.0) - 1.0) < 1e-6                     # every term saturated: lex -> 1
    assert lx.bm25_weights([], N).shape == (0,)
    assert lx.bm25_weights([3], 10, k1=0.0).tolist() == [1.0]


def test_lists_as_csr_and_hybrid_args():
    off, tok = lx.lists_as_csr([[5, 1, 5], [], np.array([7])])
    assert off.tolist() == [0, 3, 3, 4] and tok.tolist() == [5, 1, 5, 7] and tok.dtype == np.uint32 and off.dtype == np.int64
    off, tok = lx.lists_as_csr((np.array([0, 2]), np.array([3, 4], np.int32)))
    assert off.tolist() == [0, 2] and tok.tolist() == [3, 4]
    assert lx.lists_as_csr([])[0].tolist() == [0]
    with pytest.raises(ValueError, match="row 1"):
        lx.lists_as_csr([[1], [2, 1 << 24]])
    with pytest.raises(ValueError):
        lx.lists_as_csr([[-1]])
    with pytest.raises(ValueError):
        lx.lists_as_csr((np.array([0, 1]), np.array([0.5])))
    t, w, k, a, k1, b, avgdl = fi.hybrid_args([3, 9], [0.5, 0.25], 10, 0.5, 1.2, 0.75, None)
    assert t.dtype == np.uint32 and w.dtype == np.float32 and (k, a, avgdl) == (10, 0.5, None)
    for bad in (dict(terms=[3, 3], weights=[1, 1]), dict(terms=[1], weights=[1, 2]), dict(terms=[1 << 24], weights=[1]),
                dict(terms=list(range(33)), weights=[0.0] * 33), dict(weights=[float("nan")]), dict(weights=[float("inf")]),
                dict(k=0), dict(k=129), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(k1=-1.0), dict(k1=float("nan")),
                dict(b=1.5), dict(b=float("inf")), dict(avgdl=0.0), dict(avgdl=float("nan")), dict(avgdl=float("inf"))):
        args = dict(terms=[3], weights=[1.0], k=5, alpha=0.5, k1=1.2, b=0.75, avgdl=10.0)
        args.update(bad)
        with pytest.raises(ValueError):
            fi.hybrid_args(**args)


def test_the_restatements_agree_and_saturate():
    off, tok = lx.lists_as_csr([[4, 4, 9], [], [9] * 300, [1, 4]])
    poff, terms, tfs, dl = pack(off, tok)
    assert poff.tolist() == [0, 2, 2, 3, 5] and terms.tolist() == [4, 9, 9, 1, 4] and tfs.tolist() == [2, 1, 255, 1, 1]
    assert dl.tolist() == [3, 0, 300, 2]
    w = lx.bm25_weights([2, 2], 4)
    a32, a64 = bm25_f32(poff, terms, tfs, dl, [4, 9], w, 1.2, 0.75, 76.25), bm25_f64(poff, terms, tfs, dl, [4, 9], w, 1.2, 0.75, 76.25)
    assert a32.dtype == np.float32 and a32[1] == 0.0 and np.allclose(a32, a64, rtol=1e-6, atol=0)
    k1 = float(np.float32(1.2))                                                  # (the constants as the call receives them)
    K = k1 * (0.25 + 0.75 * 300 / 76.25)
    assert abs(a64[2] - float(w[1]) * 255 * (k1 + 1.0) / (255 + K)) < 1e-12


# ------------------------------------------------------------------------------------------------- search_hybrid
D_ = 4
SIMS = [1.0, 0.875, 0.875, 0.75, 0.625, 0.5, 0.5, 0.375, 0.25, 0.125, 0.0, -0.125]
KEY = "hipErrorIllegalAddress"
TEXTS = [f"chunk number {i} talks about kernels and launches {'in detail ' * (i % 4)}" for i in range(12)]
TEXTS[7] = f"{KEY} kernels {KEY} launches {KEY}"
TEXTS[2] += " launches launches"
Q = [1.0, 0.0, 0.0, 0.0]


def _use(monkeypatch, cls):
    monkeypatch.setattr(fi, "IndexFlat", cls)
    monkeypatch.setattr(fi, "IndexFlatIP", lambda d, device=0: cls(d, 0, device))
    monkeypatch.setattr(fi, "IndexFlatL2", lambda d, device=0: cls(d, 1, device))


def _chunks(lo, hi, texts=TEXTS, sims=SIMS):
    out = []
    for i in range(lo, hi):
        e = np.zeros(D_, np.float32)
        e[0] = sims[i]
        out.append(Chunk(f"c{i}", texts[i], {"project_name": "proj", "has_code": i % 2 == 0}, e))
    return out


def _storage(tmp_path, pushdown=False, n=len(SIMS), texts=TEXTS, sims=SIMS):
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=D_, normalize_embeddings=True,
                                    auto_save=False, filter_pushdown=pushdown))
    s.initialize()
    if n:
        s.add_chunks(_chunks(0, n, texts, sims))
    return s


def _ids(res):
    return [r.chunk_id for r in res]


def _pushes(s):
    return [c for c in s.faiss_index.calls if c[0] == "set_terms"]


def _restated(query, cfg, alpha, dead=(), keep=lambda i: True, texts=TEXTS, sims=SIMS, k1=1.2, b=0.75, fetch=None):
    """Plain Python: BM25 of the query's words against every live chunk's words (the statistics count every chunk that
    was indexed, dead or not: its list is still in the index), the fused value, one sort; of the first ``fetch`` those
    that pass the threshold on the RAW similarity, cut at top_k."""
    docs = [lx.terms_of(t) for t in texts]
    n = len(docs)
    avgdl = float(np.float32(sum(len(d) for d in docs) / n))
    q = [t for t in dict.fromkeys(lx.terms_of(query)) if any(t in d for d in docs)]
    df = [sum(t in d for d in docs) for t in q]
    w = lx.bm25_weights(df, n, k1=k1, normalized=True).astype(np.float64) if q else []
    rows = []
    for i in range(n):
        if i in dead or not keep(i):
            continue
        K = k1 * (1.0 - b) + k1 * b * len(docs[i]) / avgdl
        lex = sum(float(wj) * min(docs[i].count(t), 255) * (k1 + 1.0) / (min(docs[i].count(t), 255) + K)
                  for t, wj in zip(q, w) if t in docs[i])
        rows.append((-(sims[i] + alpha * lex), i, sims[i]))
    rows.sort()
    rows = rows[:cfg.top_k if fetch is None else fetch]
    return [(f"c{i}", raw) for _, i, raw in rows if raw >= cfg.similarity_threshold][:cfg.top_k]


@pytest.mark.parametrize("pushdown", [False, True])
def test_a_keyword_chunk_far_away_comes_first(tmp_path, monkeypatch, pushdown):
    _use(monkeypatch, FakeLexIndex)
    s = _storage(tmp_path, pushdown)
    cfg = SearchConfig(top_k=5)
    res = s.search_hybrid(KEY, Q, cfg, alpha=1.0)
    want = _restated(KEY, cfg, 1.0)
    assert _ids(res) == [c for c, _ in want] and [r.similarity for r in res] == [v for _, v in want]
    assert _ids(res)[0] == "c7" and res[0].similarity == 0.375                  # the RAW similarity, not the fused value
    assert _ids(res)[1:] == ["c0", "c1", "c2", "c3"]
    plain = s.search_hybrid(KEY, Q, cfg, alpha=0.0)
    assert "c7" not in _ids(plain) and _ids(plain) == _ids(s.search(Q, cfg))
    assert _pushes(s) == [("set_terms", 0, 12)]                                  # one push serves every later call
    assert s.faiss_index.calls[-2] == ("search_hybrid", 5, False, (lx.terms_of(KEY)[0],))   # (the last call is search())
    # a frequent word reorders within reach of its small weight: restated, whatever it is
    for query, alpha in (("launches", 0.5), (f"launches {KEY} detail", 2.0), ("kernels, and LAUNCHES!", 0.3)):
        res = s.search_hybrid(query, Q, SearchConfig(), alpha=alpha)
        assert _ids(res) == [c for c, _ in _restated(query, SearchConfig(), alpha)], query
    # the threshold acts on S: c7's fused value does not lift it over 0.7
    got = s.search_hybrid(KEY, Q, SearchConfig(similarity_threshold=0.7), alpha=1.0)
    assert _ids(got) == [c for c, _ in _restated(KEY, SearchConfig(similarity_threshold=0.7), 1.0)] == ["c0", "c1", "c2", "c3"]
    s.close()


def test_unknown_terms_are_dropped_and_an_empty_query_is_search(tmp_path, monkeypatch):
    _use(monkeypatch, FakeLexIndex)
    s = _storage(tmp_path)
    res = s.search_hybrid(f"zzzunknown {KEY} qqqnever {KEY}", Q, SearchConfig(top_k=5), alpha=1.0)
    assert s.faiss_index.calls[-1][3] == (lx.terms_of(KEY)[0],)                  # df == 0 terms never reach the index
    assert _ids(res) == [c for c, _ in _restated(KEY, SearchConfig(top_k=5), 1.0)]
    for query in ("", "   ", "?!", "zzzunknown qqqnever"):
        res = s.search_hybrid(query, Q, alpha=1.0)
        assert s.faiss_index.calls[-1][3] == ()
        assert _ids(res) == _ids(s.search(Q)) and [r.similarity for r in res] == [r.similarity for r in s.search(Q)]
    s.close()


def test_beyond_32_terms_the_rarest_are_kept_in_first_occurrence_order(tmp_path, monkeypatch):
    _use(monkeypatch, FakeLexIndex)
    words = [f"w{j}x" for j in range(40)]
    # word j is held by chunks 0 .. j % 12: df = j % 12 + 1
    texts = [" ".join(w for j, w in enumerate(words) if i <= j % 12) + f" tail{i}" for i in range(12)]
    s = _storage(tmp_path, texts=texts)
    query = " ".join(reversed(words)) + " " + words[5]                           # a repeat changes nothing
    s.search_hybrid(query, Q, alpha=0.5)
    order = list(reversed(range(40)))                                            # first-occurrence order of the query
    rank = sorted(range(40), key=lambda p: (order[p] % 12 + 1, p))[:32]          # rarest first, ties to the earlier word
    want = tuple(lx.terms_of(words[order[p]])[0] for p in sorted(rank))
    assert s.faiss_index.calls[-1][3] == want and len(want) == 32
    res = s.search_hybrid(query, Q, alpha=0.5)
    kept_words = " ".join(words[order[p]] for p in sorted(rank))
    assert _ids(res) == [c for c, _ in _restated(kept_words, SearchConfig(), 0.5, texts=texts)]
    s.close()


def test_only_the_tail_after_adds_everything_after_compaction(tmp_path, monkeypatch):
    _use(monkeypatch, FakeLexIndex)
    s = _storage(tmp_path, n=6)
    assert not _pushes(s)                                                        # add_chunks makes no call
    s.search_hybrid(KEY, Q, alpha=1.0)
    s.add_chunks(_chunks(6, 12))
    s.search(Q)
    assert _pushes(s) == [("set_terms", 0, 6)]                                   # ... nor does search()
    res = s.search_hybrid(KEY, Q, SearchConfig(top_k=5), alpha=1.0)
    assert _pushes(s) == [("set_terms", 0, 6), ("set_terms", 6, 6)]
    assert _ids(res) == [c for c, _ in _restated(KEY, SearchConfig(top_k=5), 1.0)]
    # tombstones never come back, and are always masked
    assert s.delete_chunk("c7") and s.delete_chunk("c1")
    res = s.search_hybrid(KEY, Q, SearchConfig(top_k=5), alpha=1.0)
    assert s.faiss_index.calls[-1][:3] == ("search_hybrid", 5, True)
    assert "c7" not in _ids(res) and "c1" not in _ids(res)
    assert _ids(res) == _ids(s.search(Q, SearchConfig(top_k=5)))                 # (the only holder of the word is gone)
    res = s.search_hybrid("launches", Q, alpha=2.0)
    assert _ids(res) == [c for c, _ in _restated("launches", SearchConfig(), 2.0, dead={1, 7})]
    # compaction renumbers the rows: every list is pushed again, and the dead chunks leave the statistics
    s.optimize()
    assert s.faiss_index.ntotal == 10
    live = [i for i in range(12) if i not in (1, 7)]
    res = s.search_hybrid("launches", Q, alpha=2.0)
    assert _pushes(s)[-1] == ("set_terms", 0, 10)
    assert _ids(res) == [f"c{live[int(c[1:])]}" for c, _ in
                         _restated("launches", SearchConfig(), 2.0, texts=[TEXTS[i] for i in live], sims=[SIMS[i] for i in live])]
    s.clear_all_data()
    assert s.search_hybrid(KEY, Q) == []
    s.add_chunks(_chunks(4, 8))
    assert _ids(s.search_hybrid(KEY, Q, alpha=1.0))[0] == "c7"
    assert _pushes(s) == [("set_terms", 0, 4)]
    s.close()


def test_filters_with_and_without_pushdown(tmp_path, monkeypatch):
    _use(monkeypatch, FakeLexIndex)
    odd = {"has_code": False}
    s = _storage(tmp_path / "a", True)
    res = s.search_hybrid(KEY, Q, SearchConfig(top_k=3), filters=odd, alpha=1.0)
    assert _ids(res) == [c for c, _ in _restated(KEY, SearchConfig(top_k=3), 1.0, keep=lambda i: i % 2 == 1)] == ["c7", "c1", "c3"]
    assert s.faiss_index.calls[-1][:3] == ("search_hybrid", 3, True)             # the filter is in the mask: top_k rows
    s.close()
    s = _storage(tmp_path / "b", False)
    res = s.search_hybrid(KEY, Q, SearchConfig(top_k=3), filters=odd, alpha=1.0)
    assert _ids(res) == ["c7", "c1", "c3"]
    assert s.faiss_index.calls[-1][:3] == ("search_hybrid", 100, False)          # max(top_k, max_results) rows, in rank order
    s.search_hybrid(KEY, Q, SearchConfig(top_k=3, max_results=500), filters=odd, alpha=1.0)
    assert s.faiss_index.calls[-1][:3] == ("search_hybrid", 128, False)          # ... at most 128
    res = s.search_hybrid(KEY, Q, SearchConfig(top_k=3, max_results=2), filters=odd, alpha=1.0)
    assert s.faiss_index.calls[-1][:3] == ("search_hybrid", 3, False) and _ids(res) == ["c7", "c1"]   # of (c7, c0, c1)
    s.search_hybrid(KEY, Q, SearchConfig(top_k=3), alpha=1.0)
    assert s.faiss_index.calls[-1][:3] == ("search_hybrid", 3, False)
    s.close()


def test_argument_errors_and_an_index_without_the_method(tmp_path, monkeypatch):
    _use(monkeypatch, FakeLexIndex)
    s = _storage(tmp_path / "a")
    for a in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            s.search_hybrid(KEY, Q, alpha=a)
    assert not _pushes(s)
    assert len(s.search_hybrid(KEY, Q)) == 10                                    # the defaults
    assert s.search_hybrid(KEY, Q, SearchConfig(top_k=0)) == []
    s.close()
    _use(monkeypatch, FakePriorIndex)
    s = _storage(tmp_path / "b")
    with pytest.raises(NotImplementedError):
        s.search_hybrid(KEY, Q)
    assert _ids(s.search(Q)) == [f"c{i}" for i in range(10)]
    s.close()
    _use(monkeypatch, FakeLexIndex)
    s = _storage(tmp_path / "c", n=0)
    assert s.search_hybrid(KEY, Q) == []
    s.close()

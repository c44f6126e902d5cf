"""Host: the passage splitter, the packer and the ranking of ``best_passages`` (claude_semantic_search_amd/passages.py),
without a GPU: a fake encoder pools given token rows with numpy."""
import random
import re
import string

import numpy as np
import pytest

from claude_semantic_search_amd.passages import Passage, _WS, best_passages, pack_passages, split_passages, texts_of
from claude_semantic_search_amd.tokenizer import HashTokenizer, WordPieceTokenizer, basic_tokenize

IS_WS = re.compile(f"[{_WS}]").fullmatch


def words_of(s):          # one token per basic word (what HashTokenizer does)
    return len(basic_tokenize(s))


PROSE = ("The index is built once. It takes a while! Why does the search return nothing?  Because the\n"
         "flag --rebuild was not given, and the stale file is used.\n\n"
         "Fix: pass it. Then it works.\nlast")
CODE = ("Use this snippet to open the store and run a query against it:\n```python\nimport os\n"
        "s = store.open(path, mode='r')\nfor hit in s.search('q. a? b!', k=10):\n    print(hit.id, hit.score)\n```\n"
        "That is all there is to it. Really.")
NOPUNCT = " ".join(f"w{i}" for i in range(150))


def _check_ranges(text, ranges):
    prev = 0
    for a, b in ranges:
        assert prev <= a < b <= len(text)
        assert not IS_WS(text[a]) and not IS_WS(text[b - 1])           # the passage itself, no surrounding whitespace
        assert a == 0 or IS_WS(text[a - 1]), (a, text[a - 1])          # cuts fall only at whitespace
        assert b == len(text) or IS_WS(text[b]), (b, text[b])
        assert basic_tokenize(text[prev:a]) == []                      # nothing that holds a token is left out
        prev = b
    assert basic_tokenize(text[prev:]) == []


@pytest.mark.parametrize("text", [PROSE, CODE, NOPUNCT])
@pytest.mark.parametrize("mn,mx", [(8, 64), (1, 5), (3, 10), (20, 40)])
def test_split_offsets_whitespace_cuts_and_size_rules(text, mn, mx):
    ranges = split_passages(text, words_of, mn, mx)
    _check_ranges(text, ranges)
    counts = [words_of(text[a:b]) for a, b in ranges]
    assert sum(counts) == words_of(text)                               # every token is in exactly one passage
    longest_word = max(words_of(w) for w in text.split())
    assert max(counts) <= max(mx, longest_word), counts                # max_tokens (a single word is never cut)
    # min_tokens: a short passage is merged into its neighbour, so only pieces cut out of an over-long passage can be
    # shorter -- and those hold about total / k >= max_tokens / 2 tokens, give or take one word
    for n in counts:
        assert n >= min(mn, sum(counts)) or n >= mx // 2 - longest_word, (n, counts)


def test_split_cuts_at_sentence_ends_and_line_breaks():
    r = split_passages(PROSE, words_of, 1, 64)
    got = [PROSE[a:b] for a, b in r]
    assert got == ["The index is built once.", "It takes a while!", "Why does the search return nothing?", "Because the",
                   "flag --rebuild was not given, and the stale file is used.", "Fix: pass it.", "Then it works.", "last"]
    # merging: "last" (1 token) goes into its predecessor, short sentences into their successors
    r8 = [PROSE[a:b] for a, b in split_passages(PROSE, words_of, 8, 64)]
    assert r8[0] == "The index is built once. It takes a while!" and r8[-1].endswith("Then it works.\nlast")
    assert all(words_of(p) >= 8 for p in r8)
    # no cut after a dot that no whitespace follows
    assert [("a.b c.d e", s, e) for s, e in split_passages("a.b c.d e", words_of, 1, 64)] == [("a.b c.d e", 0, 9)]


def test_split_empty_whitespace_and_unpunctuated_text():
    assert split_passages("", words_of) == []
    assert split_passages(" \n\t  \n", words_of) == []
    assert split_passages("\x00\x01", words_of) == []                   # characters the tokenizer drops: no tokens
    r = split_passages(NOPUNCT, words_of, 8, 64)                        # 150 tokens, no punctuation: 3 pieces of 50
    assert [words_of(NOPUNCT[a:b]) for a, b in r] == [50, 50, 50]
    assert split_passages("one", words_of, 8, 64) == [(0, 3)]           # shorter than min_tokens as a whole
    assert split_passages("  one two.  ", lambda s: basic_tokenize(s)) == [(2, 10)]   # tokens_of may return the tokens


def test_split_fenced_code_block():
    r = split_passages(CODE, words_of, 8, 64)
    _check_ranges(CODE, r)
    got = [CODE[a:b] for a, b in r]
    assert any("```python" in p for p in got) and "q. a? b!" in CODE
    assert all(words_of(p) >= 8 for p in got)
    # the fence lines are short: they are merged with code lines, never dropped
    assert sum(p.count("```") for p in got) == 2


def test_split_argument_errors():
    with pytest.raises(ValueError, match="min_tokens"):
        split_passages("a b", words_of, 0, 5)
    with pytest.raises(ValueError, match="min_tokens"):
        split_passages("a b", words_of, 9, 8)
    with pytest.raises(TypeError):
        split_passages(None, words_of)


# ---- tokenisation: the concatenated passage tokens are the tokens of the whole text

def _vocab(tmp_path, rng):
    # the synthetic vocabulary of tests/test_tokenizer.py
    words = ["".join(rng.choice(string.ascii_lowercase) for _ in range(rng.randint(1, 8))) for _ in range(800)]
    pieces = ["<s>", "<pad>", "</s>", "<unk>", "[UNK]", "<mask>"] + sorted(set(words))
    pieces += ["##" + "".join(rng.choice(string.ascii_lowercase) for _ in range(rng.randint(1, 3))) for _ in range(600)]
    pieces += list(string.punctuation) + list(string.digits) + ["##" + d for d in string.digits]
    pieces += ["é", "中", "##中", "ü", "naive", "cafe", "…", "“", "ss", "i"]
    pieces = list(dict.fromkeys(pieces))
    p = tmp_path / "vocab.txt"
    p.write_text("\n".join(pieces) + "\n", encoding="utf-8")
    return str(p), words


def _text(rng, words):
    parts = []
    for _ in range(rng.randint(1, 120)):
        r = rng.random()
        w = rng.choice(words)
        if r < 0.55:
            parts.append(w)
        elif r < 0.75:
            parts.append(w + rng.choice(".!?"))
        elif r < 0.8:
            parts.append(rng.choice(["caf\u00e9", "na\u00efve", "\u4e2d\u6587\u5b57", "a\u4e2db", "x\u200by", "a\x0bb", "q.\x1cr",
                                     "v1.2.3", "e.g.", "x" * 120, "\x00nul", "\u2026", "tab\there", "end.\x85next"]))
        elif r < 0.9:
            parts.append(rng.choice(string.punctuation) + w)
        else:
            parts.append(w.upper() + str(rng.randint(0, 999)))
    seps = [" ", " ", "  ", "\n", "\n\n", " \n", "\t", "\r\n", "\u00a0", "\u2003", "\u2028", "\u3000 "]
    return "".join(p + rng.choice(seps) for p in parts)


def test_concatenated_passage_tokens_equal_the_tokens_of_the_whole_text(tmp_path):
    rng = random.Random(3)
    vocab_path, words = _vocab(tmp_path, rng)
    toks = [WordPieceTokenizer(vocab_path), HashTokenizer(5000)]
    try:
        from claude_semantic_search_amd.tokenizer import NativeWordPieceTokenizer

        toks.append(NativeWordPieceTokenizer(vocab_path))               # the C++ tokenizer, where the library loads
    except Exception:
        pass
    texts = [_text(rng, words) for _ in range(120)] + [PROSE, CODE, NOPUNCT]
    for tk in toks:
        body = lambda s: [int(t) for t in tk.encode(s, 100000)][1:-1]   # noqa: E731
        for text in texts:
            for mn, mx in ((8, 64), (1, 3)):
                ranges = split_passages(text, lambda s: len(body(s)), mn, mx)
                _check_ranges(text, ranges)
                cat = [t for a, b in ranges for t in body(text[a:b])]
                assert cat == body(text), (type(tk).__name__, text)


def test_whitespace_class_is_the_tokenizers():
    import re
    import sys
    import unicodedata

    mine = re.compile(f"[{_WS}]")
    for cp in range(sys.maxunicode + 1):
        ch = chr(cp)
        # basic_tokenize: tab / LF / CR and Zs become a space; of the rest, what is not dropped and isspace() splits
        tok_ws = ch in "\t\n\r " or unicodedata.category(ch) == "Zs" or (
            not unicodedata.category(ch).startswith("C") and cp not in (0, 0xFFFD) and ch.isspace())
        assert bool(mine.match(ch)) == tok_ws, hex(cp)


# ---- pack_passages

def test_pack_covers_every_passage_once_and_spills():
    rng = random.Random(5)
    lists = [[rng.randint(4, 999) for _ in range(rng.randint(1, 30))] for _ in range(40)]
    for L in (34, 64, 384):
        seqs, spans = pack_passages(lists, L, bos=0, eos=2)
        assert len(spans) == len(lists) and all(3 <= len(s) <= L for s in seqs)
        assert all(s[0] == 0 and s[-1] == 2 for s in seqs)
        for toks, (si, b, e) in zip(lists, spans):
            assert 1 <= b < e <= len(seqs[si]) - 1                     # relative to the sequence, specials excluded
            assert seqs[si][b:e] == toks
        # exactly once, in order: the bodies are the concatenation of the passages
        assert [t for s in seqs for t in s[1:-1]] == [t for toks in lists for t in toks]
        assert [si for si, _, _ in spans] == sorted(si for si, _, _ in spans)
    total = sum(map(len, lists))
    seqs, spans = pack_passages(lists, 64)
    assert total > 62 and len(seqs) >= 2 and spans[-1][0] == len(seqs) - 1      # a long text spills over
    # greedy: a passage moves on only when it does not fit
    for (s0, _, e0), (s1, b1, e1) in zip(spans, spans[1:]):
        if s1 != s0:
            assert e0 - 1 + (e1 - b1) > 62
    one, sp = pack_passages([[5] * 10], 64, bos=101, eos=102)
    assert one == [[101] + [5] * 10 + [102]] and sp == [(0, 1, 11)]
    long_, sp = pack_passages([[7] * 100, [8]], 34)                       # a passage longer than a sequence is truncated
    assert long_ == [[0] + [7] * 32 + [2], [0, 8, 2]] and sp == [(0, 1, 33), (1, 1, 2)]
    assert pack_passages([], 64) == ([], [])


def test_pack_argument_errors():
    with pytest.raises(ValueError, match="max_seq_len"):
        pack_passages([[5]], 2)
    with pytest.raises(ValueError, match="passage 1 has no tokens"):
        pack_passages([[5], []], 64)


# ---- best_passages over a fake encoder

class FakeEncoder:
    """Token id t has the row E[t]; a span vector is the numpy mean of its rows (normalised on request)."""

    def __init__(self, vocab=997, hidden=16, max_seq_length=64):
        self.E = np.random.default_rng(0).standard_normal((vocab, hidden)).astype(np.float32)
        self.tk = HashTokenizer(vocab)
        self.max_seq_length = max_seq_length
        self.calls = []

    def tokenize(self, texts):
        return [self.tk.encode(t, self.max_seq_length) for t in texts]

    def get_sentence_embedding_dimension(self):
        return self.E.shape[1]

    def encode(self, text, **kw):
        v = self.E[self.tk.encode(text, self.max_seq_length)].mean(0)
        return v / np.linalg.norm(v)

    def encode_spans_ids(self, batch, spans, normalize=True, query=None, span_rows=True):
        self.calls.append((batch, list(spans)))
        rows = np.stack([self.E[np.asarray(batch[s][b:e])].mean(0) for s, b, e in spans])
        if normalize:
            rows = rows / np.linalg.norm(rows, axis=1, keepdims=True)
        seq = np.stack([self.E[np.asarray(s)].mean(0) for s in batch])
        return seq, (rows if span_rows else None), (rows @ query if query is not None else None)

    def best_passages(self, qv, texts, n=1):
        return best_passages(self, qv, texts, n=n)


TEXTS = ["alpha beta gamma delta epsilon zeta eta theta. iota kappa lambda mu nu xi omicron pi rho.\n"
         "sigma tau upsilon phi chi psi omega one two three.",
         "",
         "red green blue cyan magenta yellow black white. red green blue cyan magenta yellow black white.",
         " ".join(f"tok{i}" for i in range(200)) + "."]


def test_best_passages_ordering_ties_and_large_n():
    enc = FakeEncoder()
    q = enc.E[enc.tk.encode("iota kappa lambda mu nu xi omicron pi rho.", 64)[1:-1]].mean(0)   # that passage's own vector
    q /= np.linalg.norm(q)
    res = best_passages(enc, q, TEXTS, n=1)
    assert len(enc.calls) == 1                                           # all texts in one encoder call
    assert [len(r) for r in res] == [1, 0, 1, 1]
    assert res[0][0].text == "iota kappa lambda mu nu xi omicron pi rho." and res[0][0].score > 0.999
    assert TEXTS[0][res[0][0].start:res[0][0].end] == res[0][0].text
    # ties by position: two identical passages have equal scores, the first one wins
    assert res[2][0].start == 0 and isinstance(res[2][0], Passage)
    full = best_passages(enc, q, TEXTS, n=50)                            # n larger than the number of passages
    assert [len(r) for r in full] == [3, 0, 2, 4]
    for r in full:
        assert [p.score for p in r] == sorted((p.score for p in r), reverse=True)
    assert full[2][0].score == full[2][1].score and full[2][0].start < full[2][1].start
    # a text longer than a sequence spills: its passages are spread over several sequences, all covered
    batch, spans = enc.calls[-1]
    assert max(len(s) for s in batch) <= enc.max_seq_length and len(batch) > 3
    got = sorted(p.start for p in full[3])
    assert got == [a for a, _ in split_passages(TEXTS[3], words_of)]
    # scores are those of the spans the packer made
    ranges = split_passages(TEXTS[0], words_of)
    want = []
    for a, b in ranges:
        v = enc.E[enc.tk.encode(TEXTS[0][a:b], 64)[1:-1]].mean(0)
        want.append(float(v @ q / np.linalg.norm(v)))
    assert np.allclose(sorted(want, reverse=True), [p.score for p in full[0]], atol=1e-6)


def test_best_passages_through_the_generator_with_search_results():
    from claude_semantic_search_amd.chunk import Chunk
    from claude_semantic_search_amd.embeddings import EmbeddingConfig, EmbeddingGenerator
    from claude_semantic_search_amd.storage import SearchResult

    gen = EmbeddingGenerator(EmbeddingConfig(show_progress=False))
    gen.model = FakeEncoder()
    results = [SearchResult("a", 0.9, text=TEXTS[0]),
               SearchResult("b", 0.8, chunk=Chunk(id="b", text=TEXTS[2], metadata={})), TEXTS[3]]
    by_text = gen.best_passages("iota kappa lambda mu nu xi omicron pi rho.", results, n=2)     # a string: encoded once
    assert [len(r) for r in by_text] == [2, 2, 2] and by_text[0][0].text.startswith("iota kappa")
    qv = gen.model.encode("iota kappa lambda mu nu xi omicron pi rho.")
    by_vec = gen.best_passages(qv, [TEXTS[0], TEXTS[2], TEXTS[3]], n=2)                          # ... or a vector
    assert by_vec == by_text
    assert texts_of(results) == [TEXTS[0], TEXTS[2], TEXTS[3]]
    with pytest.raises(ValueError, match="carries no text"):
        gen.best_passages(qv, [SearchResult("c", 0.1)])


def test_best_passages_argument_errors():
    enc = FakeEncoder()
    q = np.ones(16, np.float32)
    with pytest.raises(ValueError, match="n must be"):
        best_passages(enc, q, TEXTS, n=0)
    with pytest.raises(TypeError, match="sequence of str"):
        best_passages(enc, q, "one text")
    with pytest.raises(ValueError, match="min_tokens"):
        best_passages(enc, q, TEXTS, min_tokens=5, max_tokens=2)
    assert best_passages(enc, q, []) == [] and best_passages(enc, q, ["", "  "]) == [[], []]

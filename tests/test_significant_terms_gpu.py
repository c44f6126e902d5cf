"""GPU: ``IndexFlat.subset_terms`` / ``significant_terms`` (``css_index_subset_terms``, ``css_index_significant_terms``;
kernels ``k_sig_count``, ``k_sig_nz_count`` / ``k_sig_nz_scan`` / ``k_sig_compact``, ``k_sig_score``, ``k_sig_hist`` /
``k_sig_pick`` / ``k_sig_gather`` / ``k_sig_final``).

Everything the device returns is an integer or a float64 formed by four correctly rounded operations, so every check is
BYTE equality.  Truth is numpy: the counts are one ``bincount`` over the stored form of ``lexical_fakes.pack`` of the
very tokens handed to the index (``sigterms_fakes.subset_counts``), the ranking is ``lexical.significant_from_counts`` on
those numpy counts; the code under test is never its own reference.

The corpus (built once): 3000 rows of d = 16, T = 2891 = 7 * 7 * 59 of them with lists (no multiple of 64, not ntotal),
about 5000 term ids spread over [0, 2^24) with 0 and 2^24 - 1 among the frequent ones, drawn Zipf-like, 0..200 tokens a
row, empty rows, one row of 400 distinct terms (more than one 256-entry turn of a wave's walk), terms repeated more than
255 times in a row -- one of them 2^24 - 1, whose stored entry is 0xFFFFFFFF -- and the planted terms of the ranking
cases."""
import ctypes
import functools

import numpy as np
import pytest

from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd.flat_index import IndexFlatIP, pack_allow_bits
from claude_semantic_search_amd.lexical import bm25_weights, lists_as_csr, significant_from_counts
from lexical_fakes import pack
from sigterms_fakes import subset_counts

pytestmark = pytest.mark.gpu

D_ = 16
N = 3000
T = 2891
TOP = (1 << 24) - 1
# planted terms (kept out of the drawn vocabulary)
MEAN = [5_000_001, 77, 9_000_009, 16_000_000, 1234]     # in the rows of SEL_MEAN and in two others
TIES = [3_000_003, 3_000_001, 3_000_002, 12_345_678]     # identical (fg, bg): equal scores, ordered by term
EQ7 = 4_000_004                                            # fg = 1 of FG = 413, bg = 7 of BG = 2891: 1 * 2891 == 7 * 413
EQ4 = 4_000_005                                            # fg = 4 of FG = 500, bg = 16 of BG = 2000 under the mask
PLANTED = MEAN + TIES + [EQ7, EQ4]


def _x(n, seed=3):
    return np.random.default_rng(seed).standard_normal((n, D_)).astype(np.float32)


@functools.lru_cache(maxsize=1)
def _rows():
    """The raw token lists of the T leading rows."""
    rng = np.random.default_rng(7)
    vocab = np.setdiff1d(np.unique(rng.integers(0, 1 << 24, size=5000)), PLANTED + [0, TOP])
    rng.shuffle(vocab)
    vocab = np.concatenate([vocab[:3], [0], vocab[3:40], [TOP], vocab[40:]])       # ranks 3 and 41 of the Zipf draw
    rows = []
    for r in range(T):
        idx = np.floor(vocab.shape[0] * rng.random(int(rng.integers(0, 201))) ** 3).astype(np.int64)
        rows.append(vocab[idx])
    for r in (0, 100, 639, 704, T - 2):
        rows[r] = rows[r][:0]                                                        # empty rows
    rows[5] = vocab[100:500].copy()                                                  # 400 distinct terms
    rows[77] = np.concatenate([rows[77], np.full(300, vocab[2]), np.full(256, TOP)])   # saturated counts
    rows[T - 1] = np.concatenate([rows[T - 1], np.full(260, 0)])
    sel_mean = _sel_mean()
    for r in np.flatnonzero(sel_mean)[:T]:
        rows[r] = np.concatenate([rows[r], MEAN])
    for r in (1, 2):
        rows[r] = np.concatenate([rows[r], MEAN])                                    # "almost nowhere else"
    for r in (7, 14, 21, 22, 23, 2000, 2500):                                        # 3 of r % 7 == 0, 4 others
        rows[r] = np.concatenate([rows[r], TIES])
    for r in (28, 29, 30, 31, 32, 33, 34):                                           # one of r % 7 == 0
        rows[r] = np.concatenate([rows[r], [EQ7]])
    for r in (40, 44, 48, 52) + tuple(range(1001, 1048, 4)):                         # 4 of r % 4 == 0 below 2000, 12 others
        rows[r] = np.concatenate([rows[r], [EQ4, EQ4]])
    return rows


def _sel_mean():
    sel = np.zeros(N, bool)
    sel[np.random.default_rng(19).choice(np.arange(3, T), size=150, replace=False)] = True
    return sel


@functools.lru_cache(maxsize=1)
def _packed():
    off, tok = lists_as_csr(_rows())
    poff, terms, tfs, dl = pack(off, tok)
    assert (np.diff(poff) > 256).any() and (tfs == 255).any() and (terms[tfs == 255] == TOP).any()
    return off, tok, poff, terms


@functools.lru_cache(maxsize=1)
def _index():
    off, tok, _, _ = _packed()
    ix = IndexFlatIP(D_)
    ix.add(_x(N))
    ix.set_terms((off, tok))
    return ix


def _mask(rows, n=N):
    m = np.zeros(n, bool)
    m[list(rows)] = True
    return m


def _counts(sel, poff=None, terms=None):
    """numpy: (terms, fg, FG) of a boolean selection over the N rows."""
    if poff is None:
        _, _, poff, terms = _packed()
    nl = poff.shape[0] - 1
    s = np.ones(nl, bool) if sel is None else np.asarray(sel, bool)[:nl]
    t, f = subset_counts(poff, terms, s)
    return t, f, int(s.sum())


def _rank(sel, back, m, mc):
    t, f, FG = _counts(sel)
    bt, bc, BG = _counts(back)
    return significant_from_counts(t, f, bc[np.searchsorted(bt, t)], FG, BG, m, mc)


def _raw(res):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (res.terms, res.fg, res.bg, res.score, np.array([res.n_fg, res.n_bg])))


def _same_rank(got, want, what):
    assert got.terms.dtype == np.uint32 and got.fg.dtype == np.int64 and got.bg.dtype == np.int64 and got.score.dtype == np.float64, what
    assert got.terms.tobytes() == want.terms.tobytes(), f"{what}: terms {got.terms[:8]} vs {want.terms[:8]}"
    assert got.fg.tobytes() == want.fg.tobytes() and got.bg.tobytes() == want.bg.tobytes(), f"{what}: counts"
    assert got.score.tobytes() == want.score.tobytes(), f"{what}: the scores differ in bits"
    assert (got.n_fg, got.n_bg) == (want.n_fg, want.n_bg), what


SELECTIONS = {
    "all": None,
    "random30": np.random.default_rng(1).random(N) < 0.3,
    "one_row": _mask([1500]),
    "no_row": np.zeros(N, bool),
    "beyond_T": np.arange(N) >= T,
    "63_64_65": _mask([63, 64, 65]),
    "255_256": _mask([255, 256]),
    "last_listed": _mask([T - 1]),
    "one_span": _mask(range(640, 704)),
    "long_row": _mask([5, 77]),
}


# ------------------------------------------------------------------------------------------------------- 1. counts
@pytest.mark.parametrize("name", list(SELECTIONS))
def test_subset_terms_equal_a_bincount(name):
    ix, sel = _index(), SELECTIONS[name]
    wt, wf, FG = _counts(sel)
    t, f, rows = ix._subset_terms(sel)
    print(f"{name}: {wt.size} terms, {int(wf.sum())} entries, {FG} rows")
    assert t.dtype == np.uint32 and f.dtype == np.int64
    assert t.tobytes() == wt.tobytes() and f.tobytes() == wf.tobytes() and rows == FG
    t2, f2 = ix.subset_terms(sel)
    assert t2.tobytes() == wt.tobytes() and f2.tobytes() == wf.tobytes()
    if name in ("no_row", "beyond_T"):
        assert wt.size == 0
    else:
        assert wt.size > 0


def test_two_call_sizing_of_the_library():
    ix = _index()
    wt, wf, FG = _counts(SELECTIONS["random30"])
    bits = pack_allow_bits(SELECTIONS["random30"], N)
    n, rows = ctypes.c_int64(-1), ctypes.c_int64(-1)
    fn = nat.lib().css_index_subset_terms
    nat.check(fn(ix._handle(), bits.ctypes.data, 0, None, None, ctypes.byref(n), ctypes.byref(rows)))
    assert (n.value, rows.value) == (wt.size, FG)
    t, f = np.full(wt.size, 7, np.uint32), np.full(wt.size, 7, np.int64)
    nat.check(fn(ix._handle(), bits.ctypes.data, wt.size - 1, t.ctypes.data, f.ctypes.data, ctypes.byref(n), ctypes.byref(rows)))
    assert n.value == wt.size and (t == 7).all() and (f == 7).all()               # too small: sized, nothing written
    nat.check(fn(ix._handle(), bits.ctypes.data, wt.size, t.ctypes.data, f.ctypes.data, ctypes.byref(n), ctypes.byref(rows)))
    assert t.tobytes() == wt.tobytes() and f.tobytes() == wf.tobytes()


# ---------------------------------------------------------------------------------------------- 2. a frequent term
def test_a_term_in_every_row_counts_the_selected_rows():
    n, A, Bt = 20000, 12_000_000, 9_999_999
    rng = np.random.default_rng(2)
    span = range(6400, 6464)
    rows = [np.concatenate([[A], rng.integers(0, 1 << 23, size=3), [Bt] if r in span else []]).astype(np.int64) for r in range(n)]   # (A, Bt >= 2^23)
    off, tok = lists_as_csr(rows)
    poff, terms, _, _ = pack(off, tok)
    ix = IndexFlatIP(D_)
    ix.add(_x(n, seed=4))
    ix.set_terms((off, tok))
    sels = {"all": None, "half": rng.random(n) < 0.5, "span": _mask(span, n), "span_and_one": _mask(list(span) + [19999], n)}
    for slots in (-1, 0, 16, 4096):
        ix.set_sigterm_slots(slots)
        for name, sel in sels.items():
            wt, wf, FG = _counts(sel, poff, terms)
            t, f, got_rows = ix._subset_terms(sel)
            assert t.tobytes() == wt.tobytes() and f.tobytes() == wf.tobytes() and got_rows == FG, (slots, name)
            assert int(f[t == A][0]) == FG, (slots, name)
            assert int(f[t == Bt][0]) == (64 if sel is None or name.startswith("span") else int(sel[6400:6464].sum())), (slots, name)
    for bad in (-2, 1, 8, 48, 8192):
        with pytest.raises(RuntimeError):
            ix.set_sigterm_slots(bad)
    ix.close()


# ------------------------------------------------------------------------------------------------------ 3. ranking
BACK = np.arange(N) < 2000
RANK_CASES = {
    "mod7": (np.arange(N) % 7 == 0, None),
    "random30": (SELECTIONS["random30"], None),
    "mean": (_sel_mean(), None),
    "mod4_in_2000": ((np.arange(N) % 4 == 0) & BACK, BACK),
    "mean_in_random": (_sel_mean() & (np.random.default_rng(23).random(N) < 0.8) | _mask([1, 2]),
                       _sel_mean() | (np.random.default_rng(29).random(N) < 0.4) | _mask([1, 2])),
    "one_span": (SELECTIONS["one_span"], None),
}


@pytest.mark.parametrize("case", list(RANK_CASES))
def test_significant_terms_equal_the_numpy_ranking(case):
    ix = _index()
    sel, back = RANK_CASES[case]
    short = 0
    for m in (1, 20, 256):
        for mc in (1, 2, 50):
            want = _rank(sel, back, m, mc)
            got = ix.significant_terms(allow=sel, m=m, min_count=mc, background=back)
            _same_rank(got, want, f"{case} m={m} min_count={mc}")
            short += want.terms.size < m
    print(f"{case}: FG={want.n_fg} BG={want.n_bg}, {short} of 9 answers shorter than m")
    if case == "mod7":        # fg * BG == bg * FG must not qualify; equal (fg, bg) come by ascending term
        assert (want.n_fg, want.n_bg) == (413, T)
        t, f, _ = _counts(sel)
        assert int(f[t == EQ7][0]) == 1 and int(_counts(None)[1][_counts(None)[0] == EQ7][0]) == 7
        full = ix.significant_terms(allow=sel, m=256, min_count=1)
        assert EQ7 not in full.terms.tolist()
        at = [full.terms.tolist().index(x) for x in sorted(TIES)]
        assert at == sorted(at) and np.unique(full.score[at]).size == 1 and full.fg[at].tolist() == [3] * 4
        assert full.bg[at].tolist() == [7] * 4
        assert short > 0
    if case == "mod4_in_2000":
        assert (want.n_fg, want.n_bg) == (500, 2000)
        full = ix.significant_terms(allow=sel, m=256, min_count=1, background=back)
        assert EQ4 not in full.terms.tolist() and full.terms.size == 256
        t, f, _ = _counts(sel)
        bt, bf, _ = _counts(back)
        assert int(f[t == EQ4][0]) == 4 and int(bf[bt == EQ4][0]) == 16


def test_the_unused_slots_of_the_library():
    ix = _index()
    sel = RANK_CASES["mod7"][0]
    want = _rank(sel, None, 256, 50)
    assert 0 < want.terms.size < 256
    m = 256
    terms, score = np.full(m, 5, np.uint32), np.full(m, 5.0, np.float64)
    fg, bg = np.full(m, 5, np.int64), np.full(m, 5, np.int64)
    n, nf, nb = ctypes.c_int(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    bits = pack_allow_bits(sel, N)
    nat.check(nat.lib().css_index_significant_terms(ix._handle(), bits.ctypes.data, None, m, 50, terms.ctypes.data, fg.ctypes.data,
                                                    bg.ctypes.data, score.ctypes.data, ctypes.byref(n), ctypes.byref(nf), ctypes.byref(nb)))
    k = want.terms.size
    assert n.value == k and (nf.value, nb.value) == (413, T)
    assert terms[:k].tobytes() == want.terms.tobytes() and score[:k].tobytes() == want.score.tobytes()
    assert (terms[k:] == 0xFFFFFFFF).all() and (fg[k:] == 0).all() and (bg[k:] == 0).all() and (score[k:].view(np.uint64) == 0).all()


# ------------------------------------------------------------------------------------------------------ 4. meaning
def test_planted_terms_lead():
    got = _index().significant_terms(allow=_sel_mean(), m=5, min_count=2)
    assert sorted(got.terms.tolist()) == sorted(MEAN)
    assert got.fg.tolist() == [150] * 5 and got.bg.tolist() == [152] * 5
    assert got.terms.tolist() == sorted(MEAN)                                      # equal scores: by term


# ---------------------------------------------------------------------------------------------------- 5. lifecycle
def test_counts_follow_the_index():
    rows = list(_rows())
    off, tok = lists_as_csr(rows)
    x = _x(N)
    ix = IndexFlatIP(D_)
    ix.add(x)
    ix.set_terms((off, tok))
    sel = SELECTIONS["random30"]

    def check(sel, rows_now, what, back=None):
        o, t = lists_as_csr(rows_now)
        poff, terms, _, _ = pack(o, t)
        wt, wf, FG = _counts(sel, poff, terms)
        got = ix.subset_terms(sel)
        assert got[0].tobytes() == wt.tobytes() and got[1].tobytes() == wf.tobytes(), what
        bt, bc, BG = _counts(back, poff, terms)
        want = significant_from_counts(wt, wf, bc[np.searchsorted(bt, wt)], FG, BG, 20, 2)
        a = ix.significant_terms(allow=sel, m=20, min_count=2, background=back)
        b = ix.significant_terms(allow=sel, m=20, min_count=2, background=back)
        _same_rank(a, want, what)
        assert _raw(a) == _raw(b), f"{what}: two calls in a row differ"

    # calls in between change neither the statistics nor a hybrid search
    probe = [0, TOP, MEAN[0], 424242]
    stats = ix.term_stats(probe)
    w = bm25_weights(stats[0][:3], stats[1])
    hyb = ix.search_hybrid(x[10], probe[:3], w, 10, 0.5)
    check(sel, rows, "fresh")
    check(sel, rows, "fresh, masked background", back=sel | BACK)
    again = ix.term_stats(probe)
    assert again[0].tolist() == stats[0].tolist() and again[1:] == stats[1:]
    assert all(np.array_equal(u, v) for u, v in zip(ix.search_hybrid(x[10], probe[:3], w, 10, 0.5), hyb))

    gone = np.zeros(N, bool)
    gone[np.random.default_rng(31).choice(N, size=300, replace=False)] = True
    gone[[0, 63, 64, T - 1, N - 1]] = True
    assert ix.remove_ids(gone) == int(gone.sum())
    rows = [r for r, g in zip(rows, gone[:T]) if not g]
    n1 = N - int(gone.sum())
    sel1 = sel[~gone]
    check(sel1, rows, "after remove_ids")
    check(None, rows, "after remove_ids, every row")

    rows = rows[:1000] + [np.array([TOP, 0, 0, 5]), np.array([], np.int64), np.array([5, 6, 7])]
    ix.set_terms(rows[1000:], row0=1000)                                           # the rewrite: rows 1003.. lose their lists
    check(sel1, rows, "after a set_terms rewrite")
    check(_mask([1000, 1001, 1002, 1003, 1500], n1), rows, "the rewritten rows")

    ix.add(_x(500, seed=9))                                                        # rows added after the lists have none
    sel2 = np.concatenate([sel1, np.ones(500, bool)])
    check(sel2, rows, "after add")

    ix.reset()
    assert ix.subset_terms()[0].size == 0
    empty = ix.significant_terms()
    assert empty.terms.size == 0 and (empty.n_fg, empty.n_bg) == (0, 0)
    ix.add(x[:200])
    assert ix.subset_terms()[0].size == 0 and ix.significant_terms(allow=np.ones(200, bool)).terms.size == 0
    ix.set_terms(rows[:150])
    check(np.arange(200) % 3 == 0, rows[:150], "after reset")
    ix.close()


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals():
    ix = _index()
    sel = SELECTIONS["random30"]
    before = ix.subset_terms(sel)
    with pytest.raises(ValueError, match="row 1 "):
        ix.significant_terms(allow=_mask([1, 2, 4]), background=_mask([2, 4, 6]))
    ix.significant_terms(allow=_mask([2, T + 5]), background=_mask([2]))           # rows without lists are in neither set
    for bad in (dict(m=0), dict(m=257), dict(min_count=0), dict(allow=np.ones(N - 1, bool)), dict(background=np.ones(N + 1, bool)),
                dict(allow=np.ones(N, np.int32))):
        with pytest.raises(ValueError):
            ix.significant_terms(**bad)
    with pytest.raises(ValueError):
        ix.subset_terms(np.ones(N + 3, bool))
    # the library itself: S outside B names the row and writes nothing; m and min_count are checked
    m = 4
    terms, score = np.full(m, 5, np.uint32), np.full(m, 5.0, np.float64)
    fg, bg = np.full(m, 5, np.int64), np.full(m, 5, np.int64)
    n, nf, nb = ctypes.c_int(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    a, b = pack_allow_bits(_mask([70, 2000]), N), pack_allow_bits(_mask([70]), N)
    fn = nat.lib().css_index_significant_terms
    outs = (terms.ctypes.data, fg.ctypes.data, bg.ctypes.data, score.ctypes.data, ctypes.byref(n), ctypes.byref(nf), ctypes.byref(nb))
    assert fn(ix._handle(), a.ctypes.data, b.ctypes.data, m, 1, *outs) == nat.CSS_ERR_INVALID
    assert "row 2000" in nat.last_error()
    assert (terms == 5).all() and (fg == 5).all() and (score == 5.0).all() and n.value == -1 and nf.value == -1
    for mm, mc in ((0, 1), (257, 1), (4, 0)):
        assert fn(ix._handle(), a.ctypes.data, None, mm, mc, *outs) == nat.CSS_ERR_INVALID
    after = ix.subset_terms(sel)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    freed = IndexFlatIP(D_)
    freed.close()
    for call in (freed.subset_terms, freed.significant_terms):
        with pytest.raises(RuntimeError, match="freed"):
            call()

"""GPU: attribute columns and ``IndexFlat.where`` (``css_index_set_attr`` .. ``css_index_where``, kernel ``k_where``),
and ``facets(by_attribute=)`` (``css_index_facets_attr``).

The reference is ``flat_index.where_numpy`` -- numpy's own comparisons on int32 / float32 arrays, itself checked against
a plain Python loop in ``test_where_host.py`` -- and every mask must equal it bit for bit; there is no tolerance
anywhere in this file.  The inputs come from ``where_cases.py``; ``test_where_host.py`` proves that they bind.  The
index has dimension 1, the smallest it accepts: ``where`` never reads the vectors.  ``TILE_ROWS`` is the block constant
of ``k_where`` (csrc/css_where.h ``kWhereTileRows``): the sizes include it, one less and one more."""
import ctypes

import numpy as np
import pytest

import lattice_cases as lc
import where_cases as wc
from where_cases import TILE_ROWS

pytestmark = pytest.mark.gpu

assert {TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1} <= set(wc.SIZES)


def _fi():
    from claude_semantic_search_amd import flat_index as fi
    return fi


def _index(n, cols=None):
    ix = _fi().IndexFlatIP(1)
    if n:
        ix.add(np.ones((n, 1), dtype=np.float32))
    for slot, values in (wc.columns(n) if cols is None else cols).items():
        ix.set_attribute(slot, values)
    return ix


@pytest.fixture(scope="module")
def built():
    """One index per size, shared by the read-only tests."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = (_index(n), wc.columns(n))
        return made[n]
    yield get
    for ix, _ in made.values():
        ix.close()


def _check(ix, cols, n, clauses, allow=None):
    fi = _fi()
    want = fi.where_numpy(cols, clauses, n, allow=allow)
    mask, count = ix.where(clauses, allow=allow, return_count=True)
    assert mask.dtype == np.bool_ and mask.shape == (n,)
    assert np.array_equal(mask, want), (n, clauses, np.flatnonzero(mask != want)[:8])
    assert count == int(want.sum())


@pytest.mark.parametrize("n", wc.SIZES)
def test_every_op_on_both_types_and_special_values(built, n):
    ix, cols = built(n)
    stored = cols[wc.SLOT_F].view(np.uint32)
    assert np.array_equal(ix.get_attribute(wc.SLOT_F).view(np.uint32), stored)      # NaN, -0.0 and the denormal as given
    assert np.array_equal(ix.get_attribute(wc.SLOT_I), cols[wc.SLOT_I])
    allow = wc.allow_mask(n)
    for _, clause in wc.grid_clauses(max(n, 2)) + wc.special_clauses():
        _check(ix, cols, n, [clause])
        _check(ix, cols, n, [clause], allow=allow)


@pytest.mark.parametrize("n", wc.SIZES)
def test_sixteen_clauses_one_slot_twice_allow_and_no_clause(built, n):
    ix, cols = built(n)
    allow = wc.allow_mask(n)
    many = wc.many_clauses(max(n, 2))
    assert len(many) == 16
    for a in (None, allow):
        _check(ix, cols, n, many, allow=a)
        _check(ix, cols, n, [(wc.SLOT_I, ">", -7), (wc.SLOT_I, "<=", 12)], allow=a)
        _check(ix, cols, n, [(wc.SLOT_F, ">=", -2.25), (wc.SLOT_F, "<", 3.0), (wc.SLOT_F, "!=", 0.0)], allow=a)
        _check(ix, cols, n, [], allow=a)
    mask, count = ix.where([], return_count=True)
    assert mask.all() and count == n
    none = np.zeros(n, dtype=np.bool_)
    mask, count = ix.where([(wc.SLOT_I, ">=", wc.I32_MIN)], allow=none, return_count=True)
    assert not mask.any() and count == 0


@pytest.mark.parametrize("n", wc.SIZES)
def test_output_words_tail_bits_and_sentinels(built, n):
    """Every row passes: a stray bit past ntotal, or a word past the end, would show."""
    ix, cols = built(n)
    words = (n + 31) // 32
    for clauses in ([(wc.SLOT_I, ">=", wc.I32_MIN)], []):
        buf = np.full(words + 4, 0xA5A5A5A5, dtype="<u4")
        bits, count = ix.where_bits(clauses, out=buf[:words])
        assert count == n
        assert (buf[words:] == 0xA5A5A5A5).all()
        full = np.full(words, 0xFFFFFFFF, dtype="<u4")
        if n % 32:
            full[-1] = (1 << (n % 32)) - 1
        assert np.array_equal(buf[:words], full)


@pytest.mark.parametrize("n", [s for s in wc.SIZES if s >= 97])
def test_in_tables_in_lds_and_in_global_memory(built, n):
    ix, cols = built(n)
    allow = wc.allow_mask(n)
    for name, clauses, words in wc.table_cases():
        assert _fi().where_args(clauses, ix.attribute_type).tables.shape[0] == words, name
        _check(ix, cols, n, clauses)
        _check(ix, cols, n, clauses, allow=allow)
    _check(ix, cols, n, [(wc.SLOT_CODE, "in", [])])
    _check(ix, cols, n, [(wc.SLOT_CODE, "not in", [])])


def test_second_call_returns_the_same_bytes(built):
    ix, cols = built(TILE_ROWS + 1)
    clauses = wc.many_clauses(TILE_ROWS + 1)
    first = ix.where_bits(clauses, allow=wc.allow_mask(TILE_ROWS + 1))
    second = ix.where_bits(clauses, allow=wc.allow_mask(TILE_ROWS + 1))
    assert first[0].tobytes() == second[0].tobytes() and first[1] == second[1]


def test_empty_index(built):
    ix = _fi().IndexFlatIP(1)
    mask, count = ix.where([], return_count=True)
    assert mask.shape == (0,) and count == 0
    assert ix.attribute_type(3) == -1 and ix.get_attribute(3).shape == (0,)
    ix.close()


# ---------------------------------------------------------------- refusals (CSS_ERR_INVALID, by message)
def _raw_where(ix, clauses, nclauses=None, tables=None, table_words=None):
    from claude_semantic_search_amd import _native as nat
    arr = (nat.Clause * max(len(clauses), 1))(*[nat.Clause(*c) for c in clauses])
    tab = np.zeros(0, dtype="<u4") if tables is None else np.asarray(tables, dtype="<u4")
    out = np.full((ix.ntotal + 31) // 32 + 1, 0x5A5A5A5A, dtype="<u4")
    count = ctypes.c_int64(-7)
    rc = nat.lib().css_index_where(ix._handle(), arr, len(clauses) if nclauses is None else nclauses,
                                   tab.ctypes.data if tab.size else None, tab.size if table_words is None else table_words,
                                   None, out.ctypes.data, ctypes.byref(count))
    assert (out == 0x5A5A5A5A).all() or rc == 0
    return rc, nat.last_error()


EQ, IN, NOT_IN = 0, 6, 7


@pytest.mark.parametrize("name, clauses, kw, message", [
    ("unset slot", [(2, EQ, 1, 0, 0, 0)], {}, "clause 0: attribute slot 2 was never set"),
    ("slot out of range", [(16, EQ, 1, 0, 0, 0)], {}, "clause 0: attribute slot 16 outside [0, 16)"),
    ("unknown op", [(wc.SLOT_I, 8, 1, 0, 0, 0)], {}, "clause 0: unknown op 8"),
    ("in on a float slot", [(wc.SLOT_I, EQ, 1, 0, 0, 0), (wc.SLOT_F, IN, 0, 0, 0, 8)], {"tables": [255]},
     "clause 1: IN / NOT_IN on attribute slot 1, which holds float32 values"),
    ("table past the end", [(wc.SLOT_I, IN, 0, 0, 1, 33)], {"tables": [1, 2]},
     "clause 0: the table of 33 bits at word 1 does not lie inside the 2 table words"),
    ("table offset negative", [(wc.SLOT_I, NOT_IN, 0, 0, -1, 8)], {"tables": [1]}, "does not lie inside the 1 table words"),
    ("table too large", [(wc.SLOT_I, IN, 0, 0, 0, (1 << 27) + 1)], {"tables": [1]}, "table_bits=134217729 outside [0, 134217728]"),
    ("too many clauses", [(wc.SLOT_I, EQ, 1, 0, 0, 0)] * 17, {}, "nclauses=17 outside [0, 16]"),
    ("negative clause count", [(wc.SLOT_I, EQ, 1, 0, 0, 0)], {"nclauses": -1}, "nclauses=-1 outside [0, 16]"),
])
def test_where_refuses(built, name, clauses, kw, message):
    from claude_semantic_search_amd import _native as nat
    ix, _ = built(97)
    rc, err = _raw_where(ix, clauses, **kw)
    assert rc == nat.CSS_ERR_INVALID and message in err, (name, err)


def test_set_attribute_refuses_the_other_type_and_bad_slots(built):
    from claude_semantic_search_amd import _native as nat
    fi = _fi()
    ix = _index(40)
    with pytest.raises(nat.CssError, match="attribute slot 0 holds int32 values, not float32"):
        ix.set_attribute(wc.SLOT_I, np.zeros(40, dtype=np.float32))
    with pytest.raises(nat.CssError, match="attribute slot 1 holds float32 values, not int32"):
        ix.set_attribute(wc.SLOT_F, np.zeros(40, dtype=np.int32))
    assert np.array_equal(ix.get_attribute(wc.SLOT_I), wc.columns(40)[wc.SLOT_I])       # nothing was written
    with pytest.raises(ValueError, match="outside"):
        ix.set_attribute(16, [1])
    with pytest.raises(ValueError, match="rows"):
        ix.set_attribute(2, np.zeros(41, dtype=np.int32))
    assert ix.attribute_type(2) == -1
    rc = nat.lib().css_index_set_attr(ix._handle(), 16, 0, 0, 0, None)
    assert rc == nat.CSS_ERR_INVALID and "attribute slot 16 outside [0, 16)" in nat.last_error()
    rc = nat.lib().css_index_set_attr(ix._handle(), 2, 2, 0, 0, None)
    assert rc == nat.CSS_ERR_INVALID and "type=2" in nat.last_error()
    with pytest.raises(ValueError, match="slot 2 was never set"):
        ix.facets(np.ones((1, 1), np.float32), 0.0, nbuckets=4, by_attribute=2)
    with pytest.raises(ValueError, match="slot 1 holds float32"):
        ix.facets(np.ones((1, 1), np.float32), 0.0, nbuckets=4, by_attribute=wc.SLOT_F)
    out = [np.zeros(4, dtype=np.int64) for _ in range(4)]
    q = np.ones(1, np.float32)
    for slot, message in ((wc.SLOT_F, "attribute slot 1 is float32"), (2, "attribute slot 2 was never set"),
                          (-1, "attribute slot -1 outside")):
        rc = nat.lib().css_index_facets_attr(ix._handle(), q.ctypes.data, 1, 0.0, 0, None, slot, 4, out[0].ctypes.data, None,
                                             None, out[2].ctypes.data, out[3].ctypes.data)
        assert rc == nat.CSS_ERR_INVALID and message in nat.last_error()
    assert fi.MAX_ATTRS == 16 and fi.MAX_CLAUSES == 16
    ix.close()


# ---------------------------------------------------------------- the columns follow the rows
def test_values_survive_growth_and_new_rows_start_at_the_default():
    fi = _fi()
    n, more = 1000, 700                      # (the first capacity is 1024 rows: 1700 reallocates)
    cols = wc.columns(n)
    ix = _index(n, {wc.SLOT_I: cols[wc.SLOT_I], wc.SLOT_F: cols[wc.SLOT_F]})
    ix.add(np.ones((more, 1), dtype=np.float32))
    gi, gf = ix.get_attribute(wc.SLOT_I), ix.get_attribute(wc.SLOT_F)
    assert gi.dtype == np.int32 and gf.dtype == np.float32
    assert np.array_equal(gi[:n], cols[wc.SLOT_I]) and (gi[n:] == -1).all()
    assert np.array_equal(gf[:n].view(np.uint32), cols[wc.SLOT_F].view(np.uint32)) and np.isnan(gf[n:]).all()
    assert ix.attribute_type(wc.SLOT_CODE) == -1 and (ix.get_attribute(wc.SLOT_CODE) == -1).all()    # never set: no column
    now = {wc.SLOT_I: gi, wc.SLOT_F: gf}
    for clause in [(wc.SLOT_I, "==", -1), (wc.SLOT_I, "not in", [3]), (wc.SLOT_F, "!=", 1.5), (wc.SLOT_F, "<", 2.0)]:
        _check(ix, now, n + more, [clause])
    ix.set_attribute(wc.SLOT_I, np.arange(50, dtype=np.int64), row0=n + 10)                # a partial set
    gi[n + 10:n + 60] = np.arange(50)
    assert np.array_equal(ix.get_attribute(wc.SLOT_I), gi)
    assert np.array_equal(ix.get_attribute(wc.SLOT_I, row0=n + 5, n=10), gi[n + 5:n + 15])
    ix.close()


def test_remove_ids_compacts_the_columns_reset_forgets_them_drop_frees_one():
    n = 1025
    cols = wc.columns(n)
    ix = _index(n)
    keep = np.ones(n, dtype=np.bool_)
    keep[[0, 31, 32, 63, 64, 500, 1023, 1024]] = False
    keep[100:200:3] = False
    assert ix.remove_ids(np.flatnonzero(~keep)) == int((~keep).sum())
    kept = {s: v[keep] for s, v in cols.items()}
    m = int(keep.sum())
    for s, v in kept.items():
        assert np.array_equal(ix.get_attribute(s).view(np.uint32), v.view(np.uint32)), s
    for _, clause in wc.grid_clauses(m):
        _check(ix, kept, m, [clause])
    _check(ix, kept, m, wc.many_clauses(m), allow=wc.allow_mask(m))

    ix.drop_attribute(wc.SLOT_CODE)
    assert ix.attribute_type(wc.SLOT_CODE) == -1 and ix.attribute_type(wc.SLOT_I) == _fi().ATTR_I32
    with pytest.raises(ValueError, match="slot 5 was never set"):
        ix.where([(wc.SLOT_CODE, "==", 1)])
    ix.set_attribute(wc.SLOT_CODE, np.full(m, 2.5, dtype=np.float32))              # a dropped slot takes either type
    assert ix.attribute_type(wc.SLOT_CODE) == _fi().ATTR_F32
    ix.drop_attribute(9)                                                           # (an unset slot: nothing happens)

    ix.reset()
    assert [ix.attribute_type(s) for s in range(16)] == [-1] * 16
    ix.add(np.ones((10, 1), dtype=np.float32))
    assert (ix.get_attribute(wc.SLOT_I) == -1).all()
    ix.set_attribute(wc.SLOT_I, np.linspace(0, 1, 10))                             # ... and the type with the values
    assert ix.attribute_type(wc.SLOT_I) == _fi().ATTR_F32
    ix.close()


# ---------------------------------------------------------------- neutrality: attributes change no search
LN, LD = 2000, 64


@pytest.fixture(scope="module")
def lattice():
    x, q = lc.case("T", LN, LD)
    return x, np.ascontiguousarray(q[:5])


def test_searches_return_the_same_bytes_with_attributes_set(lattice):
    x, q = lattice
    ix = _fi().IndexFlatIP(LD)
    ix.add(x)
    ix.set_groups((np.arange(LN) % 37).astype(np.int32))
    allow = wc.allow_mask(LN)

    def run():
        return (ix.search(q, 10), ix.search(q, 10, allow=allow), ix.range_search(q, 3.0), ix.search_grouped(q, 10))
    before = run()
    for slot, values in wc.columns(LN).items():
        ix.set_attribute(slot, values)
    ix.where(wc.many_clauses(LN))
    after = run()
    for b, a in zip(before, after):
        for bb, aa in zip(b, a):
            assert bb.dtype == aa.dtype and bb.tobytes() == aa.tobytes()
    ix.close()


@pytest.mark.parametrize("metric", [lc.METRIC_IP, lc.METRIC_L2])
def test_facets_by_attribute_equals_facets_with_uploaded_buckets(lattice, metric):
    """Lattice rows: every score is exact, so rows AT the radius are decided alike by construction and the two calls
    must agree in every output array."""
    x, q = lattice
    fi = _fi()
    ix = fi.IndexFlat(LD, metric)
    ix.add(x)
    slot, nb = 7, 16
    buckets = ((np.arange(LN) * 5) % 19 - 1).astype(np.int32)          # -1, and 16 .. 17 beyond the buckets
    ix.set_attribute(slot, buckets)
    ix.set_attribute(3, np.arange(LN, dtype=np.float32))
    S = lc.scores64(x, q, metric)
    radius = float(np.sort(S[0])[-50] if metric == lc.METRIC_IP else np.sort(S[0])[50])     # an attained score: ties at it
    assert (S == radius).any()
    for allow in (None, wc.allow_mask(LN)):
        got = ix.facets(q, radius, nbuckets=nb, allow=allow, by_attribute=slot)
        want = ix.facets(q, radius, buckets=ix.get_attribute(slot), nbuckets=nb, allow=allow)
        assert int(want.total.sum()) > 0 and int(want.unbucketed.sum()) > 0
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    ix.close()

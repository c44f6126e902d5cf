"""CPU: the pure helpers of ``IndexFlat.where`` -- ``where_args`` (validation, table packing) and ``where_numpy`` (the
restatement the GPU tests compare with) -- and the proof that the inputs of ``test_where_gpu.py`` bind."""
import math

import numpy as np
import pytest

import where_cases as wc
from claude_semantic_search_amd import flat_index as fi

I32, F32 = fi.ATTR_I32, fi.ATTR_F32
TYPES = {wc.SLOT_I: I32, wc.SLOT_F: F32, wc.SLOT_CODE: I32, wc.SLOT_BIG: I32}


def type_of(slot):
    return TYPES.get(slot, -1)


# ---------------------------------------------------------------- where_args
@pytest.mark.parametrize("clauses, message", [
    ([(0, "==", 1)] * 17, "17 clauses, at most 16"),
    ([(0, "==")], "clause 0 is not"),
    ([(16, "==", 1)], "attribute slot 16 outside"),
    ([(-1, "==", 1)], "attribute slot -1 outside"),
    ([(True, "==", 1)], "slot must be an integer"),
    ([(2, "==", 1)], "attribute slot 2 was never set"),
    ([(0, "=", 1)], "unknown op '='"),
    ([(0, "==", 1.5)], "must be an integer"),
    ([(0, "==", 2 ** 31)], "beyond int32"),
    ([(0, "<", "3")], "must be an integer"),
    ([(1, "<", "3")], "must be a real number"),
    ([(1, "in", [1])], "holds float32 values"),
    ([(0, "in", 3)], "iterable of integers"),
    ([(0, "in", [-1])], "must lie in"),
    ([(0, "not in", [1 << 27])], "must lie in"),
    ([(0, "in", [1.0])], "must hold integers"),
    (7, "sequence of"),
])
def test_where_args_refuses(clauses, message):
    with pytest.raises(ValueError, match=message):
        fi.where_args(clauses, type_of)


def test_where_args_packs_tables_and_operands():
    a = fi.where_args([(0, "in", [0, 33]), (1, ">=", -0.0), (0, "not in", []), (5, "in", (31,)), (0, "<", -5),
                       (0, "==", True)], type_of)
    assert a.clauses[0] == (0, 6, 0, 0, 34) and a.clauses[2] == (0, 7, 0, 2, 0) and a.clauses[3] == (5, 6, 0, 2, 32)
    assert a.tables.dtype == np.dtype("<u4") and a.tables.tolist() == [1, 2, 1 << 31]
    assert a.clauses[1] == (1, 5, -2 ** 31, 0, 0)          # the bits of -0.0 as an int32
    assert a.clauses[4] == (0, 2, -5, 0, 0) and a.clauses[5] == (0, 0, 1, 0, 0)
    empty = fi.where_args([], type_of)
    assert empty.clauses == [] and empty.tables.size == 0


def test_attr_values():
    a, t = fi.attr_values([1, -2, 3])
    assert a.dtype == np.int32 and t == I32
    a, t = fi.attr_values(np.array([True, False]))
    assert a.tolist() == [1, 0] and t == I32
    a, t = fi.attr_values(np.array([1.5, np.nan], dtype=np.float64))
    assert a.dtype == np.float32 and t == F32
    for bad, message in (([2 ** 31], "beyond int32"), (["a"], "integers or real"), ([[1, 2]], "one-dimensional")):
        with pytest.raises(ValueError, match=message):
            fi.attr_values(bad)


# ---------------------------------------------------------------- where_numpy against a plain Python loop
def _py_holds(v, op, x, is_float):
    """One comparison in plain Python (floats: IEEE through Python's own float, which float32 values convert to exactly)."""
    if op in ("in", "not in"):
        return (int(v) in set(x)) == (op == "in")
    v, x = (float(v), float(np.float32(x))) if is_float else (int(v), int(x))
    if is_float and (math.isnan(v) or math.isnan(x)):
        return op == "!="
    return {"==": v == x, "!=": v != x, "<": v < x, "<=": v <= x, ">": v > x, ">=": v >= x}[op]


@pytest.mark.parametrize("n", [0, 1, 2, 97])
def test_where_numpy_equals_a_python_loop(n):
    cols = wc.columns(n)
    allow = wc.allow_mask(n)
    calls = [[c] for _, c in wc.grid_clauses(max(n, 2))] + [[c] for _, c in wc.special_clauses()]
    calls += [wc.many_clauses(max(n, 2)), []] + [cl for _, cl, _ in wc.table_cases()]
    for clauses in calls:
        for mask in (None, allow):
            want = np.array([all(_py_holds(cols[s][r], op, x, cols[s].dtype == np.float32) for s, op, x in clauses)
                             and (mask is None or bool(mask[r])) for r in range(n)], dtype=np.bool_)
            got = fi.where_numpy(cols, clauses, n, allow=mask)
            assert got.dtype == np.bool_ and np.array_equal(got, want), clauses


def test_where_numpy_leaves_allow_alone():
    allow = wc.allow_mask(40)
    before = allow.copy()
    fi.where_numpy(wc.columns(40), [(wc.SLOT_I, ">", 0)], 40, allow=allow)
    assert np.array_equal(allow, before)


# ---------------------------------------------------------------- the GPU grid binds
@pytest.mark.parametrize("n", [s for s in wc.SIZES if s >= 2] + [2])
def test_every_grid_clause_selects_some_rows_and_leaves_some_out(n):
    cols = wc.columns(n)
    for name, clause in wc.grid_clauses(n):
        got = int(fi.where_numpy(cols, [clause], n).sum())
        assert 0 < got < n, (n, name, got)


@pytest.mark.parametrize("n", [s for s in wc.SIZES if s >= wc.SPECIALS_COMPLETE])
def test_special_clauses_bind_unless_constant_by_definition(n):
    cols = wc.columns(n)
    for v in wc.I_SPECIALS:
        assert (cols[wc.SLOT_I] == v).any()
    stored = cols[wc.SLOT_F].view(np.uint32)
    for v in wc.F_SPECIALS:                  # as stored values, by their bits (-0.0 and NaN included)
        assert (stored == np.float32(v).view(np.uint32)).any()
    for name, clause in wc.special_clauses():
        got = int(fi.where_numpy(cols, [clause], n).sum())
        if wc.constant_by_definition(clause):
            assert got in (0, n), (n, name, got)
        else:
            assert 0 < got < n, (n, name, got)


@pytest.mark.parametrize("n", [s for s in wc.SIZES if s >= 2])
def test_many_clauses_allow_and_tables_bind(n):
    cols = wc.columns(n)
    assert 0 < int(fi.where_numpy(cols, wc.many_clauses(n), n).sum())
    assert 0 < int(wc.allow_mask(n).sum()) < n
    if n >= 97:
        for name, clauses, words in wc.table_cases():
            assert fi.where_args(clauses, type_of).tables.shape[0] == words, name
            got = int(fi.where_numpy(cols, clauses, n).sum())
            assert 0 < got < n, (n, name, got)


def test_table_cases_straddle_the_lds_limit():
    words = sorted({w for _, _, w in wc.table_cases()})
    assert wc.LDS_WORDS in words and wc.LDS_WORDS + 1 in words
    assert wc.LDS_WORDS == fi.nat.WHERE_LDS_WORDS and wc.TILE_ROWS == fi.nat.WHERE_TILE_ROWS
    for c in (wc.TILE_ROWS - 1, wc.TILE_ROWS, wc.TILE_ROWS + 1, 0 + 1):
        assert c in wc.SIZES


# ---------------------------------------------------------------- compile_filters against _matches_filters
import json  # noqa: E402
from pathlib import Path  # noqa: E402

from claude_semantic_search_amd import filters as ff  # noqa: E402
from claude_semantic_search_amd.storage import HybridStorage  # noqa: E402

DECLINE_RULES = ("a value outside int32", "a NULL under a range op", "mixed-type column", "unknown op",
                 "a range bound on", "a range on the dictionary column", "None in a list", "None as the value",
                 "a list member on", "is a chunk column without an attribute slot", "more than 16 clauses")
_HOST = HybridStorage.__new__(HybridStorage)      # _matches_filters reads nothing of the instance


def _row(**kw):
    return {**{c: None for c in ff.ATTR_COLUMNS}, "id": "c", "text": "t", "metadata": "{}", "faiss_id": 0,
            "created_at": "x", "updated_at": "y", **kw}


def _device_answer(catalog, clauses):
    cols = {catalog.slot(c): catalog.codes[c] for c in ff.ATTR_COLUMNS}
    return fi.where_numpy(cols, clauses, catalog.rows)


def _compare(rows, catalog, filters):
    """True when the filter compiled.  Compiled: the clauses answer every row as the host does.  Declined: a stated rule."""
    why = []
    clauses = ff.compile_filters(filters, catalog, why)
    if clauses is None:
        assert len(why) == 1 and any(r in why[0] for r in DECLINE_RULES), (filters, why)
        return False
    fi.where_args(clauses, lambda s: fi.ATTR_I32)          # what IndexFlat.where would accept
    want = np.array([_HOST._matches_filters(dict(r), filters) for r in rows], dtype=np.bool_)
    got = _device_answer(catalog, clauses)
    assert np.array_equal(got, want), (filters, clauses, np.flatnonzero(got != want)[:5])
    return True


def test_compile_filters_on_the_golden_truth_table():
    g = json.loads((Path(__file__).resolve().parent / "golden" / "filter_truth_table.json").read_text())
    row = _row(**{k: v for k, v in g["chunk_data"].items()})
    row["has_code"] = int(row["has_code"])              # as SQLite hands a BOOLEAN back
    for c in ff.INT_COLUMNS:
        row[c] = row[c] if row[c] is not None else 0    # add_chunks stores 0 for an absent count
    catalog = ff.AttrCatalog()
    catalog.extend([row])
    compiled = 0
    for filters, want in g["cases"]:
        assert _HOST._matches_filters(dict(row), filters) is want, filters     # the row above is the table's chunk
        compiled += _compare([row], catalog, filters)
    assert compiled >= 0.8 * len(g["cases"])


def _random_corpus(n, seed):
    rng = np.random.default_rng(seed)
    projects = ["Alpha", "alpha-Two", "BETA", "beta_test", "Gamma", None]
    stamps = [f"2024-0{1 + d // 28}-{1 + d % 28:02d}T{h:02d}:00:00" for d in range(0, 160, 3) for h in (9, 17)]
    stamps += [f"2024-0{1 + d // 28}-{1 + d % 28:02d} {h:02d}:30:00Z" for d in range(1, 160, 7) for h in (8,)]   # a second format
    rows = []
    for i in range(n):
        rows.append(_row(id=f"c{i}", faiss_id=i, project_name=projects[rng.integers(len(projects))],
                         session_id=None if rng.random() < 0.1 else f"s{rng.integers(12)}",
                         chunk_type=("qa_pair", "code_block", "tool_usage", None)[rng.integers(4)],
                         file_path=f"/p/{rng.integers(20)}.jsonl", has_code=int(rng.integers(2)), has_tools=int(rng.integers(2)),
                         word_count=int(rng.integers(0, 200)), char_count=int(rng.integers(0, 5000)),
                         message_count=int(rng.integers(1, 9)), timestamp=stamps[rng.integers(len(stamps))]))   # repeated stamps
    return rows, stamps


def _random_filter(rng, stamps):
    kind = rng.integers(12)
    pick = lambda xs: xs[rng.integers(len(xs))]   # noqa: E731
    if kind == 0:
        return {"project_name": pick(["alpha", "ALPHA", "beta", "a", "two", "zzz", ""])}
    if kind == 1:
        return {"chunk_type": pick(["qa_pair", "code_block", "QA_PAIR", "nothing"])}
    if kind == 2:
        return {"chunk_type": [pick(["qa_pair", "tool_usage"]), pick(["code_block", "zzz"])]}
    if kind == 3:
        return {"session_id": [f"s{rng.integers(14)}" for _ in range(rng.integers(0, 4))]}
    if kind == 4:
        return {"word_count": {pick(["gte", "gt"]): int(rng.integers(0, 150)), pick(["lte", "lt"]): int(rng.integers(50, 220))}}
    if kind == 5:
        lo, hi = sorted([pick(stamps), pick(stamps)])
        return {"timestamp": {pick(["gte", "gt"]): lo[:rng.integers(8, len(lo) + 1)], pick(["lte", "lt"]): hi}}
    if kind == 6:
        return {"has_code": pick([True, False, 1, 0]), "project_name": pick(["beta", "Gamma"]),
                "message_count": {"gte": int(rng.integers(1, 6))}}
    if kind == 7:
        return {"no_such_key": "x", "has_tools": bool(rng.integers(2)), "related_to": "c3"}
    if kind == 8:
        return {"word_count": pick([int(rng.integers(0, 200)), 10.0, 10.5, "10"]), "char_count": [int(rng.integers(0, 5000)), 7, 8.0]}
    if kind == 9:
        return {"timestamp": pick(stamps), "file_path": f"/p/{rng.integers(25)}.jsonl"}
    if kind == 10:
        return {"timestamp": [pick(stamps), pick(stamps), "never"], "session_id": f"s{rng.integers(14)}"}
    return pick([{"word_count": {"gte": 2 ** 31}}, {"word_count": {"ge": 5}}, {"word_count": {"gte": 2.5}}, {"project_name": None},
                 {"chunk_type": [None, "qa_pair"]}, {"project_name": {"gte": "a"}}, {"text": "t"}, {"char_count": [-1, 5]},
                 {"word_count": 2 ** 40}, {"timestamp": {"gte": 5}}])


def test_compile_filters_on_a_random_corpus():
    rows, stamps = _random_corpus(400, 11)
    catalog = ff.AttrCatalog()
    first = catalog.extend(rows[:250])
    assert set(first.values()) == {0}
    first = catalog.extend(rows[250:])                 # later rows bring timestamps that sort in front of stored ones
    assert first["timestamp"] == 0 and first["project_name"] == 250
    once = ff.AttrCatalog()
    once.extend(rows)
    assert np.array_equal(once.codes["timestamp"], catalog.codes["timestamp"]) and once.sorted == catalog.sorted
    order = catalog.sorted["timestamp"]
    assert order == sorted(set(r["timestamp"] for r in rows)) and len(order) < len(rows)          # repeated, rank-coded
    assert any(" " in t for t in order) and any("T" in t for t in order)                          # two formats
    assert catalog.has_null["project_name"] and not catalog.has_null["timestamp"] and not any(catalog.mixed.values())
    rng = np.random.default_rng(12)
    filters = [_random_filter(rng, stamps) for _ in range(400)]
    compiled = sum(_compare(rows, catalog, f) for f in filters)
    assert compiled >= 0.8 * len(filters), compiled
    # every compiled kind selects somewhere and rejects somewhere: the comparison above is not vacuous
    hits = [int(_device_answer(catalog, c).sum()) for c in (ff.compile_filters(f, catalog) for f in filters) if c is not None]
    assert sum(0 < h < len(rows) for h in hits) > len(hits) // 2


def test_compile_filters_declines_what_the_host_does_differently():
    rows, _ = _random_corpus(50, 13)
    rows[7]["timestamp"] = None                         # a NULL under a range op: the host comparison raises
    rows[9]["word_count"] = None
    rows[11]["project_name"] = 5
    catalog = ff.AttrCatalog()
    catalog.extend(rows + [None])                       # (a row without a live chunk is no NULL)
    assert (catalog.codes["project_name"][-1], catalog.codes["word_count"][-1]) == (-1, -1)
    for filters, rule in (({"timestamp": {"gte": "2024"}}, "a NULL under a range op"),
                          ({"word_count": 5}, "mixed-type column"), ({"project_name": "a"}, "mixed-type column")):
        why = []
        assert ff.compile_filters(filters, catalog, why) is None and rule in why[0]
    with pytest.raises(TypeError):
        _HOST._matches_filters(dict(rows[7]), {"timestamp": {"gte": "2024"}})
    assert ff.compile_filters({"timestamp": "2024", "nope": 1}, catalog) == [(catalog.slot("timestamp"), "in", [])]
    assert ff.compile_filters({}, catalog) == [] and ff.compile_filters(None, catalog) == []

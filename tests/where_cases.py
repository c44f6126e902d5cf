"""The inputs of the ``where`` tests: attribute columns and clauses per index size, shared by ``test_where_gpu.py`` (which
runs them on the device) and ``test_where_host.py`` (which proves with numpy alone that they bind: every grid clause
selects at least one row and leaves at least one out at every size >= 2, so a kernel that answered "all" or "none"
could not pass).

Plain module like ``lattice_cases.py``; nothing here touches the GPU."""
import numpy as np

TILE_ROWS = 1024     # csrc/css_where.h kWhereTileRows: the rows one block of k_where takes per step
LDS_WORDS = 8192     # csrc/css_where.h kWhereLdsWords: table words of a call that still go to LDS
SIZES = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 255, 256, 257, 1000, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1)

I32_MIN, I32_MAX = int(np.iinfo(np.int32).min), int(np.iinfo(np.int32).max)
DENORMAL = float(np.float32(1e-40))      # a float32 denormal (the smallest normal is 1.18e-38)
assert 0.0 < DENORMAL < float(np.finfo(np.float32).tiny)

SLOT_I, SLOT_F, SLOT_CODE, SLOT_BIG = 0, 1, 5, 15   # int32 values, float32 values, dictionary codes, codes up to 2^18
COMPARE_OPS = ("==", "!=", "<", "<=", ">", ">=")

# the period of each pattern is odd, so a value meets every lane and both words of a wave over the rows
_I_PATTERN = np.array([3, -7, I32_MIN, I32_MAX, 0, 5, -1, 12, 3, 40, -7, 1, 2], dtype=np.int32)
_F_PATTERN = np.array([1.5, -2.25, 0.0, -0.0, np.inf, -np.inf, np.nan, DENORMAL, -DENORMAL, 3.0, 7.0], dtype=np.float32)
BIG_TOP = LDS_WORDS * 32 - 1     # the last bit of a table of exactly LDS_WORDS words


def columns(n):
    """``{slot: array}`` for an index of ``n`` rows."""
    r = np.arange(n)
    code = ((r * 7) % 40).astype(np.int32)
    code[r % 11 == 5] = -1                                   # NULL
    big = np.array([5, BIG_TOP, BIG_TOP + 1, -3, 31, 32, 33, BIG_TOP - 32, I32_MAX, 0, 30], dtype=np.int32)[r % 11]
    return {SLOT_I: _I_PATTERN[r % _I_PATTERN.size].copy(), SLOT_F: _F_PATTERN[r % _F_PATTERN.size].copy(),
            SLOT_CODE: code, SLOT_BIG: big}


def _operand(col, op):
    """An operand of ``op`` taken from the column so that the clause binds whenever the column has two distinct
    comparable values: for ``<`` and ``>=`` the upper median of the distinct values, else the lower one."""
    u = np.unique(col[~np.isnan(col)] if col.dtype == np.float32 else col)
    x = u[u.size // 2] if op in ("<", ">=") else u[(u.size - 1) // 2]
    return float(x) if col.dtype == np.float32 else int(x)


def grid_clauses(n):
    """Every op on both types, operands from the data: ``[(name, clause)]``.  These are the clauses that must bind."""
    cols = columns(n)
    out = []
    for slot in (SLOT_I, SLOT_F):
        for op in COMPARE_OPS:
            out.append((f"s{slot}{op}", (slot, op, _operand(cols[slot], op))))
    members = [int(v) for v in np.unique(cols[SLOT_I]) if v >= 0][::2]
    out.append(("in", (SLOT_I, "in", members)))
    out.append(("not in", (SLOT_I, "not in", members)))
    return out


I_SPECIALS = (I32_MIN, I32_MAX, -1, 0)
F_SPECIALS = (0.0, -0.0, float("inf"), float("-inf"), float("nan"), DENORMAL, -DENORMAL)


def special_clauses():
    """Every op against every special operand: ``[(name, clause)]``.  Some of these are constant by definition (see
    ``constant_by_definition``); the others bind as soon as the patterns above are complete."""
    out = []
    for slot, specials in ((SLOT_I, I_SPECIALS), (SLOT_F, F_SPECIALS)):
        for x in specials:
            for op in COMPARE_OPS:
                out.append((f"s{slot}{op}{x!r}", (slot, op, x)))
    return out


def constant_by_definition(clause):
    """True for a special clause that selects all rows or none whatever the column holds: a NaN operand (numpy: only
    ``!=`` holds, and always), and the comparisons no value can pass or fail at the ends of the int32 range; ``> inf``
    and ``< -inf`` select nothing (a stored NaN fails too)."""
    slot, op, x = clause
    if slot == SLOT_F:
        return x != x or (x == float("inf") and op == ">") or (x == float("-inf") and op == "<")
    return (x == I32_MIN and op in ("<", ">=")) or (x == I32_MAX and op in (">", "<="))


SPECIALS_COMPLETE = 31   # from this size on the columns hold every value of both patterns


def many_clauses(n):
    """16 clauses in one call that still select rows: both types, a slot used more than once, a table."""
    cols = columns(n)
    lo, hi = _operand(cols[SLOT_I], "<="), _operand(cols[SLOT_I], ">=")
    base = [(SLOT_I, ">=", I32_MIN), (SLOT_I, "<=", I32_MAX), (SLOT_I, "!=", 41), (SLOT_I, ">=", min(lo, hi) - 1),
            (SLOT_F, "!=", 99.0), (SLOT_F, "!=", float("nan")), (SLOT_CODE, "not in", [41, 42]), (SLOT_CODE, "<", 1000),
            (SLOT_BIG, "!=", 7), (SLOT_BIG, "not in", [6]), (SLOT_I, "!=", 41), (SLOT_CODE, ">=", -1),
            (SLOT_CODE, "!=", 1), (SLOT_I, "!=", -8), (SLOT_F, "!=", 99.5), (SLOT_CODE, "!=", 8)]
    assert len(base) == 16
    return base


def table_cases():
    """``in`` / ``not in`` calls by table shape: ``[(name, clauses, table words of the call)]``.  Sizes 1, 31, 32, 33 bits
    (the largest member is the size minus one); two tables in one call; tables that sum to exactly ``LDS_WORDS`` words
    (the last LDS call) and to ``LDS_WORDS + 1`` (the first global one), as one table plus a one-word table; the column
    of ``SLOT_BIG`` holds members, values just past each table, a negative value and int32 max."""
    out = []
    for bits in (1, 31, 32, 33):
        for op in ("in", "not in"):
            out.append((f"{op}-{bits}b", [(SLOT_BIG, op, [bits - 1])], (bits + 31) // 32))
            out.append((f"{op}-{bits}b-code", [(SLOT_CODE, op, [0, bits - 1])], (bits + 31) // 32))
    out.append(("two tables", [(SLOT_CODE, "in", [0, 7, 14, 21, 35]), (SLOT_BIG, "not in", [31, 33])], 4))
    for op in ("in", "not in"):
        out.append((f"{op}-lds-exact", [(SLOT_BIG, op, [5, BIG_TOP])], LDS_WORDS))
        out.append((f"{op}-lds-sum", [(SLOT_BIG, op, [5, BIG_TOP - 32]), (SLOT_CODE, "not in", [3])], LDS_WORDS))
        out.append((f"{op}-global-sum", [(SLOT_BIG, op, [5, BIG_TOP]), (SLOT_CODE, "not in", [3])], LDS_WORDS + 1))
        out.append((f"{op}-global-one", [(SLOT_BIG, op, [5, 33, BIG_TOP + 1])], LDS_WORDS + 1))
    return out


def allow_mask(n):
    """A mask with rows on and off in every word."""
    return (np.arange(n) % 5 != 2) ^ (np.arange(n) % 64 == 63)

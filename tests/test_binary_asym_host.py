"""Host: the numpy restatement of the asymmetric search of the binary store (binary.quantize_queries_numpy /
asym_scores_numpy / search_asym_numpy) on hand-written cases, and the refusals of the Python layer."""
import numpy as np
import pytest

from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd.binary import (IndexBinaryFlat, asym_scores_numpy, quantize_queries_numpy,
                                               search_asym_numpy)


def test_hand_written_case():
    """d = 32, q = (5, -128, 127, 0 ...): a row scores 5 (2 b0 - 1) - 128 (2 b1 - 1) + 127 (2 b2 - 1), whatever its other
    bits.  Rows 1 and 3 tie at 250 for rank 2, and row 1 takes it."""
    q8 = np.zeros((1, 32), dtype=np.int8)
    q8[0, :3] = (5, -128, 127)
    codes = np.array([[0b10100000, 0, 0, 0], [0b00111111, 255, 0, 1], [0b11100000, 1, 2, 3], [0b00100000, 0, 0, 0],
                      [0b10000000, 7, 7, 7]], dtype=np.uint8)
    s = asym_scores_numpy(q8, codes)
    assert s.dtype == np.int64 and s.tolist() == [[260, 250, 4, 250, 6]]
    D, I = search_asym_numpy(s, 2)
    assert D.dtype == np.int32 and I.dtype == np.int64 and D.tolist() == [[260, 250]] and I.tolist() == [[0, 1]]
    D, I = search_asym_numpy(s, 4, allow=np.array([False, False, True, True, True]))
    assert D.tolist() == [[250, 6, 4, -2 ** 31]] and I.tolist() == [[3, 4, 2, -1]]
    full = np.full((1, 32), -128, dtype=np.int8)
    assert asym_scores_numpy(full, np.array([[255] * 4, [0] * 4], dtype=np.uint8)).tolist() == [[-4096, 4096]]


def test_quantize_queries():
    """A zero query and one whose maximum is denormal give zeros; the maximum maps to +-127; a scaled value that lands
    on .5 goes to the even neighbour (x1 * 127 = 1.5 and x2 * 127 = 2.5 exactly in float32, 0.5 * 127 = 63.5)."""
    x1, x2 = float.fromhex("0x1.83060cp-7"), float.fromhex("0x1.42850ap-6")
    assert np.float32(x1) * np.float32(127) == 1.5 and np.float32(x2) * np.float32(127) == 2.5
    q = np.zeros((5, 32), dtype=np.float32)
    q[1, :3] = (1e-39, -1.1e-38, 5e-40)     # below 2^-126
    q[2, :4] = (0.5, -2.0, 1.0, 2.0)
    q[3, :5] = (1.0, x1, x2, -0.5, -x2)
    q[4, :2] = (1.1754944e-38, -1e-39)      # the smallest normal: kept; the denormal quotient rounds to 0
    q8, a = quantize_queries_numpy(q)
    assert q8.dtype == np.int8 and q8.shape == q.shape and a.dtype == np.float32
    assert not q8[:2].any() and a[0] == 0 and a[1] == np.float32(1.1e-38)
    assert q8[2, :4].tolist() == [32, -127, 64, 127] and q8[3, :5].tolist() == [127, 2, 2, -64, -2]
    assert q8[4, :2].tolist() == [127, -11] and not q8[2:, 5:].any()


def test_arguments_are_checked():
    """The Python layer refuses a wrong dtype, a wrong width and k outside [1, 128] before the library sees them."""
    if nat.device_count() == 0:
        ix = IndexBinaryFlat.__new__(IndexBinaryFlat)   # (the checks of the arguments need no store)
        ix.d, ix.code_size, ix._h = 32, 4, None
    else:
        ix = IndexBinaryFlat(32)
    q8, q = np.zeros((2, 32), dtype=np.int8), np.zeros((2, 32), dtype=np.float32)
    for k in (0, 129):
        with pytest.raises(ValueError, match=f"k={k} outside"):
            ix.search_asym(q8, k)
        with pytest.raises(ValueError, match=f"k={k} outside"):
            ix.search_asym_float(q, k)
    for bad in (q, q8.astype(np.uint8), np.zeros((2, 4), dtype=np.int8), np.zeros(32, dtype=np.int8)):
        with pytest.raises(ValueError, match="queries must be int8"):
            ix.search_asym(bad, 1)
    with pytest.raises(ValueError, match="expected shape"):
        ix.search_asym_float(np.zeros((2, 31), dtype=np.float32), 1)
    q[1, 7] = np.inf
    with pytest.raises(ValueError, match="NaN or infinite"):
        ix.search_asym_float(q, 1)
    ix.close()

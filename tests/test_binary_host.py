"""Host: the numpy restatement of the binary store (binary.binarize_numpy / hamming_numpy / search_numpy) on a
hand-written case, and the refusals of the Python layer and of css_bin_create, which checks d before it looks for a
device."""
import ctypes

import numpy as np
import pytest

from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd.binary import IndexBinaryFlat, binarize_numpy, binary_dim, hamming_numpy, search_numpy


def test_hand_written_case():
    """d = 32, the query all ones.  Row r has its first z[r] components not above zero (0.0, -0.0 and -1 among them), so
    its distance is z = (3, 1, 3, 0, 3): at k = 3 rows 0, 2 and 4 tie for the last place and row 0 takes it."""
    z = (3, 1, 3, 0, 3)
    x = np.ones((5, 32), dtype=np.float32)
    for r, m in enumerate(z):
        x[r, :m] = (0.0, -0.0, -1.0)[:m]
    x[3, 31] = 1e-45   # a denormal is above zero
    codes = binarize_numpy(x)
    assert codes.dtype == np.uint8 and codes.tolist() == [[0x1F, 255, 255, 255], [0x7F, 255, 255, 255], [0x1F, 255, 255, 255],
                                                          [255, 255, 255, 255], [0x1F, 255, 255, 255]]
    q = binarize_numpy(np.ones((1, 32), dtype=np.float32))
    h = hamming_numpy(q, codes)
    assert h.dtype == np.int64 and h.tolist() == [list(z)]
    D, I = search_numpy(h, 3)
    assert D.dtype == np.int32 and I.dtype == np.int64 and D.tolist() == [[0, 1, 3]] and I.tolist() == [[3, 1, 0]]
    D, I = search_numpy(h, 4, allow=np.array([False, True, True, False, True]))
    assert D.tolist() == [[1, 3, 3, 2 ** 31 - 1]] and I.tolist() == [[1, 2, 4, -1]]


@pytest.mark.parametrize("d", (0, 16, 40, 8224))
def test_d_refused(d):
    with pytest.raises(ValueError, match="multiple of 32"):
        binary_dim(d)
    with pytest.raises(ValueError, match="multiple of 32"):
        IndexBinaryFlat(d)
    h = ctypes.c_void_p()
    assert nat.lib().css_bin_create(d, 0, ctypes.byref(h)) == nat.CSS_ERR_INVALID
    assert f"d={d} must be a multiple of 32" in nat.last_error() and not h.value
    assert nat.lib().css_bin_create(32, 0, None) == nat.CSS_ERR_INVALID and "out is NULL" in nat.last_error()


def test_create_needs_a_device_and_arguments_are_checked():
    """Without a device a well-formed create is CSS_ERR_NO_DEVICE; the Python layer refuses k outside [1, 128], a wrong
    dtype or shape and a NaN row before the library sees them."""
    if nat.device_count() == 0:
        h = ctypes.c_void_p()
        assert nat.lib().css_bin_create(32, 0, ctypes.byref(h)) == nat.CSS_ERR_NO_DEVICE and not h.value
        ix = IndexBinaryFlat.__new__(IndexBinaryFlat)   # (the checks of the arguments need no store)
        ix.d, ix.code_size, ix._h = 32, 4, None
    else:
        ix = IndexBinaryFlat(32)
    codes, rows = np.zeros((1, 4), dtype=np.uint8), np.zeros((2, 32), dtype=np.float32)
    for k in (0, 129):
        with pytest.raises(ValueError, match=f"k={k} outside"):
            ix.search(codes, k)
        with pytest.raises(ValueError, match=f"k={k} outside"):
            ix.search_float(rows, k)
    for bad in (codes.astype(np.int8), np.zeros((1, 5), dtype=np.uint8), np.zeros(4, dtype=np.uint8)):
        with pytest.raises(ValueError, match="codes must be uint8"):
            ix.add(bad)
        with pytest.raises(ValueError, match="codes must be uint8"):
            ix.search(bad, 1)
    with pytest.raises(ValueError, match="expected shape"):
        ix.add_float(np.zeros((2, 31), dtype=np.float32))
    rows[1, 7] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        ix.add_float(rows)
    with pytest.raises(ValueError, match="NaN or infinite"):
        ix.search_float(rows, 1)
    with pytest.raises(ValueError, match="waves=-1 outside"):
        ix.set_waves(-1)
    ix.close()

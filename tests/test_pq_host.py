"""Host: the numpy restatement of the product quantizer (pq.ProductQuantizer) on a hand-computed case, and the refusals
of the Python layer and of css_pq_create, which checks its arguments before it looks for a device."""
import ctypes

import numpy as np
import pytest

from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd.pq import IndexPQ, ProductQuantizer, pq_dim, search_numpy


def hand_codebooks():
    """d = 32, M = 4.  Sub-quantizer 0: every centroid (4, .., 4) but 3 = +e0 and 5 = -e0; 1: every centroid (4, .., 4) but
    7 = (0.5, .., 0.5); 2: all zero; 3: centroid c = e1 * (c - 128) / 16."""
    cb = np.zeros((4, 256, 8), dtype=np.float32)
    cb[0], cb[1] = 4.0, 4.0
    cb[0, 3], cb[0, 5] = 0.0, 0.0
    cb[0, 3, 0], cb[0, 5, 0] = 1.0, -1.0
    cb[1, 7] = 0.5
    cb[3, :, 1] = (np.arange(256) - 128) / 16.0
    return cb


def test_hand_computed_case():
    """x = (0 x 8 | 0.5 x 8 | anything | 2 e1).  Sub-vector 0 is at squared distance 1 from centroids 3 AND 5 (every
    other is at 128): the exact tie goes to 3.  Sub-vector 1 is centroid 7; in sub-quantizer 2 all 256 centroids are
    equal and the code is 0; 2 = (160 - 128) / 16.  The decoded row sums to 1 + 4 + 0 + 2 = 7, and a query of
    1 + 2^-9 rounds to the bf16 1."""
    pq = ProductQuantizer(32, hand_codebooks())
    x = np.zeros((1, 32), dtype=np.float32)
    x[0, 8:16], x[0, 16:24], x[0, 25] = 0.5, 3.0, 2.0
    for dtype in (np.float32, np.float64):
        assert pq.encode_numpy(x, dtype).tolist() == [[3, 7, 0, 160]]
    dec = pq.decode_numpy(np.array([[3, 7, 0, 160], [5, 0, 9, 128]], dtype=np.uint8))
    want = np.zeros((2, 32), dtype=np.float32)
    want[0, 0], want[0, 8:16], want[0, 25] = 1.0, 0.5, 2.0
    want[1, 0], want[1, 8:16] = -1.0, 4.0
    assert np.array_equal(dec, want)
    q = np.full((1, 32), 1.0 + 2.0 ** -9, dtype=np.float32)
    s = pq.scores_numpy(q, np.array([[3, 7, 0, 160], [5, 0, 9, 128]], dtype=np.uint8))
    assert s.dtype == np.float64 and s.tolist() == [[7.0, 31.0]]
    D, I = search_numpy(np.array([[1.0, 2.0, 2.0, 0.5]]), 3, allow=np.array([True, True, True, False]))
    assert I.tolist() == [[1, 2, 0]] and D.tolist() == [[2.0, 2.0, 1.0]]


@pytest.mark.parametrize("d", (0, 16, 40, 8224))
def test_d_refused(d):
    with pytest.raises(ValueError, match="multiple of 32"):
        pq_dim(d)
    h = ctypes.c_void_p()
    buf = np.zeros(8, dtype=np.float32)
    assert nat.lib().css_pq_create(d, buf.ctypes.data, 0, ctypes.byref(h)) == nat.CSS_ERR_INVALID
    assert f"d={d} must be a multiple of 32" in nat.last_error() and not h.value


@pytest.mark.parametrize("value,word", ((np.nan, "NaN"), (np.inf, "infinite"), (3.4e38, "infinite once rounded to bf16")))
def test_codebooks_refused(value, word):
    cb = hand_codebooks()
    with pytest.raises(ValueError, match="shape"):
        ProductQuantizer(32, cb[:3])
    cb[2, 9, 5] = value
    with pytest.raises(ValueError, match="infinite"):
        ProductQuantizer(32, cb)
    h = ctypes.c_void_p()
    assert nat.lib().css_pq_create(32, cb.ctypes.data, 0, ctypes.byref(h)) == nat.CSS_ERR_INVALID
    assert f"component 5 of centroid 9 of codebooks[2] is {word}" in nat.last_error() and not h.value
    assert nat.lib().css_pq_create(32, None, 0, ctypes.byref(h)) == nat.CSS_ERR_INVALID and "codebooks is NULL" in nat.last_error()


def test_create_needs_a_device_and_k_is_checked():
    """Without a device a well-formed create is CSS_ERR_NO_DEVICE; with one, the Python layer refuses k > 128."""
    if nat.device_count() == 0:
        h = ctypes.c_void_p()
        assert nat.lib().css_pq_create(32, hand_codebooks().ctypes.data, 0, ctypes.byref(h)) == nat.CSS_ERR_NO_DEVICE
        assert not h.value
        ix = IndexPQ.__new__(IndexPQ)   # (the checks of the arguments need no store)
        ix.pq, ix.d, ix._h = ProductQuantizer(32, hand_codebooks()), 32, None
    else:
        ix = IndexPQ(32, hand_codebooks())
    with pytest.raises(ValueError, match="k=129 outside"):
        ix.search(np.zeros((1, 32), dtype=np.float32), 129)
    with pytest.raises(ValueError, match="k=0 outside"):
        ix.search(np.zeros((1, 32), dtype=np.float32), 0)
    ix.close()

"""CPU: the float64 restatement of the fixed-dimensional encoding on a hand-computed case, the argument checks (Python
and library: css_fde_create refuses before it looks for a device) and the default material."""
import ctypes

import numpy as np
import pytest

from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd.muvera import default_material, fde_args, fde_numpy


def test_hand_computed_case():
    """3 tokens, P = 32, k_sim = 2, one repetition.  planes = e0, e1, so bucket = (x[0] > 0) + 2 (x[1] > 0): tokens 0 and
    2 fall into bucket 1, token 1 into bucket 2; buckets 0 and 3 are empty and at Hamming distance 1 from BOTH filled
    buckets: the tie goes to token 0.  proj[j] = e_j reads off the first 16 components."""
    P, k_sim, d_proj = 32, 2, 16
    planes, proj, x = np.zeros((2, P)), np.zeros((d_proj, P)), np.zeros((3, P))
    planes[0, 0] = planes[1, 1] = 1.0
    proj[np.arange(d_proj), np.arange(d_proj)] = 1.0
    x[0, :4] = (1, -1, 2, 0)
    x[1, :4] = (-1, 1, 0, 4)
    x[2, :5] = (3, -1, 0, 0, 1)
    off = np.array([0, 3])
    doc, bk = fde_numpy(planes, proj, k_sim, d_proj, off, x, False)
    assert bk.reshape(-1).tolist() == [1, 2, 1]
    want = np.zeros((4, d_proj))
    want[0, :4] = want[3, :4] = (1, -1, 2, 0)          # the fill: token 0
    want[1, :5] = (2, -1, 1, 0, 0.5)                   # (x0 + x2) / 2
    want[2, :4] = (-1, 1, 0, 4)
    assert np.array_equal(doc.reshape(4, d_proj), want)
    qry, _ = fde_numpy(planes, proj, k_sim, d_proj, off, x, True)
    want[0] = want[3] = 0.0
    want[1, :5] = (4, -2, 2, 0, 1)
    assert np.array_equal(qry.reshape(4, d_proj), want)
    # an imposed assignment replaces the sketch; a matrix without tokens is a row of zeros
    imp, _ = fde_numpy(planes, proj, k_sim, d_proj, np.array([0, 0, 3]), x, True, buckets=np.array([[3], [3], [0]]))
    assert not imp[0].any() and np.array_equal(imp[1].reshape(4, d_proj)[3, :4], (0, 0, 2, 4))


@pytest.mark.parametrize("P,k_sim,d_proj,reps,word", [
    (48, 5, 16, 16, "P=48"), (160, 5, 16, 16, "P=160"), (128, 0, 16, 1, "k_sim=0"), (128, 7, 16, 1, "k_sim=7"),
    (128, 5, 8, 1, "d_proj=8"), (128, 5, 16, 0, "reps=0"), (128, 5, 16, 65, "reps=65"), (128, 5, 32, 16, "16384")])
def test_parameter_refusals(P, k_sim, d_proj, reps, word):
    with pytest.raises(ValueError, match=word):
        fde_args(P, k_sim, d_proj, reps)
    h = ctypes.c_void_p()
    buf = np.zeros(64 * 64 * 160, dtype=np.uint16)
    rc = nat.lib().css_fde_create(P, k_sim, d_proj, reps, buf.ctypes.data, buf.ctypes.data, 0, ctypes.byref(h))
    assert rc == nat.CSS_ERR_INVALID and word in nat.last_error() and not h.value


@pytest.mark.parametrize("which,bits,word", [("planes", 0x7FC0, "NaN"), ("proj", 0xFF80, "infinite")])
def test_material_refusals(which, bits, word):
    planes, proj = default_material(32, 2, 16, 3)
    {"planes": planes, "proj": proj}[which][4, 7] = bits
    h = ctypes.c_void_p()
    rc = nat.lib().css_fde_create(32, 2, 16, 3, planes.ctypes.data, proj.ctypes.data, 0, ctypes.byref(h))
    assert rc == nat.CSS_ERR_INVALID and f"component 7 of row 4 of {which} is {word}" in nat.last_error()


def test_default_material_is_a_function_of_the_seed():
    a, b, c = default_material(96, 4, 32, 8, seed=3), default_material(96, 4, 32, 8, seed=3), default_material(96, 4, 32, 8, seed=4)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0].tobytes() != c[0].tobytes()
    assert a[0].shape == (32, 96) and a[1].shape == (256, 96) and a[0].dtype == a[1].dtype == np.uint16
    assert set(np.unique(a[1]).tolist()) == {0x3E35, 0xBE35}   # +-bf16(1 / sqrt(32))

"""Host: the numpy restatement of the scalar-quantized store (sq.ScalarQuantizer, search_numpy) on hand-written cases, and
the refusals of the Python layer and of css_sq_create, which checks its arguments before it looks for a device."""
import ctypes

import numpy as np
import pytest

from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd import binary
from claude_semantic_search_amd.sq import IndexScalarQuantizer, ScalarQuantizer, search_numpy, train_scalar_quantizer


def unit(bits, d=32, vmin=0.0, step=1.0):
    return ScalarQuantizer(d, bits, np.full(d, vmin, np.float32), np.full(d, step, np.float32))


@pytest.mark.parametrize("bits", (4, 8))
def test_hand_written_case(bits):
    """d = 32, q8 = (5, -128, 127, 0 ...): a row scores 5 c0 - 128 c1 + 127 c2 whatever its other levels.  Rows 1 and 3
    tie at 258 for rank 2, and row 1 takes it."""
    sq = unit(bits)
    q8 = np.zeros((1, 32), dtype=np.int8)
    q8[0, :3] = (5, -128, 127)
    lv = np.zeros((5, 32), dtype=np.float32)
    lv[:, :3] = [(3, 0, 2), (1, 1, 3), (0, 2, 2), (1, 1, 3), (15, 15, 15)]
    lv[3, 3:] = 7
    codes = sq.encode_numpy(lv)
    assert codes.dtype == np.uint8 and codes.shape == (5, 32 * bits // 8) and np.array_equal(sq.levels(codes), lv)
    s = sq.scores_numpy(q8, codes)
    assert s.dtype == np.int64 and s.tolist() == [[269, 258, -2, 258, 60]]
    D, I = search_numpy(s, 2)
    assert D.dtype == np.int32 and I.dtype == np.int64 and D.tolist() == [[269, 258]] and I.tolist() == [[0, 1]]
    D, I = search_numpy(s, 4, allow=np.array([False, False, True, True, True]))
    assert D.tolist() == [[258, 60, -2, -2 ** 31]] and I.tolist() == [[3, 4, 2, -1]]
    q = np.zeros((1, 32), dtype=np.float32)
    q[0, :2] = (2.0, -1.0)   # q8 = (127, -64): the estimate of <q, (3, 0, ..)> = 6 is 2 * 381 / 127
    assert sq.estimate(q, np.array([[381, -2 ** 31]])).tolist() == [[6.0, -np.inf]]


@pytest.mark.parametrize("bits", (4, 8))
def test_encode_cases(bits):
    """Below vmin, above vmin + L step, exactly half a step between two levels (to the even one), -0.0; the nibble order
    of the 4-bit codes; decode(encode(x)) within step / 2 inside the range (a grid on which every operation is exact)."""
    sq, L = unit(bits, vmin=-1.0, step=0.5), 2 ** bits - 1
    x = np.full((1, 32), -1.0, dtype=np.float32)
    x[0, :8] = (-5.0, -1.0 + 0.5 * L + 3.0, 0.25, 0.75, -0.0, -1.0 + 0.5 * L, -1.26, 1e30)
    assert sq.levels(sq.encode_numpy(x))[0, :9].tolist() == [0, L, 2, 4, 2, L, 0, L, 0]
    assert sq.levels(unit(bits).encode_numpy(np.full((1, 32), -0.0, np.float32))).tolist() == [[0] * 32]
    ramp = (np.arange(32) % 16).astype(np.float32)[None]
    if bits == 4:
        assert unit(4).encode_numpy(ramp)[0, :3].tolist() == [0x10, 0x32, 0x54] and unit(4).code_size == 16
    g = ScalarQuantizer(32, bits, np.full(32, -2.0, np.float32), np.full(32, 0.25, np.float32))
    xs = (-2.0 + np.random.default_rng(1).integers(0, L * 256 + 1, size=(64, 32)) / 1024).astype(np.float32)
    back = g.decode_numpy(g.encode_numpy(xs))
    assert back.dtype == np.float32 and (np.abs(back - xs) <= 0.125).all() and (np.abs(back - xs) == 0.125).any()
    # 255 * 2^-30 + 1 is not a float32: the nearest one is 1 + 2^-22
    t =ScalarQuantizer(32, 8, np.full(32, 1.0, np.float32), np.full(32, 2.0 ** -30, np.float32))
    assert (t.decode_numpy(np.full((1, 32), 255, np.uint8)) == 1.0 + 2.0 ** -22).all()


def test_quantize_queries_folds_the_step():
    """The four cases of the binary store's asymmetric host test with step = 0.5 folded in (q = 2 w, exactly): a zero
    query and one whose maximum is denormal give zeros; the maximum maps to +-127; .5 goes to the even neighbour."""
    x1, x2 = float.fromhex("0x1.83060cp-7"), float.fromhex("0x1.42850ap-6")
    w = np.zeros((5, 32), dtype=np.float32)
    w[1, :3] = (1e-39, -1.1e-38, 5e-40)
    w[2, :4] = (0.5, -2.0, 1.0, 2.0)
    w[3, :5] = (1.0, x1, x2, -0.5, -x2)
    w[4, :2] = (1.1754944e-38, -1e-39)
    q8, a = unit(8, step=0.5).quantize_queries_numpy(2 * w)
    r8, ra = binary.quantize_queries_numpy(w)
    assert q8.dtype == np.int8 and np.array_equal(q8, r8) and np.array_equal(a, ra) and a[1] == np.float32(1.1e-38)
    assert not q8[:2].any() and q8[2, :4].tolist() == [32, -127, 64, 127] and q8[3, :5].tolist() == [127, 2, 2, -64, -2]
    assert q8[4, :2].tolist() == [127, -11]
    with pytest.raises(ValueError, match="times its step is infinite"):
        unit(8, step=4.0).quantize_queries_numpy(np.full((1, 32), 1e38, np.float32))


def test_train():
    x = np.random.default_rng(2).standard_normal((100, 32)).astype(np.float32)
    x[:, 5] = 3.0
    sq = train_scalar_quantizer(x, 4)
    assert np.array_equal(sq.vmin, x.min(0)) and sq.step[5] == 1.0 and np.allclose(sq.step[:5], (x.max(0) - x.min(0))[:5] / 15)
    assert (train_scalar_quantizer(x, 8, 0.9).step[:5] < train_scalar_quantizer(x, 8).step[:5]).all()


def test_quantizer_refused():
    """What ScalarQuantizer refuses, css_sq_create refuses with CSS_ERR_INVALID, before it looks for a device."""
    ok = np.ones(64, dtype=np.float32)

    def both(d, bits, vmin, step, py, c):
        with pytest.raises(ValueError, match=py):
            ScalarQuantizer(d, bits, vmin[:max(d, 0)], step[:max(d, 0)])
        h = ctypes.c_void_p()
        assert nat.lib().css_sq_create(d, bits, vmin.ctypes.data, step.ctypes.data, 0, ctypes.byref(h)) == nat.CSS_ERR_INVALID
        assert c in nat.last_error() and not h.value

    for d in (0, 16, 40, 8224):
        both(d, 8, np.ones(8224, np.float32), np.ones(8224, np.float32), "multiple of 32", f"d={d} must be a multiple of 32")
    both(32, 6, ok, ok, "bits=6 must be 4 or 8", "bits=6 must be 4 or 8")
    for i, v in ((3, 0.0), (4, -1.0), (5, np.nan), (6, np.inf)):
        bad = ok.copy()
        bad[i] = v
        both(32, 4, ok, bad, "finite and above 0", f"step[{i}]")
    bad = ok.copy()
    bad[7] = -np.inf
    both(32, 8, bad, ok, "vmin holds", "vmin[7] is infinite")
    with pytest.raises(ValueError, match="must have shape"):
        ScalarQuantizer(32, 8, ok, ok[:32])
    assert nat.lib().css_sq_create(32, 8, ok.ctypes.data, ok.ctypes.data, 0, None) == nat.CSS_ERR_INVALID and "out is NULL" in nat.last_error()


def test_create_needs_a_device_and_arguments_are_checked():
    """Without a device a well-formed create is CSS_ERR_NO_DEVICE; the Python layer refuses k outside [1, 128], a wrong
    dtype or shape and a NaN row or query before the library sees them."""
    sq = unit(4)
    if nat.device_count() == 0:
        h = ctypes.c_void_p()
        assert nat.lib().css_sq_create(32, 4, sq.vmin.ctypes.data, sq.step.ctypes.data, 0, ctypes.byref(h)) == nat.CSS_ERR_NO_DEVICE
        assert not h.value
        with pytest.raises(RuntimeError, match="no HIP device"):
            IndexScalarQuantizer(sq)
        ix = IndexScalarQuantizer.__new__(IndexScalarQuantizer)   # (the checks of the arguments need no store)
        ix.sq, ix.d, ix.code_size, ix._h = sq, 32, 16, None
    else:
        ix = IndexScalarQuantizer(sq)
    q8, q = np.zeros((2, 32), dtype=np.int8), np.zeros((2, 32), dtype=np.float32)
    for k in (0, 129):
        with pytest.raises(ValueError, match=f"k={k} outside"):
            ix.search_i8(q8, k)
        with pytest.raises(ValueError, match=f"k={k} outside"):
            ix.search(q, k)
    for bad in (q, q8.astype(np.uint8), np.zeros((2, 16), dtype=np.int8), np.zeros(32, dtype=np.int8)):
        with pytest.raises(ValueError, match="queries must be int8"):
            ix.search_i8(bad, 1)
    for bad in (np.zeros((1, 32), dtype=np.uint8), np.zeros((1, 16), dtype=np.int8), np.zeros(16, dtype=np.uint8)):
        with pytest.raises(ValueError, match="codes must be uint8"):
            ix.add_codes(bad)
    with pytest.raises(ValueError, match="expected shape"):
        ix.add(np.zeros((2, 31), dtype=np.float32))
    q[1, 7] = np.nan
    for call in (ix.add, lambda a: ix.search(a, 1)):
        with pytest.raises(ValueError, match="NaN or infinite"):
            call(q)
    with pytest.raises(ValueError, match="waves=-1 outside"):
        ix.set_waves(-1)
    ix.close()

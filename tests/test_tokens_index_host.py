"""CPU: the host side of the token matrices on the flat index -- the refusals of ``tokens_as_csr`` / ``maxsim_args``, the
numpy double against ``maxsim_numpy``, ``synth.token_matrices``, and the proof that the lattice cases of
tests/test_tokens_index_gpu.py BIND: for every (P, k) searched there, at least one query has equal scores on both sides
of rank k, counted with numpy alone."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tokens_cases as tc  # noqa: E402
import tokens_fakes as tf  # noqa: E402
from claude_semantic_search_amd import synth  # noqa: E402
from claude_semantic_search_amd.flat_index import maxsim_args, tokens_as_csr  # noqa: E402
from claude_semantic_search_amd.late_interaction import bf16_to_f32, maxsim_numpy  # noqa: E402

NAN, INF = np.uint16(0x7FC0), np.uint16(0xFF80)


def _m(m, P=32, fill=0x3F80):
    return np.full((m, P), fill, np.uint16)


def test_tokens_as_csr_forms_and_keep_flags():
    mats = [_m(3), _m(0), _m(2, fill=0x4000)]
    off, tok, P = tokens_as_csr(mats)
    assert off.tolist() == [0, 3, 3, 5] and tok.shape == (5, 32) and tok.dtype == np.uint16 and P == 32
    # the CSR triple gives itself back; float32 that IS bf16 is taken, and its bits are the bf16 bits
    off2, tok2, P2 = tokens_as_csr((off, tok, 32))
    assert np.array_equal(off2, off) and np.array_equal(tok2, tok) and P2 == 32
    _, tok3, _ = tokens_as_csr([bf16_to_f32(m) for m in mats])
    assert np.array_equal(tok3, tok)
    # a dropped token is not stored; a row whose every token is dropped is empty
    keep = [np.array([1, 0, 1], np.uint8), None, np.zeros(2, np.uint8)]
    off4, tok4, _ = tokens_as_csr(mats, keep)
    assert off4.tolist() == [0, 2, 2, 2] and np.array_equal(tok4, tok[[0, 2]])
    off5, tok5, P5 = tokens_as_csr([])
    assert off5.tolist() == [0] and tok5.shape[0] == 0 and P5 % 32 == 0


@pytest.mark.parametrize("mats, keep, message", [
    ([_m(2), _m(2, P=64)], None, r"row 1 \(of this call\) has P=64, the rows before it P=32"),
    ([_m(2, P=48)], None, r"row 0 \(of this call\) has P=48"),
    ([_m(2, P=160)], None, r"row 0 \(of this call\) has P=160"),
    ([_m(2), np.zeros(32, np.uint16)], None, r"row 1 \(of this call\) has shape \(32,\)"),
    ([_m(2), _m(513)], None, r"row 1 \(of this call\) has 513 tokens \(at most 512\)"),
    ([_m(2).astype(np.float64)], None, r"row 0 \(of this call\) must be uint16 \(bf16 bits\) or bf16-exact float32"),
    ([np.full((2, 32), 0.1, np.float32)], None, r"row 0 \(of this call\) holds float32 values that are not bf16 values"),
    ([_m(2), _m(3)], [np.ones(2), np.ones(2)], r"2 keep flags for the 3 tokens of row 1"),
    ([_m(2)], [None, None], r"2 keep arrays for 1 matrices"),
])
def test_tokens_as_csr_refuses_and_names_the_row(mats, keep, message):
    with pytest.raises(ValueError, match=message):
        tokens_as_csr(mats, keep)


@pytest.mark.parametrize("bits, word", [(NAN, "NaN or infinite"), (INF, "NaN or infinite")])
def test_tokens_as_csr_refuses_non_finite_components(bits, word):
    bad = _m(4)
    bad[2, 7] = bits
    with pytest.raises(ValueError, match=rf"token 2 of row 1 \(of this call\) has a {word} component"):
        tokens_as_csr([_m(3), bad])
    off, tok, P = tokens_as_csr([_m(3), _m(4)])
    tok[5, 0] = bits
    with pytest.raises(ValueError, match=r"token 2 of row 1"):
        tokens_as_csr((off, tok, P))
    with pytest.raises(ValueError, match=r"keep flags go with a sequence"):
        tokens_as_csr((off, _m(7), P), keep=[None, None])
    with pytest.raises(ValueError, match=r"no whole tokens of P=64"):
        tokens_as_csr((off, np.zeros(7 * 32, np.uint16), 64))


def test_maxsim_args_refuses():
    q, k, ids = maxsim_args(_m(5), 10, [3, 1, 3])
    assert q.shape == (5, 32) and k == 10 and ids.tolist() == [3, 1, 3] and ids.dtype == np.int64
    for bad, message in ((_m(0), r"0 query tokens outside \[1, 64\]"), (_m(65), r"65 query tokens"),
                         (_m(3, P=48), r"P=48"), (np.zeros(32, np.uint16), r"one query matrix \[mq, P\]"),
                         (np.full((2, 32), 0.3, np.float32), r"not bf16 values")):
        with pytest.raises(ValueError, match=message):
            maxsim_args(bad, 5)
    nan = _m(4)
    nan[3, 0] = NAN
    with pytest.raises(ValueError, match=r"query token 3 has a NaN or infinite component"):
        maxsim_args(nan, 5)
    for k in (0, 129):
        with pytest.raises(ValueError, match=rf"k={k} outside \[1, 128\]"):
            maxsim_args(_m(2), k)
    with pytest.raises(ValueError, match=r"65537 ids \(at most 65536\)"):
        maxsim_args(_m(2), ids=np.zeros(65537, np.int64), what="maxsim_ids")


def test_synth_token_matrices_have_the_length_profile_of_the_tests():
    off, tok, P = synth.token_matrices(tc.N, 96, 5)
    lens = np.diff(off)
    assert P == 96 and tok.shape == (int(off[-1]), 96) and tok.dtype == np.uint16
    assert lens[:9].tolist() == [0, 1, 15, 16, 17, 63, 64, 65, 512] and lens[9:].max() == 40 and (lens[9:] == 0).any()
    norms = np.linalg.norm(bf16_to_f32(tok).astype(np.float64), axis=1)
    assert np.abs(norms - 1.0).max() < 2.0 ** -7                       # unit rows, rounded to bf16
    for fam, values in (("T", {-1.0, 0.0, 1.0}), ("E", {v / 8.0 for v in range(-8, 9)}), (True, {v / 8.0 for v in range(-8, 9)})):
        _, t, _ = synth.token_matrices(200, 32, 6, lattice=fam)
        assert set(np.unique(bf16_to_f32(t)).tolist()) <= values
    assert np.array_equal(synth.token_matrices(50, 32, 7)[1], synth.token_matrices(50, 32, 7)[1])


def test_the_double_equals_maxsim_numpy_row_by_row():
    ms, qs = tc.gaussian(64)
    for q in (qs[0], qs[3], qs[5]):
        col = ms.scores64(q)
        rows = list(range(12)) + [100, 1500, tc.N - 1]
        for r in rows:
            d = ms.mat(r)
            want = maxsim_numpy(q, d) if d.shape[0] else -np.inf
            assert col[r] == want or abs(col[r] - want) <= 1e-12 * abs(want), (r, col[r], want)
    D, I = tf.topk(ms.scores64(qs[2]), 10, id_base=7)
    assert (np.diff(D[0]) <= 0).all() and (I[0] >= 7).all() and ms.lens[I[0] - 7].min() > 0
    # the fake index: storage rules and the two calls
    ix = tf.FakeTokenIndex(4)
    ix.add(np.zeros((30, 4), np.float32))
    ix.set_tokens(ms.rows(np.arange(20)).mats())
    ix.set_tokens(ms.rows(np.arange(10, 25)).mats(), row0=10)
    assert ix.token_rows == 25 and ix.token_dim == 64
    off, tok = ix.get_tokens()
    want = ms.rows(np.arange(25)).padded(30)
    assert np.array_equal(off, want.off) and np.array_equal(tok, want.tok)
    D, I = ix.search_maxsim(qs[1], 5)
    Dt, It = tf.topk(want.scores64(qs[1]), 5)
    assert np.array_equal(D, Dt) and np.array_equal(I, It)
    got = ix.maxsim_ids(qs[1], [It[0, 0], 0, 29, It[0, 0]])
    assert got[0] == D[0, 0] == got[3] and got[1] == -np.inf and got[2] == -np.inf


@pytest.mark.parametrize("P", tc.WIDTHS)
def test_lattice_cases_bind_at_every_k(P):
    """For every (P, k) of the GPU lattice test some query of some family has tied scores straddling rank k -- with
    and without the half mask for k = 10 -- and the lattice scores are exact in fp32."""
    allow = tc.half_mask()
    tied = {(k, masked): 0 for k in tc.KS for masked in (False, True)}
    for family in tc.FAMILIES:
        ms, qs = tc.lattice(family, P)
        assert ms.lens[:9].tolist() == list(tc.EDGE) and ms.n == tc.N
        for j, q in enumerate(qs):
            col = ms.scores64(q)
            hit = col > -np.inf
            assert np.array_equal(col[hit].astype(np.float32).astype(np.float64), col[hit])      # exact in fp32
            assert np.array_equal(col[hit] * 64, np.round(col[hit] * 64))                        # on the lattice
            for k in tc.KS:
                tied[(k, False)] += tf.ties_at(col, k)
                tied[(k, True)] += tf.ties_at(col, k, allow)
            if j == tc.PLANT_QUERY:
                top = np.flatnonzero(col == col.max())
                assert set(tc.PLANTS) <= set(top.tolist()) and tf.ties_at(col, 1)
    print(f"[tokens lattice] P={P}: queries with a tie at rank k (k, masked): {tied}")
    assert all(v >= 1 for v in tied.values()), tied


def test_negative_case_is_negative_everywhere():
    ms, q = tc.negative_case(32)
    col = ms.scores64(q)
    assert (col[ms.lens > 0] < 0).all() and (col[ms.lens == 0] == -np.inf).all()

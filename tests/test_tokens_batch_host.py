"""CPU: the argument rules of the batched MaxSim search (``flat_index.maxsim_batch_args``), its numpy double
(``tokens_batch_fakes.FakeTokenBatchIndex``), and the proof that the checks of tests/test_tokens_batch_gpu.py bind: the
six queries of every ``(family, P)`` of ``tokens_cases.lattice`` have pairwise different float64 truths at k = 10, so a
batch that mixes up its slots cannot pass."""
import numpy as np
import pytest

import tokens_cases as tc
from claude_semantic_search_amd import flat_index as fi
from tokens_batch_fakes import FakeTokenBatchIndex
from tokens_fakes import topk

P = 32


def _q(m, P=P, seed=0):
    rng = np.random.default_rng(seed + m)
    return tc.to_bits((rng.integers(-8, 9, size=(m, P)) / 8.0).astype(np.float32))


def test_maxsim_batch_args_returns_offsets_tokens_and_k():
    qs = [_q(3), _q(1), _q(64)]
    off, tok, k = fi.maxsim_batch_args(qs, 7)
    assert off.dtype == np.int64 and off.tolist() == [0, 3, 4, 68] and k == 7
    assert tok.dtype == np.uint16 and tok.shape == (68, P) and tok.flags.c_contiguous
    for b, q in enumerate(qs):
        assert np.array_equal(tok[off[b]:off[b + 1]], q)
    # bf16-exact float32 is taken as well, and gives the same bits
    f32 = [(q.astype(np.uint32) << 16).view(np.float32) for q in qs]
    off2, tok2, _ = fi.maxsim_batch_args(f32, 7)
    assert np.array_equal(off2, off) and np.array_equal(tok2, tok)
    assert fi.maxsim_batch_args([_q(1)] * fi.MAX_MAXSIM_QUERIES, 1)[0].shape == (fi.MAX_MAXSIM_QUERIES + 1,)
    assert fi.MAX_MAXSIM_QUERIES == 1024 and fi.MAXSIM_BATCH_GROUP >= 4


def test_maxsim_batch_args_refuses_and_names_the_query():
    ok = [_q(2), _q(5), _q(9)]
    with pytest.raises(ValueError, match=r"0 queries"):
        fi.maxsim_batch_args([], 5)
    with pytest.raises(ValueError, match=r"1025 queries"):
        fi.maxsim_batch_args([_q(1)] * 1025, 5)
    with pytest.raises(ValueError, match=r"query 1\b.*0 query tokens"):
        fi.maxsim_batch_args([ok[0], np.zeros((0, P), np.uint16), ok[2]], 5)
    with pytest.raises(ValueError, match=r"query 2\b.*65 query tokens"):
        fi.maxsim_batch_args([ok[0], ok[1], np.zeros((65, P), np.uint16)], 5)
    with pytest.raises(ValueError, match=r"query 2 has P=64.*P=32"):
        fi.maxsim_batch_args([ok[0], ok[1], _q(4, 64)], 5)
    with pytest.raises(ValueError, match=r"query 1\b.*P=48"):
        fi.maxsim_batch_args([ok[0], np.zeros((2, 48), np.uint16)], 5)
    bad = ok[1].copy()
    bad[3, 7] = 0x7FC0
    with pytest.raises(ValueError, match=r"query 1\b.*query token 3.*NaN"):
        fi.maxsim_batch_args([ok[0], bad, ok[2]], 5)
    inexact = (ok[2].astype(np.uint32) << 16).view(np.float32).copy()
    inexact[0, 0] = np.float32(1.0) + np.float32(2.0 ** -20)
    with pytest.raises(ValueError, match=r"query 2\b.*not bf16 values"):
        fi.maxsim_batch_args([ok[0], ok[1], inexact], 5)
    with pytest.raises(ValueError, match=r"query 0\b.*shape"):
        fi.maxsim_batch_args([np.zeros(P, np.uint16)], 5)
    for k in (0, 129):
        with pytest.raises(ValueError, match=f"k={k}"):
            fi.maxsim_batch_args(ok, k)


def test_the_double_is_the_loop_of_single_calls():
    rng = np.random.default_rng(4)
    n = 77
    ix = FakeTokenBatchIndex(8)
    ix.add((rng.integers(-8, 9, size=(n, 8)) / 8.0).astype(np.float32))
    qs = [_q(m) for m in (1, 17, 64, 5, 5, 16, 3, 2, 9, 33)]
    D_, I = ix.search_maxsim_batch(qs, 6)
    assert (I == -1).all() and D_.shape == I.shape == (10, 6) and ix.last_maxsim_passes == 0   # no matrices yet
    ix.set_tokens([_q(int(rng.integers(0, 7)), seed=100 + r) for r in range(n - 7)])
    allow = rng.random(n) < 0.6
    for al in (None, allow):
        D_, I = ix.search_maxsim_batch(qs, 6, allow=al)
        assert D_.dtype == np.float32 and I.dtype == np.int64 and D_.shape == I.shape == (10, 6)
        for b, q in enumerate(qs):
            d1, i1 = ix.search_maxsim(q, 6, allow=al)
            assert np.array_equal(D_[b:b + 1].view(np.uint32), d1.view(np.uint32)) and np.array_equal(I[b:b + 1], i1)
    assert ix.last_maxsim_passes == -(-10 // fi.MAXSIM_BATCH_GROUP)
    assert np.array_equal(I[3], I[4])                                           # equal queries, equal rows


@pytest.mark.parametrize("P", tc.WIDTHS)
@pytest.mark.parametrize("family", tc.FAMILIES)
def test_the_six_truths_differ_pairwise_so_a_slot_mix_up_cannot_pass(family, P):
    ms, qs = tc.lattice(family, P)
    truths = [topk(ms.scores64(q), 10) for q in qs]
    for a in range(len(qs)):
        for b in range(a + 1, len(qs)):
            same = np.array_equal(truths[a][0], truths[b][0]) and np.array_equal(truths[a][1], truths[b][1])
            assert not same, f"{family} P={P}: queries {a} and {b} have the same truth at k = 10"
            assert not np.array_equal(truths[a][0], truths[b][0]), f"{family} P={P}: queries {a} and {b} have the same D"
